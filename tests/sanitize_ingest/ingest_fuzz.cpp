// ingest_fuzz — the host code of the ingest section (csrc/dsm_pcm_format.h, DSM_PCM_IN: the descriptor of a format, its checked reader, the
// streaming host function) under AddressSanitizer + UBSan.  A stand-alone program with its own main:
//   1  every supported common rate x every sample format streams seeded frames, each copied into a heap buffer of exactly the
//      format's frame length (so a read past the frame is a report), through host_step_in; the outputs are finite for finite input;
//   2  random rates and formats, valid and not, go through describe() and host_new(): accepted or refused with a message; what
//      is accepted passes check() and streams two frames;
//   3  valid descriptors mutated (one word overwritten with an edge value), and wholly random ones, go through check() with
//      random arena lengths: a clean 0 or a clean DSM_ERR_INVALID; a mutated descriptor put into a live state, and frames
//      shorter or longer than declared, are refused by host_step_in before anything is read; a resampling descriptor made for
//      the other direction is refused by check().
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_pcm_format.h"

static uint64_t rng_state = 0x1A6E57ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "ingest_fuzz: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

static const uint32_t kEdgeWords[] = {0u, 1u, 2u, 3u, 4u, 24u, 25u, 67u, 68u, 136u, 137u, 639u, 640u, 1920u, 3840u, 3841u, 4096u, 4097u,
                                      7999u, 8000u, 15360u, 24000u, 48000u, 48001u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};

// a frame of exactly `bytes` bytes on the heap: finite samples whatever the format
static std::unique_ptr<uint8_t[]> frame_of(uint32_t fmt, size_t bytes) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[bytes ? bytes : 1]);
  if (fmt == DSM_PCM_F32) {
    for (size_t i = 0; i + 4 <= bytes; i += 4) {
      const float v = ((float)(rnd() >> 40) / 16777216.0f) * 2.0f - 1.0f;
      memcpy(p.get() + i, &v, 4);
    }
    for (size_t i = bytes & ~(size_t)3; i < bytes; ++i) p[i] = 0;
  } else {
    for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  }
  return p;
}

static int stream(dsm_pcm::Host* h, int frames) {
  std::string err;
  std::vector<float> out(DSM_FRAME_SIZE);
  for (int t = 0; t < frames; ++t) {
    auto f = frame_of(h->d.fmt, h->d.frame_bytes);
    CHECK(dsm_pcm::host_step_in(h, f.get(), h->d.frame_bytes, out.data(), &err) == 0);
    for (float v : out) CHECK(std::isfinite(v) && std::fabs(v) < 4.0f);
  }
  return 0;
}

int main() {
  std::string err;
  const int rates[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000};
  // 1
  for (int rate : rates)
    for (int fmt = 0; fmt < 4; ++fmt) {
      dsm_pcm::Host h;
      CHECK(dsm_pcm::host_new(DSM_PCM_IN, rate, fmt, &h, &err) == 0);
      CHECK(h.d.frame * 25u == 2u * (uint32_t)rate && h.d.taps <= DSM_PCM_MAX_TAPS_IN && h.d.frame <= DSM_PCM_MAX_FRAME);
      CHECK(h.d.frame_bytes <= DSM_PCM_MAX_FRAME_BYTES && h.coef.size() == h.d.table_words);
      if (stream(&h, 3)) return 1;
      // frames shorter and longer than declared: refused, the state as it was
      const std::vector<float> before = h.buf;
      std::vector<float> out(DSM_FRAME_SIZE);
      for (size_t bytes : {(size_t)0, (size_t)1, (size_t)h.d.frame_bytes - 1, (size_t)h.d.frame_bytes + 1, (size_t)below(h.d.frame_bytes)}) {
        auto f = frame_of((uint32_t)fmt, bytes);
        err.clear();
        CHECK(dsm_pcm::host_step_in(&h, f.get(), bytes, out.data(), &err) == DSM_ERR_INVALID && !err.empty());
      }
      CHECK(h.buf == before);
      CHECK(dsm_pcm::host_step_in(&h, nullptr, h.d.frame_bytes, out.data(), &err) == DSM_ERR_INVALID);
      // the direction is no word of the descriptor: where the two differ (every rate that resamples) check() tells them apart
      CHECK(dsm_pcm::check(DSM_PCM_OUT, &h.d, h.coef.size(), &err) == (rate == DSM_PCM_RATE ? 0 : DSM_ERR_INVALID));
      if (stream(&h, 1)) return 1;
    }
  // 2
  int accepted = 0;
  for (int it = 0; it < 400; ++it) {
    long rate, fmt;
    switch (below(4)) {
      case 0: rate = 25 * (long)(300 + below(1700)); break;                          // whole frames, around and inside the range
      case 1: rate = (long)below(60000); break;
      case 2: rate = (long)kEdgeWords[below(sizeof kEdgeWords / sizeof *kEdgeWords)]; break;
      default: rate = -(long)below(50000); break;
    }
    fmt = below(3) ? (long)below(4) : (long)(int32_t)kEdgeWords[below(sizeof kEdgeWords / sizeof *kEdgeWords)];
    dsm_pcm_desc d;
    err.clear();
    const int rc = dsm_pcm::describe(DSM_PCM_IN, rate, fmt, &d, &err);
    dsm_pcm::Host h;
    std::string err2;
    const int rc2 = dsm_pcm::host_new(DSM_PCM_IN, rate, fmt, &h, &err2);
    CHECK(rc == rc2);
    if (rc) { CHECK(rc == DSM_ERR_INVALID && !err.empty() && !err2.empty()); continue; }
    CHECK(rate >= 8000 && rate <= 48000 && rate % 25 == 0 && fmt >= 0 && fmt < 4);
    CHECK(dsm_pcm::check(DSM_PCM_IN, &h.d, h.coef.size(), &err) == 0);
    if (accepted++ < 40 && stream(&h, 2)) return 1;  // the phase table of an odd rate has up to 960 phases: a few dozen are enough
  }
  CHECK(accepted > 50);
  // 3
  for (int it = 0; it < 4000; ++it) {
    dsm_pcm_desc d;
    uint32_t w[DSM_PCM_DESC_WORDS];
    const bool mutated = below(3) != 0;
    if (mutated) {
      CHECK(dsm_pcm::describe(DSM_PCM_IN, rates[below(8)], (long)below(4), &d, &err) == 0);
      memcpy(w, &d, sizeof w);
      const uint32_t at = below(DSM_PCM_DESC_WORDS);
      w[at] = below(2) ? kEdgeWords[below(sizeof kEdgeWords / sizeof *kEdgeWords)] : w[at] + 1u - 2u * below(2);
    } else {
      for (uint32_t& x : w) x = below(2) ? (uint32_t)rnd() : kEdgeWords[below(sizeof kEdgeWords / sizeof *kEdgeWords)];
    }
    std::unique_ptr<dsm_pcm_desc> heap(new dsm_pcm_desc);
    memcpy(heap.get(), w, sizeof w);
    const size_t arena = below(2) ? (size_t)below(200000) : (size_t)heap->table_off + heap->table_words - below(2);
    err.clear();
    const int rc = dsm_pcm::check(DSM_PCM_IN, heap.get(), arena, &err);
    CHECK(rc == 0 || (rc == DSM_ERR_INVALID && !err.empty()));
    if (rc == 0) {  // then every index of a step is inside the frame, the history and the arena
      CHECK(heap->taps <= DSM_PCM_MAX_TAPS_IN && heap->frame <= DSM_PCM_MAX_FRAME && heap->taps == 2u * heap->half);
      CHECK((uint64_t)heap->table_off + (uint64_t)heap->L * heap->taps <= arena && heap->reserved == 0u);
      CHECK(heap->frame_bytes == heap->frame * dsm_pcm_sample_bytes(heap->fmt));
    }
    if (mutated && it % 8 == 0) {  // the mutated descriptor inside a live state: host_step checks before it reads
      dsm_pcm::Host h;
      CHECK(dsm_pcm::host_new(DSM_PCM_IN, rates[below(8)], (long)below(4), &h, &err) == 0);
      const dsm_pcm_desc good = h.d;
      h.d = *heap;
      std::vector<float> out(DSM_FRAME_SIZE);
      auto f = frame_of(good.fmt, good.frame_bytes);
      const int rs = dsm_pcm::host_step_in(&h, f.get(), good.frame_bytes, out.data(), &err);
      CHECK(rs == 0 || rs == DSM_ERR_INVALID);
      if (rs == 0) CHECK(h.d.frame_bytes == good.frame_bytes && h.buf.size() == (size_t)h.d.taps + h.d.frame);
    }
  }
  puts("ingest_fuzz ok");
  return 0;
}
