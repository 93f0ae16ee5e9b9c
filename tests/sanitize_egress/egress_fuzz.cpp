// egress_fuzz — the host code of the egress section (csrc/dsm_pcm_format.h, DSM_PCM_OUT: the descriptor of an output format, its checked reader,
// the sample encoders, the streaming host function) under AddressSanitizer + UBSan.  A stand-alone program with its own main:
//   1  every admitted common rate x every sample format streams frames through host_step_out into a heap row of exactly the
//      format's frame_bytes (so a write past the row is a report), from heap frames of exactly 1920 floats: seeded noise, then
//      extreme sample values — full scale, just past clip, huge, denormal, NaN, infinities;
//   2  every word of every such descriptor mutated (+1, -1, edge values): refused — but for the table offset, which only has
//      to keep the table inside the arena, and the one pair of formats that share every other word (mu-law / A-law); table
//      offsets at and past the arena's end; a mutated descriptor inside a live state is refused by host_step_out before it reads;
//      a resampling descriptor made for the other direction is refused by check();
//   3  random rates and formats, valid and not, go through describe() and host_new(): accepted or refused with a message; wholly
//      random descriptors go through check() with random arena lengths: a clean 0 or a clean DSM_ERR_INVALID;
//   4  the sample encoders over every 16-bit value against the expanders, and over odd floats.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_pcm_format.h"

static uint64_t rng_state = 0xE6E55ull;
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
      fprintf(stderr, "egress_fuzz: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

static const uint32_t kEdgeWords[] = {0u, 1u, 2u, 3u, 4u, 24u, 25u, 33u, 34u, 68u, 203u, 204u, 205u, 639u, 640u, 1920u, 3840u, 3841u, 4096u,
                                      4097u, 7999u, 8000u, 15360u, 15361u, 24000u, 48000u, 48001u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u,
                                      0xFFFFFFFFu};
static const size_t kEdges = sizeof kEdgeWords / sizeof *kEdgeWords;

static const float kExtremes[] = {1.0f, -1.0f, 0.99999994f, 1.0000001f, -1.0000001f, 1.5f / 32768.0f, 2.5f / 32768.0f, -0.5f / 32768.0f,
                                  3.0e38f, -3.0e38f, 1e-40f, -1e-40f, 0.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(),
                                  std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
static const size_t kNExtremes = sizeof kExtremes / sizeof *kExtremes;

// a frame of exactly 1920 floats on the heap
static std::unique_ptr<float[]> frame_of(bool extreme) {
  std::unique_ptr<float[]> p(new float[DSM_FRAME_SIZE]);
  for (int i = 0; i < DSM_FRAME_SIZE; ++i)
    p[i] = extreme && below(3) == 0 ? kExtremes[below((uint32_t)kNExtremes)] : ((float)(rnd() >> 40) / 16777216.0f) * 2.0f - 1.0f;
  return p;
}

static int stream(dsm_pcm::Host* h, int frames, bool extreme) {
  std::string err;
  for (int t = 0; t < frames; ++t) {
    auto f = frame_of(extreme);
    std::unique_ptr<uint8_t[]> row(new uint8_t[h->d.frame_bytes]);
    CHECK(dsm_pcm::host_step_out(h, f.get(), row.get(), &err) == 0);
    if (!extreme && h->d.fmt == DSM_PCM_F32)
      for (uint32_t n = 0; n < h->d.frame; ++n) {
        float v;
        memcpy(&v, row.get() + 4u * n, 4);
        CHECK(std::isfinite(v) && std::fabs(v) < 4.0f);
      }
  }
  return 0;
}

int main() {
  std::string err;
  const int rates[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000};
  // 1 and 2
  for (int rate : rates)
    for (int fmt = 0; fmt < 4; ++fmt) {
      dsm_pcm::Host h;
      CHECK(dsm_pcm::host_new(DSM_PCM_OUT, rate, fmt, &h, &err) == 0);
      CHECK(h.d.frame * 25u == 2u * (uint32_t)rate && h.d.taps <= DSM_PCM_MAX_TAPS_OUT && h.d.frame <= DSM_PCM_MAX_FRAME);
      CHECK(h.d.frame_bytes <= DSM_PCM_MAX_FRAME_BYTES && h.coef.size() == h.d.table_words && h.d.frame % 2u == 0u);
      if (stream(&h, 3, false)) return 1;
      if (stream(&h, 3, true)) return 1;
      std::unique_ptr<uint8_t[]> row(new uint8_t[h.d.frame_bytes]);
      auto f = frame_of(false);
      CHECK(dsm_pcm::host_step_out(&h, nullptr, row.get(), &err) == DSM_ERR_INVALID);
      CHECK(dsm_pcm::host_step_out(&h, f.get(), nullptr, &err) == DSM_ERR_INVALID);
      // the table against the arena: exactly enough, one word short, offsets at and past the end
      const dsm_pcm_desc good = h.d;
      CHECK(dsm_pcm::check(DSM_PCM_OUT, &good, good.table_words, &err) == 0);
      // the direction is no word of the descriptor: where the two differ (every rate that resamples) check() tells them apart
      CHECK(dsm_pcm::check(DSM_PCM_IN, &good, good.table_words, &err) == (rate == DSM_PCM_RATE ? 0 : DSM_ERR_INVALID));
      if (good.table_words) CHECK(dsm_pcm::check(DSM_PCM_OUT, &good, good.table_words - 1u, &err) == DSM_ERR_INVALID);
      for (uint32_t off : {1u, good.table_words, good.table_words + 1u, 0xFFFFFFFFu, 0xFFFFFFFFu - good.table_words + 1u}) {
        dsm_pcm_desc d = good;
        d.table_off = off;
        const size_t arena = (size_t)good.table_words + 1000u;
        const bool inside = (uint64_t)off + good.table_words <= (uint64_t)arena;
        err.clear();
        CHECK(dsm_pcm::check(DSM_PCM_OUT, &d, arena, &err) == (inside ? 0 : DSM_ERR_INVALID));
        CHECK(inside || !err.empty());
      }
      // every other word: any change is refused
      for (uint32_t at = 0; at < DSM_PCM_DESC_WORDS; ++at) {
        if (at == 9u) continue;  // table_off, above
        for (size_t m = 0; m < kEdges + 2; ++m) {
          uint32_t w[DSM_PCM_DESC_WORDS];
          memcpy(w, &good, sizeof w);
          const uint32_t was = w[at];
          w[at] = m < kEdges ? kEdgeWords[m] : m == kEdges ? was + 1u : was - 1u;
          if (w[at] == was) continue;
          // mu-law and A-law frames have every other word in common: that one change names another admitted format
          const bool other_g711 = at == 1u && was >= (uint32_t)DSM_PCM_MULAW && w[at] >= (uint32_t)DSM_PCM_MULAW && w[at] <= (uint32_t)DSM_PCM_ALAW;
          std::unique_ptr<dsm_pcm_desc> heap(new dsm_pcm_desc);
          memcpy(heap.get(), w, sizeof w);
          err.clear();
          const int rc = dsm_pcm::check(DSM_PCM_OUT, heap.get(), (size_t)good.table_words + 1000u, &err);
          CHECK(rc == (other_g711 ? 0 : DSM_ERR_INVALID));
          CHECK(rc == 0 || !err.empty());
          if (rc == 0) continue;
          // inside a live state: host_step checks before it reads or writes
          dsm_pcm::Host live = h;
          const std::vector<float> before = live.buf;
          live.d = *heap;
          CHECK(dsm_pcm::host_step_out(&live, f.get(), row.get(), &err) == DSM_ERR_INVALID);
          CHECK(live.buf.size() == before.size() && memcmp(live.buf.data(), before.data(), sizeof(float) * before.size()) == 0);  // NaNs inside
        }
      }
    }
  // 3
  int accepted = 0;
  for (int it = 0; it < 400; ++it) {
    long rate, fmt;
    switch (below(4)) {
      case 0: rate = 25 * (long)(300 + below(1700)); break;  // whole frames, around and inside the range
      case 1: rate = (long)below(60000); break;
      case 2: rate = (long)kEdgeWords[below((uint32_t)kEdges)]; break;
      default: rate = -(long)below(50000); break;
    }
    fmt = below(3) ? (long)below(4) : (long)(int32_t)kEdgeWords[below((uint32_t)kEdges)];
    dsm_pcm_desc d;
    err.clear();
    const int rc = dsm_pcm::describe(DSM_PCM_OUT, rate, fmt, &d, &err);
    dsm_pcm::Host h;
    std::string err2;
    const int rc2 = dsm_pcm::host_new(DSM_PCM_OUT, rate, fmt, &h, &err2);
    CHECK(rc == rc2);
    if (rc) { CHECK(rc == DSM_ERR_INVALID && !err.empty() && !err2.empty()); continue; }
    CHECK(rate >= 8000 && rate <= 48000 && rate % 25 == 0 && fmt >= 0 && fmt < 4);
    CHECK(dsm_pcm::check(DSM_PCM_OUT, &h.d, h.coef.size(), &err) == 0);
    if (accepted++ < 40 && stream(&h, 2, true)) return 1;  // an odd rate has up to 1919 phases: a few dozen are enough
  }
  CHECK(accepted > 50);
  for (int it = 0; it < 4000; ++it) {
    uint32_t w[DSM_PCM_DESC_WORDS];
    for (uint32_t& x : w) x = below(2) ? (uint32_t)rnd() : kEdgeWords[below((uint32_t)kEdges)];
    std::unique_ptr<dsm_pcm_desc> heap(new dsm_pcm_desc);
    memcpy(heap.get(), w, sizeof w);
    const size_t arena = below(2) ? (size_t)below(500000) : (size_t)heap->table_off + heap->table_words - below(2);
    err.clear();
    const int rc = dsm_pcm::check(DSM_PCM_OUT, heap.get(), arena, &err);
    CHECK(rc == 0 || (rc == DSM_ERR_INVALID && !err.empty()));
    if (rc == 0) {  // then every index of a step is inside the frame, the history, the arena and the row
      CHECK(heap->taps <= DSM_PCM_MAX_TAPS_OUT && heap->frame <= DSM_PCM_MAX_FRAME && heap->taps == 2u * heap->half);
      CHECK((uint64_t)heap->table_off + (uint64_t)heap->L * heap->taps <= arena && heap->reserved == 0u);
      CHECK(heap->frame_bytes == heap->frame * dsm_pcm_sample_bytes(heap->fmt));
    }
  }
  // 4
  for (int s = -32768; s <= 32767; ++s) {
    const float v = (float)s / 32768.0f;
    CHECK(dsm_pcm_f32_to_s16(v) == s);
    const uint32_t u = dsm_g711_s16_to_ulaw(s), a = dsm_g711_s16_to_alaw(s);
    CHECK(u < 256u && a < 256u);
    // compression then expansion lands in the segment's step around the value (mu-law clips at 32635)
    const int us = dsm_g711_ulaw_to_s16(u), as = dsm_g711_alaw_to_s16(a);
    CHECK(std::abs(us - (s > 32635 ? 32635 : s < -32635 ? -32635 : s)) <= 512 && std::abs(as - s) <= 512);
    CHECK((us < 0) == (s < 0 && us != 0) || us == 0);
    CHECK((as < 0) == (s < 0));
  }
  for (uint32_t b = 0; b < 256u; ++b) {
    CHECK(dsm_g711_s16_to_alaw(dsm_g711_alaw_to_s16(b)) == b);
    CHECK(dsm_g711_s16_to_ulaw(dsm_g711_ulaw_to_s16(b)) == (b == 0x7Fu ? 0xFFu : b));
  }
  for (size_t i = 0; i < kNExtremes; ++i)
    for (uint32_t fmt = 0; fmt < 4u; ++fmt) {
      std::unique_ptr<uint8_t[]> one(new uint8_t[dsm_pcm_sample_bytes(fmt)]);
      dsm_pcm_store(fmt, one.get(), 0, kExtremes[i]);
    }
  CHECK(dsm_pcm_f32_to_s16(kExtremes[14]) == 0 && dsm_pcm_f32_to_s16(1.0f) == 32767 && dsm_pcm_f32_to_s16(-1.0f) == -32768);
  CHECK(dsm_pcm_f32_to_s16(1.5f / 32768.0f) == 2 && dsm_pcm_f32_to_s16(2.5f / 32768.0f) == 2 && dsm_pcm_f32_to_s16(3.0e38f) == 32767);
  puts("egress_fuzz ok");
  return 0;
}
