// clip_fuzz.cpp — the host half of the clips section (csrc/dsm_asr_clip.h: the cut, the schedule, the records' reader and the
// message replay dsm_asr_collect goes through) under AddressSanitizer + UBSan, stand-alone.  Every buffer is a heap block of
// exactly the size the call is entitled to, so a read or write past it is a report.  Three parts, each seeded:
//   cut       random clips, frame sizes and frame indices (far beyond the clip and beyond 2^32 bytes included) against a
//             byte-by-byte restatement;
//   schedule  random begin / push / close / reset / run sequences with mutated lengths and caps: the table stays inside its
//             [n][B] arrays, a taken frame's bytes are all there (open) or it lies in front of n_audio + flush (closed), frames
//             come in order, DONE and WAITING slots are masked off;
//   records   record buffers and step counts that do not belong together are refused with nothing written; fitting ones are
//             read row by row, and message lists longer than the caller's arrays are counted and dropped.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_asr_clip.h"

namespace C = dsm_asr_clip;

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }  // (a zero-length block is still a block)

static void fuzz_cut(std::mt19937_64& rng) {
  const uint32_t fmts[4] = {DSM_PCM_F32, DSM_PCM_S16, DSM_PCM_MULAW, DSM_PCM_ALAW};
  for (int it = 0; it < 20000; ++it) {
    const uint32_t fmt = fmts[rng() % 4];
    const uint32_t fb = 1 + (uint32_t)(rng() % (it % 7 == 0 ? DSM_PCM_MAX_FRAME_BYTES : 97));
    const size_t n = (size_t)(rng() % (4 * (size_t)fb + 3));
    auto clip = exact<uint8_t>(n);
    for (size_t i = 0; i < n; ++i) clip[i] = (uint8_t)rng();
    uint64_t index = rng() % 7;
    if (it % 5 == 0) index = rng();              // anywhere
    if (it % 11 == 0) index = n / fb + rng() % 2;  // the frame the clip ends in, or the first silent one
    auto out = exact<uint8_t>(fb);
    memset(out.get(), 0x5A, fb);
    const uint8_t sil = C::silence_byte(fmt);
    const size_t have = C::cut(n ? clip.get() : nullptr, n, fb, sil, index, out.get());
    CHECK(have <= fb);
    for (uint32_t j = 0; j < fb; ++j) {
      const unsigned __int128 at = (unsigned __int128)index * fb + j;
      const uint8_t want = at < n ? clip[(size_t)at] : sil;
      if (out[j] != want) { CHECK(out[j] == want); break; }
      if (at < n) CHECK(j < have); else CHECK(j >= have);
    }
  }
  CHECK(C::silence_byte(DSM_PCM_MULAW) == 0xFF && dsm_g711_ulaw_to_s16(0xFF) == 0);
  CHECK(C::silence_byte(DSM_PCM_ALAW) == 0xD5 && dsm_g711_alaw_to_s16(0xD5) == 8);
  CHECK(C::silence_byte(DSM_PCM_F32) == 0 && C::silence_byte(DSM_PCM_S16) == 0);
}

static void fuzz_schedule(std::mt19937_64& rng) {
  for (int it = 0; it < 3000; ++it) {
    const int B = 1 + (int)(rng() % 9);
    const uint64_t cap = it % 13 == 0 ? ((uint64_t)1 << 31) : 1 + rng() % 5000;
    std::vector<C::Slot> slots((size_t)B);
    std::vector<uint64_t> next((size_t)B, 0);  // the frame each clip takes next
    for (int op = 0; op < 60; ++op) {
      const int b = (int)(rng() % (uint64_t)B);
      C::Slot& s = slots[(size_t)b];
      switch (rng() % 6) {
        case 0:
          if (s.status == DSM_ASR_CLIP_IDLE) {
            C::begin(&s, 1 + (uint32_t)(rng() % (it % 3 ? 50 : DSM_PCM_MAX_FRAME_BYTES)), it % 17 == 0 ? ((uint64_t)1 << 31) - 1 : rng() % 5);
            next[(size_t)b] = 0;
          }
          break;
        case 1: {
          const C::Slot before = s;
          const uint64_t n = it % 7 == 0 ? rng() : rng() % (cap + 2);  // mutated lengths: huge ones must be refused
          const bool ok = C::push(&s, n, cap);
          CHECK(ok == (before.status != DSM_ASR_CLIP_IDLE && !before.closed && n <= cap && before.bytes + n <= cap));
          if (!ok) CHECK(memcmp(&before, &s, sizeof s) == 0);
          CHECK(s.bytes <= cap);
          break;
        }
        case 2: C::close(&s); break;
        case 3:
          if (rng() % 4 == 0) s = C::Slot();
          break;
        default: {
          const int n = 1 + (int)(rng() % DSM_ASR_RUN_MAX);
          auto frame = exact<uint32_t>((size_t)n * B);
          auto mask = exact<uint8_t>((size_t)n * B);
          const std::vector<C::Slot> before = slots;
          C::plan(slots.data(), B, n, frame.get(), mask.get());
          for (int k = 0; k < n; ++k)
            for (int j = 0; j < B; ++j) {
              const C::Slot& was = before[(size_t)j];
              const uint8_t on = mask[(size_t)k * B + j];
              CHECK(on <= 1);
              if (!on) continue;
              const uint64_t f = frame[(size_t)k * B + j];
              CHECK(was.status == DSM_ASR_CLIP_RUNNING || was.status == DSM_ASR_CLIP_WAITING);
              CHECK(f == next[(size_t)j]);
              next[(size_t)j] += 1;
              if (was.closed) CHECK(f < C::n_audio(was) + was.flush);
              else CHECK((f + 1) * was.frame_bytes <= was.bytes);
            }
          for (int j = 0; j < B; ++j) {
            const C::Slot& now = slots[(size_t)j];
            CHECK(now.cursor == next[(size_t)j] || now.status == DSM_ASR_CLIP_IDLE);
            if (now.status == DSM_ASR_CLIP_DONE) CHECK(now.closed && now.cursor >= C::n_audio(now) + now.flush);
            if (now.status == DSM_ASR_CLIP_WAITING) CHECK(!now.closed && (now.cursor + 1) * now.frame_bytes > now.bytes);
          }
          break;
        }
      }
      if (slots[(size_t)b].status == DSM_ASR_CLIP_IDLE) next[(size_t)b] = 0;
    }
  }
}

static void fuzz_records(std::mt19937_64& rng) {
  for (int it = 0; it < 6000; ++it) {
    const int B = 1 + (int)(rng() % 40), heads = (int)(rng() % (DSM_MAX_EXTRA_HEADS + 1)), n = 1 + (int)(rng() % DSM_ASR_RUN_MAX);
    const size_t row = C::record_words(B, heads), words = (size_t)n * row;
    CHECK(row == (size_t)B * (2 + (size_t)heads));
    auto rec = exact<uint32_t>(words);
    for (size_t i = 0; i < words; ++i) rec[i] = (uint32_t)rng();
    auto mask = exact<uint8_t>((size_t)n * B);
    for (size_t i = 0; i < (size_t)n * B; ++i) mask[i] = (uint8_t)(rng() & 1);
    auto stepped = exact<uint8_t>((size_t)n * B);
    auto text = exact<uint32_t>((size_t)n * B);
    auto lp = exact<float>((size_t)n * B);
    auto prs = exact<float>((size_t)n * heads * B);
    // mutated tables: a step count, batch or head count the buffer was not made for
    int n2 = n, B2 = B, h2 = heads;
    size_t words2 = words;
    switch (rng() % 6) {
      case 0: n2 = (int)(rng() % 40) - 4; break;
      case 1: words2 = (size_t)(rng() % (words + 1)); break;
      case 2: B2 = (int)(rng() % 64) - 3; break;
      case 3: h2 = (int)(rng() % 12) - 2; break;
      default: break;
    }
    const bool fits = n2 >= 1 && n2 <= DSM_ASR_RUN_MAX && B2 >= 1 && h2 >= 0 && h2 <= DSM_MAX_EXTRA_HEADS &&
                      (size_t)n2 * C::record_words(B2, h2) <= words2;
    if (!fits || n2 != n || B2 != B || h2 != heads) {
      // only the refusal is driven with arrays of the original size: an accepted other shape would write by ITS size
      if (!fits) {
        memset(text.get(), 0xEE, sizeof(uint32_t) * (size_t)n * B);
        CHECK(!C::unpack(rec.get(), words2, mask.get(), n2, B2, h2, stepped.get(), text.get(), prs.get(), lp.get()));
        CHECK(text[0] == 0xEEEEEEEEu);
        const uint32_t *a, *b, *c;
        CHECK(!C::record_row(rec.get(), words2, n2, B2, h2, 0, &a, &b, &c));
      }
      continue;
    }
    CHECK(C::unpack(rec.get(), words, mask.get(), n, B, heads, stepped.get(), text.get(), heads ? prs.get() : nullptr, lp.get()));
    CHECK(C::unpack(rec.get(), words, mask.get(), n, B, heads, nullptr, nullptr, nullptr, nullptr));
    const uint32_t *a, *b, *c;
    CHECK(!C::record_row(rec.get(), words, n, B, heads, n, &a, &b, &c) && !C::record_row(rec.get(), words, n, B, heads, -1, &a, &b, &c));
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < B; ++j) {
        const size_t at = (size_t)k * B + j;
        CHECK(stepped[at] == mask[at] && text[at] == rec[(size_t)k * row + j]);
        uint32_t w;
        memcpy(&w, &lp[at], 4);
        CHECK(w == rec[(size_t)k * row + B + j]);
        for (int h = 0; h < heads; ++h) {
          memcpy(&w, &prs[((size_t)k * heads + h) * B + j], 4);
          CHECK(w == rec[(size_t)k * row + (2 + (size_t)h) * B + j]);
        }
      }
    // the replay's message lists: caps smaller than what the steps produce
    const int msgs_cap = (int)(rng() % 12), tokens_cap = (int)(rng() % 20);
    auto msgs = exact<dsm_asr_msg>((size_t)msgs_cap);
    auto msg_step = exact<int>((size_t)msgs_cap);
    auto toks = exact<uint32_t>((size_t)tokens_cap);
    auto tlps = exact<float>((size_t)tokens_cap);
    dsm_asr_block out;
    memset(&out, 0, sizeof out);
    out.msgs = msgs.get(); out.msg_step = msg_step.get(); out.msgs_cap = msgs_cap;
    out.msg_tokens = toks.get(); out.msg_logprobs = tlps.get(); out.tokens_cap = tokens_cap;
    int want_msgs = 0, want_toks = 0;
    std::vector<uint32_t> all_toks;
    for (int k = 0; k < n; ++k) {
      const size_t nm = (size_t)(rng() % 5);
      std::vector<dsm_asr_msg> step_msgs(nm);
      std::vector<uint32_t> step_toks;
      std::vector<float> step_lps;
      for (size_t i = 0; i < nm; ++i) {
        dsm_asr_msg& m = step_msgs[i];
        memset(&m, 0, sizeof m);
        m.kind = (int)(rng() % 3);
        m.batch_idx = (int)(rng() % (uint64_t)B);
        if (m.kind == DSM_MSG_WORD) {
          m.tokens_offset = (int)step_toks.size();
          m.n_tokens = (int)(rng() % 4);
          for (int t = 0; t < m.n_tokens; ++t) { step_toks.push_back((uint32_t)rng()); step_lps.push_back(-1.0f * (float)t); }
        }
      }
      C::append_step(&out, k, step_msgs.data(), nm, step_toks.data(), step_lps.data(), step_toks.size());
      for (size_t i = 0; i < nm; ++i) {
        if (want_msgs < msgs_cap) {
          CHECK(msg_step[want_msgs] == k && msgs[want_msgs].kind == step_msgs[i].kind);
          if (step_msgs[i].kind == DSM_MSG_WORD) CHECK(msgs[want_msgs].tokens_offset == step_msgs[i].tokens_offset + want_toks);
        }
        want_msgs += 1;
      }
      all_toks.insert(all_toks.end(), step_toks.begin(), step_toks.end());
      want_toks += (int)step_toks.size();
    }
    CHECK(out.n_msgs == want_msgs && out.n_tokens == want_toks);
    for (int t = 0; t < want_toks && t < tokens_cap; ++t) CHECK(toks[t] == all_toks[(size_t)t]);
  }
}

int main() {
  std::mt19937_64 rng(20261021);
  fuzz_cut(rng);
  fuzz_schedule(rng);
  fuzz_records(rng);
  if (fails) { printf("clip_fuzz: %d checks failed\n", fails); return 1; }
  printf("clip_fuzz ok\n");
  return 0;
}
