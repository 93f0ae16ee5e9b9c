// tts_xfer_fuzz.cpp — the host-side validation an import of a TTS slot blob has to make (csrc/dsm_tts_slot_layout.h: check_slot and the layout it
// reads through) under AddressSanitizer + UBSan, stand-alone: for a handful of configurations it builds a valid slot (payload in
// a heap block of exactly slot_bytes, so a read past a section's end is a report), checks that it is accepted, then feeds
// seeded mutations of the payload and of the host item — through the blob writer and the checked reader — to the validation.
// Every outcome must be a clean accept or a refusal with a message, and whatever is ACCEPTED must satisfy every bound a later step,
// upload or table read relies on, restated here independently of the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>

#include "../../delayed-streams-modeling_amd/csrc/dsm_tts_slot_layout.h"

namespace L = dsm_tts_layout;
using Item = dsm_tts_slot_blob::HostItem;

static int fails = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static dsm_tts_config tts_cfg(int kv_bf16, int cross, int cfg_rows) {
  dsm_tts_config c;
  memset(&c, 0, sizeof c);
  c.lm.d_model = 16; c.lm.num_heads = 2; c.lm.num_layers = 2; c.lm.context = 8;
  c.text_in_vocab_size = 41; c.text_out_vocab_size = 40; c.audio_vocab_size = 33; c.audio_codebooks = 6;
  c.depformer.d_model = 8; c.depformer.num_heads = 1; c.depformer.num_layers = 1; c.depformer.context = 6;
  c.dep_num_slices = 6; c.dep_weight_groups = 3;
  c.acoustic_delay = 2; c.text_pad_token = 3; c.text_eop_token = 0; c.text_audio_delay_in_tokens = 3;
  c.max_consecutive_pads = 4; c.max_steps = 16;
  c.kv_bf16 = kv_bf16; c.cross_attention = cross; c.ca_max_len = cross ? 5 : 0; c.cfg_rows = cfg_rows;
  return c;
}

static dsm_mimi_config mimi_cfg() {
  dsm_mimi_config m;
  memset(&m, 0, sizeof m);
  m.channels = 1; m.dimension = 8; m.n_filters = 4; m.n_residual_layers = 1; m.n_ratios = 2;
  m.ratios[0] = 8; m.ratios[1] = 6;
  m.kernel_size = 7; m.residual_kernel_size = 3; m.last_kernel_size = 3; m.dilation_base = 2; m.compress = 2;
  m.transformer.d_model = 8; m.transformer.num_heads = 2; m.transformer.num_layers = 1; m.transformer.context = 5;
  m.quantizer_n_q = 6; m.quantizer_bins = 32; m.quantizer_dim = 4; m.downsample_stride = 2;
  return m;
}

struct View {  // a payload through the layout's offsets, by section name
  const L::Layout& lay;
  const uint8_t* p;
  std::map<std::string, const L::Sec*> by;
  View(const L::Layout& l, const uint8_t* q) : lay(l), p(q) {
    for (const L::Sec& s : l.secs) by[s.name] = &s;
  }
  bool has(const char* n) const { return by.count(n) != 0; }
  uint32_t w(const char* n, int i = 0) const { return dsm_blob::rd32(p + by.at(n)->off + 4 * i); }
  uint32_t b(const char* n) const { return p[by.at(n)->off]; }
};

static void put32(uint8_t* p, const L::Layout& lay, const char* name, int i, uint32_t v) {
  for (const L::Sec& s : lay.secs)
    if (s.name == name) memcpy(p + s.off + 4 * i, &v, 4);
}

// a slot in the middle of a request: 5 steps done, guided and sampling where the configuration allows
static Item valid_item(const dsm_tts_config& c) {
  Item it;
  it.step_idx = 5; it.consecutive_pads = 1; it.samp_k = 4;
  it.cfg_on = c.cfg_rows ? 1 : 0; it.cond_on = 1;
  it.ca_len[0] = c.cross_attention ? 3 : 0; it.ca_len[1] = c.cfg_rows ? 2 : 0;
  it.req_flags = dsm_tts_slot_blob::kReqActive | dsm_tts_slot_blob::kReqBosDone; it.req_status = 1;
  for (int i = 0; i < 5; ++i) it.text_tokens.push_back((uint32_t)(3 + i));
  for (int i = 0; i < 5 * c.dep_num_slices; ++i) it.audio_tokens.push_back(i % 7 == 6 ? DSM_TTS_UNGENERATED : (uint32_t)(i % c.audio_vocab_size));
  it.q_tok = {1, 9, 11, 4, 5};
  it.q_end = {3, 5};
  return it;
}

static void valid_payload(const dsm_tts_config& c, const L::Layout& lay, bool dec, const Item& it, uint8_t* p) {
  memset(p, 0, (size_t)lay.slot_bytes(dec));
  for (int j = 0; j < lay.rps; ++j) {
    put32(p, lay, "lm.pos", j, 5); put32(p, lay, "lm.idx", j, 5);
    if (c.cross_attention) put32(p, lay, "ca.last", j, it.ca_len[j] ? it.ca_len[j] - 1 : 0);
  }
  p[lay.secs[(size_t)lay.cfg_on].off] = (uint8_t)it.cfg_on;
  p[lay.secs[(size_t)lay.cond_on].off] = (uint8_t)it.cond_on;
  put32(p, lay, "samp.k", 0, (uint32_t)it.samp_k);
  put32(p, lay, "text_token", 0, 3); put32(p, lay, "last", 0, 7);
  for (int k = 0; k < c.dep_num_slices; ++k) { put32(p, lay, "lat", k, (uint32_t)k); put32(p, lay, "row0", k, 32); }
  for (int k = 0; k <= c.acoustic_delay; ++k) put32(p, lay, "ring", k, 32);
  const int32_t req[13] = {1, 5, 1, 1, 1, 0, 2, 9, 1, 16, 2, 2, 0};
  for (int i = 0; i < 13; ++i) put32(p, lay, "req", i, (uint32_t)req[i]);
  if (dec) { p[lay.secs[(size_t)lay.dec_started].off] = 1; put32(p, lay, "dec.pos", 0, 7); put32(p, lay, "dec.idx", 0, 2); }
}

// what an accepted slot must satisfy, independently of check_slot
static void holds(const dsm_tts_config& c, const dsm_mimi_config& m, const L::Layout& lay, const uint8_t* p, bool dec, const Item& it) {
  View v(lay, p);
  const uint32_t V = (uint32_t)c.audio_vocab_size, UNG = DSM_TTS_UNGENERATED;
  const uint32_t tv = (uint32_t)(c.text_in_vocab_size > c.text_out_vocab_size ? c.text_in_vocab_size : c.text_out_vocab_size);
  const uint32_t qcap = (uint32_t)(c.max_steps + c.acoustic_delay);
  CHECK(it.step_idx <= qcap && it.text_tokens.size() == it.step_idx && it.audio_tokens.size() == it.step_idx * (uint64_t)c.dep_num_slices);
  for (uint32_t t : it.audio_tokens) CHECK(t == UNG || t < V);
  for (uint32_t t : it.text_tokens) CHECK(t == UNG || t < tv);
  CHECK(it.samp_k >= 0 && it.cfg_on <= 1 && it.cond_on <= 1);
  CHECK(it.q_tok.size() <= qcap && it.q_end.size() <= qcap);
  int32_t prev = 0;
  for (int32_t e : it.q_end) { CHECK(e >= prev && (size_t)e <= it.q_tok.size()); prev = e; }
  for (int j = 0; j < lay.rps; ++j) {
    CHECK(v.w("lm.idx", j) < (uint32_t)c.lm.context);
    CHECK(it.ca_len[j] <= (uint32_t)c.ca_max_len);
    if (c.cross_attention) CHECK(v.w("ca.last", j) < (uint32_t)c.ca_max_len && v.w("ca.last", j) == (it.ca_len[j] ? it.ca_len[j] - 1 : 0));
  }
  CHECK(v.b("cfg.on") == it.cfg_on && v.b("cond.on") == it.cond_on && v.w("samp.k") == (uint32_t)it.samp_k);
  CHECK(!it.cfg_on || lay.rps == 2);
  for (int k = 0; k < c.dep_num_slices; ++k) CHECK(v.w("lat", k) < V && v.w("row0", k) < V);
  for (int k = 0; k <= c.acoustic_delay; ++k) CHECK(v.w("ring", k) < V);
  const int32_t cur = (int32_t)v.w("req", L::RQ_CUR_WORD), tok = (int32_t)v.w("req", L::RQ_TOKEN_IDX), nw = (int32_t)v.w("req", L::RQ_N_WORDS);
  const int32_t step = (int32_t)v.w("req", L::RQ_STEP), st = (int32_t)v.w("req", L::RQ_STATUS);
  CHECK(st >= 0 && st <= 4 && step >= 0 && (uint32_t)step <= qcap);
  if (it.req_flags & dsm_tts_slot_blob::kReqActive) {
    CHECK((size_t)nw == it.q_end.size() && cur >= -1 && cur < nw && tok >= 0 && (size_t)tok <= it.q_tok.size());
    CHECK(v.w("req", L::RQ_HAS_WORD) <= 1 && v.w("req", L::RQ_CLOSED) <= 1 && (uint64_t)step == it.step_idx);
  } else {  // no request: an idle record and an empty queue, nothing a scheduler step would index with
    CHECK(st == 0 && cur == 0 && tok == 0 && nw == 0 && it.q_end.empty() && it.q_tok.empty());
  }
  if (dec) CHECK(v.b("dec.started") <= 1 && v.w("dec.idx") < (uint32_t)m.transformer.context);
}

int main() {
  std::mt19937_64 rng(20250107);
  const dsm_mimi_config m = mimi_cfg();
  long accepted = 0, refused = 0;
  for (int variant = 0; variant < 8; ++variant) {
    const int cross = variant & 1, rows = cross && (variant & 2), dec = (variant & 4) != 0;
    const dsm_tts_config c = tts_cfg(variant & 1, cross, rows);
    L::Layout lay;
    std::string err;
    CHECK(L::build(c, dec ? &m : nullptr, &lay, &err));
    const size_t sb = (size_t)lay.slot_bytes(dec);
    CHECK(sb % 16 == 0 && sb > 0);
    for (const L::Sec& s : lay.secs) CHECK(s.off % 16 == 0 && s.off + s.bytes <= (long)sb && s.bytes > 0);
    const Item good = valid_item(c);
    std::unique_ptr<uint8_t[]> base(new uint8_t[sb]);
    valid_payload(c, lay, dec, good, base.get());
    const std::string why = L::check_slot(lay, c, dec ? &m : nullptr, base.get(), dec, good);
    if (!why.empty()) printf("variant %d: the valid slot is refused: %s\n", variant, why.c_str());
    CHECK(why.empty());
    holds(c, m, lay, base.get(), dec, good);
    // a payload with the decode group needs a Mimi configuration
    if (dec) CHECK(!L::check_slot(lay, c, nullptr, base.get(), true, good).empty());
    for (int round = 0; round < 7500; ++round) {
      std::unique_ptr<uint8_t[]> p(new uint8_t[sb]);  // exactly slot_bytes: a read past it is a report
      memcpy(p.get(), base.get(), sb);
      Item it = good;
      const int n_mut = 1 + (int)(rng() % 3);
      for (int k = 0; k < n_mut; ++k) {
        switch (rng() % 6) {
          case 0: {  // a word of a small section: an index, a token, a cursor
            const L::Sec& s = lay.secs[rng() % lay.secs.size()];
            if (s.bytes >= 4 && s.bytes <= 64) {
              const uint32_t choices[] = {0u, 1u, 4u, 5u, 7u, 8u, 32u, 33u, 40u, 41u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, (uint32_t)rng()};
              const uint32_t val = choices[rng() % 14];
              memcpy(p.get() + s.off + 4 * (rng() % (uint64_t)(s.bytes / 4)), &val, 4);
            } else if (s.bytes < 4) {
              p[(size_t)s.off] = (uint8_t)rng();
            }
            break;
          }
          case 1: p[rng() % sb] = (uint8_t)rng(); break;
          case 2: it.step_idx = rng() % 24; break;  // the tables no longer match: through the blob this is a parse error
          case 3: it.samp_k = (int32_t)rng(); it.cfg_on = (uint32_t)(rng() % 3); it.cond_on = (uint32_t)(rng() % 3); break;
          case 4: it.ca_len[rng() % 2] = (uint32_t)(rng() % 8); it.req_flags = (uint32_t)(rng() % 8); it.req_status = (int32_t)(rng() % 7) - 1; break;
          case 5:
            if (rng() % 2 && !it.q_end.empty()) it.q_end[rng() % it.q_end.size()] = (int32_t)(rng() % 9) - 2;
            else if (rng() % 2) it.q_tok.push_back((uint32_t)rng());
            else if (!it.audio_tokens.empty()) it.audio_tokens[rng() % it.audio_tokens.size()] = (uint32_t)(rng() % 40);
            break;
        }
      }
      // through the container: what the writer encodes, the checked reader hands to the validation
      std::vector<uint8_t> blob;
      dsm_tts_slot_blob::write_front(blob, dec ? DSM_TTS_SLOT_BLOB_HAS_MIMI_DEC : 0u, (uint32_t)c.dep_num_slices, L::signature(lay, dec), {it}, sb);
      blob.insert(blob.end(), p.get(), p.get() + sb);
      dsm_tts_slot_blob::Header h;
      std::vector<Item> items;
      if (dsm_tts_slot_blob::read_header(blob.data(), blob.size(), &h, &err) || dsm_tts_slot_blob::read_host(blob.data(), h, &items, &err)) {
        ++refused;
        continue;
      }
      CHECK(items.size() == 1 && h.slot_bytes == sb);
      std::unique_ptr<uint8_t[]> q(new uint8_t[sb]);
      memcpy(q.get(), blob.data() + h.payload_offset(), sb);
      const std::string bad = L::check_slot(lay, c, dec ? &m : nullptr, q.get(), dec, items[0]);
      if (bad.empty()) {
        ++accepted;
        holds(c, m, lay, q.get(), dec, items[0]);
      } else {
        ++refused;
      }
    }
  }
  CHECK(accepted > 1000 && refused > 1000);  // the mutations reach both sides
  if (fails) {
    printf("tts_xfer_fuzz: %d checks failed\n", fails);
    return 1;
  }
  printf("tts_xfer_fuzz ok: %ld accepted, %ld refused\n", accepted, refused);
  return 0;
}
