// dsm_tts_slot_layout.h — what a TTS slot's device payload is, as a function of the configuration alone: the section list of
// DESIGN.md section 7.2 (names, bytes per slot, where the engine keeps them relative to a slot), the signature, and the checks
// of every index-valued field of a payload and a host item.  Host only, header only, no device: dsm_tts_slot_layout prints it
// and tests/sanitize_tts_xfer/ runs the checks under ASan + UBSan against mutated payloads.  It is what the engine calls (not in
// the library) are to be built on: a SlotXfer table is this list plus the engine's base addresses
// (`Buf` names the buffer, `stride` the distance between slots), and an import is check_slot before the first write.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dsm.h"
#include "dsm_tts_slot_blob.h"

namespace dsm_tts_layout {

// Where the engine keeps a section.  The layout names the buffer; the engine resolves it to an address.
enum Buf {
  LM_POS, LM_IDX, LM_K, LM_V, CA_LAST, CA_K, CA_V, CFG_ON, CFG_FA, CFG_FB, SAMP_K, SAMP_INVT, RNG_KEY, RNG_POS_TEXT,
  RNG_POS_AUDIO, TEXT_TOKEN, LAST, LAT, RING, ROW0, COND, COND_ON, REQ,
  DEC_STARTED, DEC_POS, DEC_IDX, DEC_K, DEC_V, DEC_UP_CARRY, DEC_CARRY, DEC_CONV
};

struct Sec {
  std::string name;
  long bytes = 0;    // per slot
  long stride = 0;   // between consecutive slots in the engine's buffer
  long off = 0;      // inside a slot's payload, a multiple of 16
  Buf buf = LM_POS;
  int a = 0, b = 0;  // layer (rings, source blocks), batch row of the slot (source blocks), stage / descriptor index (decoder)
};

// The device-side request record as the payload holds it (TtsReqState of dsm_kernels.h: 13 words).
constexpr long kReqBytes = 52;
enum ReqWord { RQ_STATUS, RQ_STEP, RQ_CUR_WORD, RQ_HAS_WORD, RQ_TOKEN_IDX, RQ_STEP_PAST_LAST, RQ_LAST_EPAD, RQ_LAST_TEXT, RQ_CPADS,
               RQ_MAX_SEQ_LEN, RQ_EXTRA_STEPS, RQ_N_WORDS, RQ_CLOSED };

struct Layout {
  std::vector<Sec> secs;  // base group, then the Mimi decode group (there when a Mimi configuration was given)
  int nsec_base = 0;
  long bytes_base = 0, bytes_dec = 0;
  std::vector<uint32_t> sig;
  size_t sig_base = 0;  // signature words in front of the Mimi configuration's
  int rps = 1, n_steps = 0;
  // sections the checks read
  int lm_idx = -1, ca_last = -1, cfg_on = -1, samp_k = -1, text_token = -1, last = -1, lat = -1, ring = -1, row0 = -1, cond_on = -1,
      req = -1, dec_started = -1, dec_idx = -1;
  long slot_bytes(bool with_dec) const { return bytes_base + (with_dec ? bytes_dec : 0); }
  int nsec(bool with_dec) const { return with_dec ? (int)secs.size() : nsec_base; }
};

inline const char* sig_name(size_t i) {
  static const char* const names[] = {
      "lm.num_layers", "lm.num_heads", "lm head dim", "lm.context", "kv_bf16", "text_in_vocab_size", "text_out_vocab_size",
      "audio_vocab_size", "audio_codebooks", "dep_num_slices", "acoustic_delay", "text_audio_delay_in_tokens", "max_steps",
      "cross_attention", "ca_dim", "ca_max_len", "cfg_rows", "request queue capacity", "text_pad_token", "text_eop_token",
      "max_consecutive_pads",
      // with decode state
      "mimi.dimension", "mimi.n_filters", "mimi.n_ratios", "mimi.kernel_size", "mimi.residual_kernel_size", "mimi.last_kernel_size",
      "mimi.compress", "mimi.downsample_stride", "mimi.transformer.num_layers", "mimi.transformer.num_heads",
      "mimi transformer head dim", "mimi.transformer.context", "mimi.quantizer_n_q"};
  return i < sizeof names / sizeof names[0] ? names[i] : "mimi.ratios";
}

// The Mimi decoder's per-slot geometry from the configuration, as load_mimi / alloc_dec_state derive it.
struct DecGeom {
  struct Conv { int S, C; long bstride; };  // carried frames, channels, floats between slots of the concat buffer
  std::vector<Conv> convs;                  // the streaming convolutions that carry state, in descriptor order
  std::vector<long> carry;                  // floats per slot of every conv-transpose's overlap carry
  bool ok = false;
};
inline DecGeom dec_geom(const dsm_mimi_config& m) {
  DecGeom g;
  if (m.n_ratios < 1 || m.n_ratios > DSM_MAX_RATIOS || m.compress < 1 || m.n_filters < 1 || m.dimension < 1) return g;
  int T = DSM_FRAME_SIZE;
  for (int i = 0; i < m.n_ratios; ++i) {
    if (m.ratios[i] < 1 || T % m.ratios[i]) return g;
    T /= m.ratios[i];
  }
  auto conv = [&](int in_c, int k, int t_in) {
    const int S = k - 1;  // stride 1, dilation 1
    if (S > 0) g.convs.push_back({S, in_c, (long)(S + t_in) * in_c});
  };
  int mult = 1 << m.n_ratios;
  conv(m.dimension, m.kernel_size, T);
  for (int i = 0; i < m.n_ratios; ++i) {
    const int ratio = m.ratios[i], in_c = mult * m.n_filters, out_c = in_c / 2;
    g.carry.push_back((long)(2 * ratio - ratio) * out_c);
    T *= ratio;
    conv(out_c, m.residual_kernel_size, T);
    conv(out_c / m.compress, 1, T);
    mult /= 2;
  }
  conv(m.n_filters, m.last_kernel_size, T);
  g.ok = T == DSM_FRAME_SIZE;
  return g;
}

// The layout of configuration c, with the decode group of Mimi configuration m (nullptr: none).  False with *err for a
// configuration no engine can be created with.
inline bool build(const dsm_tts_config& c, const dsm_mimi_config* m, Layout* out, std::string* err) {
  Layout& L = *out;
  L = Layout{};
  auto fail = [&](const char* what) { if (err) *err = what; return false; };
  if (c.lm.num_layers < 1 || c.lm.num_heads < 1 || c.lm.d_model < 1 || c.lm.d_model % c.lm.num_heads || c.lm.context < 1)
    return fail("main LM dimensions out of range");
  if (c.dep_num_slices < 1 || c.dep_num_slices > (int)dsm_tts_slot_blob::kMaxSlices || c.acoustic_delay < 0 || c.max_steps < 1 ||
      c.text_audio_delay_in_tokens < 0)
    return fail("slices, delays or max_steps out of range");
  if (c.cross_attention && c.ca_max_len < 1) return fail("cross_attention needs ca_max_len > 0");
  if (c.cfg_rows && !c.cross_attention) return fail("cfg_rows needs cross_attention");
  const int rps = c.cfg_rows ? 2 : 1, S = c.dep_num_slices;
  const long kv = c.kv_bf16 ? 2 : 4;
  L.rps = rps;
  L.n_steps = c.max_steps + c.acoustic_delay;
  auto add = [&](const std::string& name, long bytes, long stride, Buf buf, int a = 0, int b = 0) {
    Sec s;
    s.name = name; s.bytes = bytes; s.stride = stride; s.buf = buf; s.a = a; s.b = b;
    L.secs.push_back(s);
    return (int)L.secs.size() - 1;
  };
  auto same = [&](const std::string& name, long bytes, Buf buf, int a = 0, int b = 0) { return add(name, bytes, bytes, buf, a, b); };
  auto num = [](const char* fmt, ...) {
    char buf[64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return std::string(buf);
  };
  same("lm.pos", 4L * rps, LM_POS);
  L.lm_idx = same("lm.idx", 4L * rps, LM_IDX);
  const long ring = (long)rps * c.lm.d_model * c.lm.context * kv;
  for (int l = 0; l < c.lm.num_layers; ++l) {
    same(num("lm.k.%d", l), ring, LM_K, l);
    same(num("lm.v.%d", l), ring, LM_V, l);
  }
  if (c.cross_attention) {
    L.ca_last = same("ca.last", 4L * rps, CA_LAST);
    const long blk = (long)c.lm.d_model * c.ca_max_len * kv;
    for (int l = 0; l < c.lm.num_layers; ++l)
      for (int j = 0; j < rps; ++j) {
        add(num("ca.k.%d.%d", l, j), blk, blk * rps, CA_K, l, j);
        add(num("ca.v.%d.%d", l, j), blk, blk * rps, CA_V, l, j);
      }
  }
  L.cfg_on = same("cfg.on", 1, CFG_ON);
  same("cfg.fa", 4, CFG_FA);
  same("cfg.fb", 4, CFG_FB);
  L.samp_k = same("samp.k", 4, SAMP_K);
  same("samp.invt", 4, SAMP_INVT);
  same("rng.key", 32, RNG_KEY);
  same("rng.pos_text", 4, RNG_POS_TEXT);
  same("rng.pos_audio", 4, RNG_POS_AUDIO);
  L.text_token = same("text_token", 4, TEXT_TOKEN);
  L.last = same("last", 4, LAST);
  L.lat = same("lat", 4L * S, LAT);
  L.ring = same("ring", 4L * (c.acoustic_delay + 1), RING);
  L.row0 = same("row0", 4L * S, ROW0);
  same("cond.row", 4L * c.lm.d_model, COND);
  L.cond_on = same("cond.on", 1, COND_ON);
  L.req = same("req", kReqBytes, REQ);
  L.nsec_base = (int)L.secs.size();
  L.sig = {(uint32_t)c.lm.num_layers, (uint32_t)c.lm.num_heads, (uint32_t)(c.lm.d_model / c.lm.num_heads), (uint32_t)c.lm.context,
           (uint32_t)(c.kv_bf16 ? 1 : 0), (uint32_t)c.text_in_vocab_size, (uint32_t)c.text_out_vocab_size, (uint32_t)c.audio_vocab_size,
           (uint32_t)c.audio_codebooks, (uint32_t)S, (uint32_t)c.acoustic_delay, (uint32_t)c.text_audio_delay_in_tokens,
           (uint32_t)c.max_steps, (uint32_t)(c.cross_attention ? 1 : 0), (uint32_t)(c.cross_attention ? c.ca_dim : 0),
           (uint32_t)(c.cross_attention ? c.ca_max_len : 0), (uint32_t)(c.cfg_rows ? 1 : 0), (uint32_t)L.n_steps,
           (uint32_t)c.text_pad_token, (uint32_t)c.text_eop_token, (uint32_t)c.max_consecutive_pads};
  L.sig_base = L.sig.size();
  if (m) {
    const dsm_transformer_config& t = m->transformer;
    if (t.num_layers < 1 || t.num_heads < 1 || t.d_model < 1 || t.d_model % t.num_heads || t.context < 1 || m->downsample_stride < 1)
      return fail("Mimi transformer dimensions out of range");
    const DecGeom g = dec_geom(*m);
    if (!g.ok) return fail("the Mimi configuration's ratios do not give one frame of samples per step");
    L.dec_started = same("dec.started", 1, DEC_STARTED);
    same("dec.pos", 4, DEC_POS);
    L.dec_idx = same("dec.idx", 4, DEC_IDX);
    const long dring = (long)t.d_model * t.context * 4;
    for (int l = 0; l < t.num_layers; ++l) {
      same(num("dec.k.%d", l), dring, DEC_K, l);
      same(num("dec.v.%d", l), dring, DEC_V, l);
    }
    same("dec.up_carry", 4L * m->downsample_stride * m->dimension, DEC_UP_CARRY);
    for (size_t i = 0; i < g.carry.size(); ++i) same(num("dec.carry.%d", (int)i), 4 * g.carry[i], DEC_CARRY, (int)i);
    for (size_t i = 0; i < g.convs.size(); ++i)
      add(num("dec.conv.%d", (int)i), 4L * g.convs[i].S * g.convs[i].C, 4 * g.convs[i].bstride, DEC_CONV, (int)i);
    for (uint32_t w : {(uint32_t)m->dimension, (uint32_t)m->n_filters, (uint32_t)m->n_ratios, (uint32_t)m->kernel_size,
                       (uint32_t)m->residual_kernel_size, (uint32_t)m->last_kernel_size, (uint32_t)m->compress,
                       (uint32_t)m->downsample_stride, (uint32_t)t.num_layers, (uint32_t)t.num_heads,
                       (uint32_t)(t.d_model / t.num_heads), (uint32_t)t.context, (uint32_t)m->quantizer_n_q})
      L.sig.push_back(w);
    for (int i = 0; i < m->n_ratios; ++i) L.sig.push_back((uint32_t)m->ratios[i]);
  }
  long off = 0;
  for (int i = 0; i < (int)L.secs.size(); ++i) {
    if (i == L.nsec_base) L.bytes_base = off;
    L.secs[(size_t)i].off = off;
    off += (long)dsm_blob::align16((uint64_t)L.secs[(size_t)i].bytes);
  }
  if (!m) L.bytes_base = off;
  L.bytes_dec = off - L.bytes_base;
  return true;
}

// The signature a blob with / without the decode group carries.
inline std::vector<uint32_t> signature(const Layout& L, bool with_dec) {
  return with_dec ? L.sig : std::vector<uint32_t>(L.sig.begin(), L.sig.begin() + (long)L.sig_base);
}

inline std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// Every index-valued field of one slot — its payload (slot_bytes(with_dec) readable bytes at p) and its host item — against the
// configuration: a value that passes cannot make a later step, upload or table read leave its allocation.  The mirrors must agree
// with the device values they mirror (a wrong samp_k mirror replays the wrong captured variant).  Empty string: accepted.
inline std::string check_slot(const Layout& L, const dsm_tts_config& c, const dsm_mimi_config* m, const uint8_t* p, bool with_dec,
                              const dsm_tts_slot_blob::HostItem& it) {
  using dsm_blob::rd32;
  const int rps = L.rps, S = c.dep_num_slices;
  const uint32_t UNG = DSM_TTS_UNGENERATED;
  auto w = [&](int sec, int i) { return rd32(p + L.secs[(size_t)sec].off + 4 * (long)i); };
  auto byte = [&](int sec) { return (uint32_t)p[L.secs[(size_t)sec].off]; };
  // ---- host item ----
  if (it.step_idx > (uint64_t)L.n_steps) return fmt("step index %llu beyond the token tables (%d rows)", (unsigned long long)it.step_idx, L.n_steps);
  if (it.text_tokens.size() != it.step_idx || it.audio_tokens.size() != it.step_idx * (uint64_t)S) return "token tables do not match the step index";
  if (it.consecutive_pads > it.step_idx) return "consecutive_pads beyond the step index";
  if (it.samp_k < 0) return fmt("samp_k %d is negative", it.samp_k);
  if (it.cfg_on > 1 || it.cond_on > 1) return "cfg_on / cond_on is not 0 or 1";
  if (it.cfg_on && rps != 2) return "cfg_on without cfg_rows";
  const uint32_t text_vocab = (uint32_t)(c.text_in_vocab_size > c.text_out_vocab_size ? c.text_in_vocab_size : c.text_out_vocab_size);
  for (uint32_t t : it.text_tokens)
    if (t != UNG && t >= text_vocab) return fmt("text token %u outside the vocabulary (%u)", t, text_vocab);
  for (uint32_t t : it.audio_tokens)
    if (t != UNG && t >= (uint32_t)c.audio_vocab_size) return fmt("audio token %u >= audio_vocab_size %d", t, c.audio_vocab_size);
  for (int j = 0; j < 2; ++j) {
    const uint32_t len = it.ca_len[j];
    if (len > (uint32_t)(c.cross_attention ? c.ca_max_len : 0) || (j >= rps && len)) return fmt("ca_len[%d] %u > ca_max_len", j, len);
  }
  if (it.cfg_on && (!it.ca_len[0] || !it.ca_len[1])) return "a guided slot without both sources";
  const uint32_t nw = (uint32_t)it.q_end.size(), nt = (uint32_t)it.q_tok.size();
  if (nw > (uint32_t)L.n_steps || nt > (uint32_t)L.n_steps) return fmt("request queue of %u words / %u tokens, capacity %d", nw, nt, L.n_steps);
  if (!(it.req_flags & dsm_tts_slot_blob::kReqActive) && (nw || nt || it.req_flags || it.req_status)) return "request state on a slot without a request";
  if (it.req_status < 0 || it.req_status > 4) return fmt("request status %d", it.req_status);
  int32_t prev = 0;
  for (int32_t e : it.q_end) {
    if (e < prev || (uint32_t)e > nt) return fmt("word end %d outside the %u queued tokens or out of order", e, nt);
    prev = e;
  }
  if (nw ? (uint32_t)prev != nt : nt != 0) return "queued tokens beyond the last word's end";
  // ---- payload: rings, sources ----
  for (int j = 0; j < rps; ++j) {
    const uint32_t idx = w(L.lm_idx, j);
    if (idx >= (uint32_t)c.lm.context) return fmt("LM ring index %u >= context %d", idx, c.lm.context);
    if (L.ca_last >= 0) {
      const uint32_t last = w(L.ca_last, j);
      if (last >= (uint32_t)c.ca_max_len) return fmt("ca.last %u >= ca_max_len %d", last, c.ca_max_len);
      if (last != (it.ca_len[j] ? it.ca_len[j] - 1 : 0u)) return fmt("ca.last %u does not match ca_len %u", last, it.ca_len[j]);
    }
  }
  // ---- the mirrors' device values ----
  if (byte(L.cfg_on) != it.cfg_on) return "cfg_on differs between the payload and the host item";
  if (byte(L.cond_on) != it.cond_on) return "cond_on differs between the payload and the host item";
  if (w(L.samp_k, 0) != (uint32_t)it.samp_k) return fmt("samp_k %d in the payload, %d in the host item", (int32_t)w(L.samp_k, 0), it.samp_k);
  // ---- tokens the next step embeds ----
  if (w(L.text_token, 0) >= text_vocab && w(L.text_token, 0) != UNG) return fmt("text token %u outside the vocabulary", w(L.text_token, 0));
  const uint32_t any_vocab = text_vocab > (uint32_t)c.audio_vocab_size ? text_vocab : (uint32_t)c.audio_vocab_size;
  if (w(L.last, 0) >= any_vocab) return fmt("last token %u outside every vocabulary", w(L.last, 0));
  for (int k = 0; k < S; ++k) {
    if (w(L.lat, k) >= (uint32_t)c.audio_vocab_size) return fmt("depformer sample %u >= audio_vocab_size %d", w(L.lat, k), c.audio_vocab_size);
    if (w(L.row0, k) >= (uint32_t)c.audio_vocab_size) return fmt("row-0 token %u >= audio_vocab_size %d", w(L.row0, k), c.audio_vocab_size);
  }
  for (int k = 0; k <= c.acoustic_delay; ++k)
    if (w(L.ring, k) >= (uint32_t)c.audio_vocab_size) return fmt("codebook-0 ring token %u >= audio_vocab_size %d", w(L.ring, k), c.audio_vocab_size);
  // ---- the request's cursors ----
  {
    auto r = [&](int i) { return (int32_t)w(L.req, i); };
    const bool active = (it.req_flags & dsm_tts_slot_blob::kReqActive) != 0;
    if (r(RQ_STATUS) < 0 || r(RQ_STATUS) > 4) return fmt("request status %d", r(RQ_STATUS));
    if (!active) {  // no request: the record is the zeros dsm_tts_reset_slot leaves
      for (int i = 0; i < 13; ++i)
        if (r(i)) return "a device request on a slot whose host item has none";
    } else {
      if (r(RQ_STATUS) == 0) return "the host item has a request, the device record is idle";
      if (r(RQ_STEP) < 0 || r(RQ_STEP) > L.n_steps) return fmt("request step %d outside the token tables", r(RQ_STEP));
      if ((uint64_t)r(RQ_STEP) != it.step_idx) return fmt("request step %d, step index %llu", r(RQ_STEP), (unsigned long long)it.step_idx);
      if (r(RQ_N_WORDS) != (int32_t)nw) return fmt("request n_words %d, %u word ends in the host item", r(RQ_N_WORDS), nw);
      if (r(RQ_CUR_WORD) < -1 || r(RQ_CUR_WORD) >= (int32_t)nw)
        return fmt("request cur_word %d of %u words", r(RQ_CUR_WORD), nw);
      if (r(RQ_TOKEN_IDX) < 0 || (uint32_t)r(RQ_TOKEN_IDX) > nt) return fmt("request token_idx %d past n_tok %u", r(RQ_TOKEN_IDX), nt);
      if ((uint32_t)r(RQ_HAS_WORD) > 1 || (uint32_t)r(RQ_CLOSED) > 1) return "request has_word / closed is not 0 or 1";
      if (((it.req_flags & dsm_tts_slot_blob::kReqClosed) != 0) != (r(RQ_CLOSED) != 0)) return "request closed flag differs between the payload and the host item";
      if (r(RQ_STEP_PAST_LAST) < 0 || r(RQ_STEP_PAST_LAST) > L.n_steps + 1) return fmt("request step_past_last %d", r(RQ_STEP_PAST_LAST));
      if (r(RQ_LAST_EPAD) < 0 || r(RQ_LAST_EPAD) > r(RQ_STEP)) return fmt("request last_epad %d past its step %d", r(RQ_LAST_EPAD), r(RQ_STEP));
      if (r(RQ_CPADS) < 0 || r(RQ_CPADS) > r(RQ_STEP)) return fmt("request consecutive pads %d past its step %d", r(RQ_CPADS), r(RQ_STEP));
      if (r(RQ_MAX_SEQ_LEN) < 0 || r(RQ_EXTRA_STEPS) < 0) return "request max_seq_len / extra_steps negative";
    }
  }
  if (with_dec) {
    if (!m || L.dec_started < 0) return "decode state without a Mimi configuration";
    if (byte(L.dec_started) > 1) return "dec.started is not 0 or 1";
    const uint32_t di = w(L.dec_idx, 0);
    if (di >= (uint32_t)m->transformer.context) return fmt("Mimi decoder ring index %u >= context %d", di, m->transformer.context);
  }
  return std::string();
}

// The layout as text: one line per section "name bytes_per_slot payload_offset", then "slot_bytes N", then "signature w0 w1 ...".
inline std::string print(const Layout& L) {
  std::string s;
  for (const Sec& x : L.secs) s += fmt("%s %ld %ld\n", x.name.c_str(), x.bytes, x.off);
  s += fmt("slot_bytes %ld\n", L.slot_bytes(!L.secs.empty() && (int)L.secs.size() > L.nsec_base));
  s += "signature";
  for (uint32_t w : L.sig) s += fmt(" %u", w);
  s += "\n";
  return s;
}

}  // namespace dsm_tts_layout
