// dsm_worker.inc — host side of moshi-server's BatchedAsr module above the engine (SURVEY.md §8(f) rank 1):
//   * the wire format: rmp_serde struct-map encoding of `InMsg` / `OutMsg` (srv/asr.rs:15-34,
//     srv/batched_asr.rs:877-880,969-975; client/rust/kyutai-client/src/stt/protocol.rs:47-62)
//   * the slot table and per-channel PCM queue (`BatchedAsr::channels`, `Channel::extend_data`,
//     srv/batched_asr.rs:92-116,796-808)
//   * one pass of encoder_loop -> model_loop -> post_process per dsm_worker_step (srv/batched_asr.rs:314-522,
//     527-718): Init -> Ready + slot reset, markers scheduled `asr_delay_in_tokens` + buffered frames ahead and
//     released from a min-heap, Word / EndWord / Step fan-out guarded by the channel id the step was built for.
// The reference runs the three loops on three threads joined by bounded channels; that changes latency, not what a
// client receives or in which order, so one call runs the three stages back to back.  Ogg/Opus bodies are decoded by
// `kaudio` in handle_socket before they reach this logic (srv/batched_asr.rs:941-949); no Opus decoder is built here,
// such messages are rejected.
#include <algorithm>
#include <deque>
#include <memory>
#include <queue>

#include "dsm_spm.h"  // guarded: the library's translation unit has it already, the host-only harnesses get it here

namespace {

// ---- msgpack writer: the subset rmp_serde emits for these types (smallest integer form, f32/f64 as typed) ----
struct MpW {
  std::vector<uint8_t>& b;
  void u8(uint8_t v) { b.push_back(v); }
  void be(uint64_t v, int n) { for (int i = n - 1; i >= 0; --i) b.push_back((uint8_t)(v >> (8 * i))); }
  void map(size_t n) { if (n < 16) u8(0x80 | (uint8_t)n); else { u8(0xde); be(n, 2); } }
  void arr(size_t n) { if (n < 16) u8(0x90 | (uint8_t)n); else if (n < 65536) { u8(0xdc); be(n, 2); } else { u8(0xdd); be(n, 4); } }
  void str(const char* s, size_t n) {
    if (n < 32) u8(0xa0 | (uint8_t)n); else if (n < 256) { u8(0xd9); u8((uint8_t)n); } else if (n < 65536) { u8(0xda); be(n, 2); } else { u8(0xdb); be(n, 4); }
    b.insert(b.end(), s, s + n);
  }
  void str(const char* s) { str(s, strlen(s)); }
  void uint(uint64_t v) {
    if (v < 128) u8((uint8_t)v); else if (v < 256) { u8(0xcc); u8((uint8_t)v); } else if (v < 65536) { u8(0xcd); be(v, 2); }
    else if (v < (1ull << 32)) { u8(0xce); be(v, 4); } else { u8(0xcf); be(v, 8); }
  }
  void sint(int64_t v) {  // rmp::encode::write_sint
    if (v >= 0) return uint((uint64_t)v);
    if (v >= -32) u8((uint8_t)v); else if (v >= -128) { u8(0xd0); u8((uint8_t)v); } else if (v >= -32768) { u8(0xd1); be((uint64_t)v, 2); }
    else if (v >= -(1ll << 31)) { u8(0xd2); be((uint64_t)v, 4); } else { u8(0xd3); be((uint64_t)v, 8); }
  }
  void f32(float v) { uint32_t u; memcpy(&u, &v, 4); u8(0xca); be(u, 4); }
  void f64(double v) { uint64_t u; memcpy(&u, &v, 8); u8(0xcb); be(u, 8); }
  void bin(const uint8_t* p, size_t n) { if (n < 256) { u8(0xc4); u8((uint8_t)n); } else if (n < 65536) { u8(0xc5); be(n, 2); } else { u8(0xc6); be(n, 4); } b.insert(b.end(), p, p + n); }
};

// ---- msgpack reader ----
struct MpR {
  const uint8_t* p;
  size_t n, o = 0;
  bool ok = true;
  uint8_t peek() { return o < n ? p[o] : (ok = false, 0); }
  uint8_t get() { if (o >= n) { ok = false; return 0; } return p[o++]; }
  uint64_t be(int k) { uint64_t v = 0; for (int i = 0; i < k; ++i) v = (v << 8) | get(); return v; }
  bool map_len(size_t& len) { uint8_t t = get(); if ((t & 0xf0) == 0x80) len = t & 15; else if (t == 0xde) len = be(2); else if (t == 0xdf) len = be(4); else return ok = false; return ok; }
  bool arr_len(size_t& len) { uint8_t t = get(); if ((t & 0xf0) == 0x90) len = t & 15; else if (t == 0xdc) len = be(2); else if (t == 0xdd) len = be(4); else return ok = false; return ok; }
  bool str(std::string& s) {
    uint8_t t = get(); size_t len;
    if ((t & 0xe0) == 0xa0) len = t & 31; else if (t == 0xd9) len = be(1); else if (t == 0xda) len = be(2); else if (t == 0xdb) len = be(4); else return ok = false;
    if (!ok || len > n - o) return ok = false;
    s.assign((const char*)p + o, len); o += len; return true;
  }
  bool number(double& d, int64_t& i, bool& is_int) {  // any numeric type (serde's numeric visitors accept them)
    uint8_t t = get(); is_int = true;
    if (t < 0x80) i = t; else if (t >= 0xe0) i = (int8_t)t;
    else switch (t) {
      case 0xcc: i = (int64_t)be(1); break; case 0xcd: i = (int64_t)be(2); break; case 0xce: i = (int64_t)be(4); break; case 0xcf: i = (int64_t)be(8); break;
      case 0xd0: i = (int8_t)be(1); break; case 0xd1: i = (int16_t)be(2); break; case 0xd2: i = (int32_t)be(4); break; case 0xd3: i = (int64_t)be(8); break;
      case 0xca: { uint32_t u = (uint32_t)be(4); float f; memcpy(&f, &u, 4); d = f; is_int = false; break; }
      case 0xcb: { uint64_t u = be(8); memcpy(&d, &u, 8); is_int = false; break; }
      default: return ok = false;
    }
    if (is_int) d = (double)i; else i = (int64_t)d;
    return ok;
  }
  // any value.  Iterative with a counter of values still owed per nesting level: a client controls the nesting of an
  // unknown field, and a recursive skip could be driven through the stack by one ~3 MB message (rmp_serde refuses
  // beyond its depth limit of 1024 and recv_loop logs and carries on: srv/batched_asr.rs:927-951)
  static constexpr size_t kMaxDepth = 1024;
  bool skip() {
    std::vector<uint64_t> owed;
    uint64_t here = 1;  // values still to read at the current level
    for (;;) {
      while (here == 0) {
        if (owed.empty()) return ok;
        here = owed.back();
        owed.pop_back();
      }
      here -= 1;
      uint8_t t = peek(); size_t len;
      if (!ok) return false;
      if (t < 0x80 || t >= 0xe0 || t == 0xc0 || t == 0xc2 || t == 0xc3) { get(); }
      else if ((t & 0xe0) == 0xa0 || t == 0xd9 || t == 0xda || t == 0xdb) { std::string s; if (!str(s)) return false; }
      else if ((t & 0xf0) == 0x90 || t == 0xdc || t == 0xdd || (t & 0xf0) == 0x80 || t == 0xde || t == 0xdf) {
        const bool is_map = (t & 0xf0) == 0x80 || t == 0xde || t == 0xdf;
        if (!(is_map ? map_len(len) : arr_len(len))) return false;
        const uint64_t items = is_map ? 2 * (uint64_t)len : (uint64_t)len;
        if (items > n - o) return ok = false;  // every item takes at least one byte
        if (owed.size() + 1 >= kMaxDepth) return ok = false;
        owed.push_back(here);
        here = items;
      }
      else if (t == 0xc4 || t == 0xc5 || t == 0xc6) { get(); len = be(t == 0xc4 ? 1 : t == 0xc5 ? 2 : 4); if (!ok || len > n - o) return ok = false; o += len; }
      else if (t == 0xc7 || t == 0xc8 || t == 0xc9) { get(); len = be(t == 0xc7 ? 1 : t == 0xc8 ? 2 : 4); get(); if (!ok || len > n - o) return ok = false; o += len; }  // ext 8/16/32
      else if (t >= 0xd4 && t <= 0xd8) { get(); get(); len = (size_t)1 << (t - 0xd4); if (!ok || len > n - o) return ok = false; o += len; }  // fixext 1..16
      else { double d; int64_t i; bool b; if (!number(d, i, b)) return false; }
      if (!ok) return false;
    }
  }
};

const char* kInNames[] = {"Init", "Marker", "Audio", "OggOpus", "Ping"};
const char* kOutNames[] = {"Word", "EndWord", "Marker", "Step", "Error", "Ready"};

// word_lp: null, or a Word's { logprob, min_logprob } (dsm_worker_set_word_scores) — two more entries behind the reference's
// fields; a map, so decoders that do not know the keys skip them
void encode_out(std::vector<uint8_t>& buf, const dsm_out_msg& m, const double* word_lp = nullptr) {  // field order = declaration order (srv/asr.rs:25-34)
  MpW w{buf};
  auto head = [&](size_t fields) { w.map(1 + fields); w.str("type"); w.str(kOutNames[m.kind]); };
  switch (m.kind) {
    case DSM_OUT_WORD:
      head(word_lp ? 4 : 2); w.str("text"); w.str(m.text ? m.text : ""); w.str("start_time"); w.f64(m.time);
      if (word_lp) { w.str("logprob"); w.f64(word_lp[0]); w.str("min_logprob"); w.f64(word_lp[1]); }
      break;
    case DSM_OUT_ENDWORD: head(1); w.str("stop_time"); w.f64(m.time); break;
    case DSM_OUT_MARKER: head(1); w.str("id"); w.sint(m.id); break;
    case DSM_OUT_STEP:
      head(3); w.str("step_idx"); w.uint(m.step_idx); w.str("prs"); w.arr(m.n_prs);
      for (size_t i = 0; i < m.n_prs; ++i) w.f32(m.prs[i]);
      w.str("buffered_pcm"); w.uint(m.buffered_pcm); break;
    case DSM_OUT_ERROR: head(1); w.str("message"); w.str(m.text ? m.text : ""); break;
    default: head(0); break;  // Ready
  }
}

void encode_in(std::vector<uint8_t>& buf, const dsm_in_msg& m) {
  MpW w{buf};
  auto head = [&](size_t fields) { w.map(1 + fields); w.str("type"); w.str(kInNames[m.kind]); };
  switch (m.kind) {
    case DSM_IN_MARKER: head(1); w.str("id"); w.sint(m.id); break;
    case DSM_IN_AUDIO: head(1); w.str("pcm"); w.arr(m.n_pcm); for (size_t i = 0; i < m.n_pcm; ++i) w.f32(m.pcm[i]); break;
    case DSM_IN_OGGOPUS: head(1); w.str("data"); w.arr(m.n_data); for (size_t i = 0; i < m.n_data; ++i) w.uint(m.data[i]); break;  // Vec<u8> without serde_bytes: a sequence
    default: head(0); break;  // Init, Ping
  }
}

struct InDecoded {
  int kind = -1;
  int64_t id = 0;
  std::vector<float> pcm;
  std::vector<uint8_t> data;
};

// serde internally-tagged enum: a map whose "type" entry names the variant; the other entries are its fields, in any
// order; unknown fields are ignored (serde default), a missing field is an error
// axum / tungstenite refuse websocket messages beyond 64 MiB by default (the reference sets no other limit)
constexpr size_t kMaxInMsgBytes = (size_t)64 << 20;

bool decode_in(const uint8_t* p, size_t n, InDecoded& out) {
  if (n > kMaxInMsgBytes) return false;
  MpR r{p, n};
  size_t len;
  if (!r.map_len(len)) return false;
  bool have_id = false, have_pcm = false, have_data = false;
  std::string key, type;
  for (size_t e = 0; e < len && r.ok; ++e) {
    if (!r.str(key)) return false;
    if (key == "type") { if (!r.str(type)) return false; }
    else if (key == "id") { double d; bool is_int; if (!r.number(d, out.id, is_int) || !is_int) return false; have_id = true; }
    else if (key == "pcm") {
      size_t k; if (!r.arr_len(k) || k > (n - r.o)) return false;
      out.pcm.resize(k);
      for (size_t i = 0; i < k; ++i) { double d; int64_t iv; bool is_int; if (!r.number(d, iv, is_int)) return false; out.pcm[i] = (float)d; }
      have_pcm = true;
    } else if (key == "data") {
      uint8_t t = r.peek();
      if (t == 0xc4 || t == 0xc5 || t == 0xc6) { r.get(); size_t k = r.be(t == 0xc4 ? 1 : t == 0xc5 ? 2 : 4); if (!r.ok || k > n - r.o) return false; out.data.assign(p + r.o, p + r.o + k); r.o += k; }
      else { size_t k; if (!r.arr_len(k) || k > (n - r.o)) return false; out.data.resize(k); for (size_t i = 0; i < k; ++i) { double d; int64_t iv; bool is_int; if (!r.number(d, iv, is_int) || !is_int || iv < 0 || iv > 255) return false; out.data[i] = (uint8_t)iv; } }
      have_data = true;
    } else if (!r.skip()) return false;
  }
  if (!r.ok) return false;
  for (int k = 0; k < 5; ++k) if (type == kInNames[k]) out.kind = k;
  if (out.kind < 0) return false;
  if (out.kind == DSM_IN_MARKER && !have_id) return false;
  if (out.kind == DSM_IN_AUDIO && !have_pcm) return false;
  if (out.kind == DSM_IN_OGGOPUS && !have_data) return false;
  return true;
}

struct WMarker {  // srv/batched_asr.rs:31-49
  uint64_t channel_id;
  int batch_idx;
  size_t step_idx;
  int64_t marker_id;
  uint64_t seq;  // insertion order: BinaryHeap gives no order among equal keys; ties are released oldest first here
};
struct WMarkerCmp { bool operator()(const WMarker& a, const WMarker& b) const { return a.step_idx != b.step_idx ? a.step_idx > b.step_idx : a.seq > b.seq; } };

// per-socket kaudio::ogg_opus::Decoder state (container half) with the lock of ITS socket: the demultiplexer and the
// host's Opus decoder run under this lock, never under the worker-wide one (the reference decodes in the per-socket
// recv_loop, outside any shared lock: srv/batched_asr.rs:941-949)
struct WOgg {
  std::mutex mu;
  dsm_ogg_demux* d = nullptr;
  ~WOgg() { dsm_ogg_demux_free(d); }
};
// An OggOpus body is one websocket message of a live stream: at Opus' top rate (510 kbit/s) 8 MiB are two minutes of audio.
// Larger bodies are refused (the 64 MiB message limit stays for the other variants).
constexpr size_t kMaxOggBodyBytes = (size_t)8 << 20;

struct WPipelineMsg {  // srv/batched_asr.rs:51-67 PipelineMsg (the codes stay inside the backend: `ticket` names them)
  std::vector<uint8_t> mask;
  std::vector<uint64_t> ref_ids;
  std::vector<int> resets;
  std::vector<WMarker> new_markers;
  std::vector<size_t> buffered;
  int ticket = -1;
};

struct WChannel {  // srv/batched_asr.rs:69-116
  std::shared_ptr<WOgg> ogg;  // created on the first OggOpus body; shared so that a send in flight outlives a slot re-assignment
  uint64_t id = 0;
  bool open = false;         // Some(channel)
  bool out_closed = false;   // out_tx.is_closed(): the socket side went away
  bool in_closed = false;    // in_rx disconnected
  std::deque<InDecoded> in;  // in_rx
  std::deque<std::vector<uint8_t>> out;  // out_rx (already serialised: send_loop's job)
  std::deque<float> data;
  size_t steps = 0;
  int bias_set = 0;  // dsm_worker_set_bias: what the channel's slot is attached to; detached when the channel closes
  // dsm_worker_set_input_rate: the rate of the channel's Audio samples and its frame of 80 ms in them; back to 24000 / 1920 when
  // the channel closes
  int rate = 24000;
  size_t frame = DSM_FRAME_SIZE;
};

}  // namespace

struct dsm_worker {
  dsm_worker_backend be{};
  int B = 0, delay = 0;
  std::vector<WChannel> ch;
  std::deque<int> active, free_slots;
  std::priority_queue<WMarker, std::vector<WMarker>, WMarkerCmp> markers;
  uint64_t next_channel_id = 1, marker_seq = 0;
  size_t enc_step_idx = 0, model_step_idx = 0;
  std::vector<float> batch_pcm;
  std::vector<float> batch_raw;  // [B][48 kHz frame]: in being once a channel has a rate of its own; a step uses it at that step's pitch
  std::vector<uint8_t> mask;
  std::vector<uint64_t> channel_ids;  // 0 = None
  std::deque<WPipelineMsg> pipe;      // encoder_loop -> model_loop (sync_channel, srv/batched_asr.rs:291)
  dsm_detok_fn detok = nullptr;
  void* detok_user = nullptr;
  std::unique_ptr<dsm_spm> tok;  // dsm_worker_set_tokenizer_file: Word.text when no detok callback is set
  dsm_opus_decode_fn opus = nullptr;
  void* opus_user = nullptr;
  dsm_engine* eng = nullptr;  // dsm_worker_create: the engine behind `be` (null with a caller-supplied backend)
  bool word_scores = false;   // dsm_worker_set_word_scores
  std::mutex mu;
  std::string err;

  bool extend_data(WChannel& c, const float* pcm, size_t n, float* out_pcm) {  // Channel::extend_data, in frames of the channel's rate
    const size_t F = c.frame;
    if (n == 0 && c.data.size() < F) return false;
    if (c.data.empty() && n >= F) {
      memcpy(out_pcm, pcm, sizeof(float) * F);
      c.data.insert(c.data.end(), pcm + F, pcm + n);
      return true;
    }
    c.data.insert(c.data.end(), pcm, pcm + n);
    if (c.data.size() >= F) {
      std::copy(c.data.begin(), c.data.begin() + (long)F, out_pcm);
      c.data.erase(c.data.begin(), c.data.begin() + (long)F);
      return true;
    }
    return false;
  }
  void send(int slot, const dsm_out_msg& m, uint64_t ref_channel_id, const double* word_lp = nullptr) {  // Channel::send
    WChannel& c = ch[slot];
    if (!c.open || c.id != ref_channel_id) return;  // the slot was re-assigned since the step was built
    if (c.out_closed) { c.open = false; return; }   // send error -> *channel = None
    c.out.emplace_back();
    encode_out(c.out.back(), m, word_lp);
  }
};

extern "C" {

int dsm_inmsg_encode(const dsm_in_msg* m, uint8_t* buf, size_t cap) {
  if (!m || m->kind < 0 || m->kind > DSM_IN_PING) return DSM_ERR_INVALID;
  std::vector<uint8_t> b;
  encode_in(b, *m);
  if (buf && b.size() <= cap) memcpy(buf, b.data(), b.size());
  return (int)b.size();
}

int dsm_outmsg_encode(const dsm_out_msg* m, uint8_t* buf, size_t cap) {
  if (!m || m->kind < 0 || m->kind > DSM_OUT_READY) return DSM_ERR_INVALID;
  std::vector<uint8_t> b;
  encode_out(b, *m);
  if (buf && b.size() <= cap) memcpy(buf, b.data(), b.size());
  return (int)b.size();
}

int dsm_inmsg_decode(const uint8_t* bytes, size_t len, dsm_in_msg* out, float* pcm_buf, size_t pcm_cap, uint8_t* data_buf,
                     size_t data_cap) {
  if (!bytes || !out) return DSM_ERR_INVALID;
  InDecoded d;
  if (!decode_in(bytes, len, d)) return DSM_ERR_IO;
  memset(out, 0, sizeof *out);
  out->kind = d.kind;
  out->id = d.id;
  out->n_pcm = d.pcm.size();
  out->n_data = d.data.size();
  if (pcm_buf && !d.pcm.empty()) memcpy(pcm_buf, d.pcm.data(), sizeof(float) * std::min(pcm_cap, d.pcm.size()));  // empty vector: data() may be null
  if (data_buf && !d.data.empty()) memcpy(data_buf, d.data.data(), std::min(data_cap, d.data.size()));
  out->pcm = pcm_buf;
  out->data = data_buf;
  return 0;
}

// client side: protocol.rs:60-62 decode_out_msg
int dsm_outmsg_decode(const uint8_t* bytes, size_t len, dsm_out_msg* out, char* text_buf, size_t text_cap, float* prs_buf,
                      size_t prs_cap) {
  if (!bytes || !out) return DSM_ERR_INVALID;
  MpR r{bytes, len};
  size_t n;
  if (!r.map_len(n)) return DSM_ERR_IO;
  memset(out, 0, sizeof *out);
  std::string key, type, text;
  std::vector<float> prs;
  bool have[6] = {false, false, false, false, false, false};  // text/message, time, id, step_idx, prs, buffered_pcm
  for (size_t e = 0; e < n && r.ok; ++e) {
    if (!r.str(key)) return DSM_ERR_IO;
    double d; int64_t i; bool is_int;
    if (key == "type") { if (!r.str(type)) return DSM_ERR_IO; }
    else if (key == "text" || key == "message") { if (!r.str(text)) return DSM_ERR_IO; have[0] = true; }
    else if (key == "start_time" || key == "stop_time") { if (!r.number(d, i, is_int)) return DSM_ERR_IO; out->time = d; have[1] = true; }
    else if (key == "id") { if (!r.number(d, i, is_int) || !is_int) return DSM_ERR_IO; out->id = i; have[2] = true; }
    else if (key == "step_idx") { if (!r.number(d, i, is_int) || !is_int || i < 0) return DSM_ERR_IO; out->step_idx = (uint64_t)i; have[3] = true; }
    else if (key == "buffered_pcm") { if (!r.number(d, i, is_int) || !is_int || i < 0) return DSM_ERR_IO; out->buffered_pcm = (uint64_t)i; have[5] = true; }
    else if (key == "prs") {
      size_t k; if (!r.arr_len(k) || k > len) return DSM_ERR_IO;
      for (size_t j = 0; j < k; ++j) { if (!r.number(d, i, is_int)) return DSM_ERR_IO; prs.push_back((float)d); }
      have[4] = true;
    } else if (!r.skip()) return DSM_ERR_IO;
  }
  if (!r.ok) return DSM_ERR_IO;
  out->kind = -1;
  for (int k = 0; k < 6; ++k) if (type == kOutNames[k]) out->kind = k;
  const bool need_ok = out->kind == DSM_OUT_WORD ? have[0] && have[1] : out->kind == DSM_OUT_ENDWORD ? have[1] :
                       out->kind == DSM_OUT_MARKER ? have[2] : out->kind == DSM_OUT_STEP ? have[3] && have[4] && have[5] :
                       out->kind == DSM_OUT_ERROR ? have[0] : out->kind == DSM_OUT_READY;
  if (!need_ok) return DSM_ERR_IO;
  if (text_buf && text_cap) { size_t k = std::min(text_cap - 1, text.size()); memcpy(text_buf, text.data(), k); text_buf[k] = 0; }
  out->text = text_buf;
  out->n_prs = prs.size();
  if (prs_buf && !prs.empty()) memcpy(prs_buf, prs.data(), sizeof(float) * std::min(prs_cap, prs.size()));
  out->prs = prs_buf;
  return 0;
}

#ifndef DSM_HOST_ONLY  // tests/sanitize builds this file without the engine (host sanitizer harness)
// the engine as a worker backend
static int be_encode(void* self, const float* pcm, const uint8_t* mask) {
  int produced = 0;
  return dsm_mimi_encode_step((dsm_engine*)self, pcm, mask, nullptr, &produced);  // codes stay on the device
}
static int be_reset(void* self, int slot) { return dsm_asr_reset_slot((dsm_engine*)self, slot); }
static int be_step(void* self, const uint8_t* mask, uint32_t* text, float* prs) {
  return dsm_asr_step_tokens((dsm_engine*)self, nullptr, mask, text, prs);
}
static int be_poll(void* self, dsm_asr_msg* msgs, int cap, uint32_t* toks, int tcap) {
  return dsm_asr_poll_msgs((dsm_engine*)self, msgs, cap, toks, tcap);
}
static const char* be_error(void* self) { return dsm_last_error((dsm_engine*)self); }
static int be_encode_async(void* self, const float* pcm, const uint8_t* mask, int* ticket) {
  return dsm_mimi_encode_step_async((dsm_engine*)self, pcm, mask, ticket);
}
static int be_step_ticket(void* self, int ticket, const uint8_t* mask, uint32_t* text, float* prs) {
  return dsm_asr_step_tokens_ticket((dsm_engine*)self, ticket, mask, text, prs);
}

int dsm_worker_create(dsm_engine* e, dsm_worker** out) {
  if (!e || !out) return DSM_ERR_INVALID;
  dsm_worker_backend be{};
  be.self = e;
  be.batch_size = e->B;
  be.asr_delay_in_tokens = e->cfg.asr_delay_in_tokens;
  be.extra_heads_num = e->cfg.extra_heads_num;
  be.encode_step = be_encode;
  be.reset_slot = be_reset;
  be.step_tokens = be_step;
  be.poll_msgs = be_poll;
  be.last_error = be_error;
  be.encode_async = be_encode_async;
  be.step_ticket = be_step_ticket;
  be.text_out_vocab_size = e->cfg.text_out_vocab_size;
  const int rc = dsm_worker_create_with_backend(&be, out);
  if (rc == 0) (*out)->eng = e;
  return rc;
}

#endif  // DSM_HOST_ONLY

int dsm_worker_create_with_backend(const dsm_worker_backend* be, dsm_worker** out) {
  if (!be || !out || be->batch_size <= 0 || !be->encode_step || !be->reset_slot || !be->step_tokens || !be->poll_msgs ||
      be->extra_heads_num < 0 || be->extra_heads_num > DSM_MAX_EXTRA_HEADS || (!be->encode_async != !be->step_ticket))
    return DSM_ERR_INVALID;
  dsm_worker* w = new dsm_worker();
  w->be = *be;
  w->B = be->batch_size;
  w->delay = be->asr_delay_in_tokens;
  w->ch.resize(w->B);
  for (int i = 0; i < w->B; ++i) w->free_slots.push_back(i);  // srv/batched_asr.rs:775-777
  w->batch_pcm.assign((size_t)w->B * DSM_FRAME_SIZE, 0.0f);
  w->mask.assign(w->B, 0);
  w->channel_ids.assign(w->B, 0);
  *out = w;
  return 0;
}

void dsm_worker_destroy(dsm_worker* w) {
  if (!w) return;
#ifndef DSM_HOST_ONLY
  // dsm_worker_set_bias: what the worker attached it detaches, so that the engine's owner can destroy the sets
  for (int b = 0; b < w->B && w->eng; ++b)
    if (w->ch[(size_t)b].bias_set) (void)dsm_asr_set_bias(w->eng, b, 0);
  // dsm_worker_set_input_rate: the slots go back to 24 kHz, so that the engine's owner finds them as the worker found them
  for (int b = 0; b < w->B && w->eng; ++b)
    if (w->ch[(size_t)b].rate != 24000) (void)dsm_asr_set_input_format(w->eng, b, 24000, DSM_PCM_F32);
#endif
  delete w;
}
const char* dsm_worker_last_error(const dsm_worker* w) { return w ? w->err.c_str() : ""; }
void dsm_worker_set_detokenizer(dsm_worker* w, dsm_detok_fn fn, void* user) {
  if (!w) return;
  std::lock_guard<std::mutex> lk(w->mu);
  w->detok = fn;
  w->detok_user = user;
}

int dsm_worker_set_tokenizer_file(dsm_worker* w, const char* path) {
  if (!w || !path) return DSM_ERR_INVALID;
  dsm_spm* tok = nullptr;
  const int rc = dsm_spm_load(path, &tok);  // outside the lock: reading and indexing the file holds up no step
  std::lock_guard<std::mutex> lk(w->mu);
  if (rc) { w->err = std::string("tokenizer ") + path + ": " + dsm_spm_last_error(nullptr); return rc; }
  const int pieces = dsm_spm_vocab_size(tok), vocab = w->be.text_out_vocab_size;
  if (vocab > 0 && pieces > vocab) {
    w->err = std::string("tokenizer ") + path + " has " + std::to_string(pieces) + " pieces, the model's text_out_vocab_size is " + std::to_string(vocab);
    dsm_spm_free(tok);
    return DSM_ERR_INVALID;
  }
  w->tok.reset(tok);
  return 0;
}

int dsm_worker_set_word_scores(dsm_worker* w, int on) {
  if (!w) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (!w->eng) { w->err = "word scores need the engine as backend (dsm_worker_create): a caller-supplied backend has no scores"; return DSM_ERR_STATE; }
#ifndef DSM_HOST_ONLY
  if (on && w->eng->scores_top_n < 0)
    if (int rc = dsm_asr_set_token_scores(w->eng, 0)) { w->err = dsm_last_error(w->eng); return rc; }
#endif
  w->word_scores = on != 0;
  return 0;
}

int dsm_worker_set_bias(dsm_worker* w, int slot, int set) {
  if (!w || slot < 0 || slot >= w->B) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (!w->eng) { w->err = "text bias needs the engine as backend (dsm_worker_create): a caller-supplied backend has no bias sets"; return DSM_ERR_STATE; }
  WChannel& c = w->ch[slot];
  if (!c.open || c.in_closed) { w->err = "channel is closed"; return DSM_ERR_STATE; }
#ifndef DSM_HOST_ONLY
  if (int rc = dsm_asr_set_bias(w->eng, slot, set)) { w->err = dsm_last_error(w->eng); return rc; }
#endif
  c.bias_set = set;
  return 0;
}

int dsm_worker_set_input_rate(dsm_worker* w, int slot, int hz) {
  if (!w || slot < 0 || slot >= w->B) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (!w->eng) { w->err = "an input rate needs the engine as backend (dsm_worker_create): a caller-supplied backend takes 24 kHz"; return DSM_ERR_STATE; }
  WChannel& c = w->ch[slot];
  if (!c.open || c.in_closed) { w->err = "channel is closed"; return DSM_ERR_STATE; }
  if (hz == c.rate) return 0;
  // samples already queued or cut were counted in frames of the old rate
  if (!c.data.empty() || c.steps) { w->err = "the input rate is set before the channel's first audio is cut into frames"; return DSM_ERR_STATE; }
#ifndef DSM_HOST_ONLY
  dsm_pcm_desc d;
  std::string derr;
  if (int rc = dsm_pcm::describe(DSM_PCM_IN, hz, DSM_PCM_F32, &d, &derr)) { w->err = derr; return rc; }
  if (int rc = dsm_asr_set_ingest(w->eng, 1)) { w->err = dsm_last_error(w->eng); return rc; }  // a no-op once it is on
  if (int rc = dsm_asr_set_input_format(w->eng, slot, hz, DSM_PCM_F32)) { w->err = dsm_last_error(w->eng); return rc; }
  if (w->batch_raw.empty()) w->batch_raw.assign((size_t)w->B * DSM_PCM_MAX_FRAME, 0.0f);
  c.rate = hz;
  c.frame = d.frame;
#endif
  return 0;
}

void dsm_worker_set_opus_decoder(dsm_worker* w, dsm_opus_decode_fn fn, void* user) {
  if (!w) return;
  std::lock_guard<std::mutex> lk(w->mu);
  w->opus = fn;
  w->opus_user = user;
}

// BatchedAsr::channels() + the `in_tx.send(InMsg::Init)` of handle_socket / handle_query (srv/batched_asr.rs:796-808,893)
int dsm_worker_open(dsm_worker* w, uint64_t* channel_id) {
  if (!w) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  if (w->free_slots.empty()) {
    w->err = "Server at capacity - no free channels available";  // OutMsg::Error text of srv/batched_asr.rs:875
    return DSM_ERR_STATE;
  }
  const int slot = w->free_slots.front();
  w->free_slots.pop_front();
  WChannel& c = w->ch[slot];
  c = WChannel();
  c.open = true;
  c.id = w->next_channel_id++;
  w->active.push_back(slot);
  InDecoded init;
  init.kind = DSM_IN_INIT;
  c.in.push_back(std::move(init));
  if (channel_id) *channel_id = c.id;
  return slot;
}

int dsm_worker_close(dsm_worker* w, int slot) {  // both halves of the socket drop
  if (!w || slot < 0 || slot >= w->B) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  w->ch[slot].out_closed = true;
  w->ch[slot].in_closed = true;
  return 0;
}

// recv_loop body for one binary websocket message (srv/batched_asr.rs:927-951).  Returns 0 queued, 1 skipped
// (undecodable: the reference logs and continues), DSM_ERR_STATE for OggOpus (no Opus decoder in this build).
int dsm_worker_send(dsm_worker* w, int slot, const uint8_t* msgpack, size_t len) {
  if (!w || slot < 0 || slot >= w->B || !msgpack) return DSM_ERR_INVALID;
  InDecoded d;
  if (!decode_in(msgpack, len, d)) return 1;
  if (d.kind == DSM_IN_OGGOPUS) {  // recv_loop decodes these before they reach the channel (:941-949)
    // Demultiplexing and Opus decoding run under the CHANNEL's lock only: one client's body (hostile or merely long) must
    // not hold up dsm_worker_step_encode / _model / _recv of every other slot (ADVICE r02).  The worker lock is taken twice,
    // briefly: to find the channel's decoder state, and to queue the decoded audio.
    std::shared_ptr<WOgg> og;
    uint64_t cid = 0;
    dsm_opus_decode_fn opus = nullptr;
    void* opus_user = nullptr;
    {
      std::lock_guard<std::mutex> lk(w->mu);
      WChannel& c = w->ch[slot];
      if (!c.open || c.in_closed) { w->err = "channel is closed"; return DSM_ERR_STATE; }
      if (!w->opus) { w->err = "OggOpus bodies need an Opus decoder: none is built here, set one with dsm_worker_set_opus_decoder"; return DSM_ERR_STATE; }
      if (d.data.size() > kMaxOggBodyBytes) { w->err = "OggOpus body beyond 8 MiB refused"; return DSM_ERR_STATE; }
      if (!c.ogg) { c.ogg = std::make_shared<WOgg>(); c.ogg->d = dsm_ogg_demux_new(); }
      if (!c.ogg->d) { w->err = "Ogg demultiplexer failure"; return DSM_ERR_STATE; }
      og = c.ogg;
      cid = c.id;
      opus = w->opus;
      opus_user = w->opus_user;
    }
    InDecoded audio;
    audio.kind = DSM_IN_AUDIO;
    int rc = 0;
    // bodies of one socket are decoded AND queued in order: the decoded audio goes into the channel while the channel's Ogg
    // lock is still held, so two concurrent sends to one slot cannot enqueue out of order (ADVICE r03).  Lock order og -> w.
    std::lock_guard<std::mutex> ol(og->mu);
    if (dsm_ogg_demux_push(og->d, d.data.data(), d.data.size()) < 0) {
      std::lock_guard<std::mutex> lk(w->mu);
      w->err = "Ogg demultiplexer failure";
      return DSM_ERR_STATE;
    }
    {
      const uint8_t* pkt;
      size_t plen;
      int is_header = 0;
      std::vector<float> pcm(5760);  // 120 ms at 48 kHz: the longest Opus frame at any rate
      while (dsm_ogg_demux_next(og->d, &pkt, &plen, &is_header) == 1) {
        if (is_header) continue;  // OpusHead / OpusTags
        const int n = opus(opus_user, slot, pkt, plen, pcm.data(), pcm.size());
        if (n < 0 || (size_t)n > pcm.size()) { rc = 1; continue; }  // logged and skipped upstream
        audio.pcm.insert(audio.pcm.end(), pcm.begin(), pcm.begin() + n);
      }
    }
    std::lock_guard<std::mutex> lk(w->mu);
    if (rc) w->err = "oggopus decoding error";
    WChannel& c = w->ch[slot];
    if (!c.open || c.in_closed || c.id != cid) { w->err = "channel is closed"; return DSM_ERR_STATE; }  // re-assigned meanwhile
    if (!audio.pcm.empty()) c.in.push_back(std::move(audio));  // Ok(Some(pcm)) -> InMsg::Audio { pcm }
    return rc;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  WChannel& c = w->ch[slot];
  if (!c.open || c.in_closed) { w->err = "channel is closed"; return DSM_ERR_STATE; }
  c.in.push_back(std::move(d));
  return 0;
}

// BatchedAsr::handle_query — srv/batched_asr.rs:811-842: an HTTP POST body (an audio file) on a fresh channel (dsm_worker_open has
// queued the Init of :833 already): the whole decoded clip as ONE Audio message (pcm_decode, resampled to 24 kHz when the file says another rate), Marker { id: 0 }, ten
// seconds of silence to flush the delayed tokens.  The caller drains OutMsgs until the Marker comes back (:843-851).
int dsm_worker_send_body(dsm_worker* w, int slot, const uint8_t* body, size_t len) {
  if (!w || slot < 0 || slot >= w->B || !body) return DSM_ERR_INVALID;
  float* pcm = nullptr;
  size_t n = 0;
  int rate = 0;
  if (int rc = dsm_pcm_decode(body, len, &pcm, &n, &rate)) {
    std::lock_guard<std::mutex> lk(w->mu);
    w->err = "the body is neither RIFF/WAVE nor MPEG-1 Layer III (pcm_decode)";
    return rc;
  }
  InDecoded audio;
  audio.kind = DSM_IN_AUDIO;
  if (rate == 24000) {
    audio.pcm.assign(pcm, pcm + n);
  } else {
    float* r = nullptr;
    size_t nr = 0;
    const int rc = dsm_resample(pcm, n, rate, 24000, &r, &nr);
    if (rc) { free(pcm); std::lock_guard<std::mutex> lk(w->mu); w->err = "unsupported sample rate"; return rc; }
    audio.pcm.assign(r, r + nr);
    free(r);
  }
  free(pcm);
  InDecoded marker, flush;
  marker.kind = DSM_IN_MARKER; marker.id = 0;
  flush.kind = DSM_IN_AUDIO; flush.pcm.assign(240000, 0.0f);
  std::lock_guard<std::mutex> lk(w->mu);
  WChannel& c = w->ch[slot];
  if (!c.open || c.in_closed) { w->err = "channel is closed"; return DSM_ERR_STATE; }
  c.in.push_back(std::move(audio));
  c.in.push_back(std::move(marker));
  c.in.push_back(std::move(flush));
  return 0;
}

int dsm_worker_recv(dsm_worker* w, int slot, uint8_t* buf, size_t cap, size_t* len) {
  if (!w || slot < 0 || slot >= w->B || !len) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  WChannel& c = w->ch[slot];
  if (c.out.empty()) return 0;
  *len = c.out.front().size();
  if (!buf || cap < *len) return DSM_ERR_INVALID;  // *len tells the size needed
  memcpy(buf, c.out.front().data(), *len);
  c.out.pop_front();
  return 1;
}

int dsm_worker_buffered(dsm_worker* w, int slot) {
  if (!w || slot < 0 || slot >= w->B) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> lk(w->mu);
  return (int)w->ch[slot].data.size();
}

// encoder_loop iteration (srv/batched_asr.rs:314-403): pre_process_pipelined, Mimi::encode_step, one PipelineMsg into the
// channel towards model_loop.  Returns 1 if a message was produced (data, reset or marker), 0 if idle or if the channel is
// full (back-pressure; the reference's bound is 100 frames, here the engine's ring of 4), <0 on a backend error.
int dsm_worker_step_encode(dsm_worker* w) {
  if (!w) return DSM_ERR_INVALID;
  std::unique_lock<std::mutex> lk(w->mu);
  const dsm_worker_backend& be = w->be;
  const int B = w->B;
  const size_t cap = be.encode_async ? 3 : 1;  // a synchronous backend keeps ONE frame's codes inside itself
  if (w->pipe.size() >= cap) return 0;
  WPipelineMsg pm;
  std::fill(w->mask.begin(), w->mask.end(), 0);
  std::fill(w->channel_ids.begin(), w->channel_ids.end(), 0);
  // dsm_worker_set_input_rate: while an open channel has a rate of its own the step goes through the raw entry point, every
  // channel's frame — 1920 samples of a 24 kHz channel among them — in a row of the step's pitch: the longest open frame
  size_t row = DSM_FRAME_SIZE;
  bool raw = false;
  for (int bid : w->active) {
    const WChannel& c = w->ch[bid];
    if (c.open && c.rate != 24000) raw = true;
    if (c.open) row = std::max(row, c.frame);
  }
  if (!raw) row = DSM_FRAME_SIZE;
  row = (row + 3) & ~(size_t)3;  // a pitch of whole 16 bytes
  float* const batch = raw ? w->batch_raw.data() : w->batch_pcm.data();
  // ---- pre_process_pipelined — srv/batched_asr.rs:527-659 ----
  for (int bid : w->active) {
    WChannel& c = w->ch[bid];
    float* out_pcm = batch + (size_t)bid * row;
    std::fill(out_pcm, out_pcm + row, 0.0f);
    if (!c.open) continue;
    w->channel_ids[bid] = c.id;
    if (c.out_closed) continue;
    bool mask_val = false;
    for (;;) {
      if (c.in.empty()) {
        if (c.in_closed) break;  // TryRecvError::Disconnected
        if (w->extend_data(c, nullptr, 0, out_pcm)) { c.steps += 1; mask_val = true; }
        break;  // TryRecvError::Empty
      }
      InDecoded m = std::move(c.in.front());
      c.in.pop_front();
      if (m.kind == DSM_IN_INIT) {
        dsm_out_msg ready{};
        ready.kind = DSM_OUT_READY;
        if (c.out_closed) break;
        c.out.emplace_back();
        encode_out(c.out.back(), ready);
        pm.resets.push_back(bid);
      } else if (m.kind == DSM_IN_MARKER) {
        // queued frames in the channel's own frame length; a resampled channel's last D output samples in front of the marker
        // land in the frame after, so its marker is due one step later
        const size_t current_data = c.data.size() / c.frame + (c.rate != 24000 ? 1 : 0);
        pm.new_markers.push_back(WMarker{c.id, bid, w->enc_step_idx + (size_t)w->delay + current_data, m.id, w->marker_seq++});
      } else if (m.kind == DSM_IN_AUDIO) {
        if (w->extend_data(c, m.pcm.data(), m.pcm.size(), out_pcm)) { c.steps += 1; mask_val = true; }
      }  // Ping: nothing
    }
    w->mask[bid] = mask_val ? 1 : 0;
  }
  // closed channels go back to the free list (:634-658)
  for (size_t i = 0; i < w->active.size();) {
    const int bid = w->active[i];
    WChannel& c = w->ch[bid];
    if (!c.open || c.out_closed) {
#ifndef DSM_HOST_ONLY
      // dsm_worker_set_bias: the next channel of this slot starts unbiased.  The call waits for the model and group streams
      // (this is the encoder thread, and w->mu is held: the model thread takes it only outside its engine calls, so it cannot
      // be waiting for us).  Frames of this slot that the run-ahead pipeline still holds then step detached: their output goes
      // to a channel that is closed.  A failure is the step's failure; the channel stays listed and the detach is tried again.
      if (c.bias_set && w->eng)
        if (int brc = dsm_asr_set_bias(w->eng, bid, 0)) { w->err = dsm_last_error(w->eng); return brc; }
      // dsm_worker_set_input_rate: the next channel of this slot is a 24 kHz channel again (same place, same lock rules).  The
      // slot is masked off in this step — a closed channel cuts no frame — so the step's raw rows do not hold a frame of it.
      if (c.rate != 24000 && w->eng)
        if (int irc = dsm_asr_set_input_format(w->eng, bid, 24000, DSM_PCM_F32)) { w->err = dsm_last_error(w->eng); return irc; }
#endif
      c.rate = 24000;
      c.frame = DSM_FRAME_SIZE;
      c.open = false;
      c.bias_set = 0;
      w->active.erase(w->active.begin() + (long)i);
      w->free_slots.push_back(bid);
    } else {
      ++i;
    }
  }
  bool with_data = false;
  for (int b = 0; b < B; ++b) with_data = with_data || w->mask[b];
  if (!with_data && pm.resets.empty() && pm.new_markers.empty()) return 0;  // encoder_loop sleeps 2 ms here (:399)
  w->enc_step_idx += 1;
  pm.mask = w->mask;
  pm.ref_ids = w->channel_ids;
  for (int b = 0; b < B; ++b) pm.buffered.push_back(w->ch[b].data.size());
  const std::vector<float> pcm(batch, batch + (size_t)B * row);  // the engine call runs outside the lock: a private copy of the frame
  lk.unlock();
  // ---- Mimi::encode_step — :351-377 ----
  int rc;
#ifndef DSM_HOST_ONLY
  if (raw) rc = dsm_mimi_encode_step_raw_async(w->eng, pcm.data(), sizeof(float) * row, pm.mask.data(), &pm.ticket);
  else
#endif
  if (be.encode_async) rc = be.encode_async(be.self, pcm.data(), pm.mask.data(), &pm.ticket);
  else rc = be.encode_step(be.self, pcm.data(), pm.mask.data());
  lk.lock();
  if (rc) { w->err = be.last_error ? be.last_error(be.self) : "backend error"; return rc; }
  w->pipe.push_back(std::move(pm));  // sync_channel towards model_loop (:291,378-394)
  return 1;
}

// model_loop iteration (:432-522) + post_process (:655-718) for the oldest PipelineMsg: slot resets, step_tokens, then the
// Word / EndWord / Step fan-out and the markers that came due.  1 a step ran, 0 nothing queued, <0 backend error.
int dsm_worker_step_model(dsm_worker* w) {
  if (!w) return DSM_ERR_INVALID;
  std::unique_lock<std::mutex> lk(w->mu);
  if (w->pipe.empty()) return 0;
  const dsm_worker_backend& be = w->be;
  const int B = w->B;
  WPipelineMsg pm = std::move(w->pipe.front());
  lk.unlock();  // the engine call does not touch the slot table
  int rc = 0;
  for (int bid : pm.resets) if ((rc = be.reset_slot(be.self, bid))) break;  // :467-471
  const int nh = be.extra_heads_num;
  std::vector<uint32_t> text(B);
  std::vector<float> prs((size_t)std::max(nh, 1) * B);
  if (rc == 0) {
    if (be.encode_async) rc = be.step_ticket(be.self, pm.ticket, pm.mask.data(), text.data(), nh ? prs.data() : nullptr);
    else rc = be.step_tokens(be.self, pm.mask.data(), text.data(), nh ? prs.data() : nullptr);
  }
  lk.lock();
  w->pipe.pop_front();  // popped only now: a synchronous backend must not see the next encode before this step consumed its codes
  if (rc) { w->err = be.last_error ? be.last_error(be.self) : "backend error"; return rc; }
  w->model_step_idx += 1;
  for (auto& m : pm.new_markers) w->markers.push(m);
  const std::vector<uint8_t>& mask = pm.mask;
  const std::vector<uint64_t>& ref_ids = pm.ref_ids;
  // ---- post_process — :661-718 ----
  // A step yields at most one Step plus a Word and an EndWord per slot.  poll_msgs does not consume (the list lives
  // until the next step), so a token buffer that turns out too small for a long word is grown and the poll repeated.
  std::vector<dsm_asr_msg> msgs((size_t)2 * B + 2);
  std::vector<uint32_t> toks((size_t)8 * B + 64);
  int n = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    n = be.poll_msgs(be.self, msgs.data(), (int)msgs.size(), toks.data(), (int)toks.size());
    if (n < 0) { w->err = be.last_error ? be.last_error(be.self) : "backend error"; return n; }
    size_t need = 0;
    for (int i = 0; i < n; ++i)
      if (msgs[i].kind == DSM_MSG_WORD) {
        if (msgs[i].tokens_offset < 0 || msgs[i].n_tokens < 0) { w->err = "backend returned a malformed Word message"; return DSM_ERR_STATE; }
        need = std::max(need, (size_t)msgs[i].tokens_offset + (size_t)msgs[i].n_tokens);
      }
    if (need <= toks.size()) break;
    if (attempt == 1) { w->err = "backend token list changed between two polls"; return DSM_ERR_STATE; }
    toks.assign(need, 0);
  }
  // Word.logprob / min_logprob: the engine's per-token scores, parallel to toks.  Scores switched off behind the worker's back:
  // the words go out without the two keys.
  std::vector<float> lps;
  bool have_lps = false;
#ifndef DSM_HOST_ONLY
  if (w->word_scores && w->eng) {
    lps.assign(toks.size(), 0.0f);
    const int got = dsm_asr_poll_word_scores(w->eng, lps.data(), (int)lps.size());
    have_lps = got >= 0;
    if (have_lps) lps.resize((size_t)got);
  }
#endif
  for (int i = 0; i < n; ++i) {
    const dsm_asr_msg& am = msgs[i];
    dsm_out_msg om{};
    if ((am.kind == DSM_MSG_WORD || am.kind == DSM_MSG_END_WORD) && (am.batch_idx < 0 || am.batch_idx >= B)) {
      w->err = "backend message for a slot outside the batch";
      return DSM_ERR_STATE;
    }
    if (am.kind == DSM_MSG_WORD) {
      std::string textbuf;
      const uint32_t* tk = toks.data() + am.tokens_offset;
      if (w->detok) {  // text_tokenizer.decode_piece_ids(&tokens) — :667
        std::vector<char> tmp(64 + 32 * (size_t)am.n_tokens);
        int k = w->detok(w->detok_user, tk, am.n_tokens, tmp.data(), tmp.size());
        if (k < 0) { w->err = "detokenizer failed"; return DSM_ERR_STATE; }
        textbuf.assign(tmp.data(), (size_t)k);
      } else if (w->tok) {  // the native tokenizer; an id outside the model ends the step like the `?` at :667
        std::string derr;
        if (dsm_spm_ns::decode(w->tok->m, tk, (size_t)am.n_tokens, textbuf, derr)) { w->err = "Word of slot " + std::to_string(am.batch_idx) + ": " + derr; return DSM_ERR_STATE; }
      } else {  // neither a callback nor a model: the piece ids themselves
        for (int j = 0; j < am.n_tokens; ++j) textbuf += (j ? " " : "") + std::to_string(tk[j]);
      }
      om.kind = DSM_OUT_WORD; om.text = textbuf.c_str(); om.time = am.time;
      double word_lp[2] = {0.0, 0.0};  // mean and minimum of the word's token logprobs; left out when one was not recorded (NaN)
      bool scored = have_lps && am.n_tokens > 0 && (size_t)am.tokens_offset + (size_t)am.n_tokens <= lps.size();
      for (int j = 0; scored && j < am.n_tokens; ++j) {
        const double v = (double)lps[(size_t)am.tokens_offset + (size_t)j];
        if (v != v) { scored = false; break; }
        word_lp[0] += v;
        word_lp[1] = j == 0 || v < word_lp[1] ? v : word_lp[1];
      }
      if (scored) word_lp[0] /= (double)am.n_tokens;
      w->send(am.batch_idx, om, ref_ids[am.batch_idx], scored ? word_lp : nullptr);
    } else if (am.kind == DSM_MSG_END_WORD) {
      om.kind = DSM_OUT_ENDWORD; om.time = am.time;
      w->send(am.batch_idx, om, ref_ids[am.batch_idx]);
    } else {  // Step: fan out to every active slot with that slot's head probabilities (:684-701)
      for (int b = 0; b < B; ++b) {
        if (!mask[b]) continue;
        float p[DSM_MAX_EXTRA_HEADS];
        for (int h = 0; h < nh; ++h) p[h] = prs[(size_t)h * B + b];
        om.kind = DSM_OUT_STEP; om.step_idx = (uint64_t)am.step_idx; om.prs = p; om.n_prs = (size_t)nh;
        om.buffered_pcm = pm.buffered[b];  // :693 reads ch.data.len() when post_process runs — under the reference's threads whatever the encoder
                                           // thread has queued by then; the snapshot from when this frame was cut is what one thread sees, and is deterministic
        w->send(b, om, ref_ids[b]);
      }
    }
  }
  while (!w->markers.empty() && w->markers.top().step_idx <= w->model_step_idx) {  // :702-716
    const WMarker m = w->markers.top();
    w->markers.pop();
    dsm_out_msg om{};
    om.kind = DSM_OUT_MARKER; om.id = m.marker_id;
    w->send(m.batch_idx, om, m.channel_id);
  }
  return 1;
}

// One pass of all three loops on the calling thread: encode, then the model step and post-processing of that same frame
// (everything queued earlier by dsm_worker_step_encode goes first).  1 a step ran, 0 idle, <0 backend error.
int dsm_worker_step(dsm_worker* w) {
  if (!w) return DSM_ERR_INVALID;
  const int produced = dsm_worker_step_encode(w);
  if (produced < 0) return produced;
  int ran = 0;
  for (;;) {
    const int rc = dsm_worker_step_model(w);
    if (rc < 0) return rc;
    if (rc == 0) break;
    ran = 1;
  }
  return ran;
}

}  // extern "C"
