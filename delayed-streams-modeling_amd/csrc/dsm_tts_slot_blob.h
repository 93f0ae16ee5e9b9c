// dsm_tts_slot_blob.h — the blob a TTS generation's slot state travels in: format, writer and checked reader.  The engine calls
// that fill and consume it are not in the library yet; dsm_tts_slot_blob_info is the reader's entry point.
//
// Host only and header only.  The container — header, signature, host-section frame, sizes, every bound on them — is dsm_blob
// of dsm_slot_blob.h, shared with the STT slot blob; this file is the TTS kind: its magic, its flag, `slices` at offset 20 and the
// host item with its codec.  The magic is its own: the STT calls refuse a TTS blob with "bad magic", and the other way round.
//
//   offset  0  u32 magic        "DTSB" (0x42535444)
//           4  u32 version      1
//           8  u32 n_slots      >= 1
//          12  u32 flags        bit 0: the payload carries the slot's Mimi decode state (DSM_TTS_SLOT_BLOB_HAS_MIMI_DEC)
//          16  u32 sig_words    length of the signature in 32-bit words
//          20  u32 slices       S = dep_num_slices: tokens per row of a slot's audio-token table (1 .. kMaxSlices)
//          24  u64 host_bytes   length of the host section (a multiple of 16)
//          32  u64 slot_bytes   device payload per slot (a multiple of 16)
//          40  u64 total_bytes  48 + align16(4 * sig_words) + host_bytes + n_slots * slot_bytes
//          48  signature        sig_words x u32, zero padded to 16 bytes: every configuration field that fixes a size or a
//                               meaning (the engine lists them where it builds it)
//              host section     per slot, in order, a fixed part of 64 bytes:
//                                 u64 step_idx, u64 consecutive_pads, i32 samp_k, u32 cfg_on, u32 cond_on, u32 ca_len[2],
//                                 u32 req_flags (bit 0 active, 1 closed, 2 bos_done), i32 req_status, u32 n_words, u32 n_tok,
//                                 3 x u32 reserved (0)
//                               then step_idx x u32 text tokens, step_idx x S x u32 audio tokens (the rows of the token tables
//                               that a step has written), n_tok x u32 queue tokens and n_words x i32 word ends (the used prefix
//                               of the request's word queue); the whole section zero padded to 16
//              device payload   n_slots x slot_bytes; inside a slot every section starts on a 16-byte boundary, the gaps
//                               are zero.  The section list is the importer's own (it never reads an offset from the blob).
#pragma once
#include "dsm_slot_blob.h"

namespace dsm_tts_slot_blob {

using namespace dsm_blob;
constexpr uint32_t kMagic = 0x42535444u;
constexpr size_t kItemBytes = 64;
constexpr uint32_t kMaxSlices = 1u << 10;    // a frame of 1024 codebooks is no frame
constexpr uint32_t kMaxSteps = 1u << 20;     // rows of a token table: 23 hours of audio at 12.5 Hz
constexpr uint32_t kMaxQueue = 1u << 20;     // tokens, and words, of a request's queue (the engine's is max_steps + acoustic_delay)
constexpr uint32_t kReqActive = 1u, kReqClosed = 2u, kReqBosDone = 4u;

struct HostItem {  // dsm_tts::Item, the host mirrors of the slot and its request (dsm_tts::ReqHost with the queue's used prefix)
  uint64_t step_idx = 0, consecutive_pads = 0;
  int32_t samp_k = 0;
  uint32_t cfg_on = 0, cond_on = 0, ca_len[2] = {0, 0};
  uint32_t req_flags = 0;
  int32_t req_status = 0;
  std::vector<uint32_t> text_tokens, audio_tokens;  // [step_idx], [step_idx][S]
  std::vector<uint32_t> q_tok;                      // [n_tok]
  std::vector<int32_t> q_end;                       // [n_words]
};

struct Tts {
  using Item = HostItem;
  static constexpr Kind kind{kMagic, DSM_TTS_SLOT_BLOB_HAS_MIMI_DEC, "tts slot blob", kItemBytes};
  // aux is `slices`, range-checked; an item's reserved words must be 0 (decode_item), unlike the STT kind's
  static const char* check_aux(uint32_t slices, uint64_t* item_max) {
    if (slices < 1 || slices > kMaxSlices) return "slice count out of range";
    // per slot at most: the fixed part, kMaxSteps rows of 1 + S tokens, 2 * kMaxQueue queue words
    *item_max = kItemBytes + 4ull * kMaxSteps * (1 + (uint64_t)slices) + 8ull * kMaxQueue;
    return nullptr;
  }
  static const char* decode_item(Cursor& c, const Header& h, HostItem* it) {
    it->step_idx = c.u64();
    it->consecutive_pads = c.u64();
    it->samp_k = (int32_t)c.u32();
    it->cfg_on = c.u32();
    it->cond_on = c.u32();
    it->ca_len[0] = c.u32();
    it->ca_len[1] = c.u32();
    it->req_flags = c.u32();
    it->req_status = (int32_t)c.u32();
    const uint32_t nw = c.u32(), nt = c.u32();
    if (c.u32() | c.u32() | c.u32()) return "reserved item words are not zero";
    if (it->step_idx > kMaxSteps) return "step index too large";
    if (it->cfg_on > 1 || it->cond_on > 1) return "cfg_on / cond_on is not 0 or 1";
    if (it->req_flags & ~(kReqActive | kReqClosed | kReqBosDone)) return "unknown request flags";
    if (nw > kMaxQueue || nt > kMaxQueue) return "request queue too long";
    const uint64_t n_text = it->step_idx, n_audio = it->step_idx * h.aux;  // <= 2^30
    if (!c.has(4ull * (n_text + n_audio + nt + nw))) return "host section ends inside an item's tables";
    c.words(n_text, &it->text_tokens);
    c.words(n_audio, &it->audio_tokens);
    c.words(nt, &it->q_tok);
    c.words(nw, &it->q_end);
    return nullptr;
  }
  static void encode_item(std::vector<uint8_t>& host, const HostItem& it) {
    put<uint64_t>(host, it.step_idx);
    put<uint64_t>(host, it.consecutive_pads);
    put<int32_t>(host, it.samp_k);
    put<uint32_t>(host, it.cfg_on);
    put<uint32_t>(host, it.cond_on);
    put<uint32_t>(host, it.ca_len[0]);
    put<uint32_t>(host, it.ca_len[1]);
    put<uint32_t>(host, it.req_flags);
    put<int32_t>(host, it.req_status);
    put<uint32_t>(host, (uint32_t)it.q_end.size());
    put<uint32_t>(host, (uint32_t)it.q_tok.size());
    for (int i = 0; i < 3; ++i) put<uint32_t>(host, 0);
    for (uint32_t t : it.text_tokens) put<uint32_t>(host, t);
    for (uint32_t t : it.audio_tokens) put<uint32_t>(host, t);
    for (uint32_t t : it.q_tok) put<uint32_t>(host, t);
    for (int32_t t : it.q_end) put<int32_t>(host, t);
  }
};

inline int read_header(const void* buf, size_t len, Header* h, std::string* err) { return dsm_blob::read_header<Tts>(buf, len, h, err); }
inline int read_host(const void* buf, const Header& h, std::vector<HostItem>* out, std::string* err) {
  return dsm_blob::read_host<Tts>(buf, h, out, err);
}
inline void write_front(std::vector<uint8_t>& out, uint32_t flags, uint32_t slices, const std::vector<uint32_t>& sig,
                        const std::vector<HostItem>& items, uint64_t slot_bytes) {
  dsm_blob::write_front<Tts>(out, flags, slices, sig, items, slot_bytes);
}
inline int info(const void* buf, size_t len, struct dsm_tts_slot_blob_info* out, std::string* err) {
  Header h;
  const int rc = dsm_blob::info<Tts>(buf, len, out, err, &h);
  if (!rc && out) {
    out->slices = h.aux;
    out->reserved = 0;
  }
  return rc;
}

}  // namespace dsm_tts_slot_blob
