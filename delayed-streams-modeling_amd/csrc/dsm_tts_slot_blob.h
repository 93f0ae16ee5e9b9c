// dsm_tts_slot_blob.h — the blob a TTS generation's slot state travels in: format, writer and checked reader.  The engine calls
// that fill and consume it are not in the library yet; dsm_tts_slot_blob_info is the reader's entry point.
//
// Host only and header only, like dsm_slot_blob.h (whose conventions it keeps): the engine includes it, and so do the CPU tests
// and the sanitizer program, which never see a device.  Everything is little-endian; every read goes through memcpy with the
// bounds checked first.  The magic is its own: the STT calls refuse a TTS blob with "bad magic", and the other way round.
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
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dsm.h"

namespace dsm_tts_slot_blob {

constexpr uint32_t kMagic = 0x42535444u;
constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 48;
constexpr size_t kItemBytes = 64;
constexpr uint32_t kMaxSlots = 1u << 20;     // far above any batch size; keeps n * slot_bytes inside 64 bits
constexpr uint32_t kMaxSigWords = 1u << 12;
constexpr uint32_t kMaxSlices = 1u << 10;    // a frame of 1024 codebooks is no frame
constexpr uint32_t kMaxSteps = 1u << 20;     // rows of a token table: 23 hours of audio at 12.5 Hz
constexpr uint32_t kMaxQueue = 1u << 20;     // tokens, and words, of a request's queue (the engine's is max_steps + acoustic_delay)
constexpr uint64_t kMaxSlotBytes = 1ull << 40;
constexpr uint32_t kReqActive = 1u, kReqClosed = 2u, kReqBosDone = 4u;

inline uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

struct Header {
  uint32_t magic = 0, version = 0, n_slots = 0, flags = 0, sig_words = 0, slices = 0;
  uint64_t host_bytes = 0, slot_bytes = 0, total_bytes = 0;
  uint64_t sig_offset() const { return kHeaderBytes; }
  uint64_t host_offset() const { return kHeaderBytes + align16(4ull * sig_words); }
  uint64_t payload_offset() const { return host_offset() + host_bytes; }
};

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

inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
template <typename T>
inline void put(std::vector<uint8_t>& out, T v) {
  const size_t at = out.size();
  out.resize(at + sizeof(T));
  memcpy(&out[at], &v, sizeof(T));
}
inline void pad16(std::vector<uint8_t>& out) { out.resize((size_t)align16(out.size()), 0); }

// The header, checked against the buffer: magic, version, counts within their limits, sizes multiples of 16 and consistent
// with each other and with `len` (a buffer shorter than total_bytes is a truncated blob).  0 or DSM_ERR_INVALID with *err.
inline int read_header(const void* buf, size_t len, Header* h, std::string* err) {
  auto fail = [&](const char* m) { if (err) *err = m; return (int)DSM_ERR_INVALID; };
  if (!buf || !h) return fail("tts slot blob: null argument");
  if (len < kHeaderBytes) return fail("tts slot blob: shorter than its header");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  h->magic = rd32(p); h->version = rd32(p + 4); h->n_slots = rd32(p + 8); h->flags = rd32(p + 12);
  h->sig_words = rd32(p + 16); h->slices = rd32(p + 20);
  h->host_bytes = rd64(p + 24); h->slot_bytes = rd64(p + 32); h->total_bytes = rd64(p + 40);
  if (h->magic != kMagic) return fail("tts slot blob: bad magic");
  if (h->version != kVersion) return fail("tts slot blob: unsupported version");
  if (h->n_slots < 1 || h->n_slots > kMaxSlots) return fail("tts slot blob: slot count out of range");
  if (h->sig_words > kMaxSigWords) return fail("tts slot blob: signature too long");
  if (h->flags & ~(uint32_t)DSM_TTS_SLOT_BLOB_HAS_MIMI_DEC) return fail("tts slot blob: unknown flags");
  if (h->slices < 1 || h->slices > kMaxSlices) return fail("tts slot blob: slice count out of range");
  if (h->slot_bytes % 16 || h->slot_bytes > kMaxSlotBytes) return fail("tts slot blob: bad payload size per slot");
  // per slot at most: the fixed part, kMaxSteps rows of 1 + S tokens, 2 * kMaxQueue queue words — below 2^34 bytes, times 2^20 slots
  const uint64_t item_max = kItemBytes + 4ull * kMaxSteps * (1 + (uint64_t)h->slices) + 8ull * kMaxQueue;
  if (h->host_bytes % 16 || h->host_bytes > (uint64_t)h->n_slots * item_max + 16) return fail("tts slot blob: bad host section size");
  if (h->host_bytes < (uint64_t)kItemBytes * h->n_slots) return fail("tts slot blob: host section too short for its slots");
  const uint64_t total = h->payload_offset() + (uint64_t)h->n_slots * h->slot_bytes;  // < 2^61: no overflow
  if (h->total_bytes != total) return fail("tts slot blob: total size does not match its parts");
  if ((uint64_t)len < total) return fail("tts slot blob: truncated");
  return 0;
}

// The host section of a blob whose header read_header accepted.
inline int read_host(const void* buf, const Header& h, std::vector<HostItem>* out, std::string* err) {
  auto fail = [&](const char* m) { if (err) *err = m; return (int)DSM_ERR_INVALID; };
  const uint8_t* p = static_cast<const uint8_t*>(buf) + h.host_offset();
  uint64_t at = 0;
  const uint64_t end = h.host_bytes;
  out->clear();
  out->reserve(h.n_slots < 4096 ? h.n_slots : 4096);
  for (uint32_t i = 0; i < h.n_slots; ++i) {
    if (end - at < kItemBytes) return fail("tts slot blob: host section ends inside an item");
    HostItem it;
    it.step_idx = rd64(p + at);
    it.consecutive_pads = rd64(p + at + 8);
    it.samp_k = (int32_t)rd32(p + at + 16);
    it.cfg_on = rd32(p + at + 20);
    it.cond_on = rd32(p + at + 24);
    it.ca_len[0] = rd32(p + at + 28);
    it.ca_len[1] = rd32(p + at + 32);
    it.req_flags = rd32(p + at + 36);
    it.req_status = (int32_t)rd32(p + at + 40);
    const uint32_t nw = rd32(p + at + 44), nt = rd32(p + at + 48);
    if (rd32(p + at + 52) || rd32(p + at + 56) || rd32(p + at + 60)) return fail("tts slot blob: reserved item words are not zero");
    at += kItemBytes;
    if (it.step_idx > kMaxSteps) return fail("tts slot blob: step index too large");
    if (it.cfg_on > 1 || it.cond_on > 1) return fail("tts slot blob: cfg_on / cond_on is not 0 or 1");
    if (it.req_flags & ~(kReqActive | kReqClosed | kReqBosDone)) return fail("tts slot blob: unknown request flags");
    if (nw > kMaxQueue || nt > kMaxQueue) return fail("tts slot blob: request queue too long");
    const uint64_t n_text = it.step_idx, n_audio = it.step_idx * h.slices;  // <= 2^30
    const uint64_t need = 4ull * (n_text + n_audio + nt + nw);
    if (end - at < need) return fail("tts slot blob: host section ends inside an item's tables");
    it.text_tokens.resize((size_t)n_text);
    for (uint64_t j = 0; j < n_text; ++j) it.text_tokens[(size_t)j] = rd32(p + at + 4 * j);
    at += 4 * n_text;
    it.audio_tokens.resize((size_t)n_audio);
    for (uint64_t j = 0; j < n_audio; ++j) it.audio_tokens[(size_t)j] = rd32(p + at + 4 * j);
    at += 4 * n_audio;
    it.q_tok.resize(nt);
    for (uint32_t j = 0; j < nt; ++j) it.q_tok[j] = rd32(p + at + 4ull * j);
    at += 4ull * nt;
    it.q_end.resize(nw);
    for (uint32_t j = 0; j < nw; ++j) it.q_end[j] = (int32_t)rd32(p + at + 4ull * j);
    at += 4ull * nw;
    out->push_back(std::move(it));
  }
  if (align16(at) != end) return fail("tts slot blob: host section length does not match its items");
  return 0;
}

// Header + signature + host section, appended to `out` (empty on entry); the device payload follows at out.size().
inline void write_front(std::vector<uint8_t>& out, uint32_t flags, uint32_t slices, const std::vector<uint32_t>& sig,
                        const std::vector<HostItem>& items, uint64_t slot_bytes) {
  std::vector<uint8_t> host;
  for (const HostItem& it : items) {
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
  pad16(host);
  put<uint32_t>(out, kMagic);
  put<uint32_t>(out, kVersion);
  put<uint32_t>(out, (uint32_t)items.size());
  put<uint32_t>(out, flags);
  put<uint32_t>(out, (uint32_t)sig.size());
  put<uint32_t>(out, slices);
  put<uint64_t>(out, (uint64_t)host.size());
  put<uint64_t>(out, slot_bytes);
  put<uint64_t>(out, kHeaderBytes + align16(4ull * sig.size()) + host.size() + (uint64_t)items.size() * slot_bytes);
  for (uint32_t w : sig) put<uint32_t>(out, w);
  pad16(out);
  out.insert(out.end(), host.begin(), host.end());
}

// dsm_tts_slot_blob_info: the header and the host section must both read cleanly.
inline int info(const void* buf, size_t len, struct dsm_tts_slot_blob_info* out, std::string* err) {
  Header h;
  if (int rc = read_header(buf, len, &h, err)) return rc;
  std::vector<HostItem> items;
  if (int rc = read_host(buf, h, &items, err)) return rc;
  if (out) {
    out->version = h.version;
    out->n_slots = h.n_slots;
    out->flags = h.flags;
    out->sig_words = h.sig_words;
    out->slices = h.slices;
    out->reserved = 0;
    out->host_bytes = h.host_bytes;
    out->slot_bytes = h.slot_bytes;
    out->total_bytes = h.total_bytes;
  }
  return 0;
}

}  // namespace dsm_tts_slot_blob
