// dsm_slot_blob.h — the slot-state blob of dsm_asr_export_slots / dsm_asr_import_slots: format, writer and checked reader.
//
// Host only and header only (no HIP, like dsm_spm.h): the engine includes it, and so do the CPU tests and the sanitizer
// program, which never see a device.  Everything is little-endian; every read goes through memcpy with the bounds checked first.
//
//   offset  0  u32 magic        "DSLB" (0x424C5344)
//           4  u32 version      1
//           8  u32 n_slots      >= 1
//          12  u32 flags        bit 0: the payload carries the model-side Mimi (DSM_SLOT_BLOB_HAS_MODEL_MIMI)
//          16  u32 sig_words    length of the signature in 32-bit words
//          20  u32 reserved     0
//          24  u64 host_bytes   length of the host section (a multiple of 16)
//          32  u64 slot_bytes   device payload per slot (a multiple of 16)
//          40  u64 total_bytes  48 + align16(4 * sig_words) + host_bytes + n_slots * slot_bytes
//          48  signature        sig_words x u32, zero padded to 16 bytes: every configuration field that fixes a size or a
//                               meaning (the engine lists them where it builds it)
//              host section     per slot, in order:  u64 step_idx, f64 last_stop_time, u32 unended_word, u32 side_flags,
//                               u32 n_word_tokens, u32 reserved (0), n_word_tokens x u32; the whole section zero padded to 16
//                               side_flags bit s: the slot's state on Mimi side s (0 encoder thread, 1 model side) is that of
//                               a module whose first call has not run (DSM_SLOT_SIDE_PRISTINE0 << s)
//              device payload   n_slots x slot_bytes; inside a slot every section starts on a 16-byte boundary, the gaps
//                               are zero.  The section list is the importer's own (it never reads an offset from the blob).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dsm.h"

namespace dsm_slot_blob {

constexpr uint32_t kMagic = 0x424C5344u;
constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 48;
constexpr uint32_t kMaxSlots = 1u << 20;       // far above any batch size; keeps n * slot_bytes inside 64 bits
constexpr uint32_t kMaxSigWords = 1u << 12;
constexpr uint32_t kMaxWordTokens = 1u << 16;  // a word of 65536 tokens is no word
constexpr uint64_t kMaxSlotBytes = 1ull << 40;

inline uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

struct Header {
  uint32_t magic = 0, version = 0, n_slots = 0, flags = 0, sig_words = 0, reserved = 0;
  uint64_t host_bytes = 0, slot_bytes = 0, total_bytes = 0;
  uint64_t sig_offset() const { return kHeaderBytes; }
  uint64_t host_offset() const { return kHeaderBytes + align16(4ull * sig_words); }
  uint64_t payload_offset() const { return host_offset() + host_bytes; }
};

struct HostItem {  // what HostItem of the engine carries, plus the slot's per-side flags
  uint64_t step_idx = 0;
  double last_stop_time = 0.0;
  uint32_t unended_word = 0, side_flags = 0;
  std::vector<uint32_t> word_tokens;
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
  if (!buf || !h) return fail("slot blob: null argument");
  if (len < kHeaderBytes) return fail("slot blob: shorter than its header");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  h->magic = rd32(p); h->version = rd32(p + 4); h->n_slots = rd32(p + 8); h->flags = rd32(p + 12);
  h->sig_words = rd32(p + 16); h->reserved = rd32(p + 20);
  h->host_bytes = rd64(p + 24); h->slot_bytes = rd64(p + 32); h->total_bytes = rd64(p + 40);
  if (h->magic != kMagic) return fail("slot blob: bad magic");
  if (h->version != kVersion) return fail("slot blob: unsupported version");
  if (h->n_slots < 1 || h->n_slots > kMaxSlots) return fail("slot blob: slot count out of range");
  if (h->sig_words > kMaxSigWords) return fail("slot blob: signature too long");
  if (h->flags & ~(uint32_t)DSM_SLOT_BLOB_HAS_MODEL_MIMI) return fail("slot blob: unknown flags");
  if (h->slot_bytes % 16 || h->slot_bytes > kMaxSlotBytes) return fail("slot blob: bad payload size per slot");
  if (h->host_bytes % 16 || h->host_bytes > (uint64_t)h->n_slots * (32 + 4ull * kMaxWordTokens) + 16)
    return fail("slot blob: bad host section size");
  if (h->host_bytes < 32ull * h->n_slots) return fail("slot blob: host section too short for its slots");
  const uint64_t total = h->payload_offset() + (uint64_t)h->n_slots * h->slot_bytes;  // < 2^61: no overflow
  if (h->total_bytes != total) return fail("slot blob: total size does not match its parts");
  if ((uint64_t)len < total) return fail("slot blob: truncated");
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
    if (end - at < 32) return fail("slot blob: host section ends inside an item");
    HostItem it;
    it.step_idx = rd64(p + at);
    memcpy(&it.last_stop_time, p + at + 8, 8);
    it.unended_word = rd32(p + at + 16);
    it.side_flags = rd32(p + at + 20);
    const uint32_t nt = rd32(p + at + 24);
    at += 32;
    if (it.unended_word > 1) return fail("slot blob: unended_word is not 0 or 1");
    if (it.side_flags & ~3u) return fail("slot blob: unknown side flags");
    if (nt > kMaxWordTokens) return fail("slot blob: word too long");
    if (end - at < 4ull * nt) return fail("slot blob: host section ends inside a word");
    it.word_tokens.resize(nt);
    for (uint32_t j = 0; j < nt; ++j) it.word_tokens[j] = rd32(p + at + 4ull * j);
    at += 4ull * nt;
    out->push_back(std::move(it));
  }
  if (align16(at) != end) return fail("slot blob: host section length does not match its items");
  return 0;
}

// Header + signature + host section, appended to `out` (empty on entry); the device payload follows at out.size().
inline void write_front(std::vector<uint8_t>& out, uint32_t flags, const std::vector<uint32_t>& sig,
                        const std::vector<HostItem>& items, uint64_t slot_bytes) {
  std::vector<uint8_t> host;
  for (const HostItem& it : items) {
    put<uint64_t>(host, it.step_idx);
    put<double>(host, it.last_stop_time);
    put<uint32_t>(host, it.unended_word);
    put<uint32_t>(host, it.side_flags);
    put<uint32_t>(host, (uint32_t)it.word_tokens.size());
    put<uint32_t>(host, 0);
    for (uint32_t t : it.word_tokens) put<uint32_t>(host, t);
  }
  pad16(host);
  put<uint32_t>(out, kMagic);
  put<uint32_t>(out, kVersion);
  put<uint32_t>(out, (uint32_t)items.size());
  put<uint32_t>(out, flags);
  put<uint32_t>(out, (uint32_t)sig.size());
  put<uint32_t>(out, 0);
  put<uint64_t>(out, (uint64_t)host.size());
  put<uint64_t>(out, slot_bytes);
  put<uint64_t>(out, kHeaderBytes + align16(4ull * sig.size()) + host.size() + (uint64_t)items.size() * slot_bytes);
  for (uint32_t w : sig) put<uint32_t>(out, w);
  pad16(out);
  out.insert(out.end(), host.begin(), host.end());
}

// dsm_slot_blob_info: the header and the host section must both read cleanly.
inline int info(const void* buf, size_t len, struct dsm_slot_blob_info* out, std::string* err) {
  Header h;
  if (int rc = read_header(buf, len, &h, err)) return rc;
  std::vector<HostItem> items;
  if (int rc = read_host(buf, h, &items, err)) return rc;
  if (out) {
    out->version = h.version;
    out->n_slots = h.n_slots;
    out->flags = h.flags;
    out->sig_words = h.sig_words;
    out->host_bytes = h.host_bytes;
    out->slot_bytes = h.slot_bytes;
    out->total_bytes = h.total_bytes;
  }
  return 0;
}

}  // namespace dsm_slot_blob
