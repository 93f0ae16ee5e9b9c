// dsm_slot_blob.h — the slot-state blob of dsm_asr_export_slots / dsm_asr_import_slots: format, writer and checked reader.
// The container (namespace dsm_blob below: header, signature, host-section frame, payload sizes) is shared with the TTS slot
// blob (dsm_tts_slot_blob.h), which differs in its magic, its flag, the word at offset 20 and its host items; what is STT —
// the host item and its codec — is namespace dsm_slot_blob at the end of this file.
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

// ---- the container.  A kind K supplies: K::kind, K::Item, K::check_aux, K::decode_item, K::encode_item (see Stt below) ----
namespace dsm_blob {

constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 48;
constexpr uint32_t kMaxSlots = 1u << 20;  // far above any batch size; keeps n * slot_bytes inside 64 bits
constexpr uint32_t kMaxSigWords = 1u << 12;
constexpr uint64_t kMaxSlotBytes = 1ull << 40;

inline uint64_t align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }
inline uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
template <typename T>
inline void put(std::vector<uint8_t>& out, T v) {
  const size_t at = out.size();
  out.resize(at + sizeof(T));
  memcpy(&out[at], &v, sizeof(T));
}
inline void pad16(std::vector<uint8_t>& out) { out.resize((size_t)align16(out.size()), 0); }

struct Header {
  uint32_t magic = 0, version = 0, n_slots = 0, flags = 0, sig_words = 0, aux = 0;  // aux: the kind's word at offset 20
  uint64_t host_bytes = 0, slot_bytes = 0, total_bytes = 0;
  uint64_t sig_offset() const { return kHeaderBytes; }
  uint64_t host_offset() const { return kHeaderBytes + align16(4ull * sig_words); }
  uint64_t payload_offset() const { return host_offset() + host_bytes; }
};

struct Kind {
  uint32_t magic, known_flags;
  const char* prefix;   // of every message
  uint64_t item_bytes;  // the fixed part of a host item
};
inline int fail(const Kind& k, std::string* err, const char* m) {
  if (err) *err = std::string(k.prefix) + ": " + m;
  return (int)DSM_ERR_INVALID;
}

// What is left of the host section.  take() — n bytes or nothing — is the only way at the bytes; a codec asks has() first
// where running short has a message of its own.
struct Cursor {
  const uint8_t* p;
  uint64_t left;
  bool has(uint64_t n) const { return left >= n; }
  const uint8_t* take(uint64_t n) {
    if (left < n) return nullptr;
    const uint8_t* q = p;
    p += n;
    left -= n;
    return q;
  }
  uint32_t u32() { const uint8_t* q = take(4); return q ? rd32(q) : 0; }
  uint64_t u64() { const uint8_t* q = take(8); return q ? rd64(q) : 0; }
  template <typename T>
  void words(uint64_t n, std::vector<T>* out) {  // n x 32 bits; out stays empty when they are not there
    const uint8_t* q = take(4 * n);
    if (!q) return;
    out->resize((size_t)n);
    for (uint64_t j = 0; j < n; ++j) (*out)[(size_t)j] = (T)rd32(q + 4 * j);
  }
};

// The header, checked against the buffer: magic, version, counts within their limits, sizes multiples of 16 and consistent
// with each other and with `len` (a buffer shorter than total_bytes is a truncated blob).  0 or DSM_ERR_INVALID with *err.
template <class K>
inline int read_header(const void* buf, size_t len, Header* h, std::string* err) {
  const Kind& k = K::kind;
  if (!buf || !h) return fail(k, err, "null argument");
  if (len < kHeaderBytes) return fail(k, err, "shorter than its header");
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  h->magic = rd32(p); h->version = rd32(p + 4); h->n_slots = rd32(p + 8); h->flags = rd32(p + 12);
  h->sig_words = rd32(p + 16); h->aux = rd32(p + 20);
  h->host_bytes = rd64(p + 24); h->slot_bytes = rd64(p + 32); h->total_bytes = rd64(p + 40);
  if (h->magic != k.magic) return fail(k, err, "bad magic");
  if (h->version != kVersion) return fail(k, err, "unsupported version");
  if (h->n_slots < 1 || h->n_slots > kMaxSlots) return fail(k, err, "slot count out of range");
  if (h->sig_words > kMaxSigWords) return fail(k, err, "signature too long");
  if (h->flags & ~k.known_flags) return fail(k, err, "unknown flags");
  uint64_t item_max = 0;  // of one slot's part of the host section; below 2^34 bytes, times 2^20 slots
  if (const char* m = K::check_aux(h->aux, &item_max)) return fail(k, err, m);
  if (h->slot_bytes % 16 || h->slot_bytes > kMaxSlotBytes) return fail(k, err, "bad payload size per slot");
  if (h->host_bytes % 16 || h->host_bytes > (uint64_t)h->n_slots * item_max + 16) return fail(k, err, "bad host section size");
  if (h->host_bytes < k.item_bytes * h->n_slots) return fail(k, err, "host section too short for its slots");
  const uint64_t total = h->payload_offset() + (uint64_t)h->n_slots * h->slot_bytes;  // < 2^61: no overflow
  if (h->total_bytes != total) return fail(k, err, "total size does not match its parts");
  if ((uint64_t)len < total) return fail(k, err, "truncated");
  return 0;
}

// The host section of a blob whose header read_header accepted.
template <class K>
inline int read_host(const void* buf, const Header& h, std::vector<typename K::Item>* out, std::string* err) {
  Cursor c{static_cast<const uint8_t*>(buf) + h.host_offset(), h.host_bytes};
  out->clear();
  out->reserve(h.n_slots < 4096 ? h.n_slots : 4096);
  for (uint32_t i = 0; i < h.n_slots; ++i) {
    if (!c.has(K::kind.item_bytes)) return fail(K::kind, err, "host section ends inside an item");
    typename K::Item it;
    if (const char* m = K::decode_item(c, h, &it)) return fail(K::kind, err, m);
    out->push_back(std::move(it));
  }
  if (align16(h.host_bytes - c.left) != h.host_bytes) return fail(K::kind, err, "host section length does not match its items");
  return 0;
}

// Header + signature + host section, appended to `out` (empty on entry); the device payload follows at out.size().
template <class K>
inline void write_front(std::vector<uint8_t>& out, uint32_t flags, uint32_t aux, const std::vector<uint32_t>& sig,
                        const std::vector<typename K::Item>& items, uint64_t slot_bytes) {
  std::vector<uint8_t> host;
  for (const typename K::Item& it : items) K::encode_item(host, it);
  pad16(host);
  put<uint32_t>(out, K::kind.magic);
  put<uint32_t>(out, kVersion);
  put<uint32_t>(out, (uint32_t)items.size());
  put<uint32_t>(out, flags);
  put<uint32_t>(out, (uint32_t)sig.size());
  put<uint32_t>(out, aux);
  put<uint64_t>(out, (uint64_t)host.size());
  put<uint64_t>(out, slot_bytes);
  put<uint64_t>(out, kHeaderBytes + align16(4ull * sig.size()) + host.size() + (uint64_t)items.size() * slot_bytes);
  for (uint32_t w : sig) put<uint32_t>(out, w);
  pad16(out);
  out.insert(out.end(), host.begin(), host.end());
}

// The *_blob_info calls: the header and the host section must both read cleanly; fills the fields both info structs have.
template <class K, class Info>
inline int info(const void* buf, size_t len, Info* out, std::string* err, Header* h) {
  if (int rc = read_header<K>(buf, len, h, err)) return rc;
  std::vector<typename K::Item> items;
  if (int rc = read_host<K>(buf, *h, &items, err)) return rc;
  if (out) {
    out->version = h->version;
    out->n_slots = h->n_slots;
    out->flags = h->flags;
    out->sig_words = h->sig_words;
    out->host_bytes = h->host_bytes;
    out->slot_bytes = h->slot_bytes;
    out->total_bytes = h->total_bytes;
  }
  return 0;
}

}  // namespace dsm_blob

// ---- the STT kind ----
namespace dsm_slot_blob {

using namespace dsm_blob;
constexpr uint32_t kMagic = 0x424C5344u;
constexpr uint32_t kMaxWordTokens = 1u << 16;  // a word of 65536 tokens is no word

struct HostItem {  // what HostItem of the engine carries, plus the slot's per-side flags
  uint64_t step_idx = 0;
  double last_stop_time = 0.0;
  uint32_t unended_word = 0, side_flags = 0;
  std::vector<uint32_t> word_tokens;
};

struct Stt {
  using Item = HostItem;
  static constexpr Kind kind{kMagic, DSM_SLOT_BLOB_HAS_MODEL_MIMI, "slot blob", 32};
  // aux is "reserved, 0" and written as 0, but a non-zero value is not refused (nor is an item's reserved word): as the format shipped
  static const char* check_aux(uint32_t, uint64_t* item_max) {
    *item_max = 32 + 4ull * kMaxWordTokens;
    return nullptr;
  }
  static const char* decode_item(Cursor& c, const Header&, HostItem* it) {
    it->step_idx = c.u64();
    const uint64_t t = c.u64();
    memcpy(&it->last_stop_time, &t, 8);
    it->unended_word = c.u32();
    it->side_flags = c.u32();
    const uint32_t nt = c.u32();
    c.u32();
    if (it->unended_word > 1) return "unended_word is not 0 or 1";
    if (it->side_flags & ~3u) return "unknown side flags";
    if (nt > kMaxWordTokens) return "word too long";
    if (!c.has(4ull * nt)) return "host section ends inside a word";
    c.words(nt, &it->word_tokens);
    return nullptr;
  }
  static void encode_item(std::vector<uint8_t>& host, const HostItem& it) {
    put<uint64_t>(host, it.step_idx);
    put<double>(host, it.last_stop_time);
    put<uint32_t>(host, it.unended_word);
    put<uint32_t>(host, it.side_flags);
    put<uint32_t>(host, (uint32_t)it.word_tokens.size());
    put<uint32_t>(host, 0);
    for (uint32_t t : it.word_tokens) put<uint32_t>(host, t);
  }
};

inline int read_header(const void* buf, size_t len, Header* h, std::string* err) { return dsm_blob::read_header<Stt>(buf, len, h, err); }
inline int read_host(const void* buf, const Header& h, std::vector<HostItem>* out, std::string* err) {
  return dsm_blob::read_host<Stt>(buf, h, out, err);
}
inline void write_front(std::vector<uint8_t>& out, uint32_t flags, const std::vector<uint32_t>& sig, const std::vector<HostItem>& items,
                        uint64_t slot_bytes) {
  dsm_blob::write_front<Stt>(out, flags, 0, sig, items, slot_bytes);
}
inline int info(const void* buf, size_t len, struct dsm_slot_blob_info* out, std::string* err) {
  Header h;
  return dsm_blob::info<Stt>(buf, len, out, err, &h);
}

}  // namespace dsm_slot_blob
