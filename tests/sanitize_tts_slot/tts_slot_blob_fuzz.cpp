// tts_slot_blob_fuzz — the TTS slot blob's header and host-section parser (csrc/dsm_tts_slot_blob.h) under AddressSanitizer +
// UBSan.  A stand-alone program: valid blobs are written with the header's own writer and must read back field for field; then
// seeded mutations (byte flips, 32- and 64-bit fields overwritten with edge values, truncations at every length class) go
// through dsm_tts_slot_blob::info, each copied into a heap buffer of exactly its length so that any read past the end is
// caught.  Every outcome must be a clean accept or a clean DSM_ERR_INVALID with a message.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_tts_slot_blob.h"

namespace sb = dsm_tts_slot_blob;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      fprintf(stderr, "tts_slot_blob_fuzz: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static std::vector<uint8_t> make_blob(uint32_t n, uint32_t sig_words, uint32_t slices, uint64_t slot_bytes, uint32_t flags,
                                      std::vector<sb::HostItem>* items_out) {
  std::vector<sb::HostItem> items(n);
  for (auto& it : items) {
    it.step_idx = rnd() % 12;
    it.consecutive_pads = rnd() % 5;
    it.samp_k = (int32_t)(rnd() % 3 == 0 ? 0 : 2 + rnd() % 250);
    it.cfg_on = (uint32_t)(rnd() & 1);
    it.cond_on = (uint32_t)(rnd() & 1);
    it.ca_len[0] = (uint32_t)(rnd() % 9);
    it.ca_len[1] = (uint32_t)(rnd() % 9);
    it.req_flags = (uint32_t)(rnd() & 7);
    it.req_status = (int32_t)(rnd() % 5);
    it.text_tokens.resize((size_t)it.step_idx);
    for (auto& t : it.text_tokens) t = (uint32_t)(rnd() % 8000);
    it.audio_tokens.resize((size_t)it.step_idx * slices);
    for (auto& t : it.audio_tokens) t = rnd() % 7 == 0 ? 0xFFFFFFFFu : (uint32_t)(rnd() % 2049);
    it.q_tok.resize(rnd() % 9);
    for (auto& t : it.q_tok) t = (uint32_t)(rnd() % 8000);
    it.q_end.resize(rnd() % 4);
    for (auto& t : it.q_end) t = (int32_t)(rnd() % 9);
  }
  std::vector<uint32_t> sig(sig_words);
  for (auto& w : sig) w = (uint32_t)(rnd() % 4096);
  std::vector<uint8_t> out;
  sb::write_front(out, flags, slices, sig, items, slot_bytes);
  const size_t front = out.size();
  out.resize(front + (size_t)n * slot_bytes);
  for (size_t i = front; i < out.size(); ++i) out[i] = (uint8_t)rnd();
  if (items_out) *items_out = items;
  return out;
}

// the parser on a heap copy of exactly `len` bytes
static int parse_exact(const uint8_t* data, size_t len, std::string* err) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
  if (len) memcpy(copy.get(), data, len);
  struct dsm_tts_slot_blob_info info;
  memset(&info, 0, sizeof info);
  const int rc = sb::info(copy.get(), len, &info, err);
  if (rc == 0) {  // what it accepted must hang together
    if (info.total_bytes > len || info.n_slots < 1 || info.slices < 1 || info.host_bytes % 16 || info.slot_bytes % 16) return 1;
    if (info.total_bytes != 48 + sb::align16(4ull * info.sig_words) + info.host_bytes + (uint64_t)info.n_slots * info.slot_bytes) return 1;
  } else if (rc != DSM_ERR_INVALID || err->empty()) {
    return 1;
  }
  return rc;
}

int main() {
  // ---- valid blobs read back ----
  for (int round = 0; round < 200; ++round) {
    const uint32_t n = 1 + (uint32_t)(rnd() % 5), sw = (uint32_t)(rnd() % 60), flags = (uint32_t)(rnd() & 1);
    const uint32_t slices = 1 + (uint32_t)(rnd() % 33);
    const uint64_t slot_bytes = 16 * (rnd() % 40);
    std::vector<sb::HostItem> items;
    const std::vector<uint8_t> blob = make_blob(n, sw, slices, slot_bytes, flags, &items);
    sb::Header h;
    std::string err;
    CHECK(sb::read_header(blob.data(), blob.size(), &h, &err) == 0);
    CHECK(h.n_slots == n && h.sig_words == sw && h.flags == flags && h.slices == slices && h.slot_bytes == slot_bytes &&
          h.total_bytes == blob.size());
    std::vector<sb::HostItem> back;
    CHECK(sb::read_host(blob.data(), h, &back, &err) == 0);
    CHECK(back.size() == items.size());
    for (size_t i = 0; i < items.size(); ++i) {
      const sb::HostItem &a = back[i], &b = items[i];
      CHECK(a.step_idx == b.step_idx && a.consecutive_pads == b.consecutive_pads && a.samp_k == b.samp_k && a.cfg_on == b.cfg_on &&
            a.cond_on == b.cond_on && a.ca_len[0] == b.ca_len[0] && a.ca_len[1] == b.ca_len[1] && a.req_flags == b.req_flags &&
            a.req_status == b.req_status && a.text_tokens == b.text_tokens && a.audio_tokens == b.audio_tokens &&
            a.q_tok == b.q_tok && a.q_end == b.q_end);
    }
    CHECK(parse_exact(blob.data(), blob.size(), &err) == 0);
  }
  // ---- mutations and truncations ----
  static const uint64_t edge[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 0xFFFFFull, 0x100000ull, 0x100001ull,
                                  0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x7FFFFFFFFFFFFFFFull,
                                  0x8000000000000000ull, 0xFFFFFFFFFFFFFFF0ull, 0xFFFFFFFFFFFFFFFFull};
  const size_t n_edge = sizeof edge / sizeof edge[0];
  long accepted = 0, refused = 0;
  for (int round = 0; round < 60000; ++round) {
    const uint32_t n = 1 + (uint32_t)(rnd() % 4), sw = (uint32_t)(rnd() % 24);
    std::vector<uint8_t> blob = make_blob(n, sw, 1 + (uint32_t)(rnd() % 9), 16 * (rnd() % 12), (uint32_t)(rnd() & 1), nullptr);
    const size_t front = 48 + (size_t)sb::align16(4ull * sw);
    const int kind = (int)(rnd() % 7);
    size_t len = blob.size();
    if (kind == 0) {  // truncate anywhere
      len = (size_t)(rnd() % (blob.size() + 1));
    } else if (kind == 1) {  // a header field takes an edge value
      static const int off32[] = {0, 4, 8, 12, 16, 20};
      static const int off64[] = {24, 32, 40};
      if (rnd() & 1) { const uint32_t v = (uint32_t)edge[rnd() % n_edge]; memcpy(&blob[(size_t)off32[rnd() % 6]], &v, 4); }
      else { const uint64_t v = edge[rnd() % n_edge]; memcpy(&blob[(size_t)off64[rnd() % 3]], &v, 8); }
    } else if (kind == 2) {  // a 32-bit word of the host section takes an edge value
      const size_t words = (blob.size() - front) / 4;
      if (words) { const uint32_t v = (uint32_t)edge[rnd() % n_edge]; memcpy(&blob[front + 4 * (size_t)(rnd() % words)], &v, 4); }
    } else if (kind == 3) {  // byte flips anywhere
      for (int f = 1 + (int)(rnd() % 8); f > 0; --f) blob[(size_t)(rnd() % blob.size())] ^= (uint8_t)(1u << (rnd() % 8));
    } else if (kind == 4) {  // header field and truncation together
      const uint64_t v = edge[rnd() % n_edge];
      memcpy(&blob[24 + 8 * (size_t)(rnd() % 3)], &v, 8);
      len = (size_t)(rnd() % (blob.size() + 1));
    } else if (kind == 5) {  // a count of the first item (step_idx, n_words, n_tok) takes an edge value
      static const int off[] = {0, 44, 48};
      const uint32_t v = (uint32_t)edge[rnd() % n_edge];
      memcpy(&blob[front + (size_t)off[rnd() % 3]], &v, 4);
    } else {  // sizes grown consistently, buffer not: total_bytes says more than there is
      uint64_t total;
      memcpy(&total, &blob[40], 8);
      total += 16 * (1 + rnd() % 4);
      memcpy(&blob[40], &total, 8);
    }
    std::string err;
    const int rc = parse_exact(blob.data(), len, &err);
    CHECK(rc == 0 || rc == DSM_ERR_INVALID);
    (rc == 0 ? accepted : refused) += 1;
  }
  CHECK(refused > 20000);   // most mutations break something the reader checks
  CHECK(accepted > 1000);   // and harmless ones (payload bytes, token values) still read
  printf("tts_slot_blob_fuzz ok: %ld mutated blobs refused, %ld accepted\n", refused, accepted);
  return 0;
}
