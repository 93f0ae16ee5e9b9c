// slot_blob_fuzz — the header and host-section parser of both slot blob kinds (csrc/dsm_slot_blob.h: the container and the
// STT items; csrc/dsm_tts_slot_blob.h: the TTS items) under AddressSanitizer + UBSan.  A stand-alone program, one driver run
// once per kind: valid blobs are written with the kind's own writer and must read back field for field; then seeded mutations
// (byte flips, 32- and 64-bit fields overwritten with edge values, truncations at every length class) go through the kind's
// info(), each copied into a heap buffer of exactly its length so that any read past the end is caught.  Every outcome must be
// a clean accept or a clean DSM_ERR_INVALID with a message.
//
// The generator is seeded, so a run is one fixed sequence of blobs and outcomes.  Each kind pins four numbers of it: an FNV-1a
// hash of every valid blob written, one of every mutation's (return code, message), and the two counts.  They were taken from
// the writers and readers as they were when each kind had a header and a fuzz program of its own, before the two were folded
// into one container: a blob byte, an accept, a return code or a message text that moves shows here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_tts_slot_blob.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t fnv(uint64_t h, const void* p, size_t n) {  // FNV-1a 64
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001B3ull;
  return h;
}

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s: %s failed (line %d)\n", F::name, #cond, __LINE__); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

// ---- per kind: the item maker, the read-back comparison, what the kind's info() adds, its pins ----
struct SttFuzz {
  static constexpr const char* name = "slot_blob_fuzz";
  using Item = dsm_slot_blob::HostItem;
  using Info = struct dsm_slot_blob_info;
  static constexpr uint32_t kSigWords = 40;     // read-back rounds draw sig_words below this
  static constexpr bool kItemEdges = false;     // the edge values around an item's size and its count limits
  static constexpr int kCountOffs = 0;          // no mutation kind of its own
  static constexpr int count_off[1] = {0};
  static constexpr uint64_t kPinBlobs = 0xb0eaf0dc6603f0bdull, kPinOutcomes = 0xf10153027e91e465ull;
  static constexpr long kPinRefused = 45070, kPinAccepted = 14930;
  static uint32_t draw_aux(uint32_t) { return 0; }
  static Item make_item(uint32_t) {
    Item it;
    it.step_idx = rnd() % 100000;
    it.last_stop_time = (double)(rnd() % 10000) / 12.5;
    it.unended_word = (uint32_t)(rnd() & 1);
    it.side_flags = (uint32_t)(rnd() & 3);
    it.word_tokens.resize(rnd() % 9);
    for (auto& t : it.word_tokens) t = (uint32_t)(rnd() % 32000);
    return it;
  }
  static bool same(const Item& a, const Item& b) {
    return a.step_idx == b.step_idx && a.last_stop_time == b.last_stop_time && a.unended_word == b.unended_word &&
           a.side_flags == b.side_flags && a.word_tokens == b.word_tokens;
  }
  static void write(std::vector<uint8_t>& out, uint32_t flags, uint32_t, const std::vector<uint32_t>& sig, const std::vector<Item>& items,
                    uint64_t slot_bytes) {
    dsm_slot_blob::write_front(out, flags, sig, items, slot_bytes);
  }
  static int read_header(const void* b, size_t n, dsm_blob::Header* h, std::string* e) { return dsm_slot_blob::read_header(b, n, h, e); }
  static int read_host(const void* b, const dsm_blob::Header& h, std::vector<Item>* o, std::string* e) { return dsm_slot_blob::read_host(b, h, o, e); }
  static int info(const void* b, size_t n, Info* o, std::string* e) { return dsm_slot_blob::info(b, n, o, e); }
  static bool info_ok(const Info&) { return true; }
};

struct TtsFuzz {
  static constexpr const char* name = "tts_slot_blob_fuzz";
  using Item = dsm_tts_slot_blob::HostItem;
  using Info = struct dsm_tts_slot_blob_info;
  static constexpr uint32_t kSigWords = 60;
  static constexpr bool kItemEdges = true;
  static constexpr int kCountOffs = 3;          // mutation kind 5: a count of the first item takes an edge value
  static constexpr int count_off[3] = {0, 44, 48};  // step_idx, n_words, n_tok
  static constexpr uint64_t kPinBlobs = 0x81a663f38d3bc986ull, kPinOutcomes = 0x61656e42059538f2ull;
  static constexpr long kPinRefused = 48280, kPinAccepted = 11720;
  static uint32_t draw_aux(uint32_t m) { return 1 + (uint32_t)(rnd() % m); }  // slices
  static Item make_item(uint32_t slices) {
    Item it;
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
    return it;
  }
  static bool same(const Item& a, const Item& b) {
    return a.step_idx == b.step_idx && a.consecutive_pads == b.consecutive_pads && a.samp_k == b.samp_k && a.cfg_on == b.cfg_on &&
           a.cond_on == b.cond_on && a.ca_len[0] == b.ca_len[0] && a.ca_len[1] == b.ca_len[1] && a.req_flags == b.req_flags &&
           a.req_status == b.req_status && a.text_tokens == b.text_tokens && a.audio_tokens == b.audio_tokens && a.q_tok == b.q_tok &&
           a.q_end == b.q_end;
  }
  static void write(std::vector<uint8_t>& out, uint32_t flags, uint32_t slices, const std::vector<uint32_t>& sig,
                    const std::vector<Item>& items, uint64_t slot_bytes) {
    dsm_tts_slot_blob::write_front(out, flags, slices, sig, items, slot_bytes);
  }
  static int read_header(const void* b, size_t n, dsm_blob::Header* h, std::string* e) { return dsm_tts_slot_blob::read_header(b, n, h, e); }
  static int read_host(const void* b, const dsm_blob::Header& h, std::vector<Item>* o, std::string* e) { return dsm_tts_slot_blob::read_host(b, h, o, e); }
  static int info(const void* b, size_t n, Info* o, std::string* e) { return dsm_tts_slot_blob::info(b, n, o, e); }
  static bool info_ok(const Info& i) { return i.slices >= 1; }
};

// ---- the driver, once ----
template <class F>
static std::vector<uint8_t> make_blob(uint32_t n, uint32_t sig_words, uint32_t aux, uint64_t slot_bytes, uint32_t flags,
                                      std::vector<typename F::Item>* items_out) {
  std::vector<typename F::Item> items;
  for (uint32_t i = 0; i < n; ++i) items.push_back(F::make_item(aux));
  std::vector<uint32_t> sig(sig_words);
  for (auto& w : sig) w = (uint32_t)(rnd() % 4096);
  std::vector<uint8_t> out;
  F::write(out, flags, aux, sig, items, slot_bytes);
  const size_t front = out.size();
  out.resize(front + (size_t)n * slot_bytes);
  for (size_t i = front; i < out.size(); ++i) out[i] = (uint8_t)rnd();
  if (items_out) *items_out = items;
  return out;
}

// the parser on a heap copy of exactly `len` bytes
template <class F>
static int parse_exact(const uint8_t* data, size_t len, std::string* err) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
  if (len) memcpy(copy.get(), data, len);
  typename F::Info info;
  memset(&info, 0, sizeof info);
  const int rc = F::info(copy.get(), len, &info, err);
  if (rc == 0) {  // what it accepted must hang together
    if (info.total_bytes > len || info.n_slots < 1 || !F::info_ok(info) || info.host_bytes % 16 || info.slot_bytes % 16) return 1;
    if (info.total_bytes != 48 + dsm_blob::align16(4ull * info.sig_words) + info.host_bytes + (uint64_t)info.n_slots * info.slot_bytes) return 1;
  } else if (rc != DSM_ERR_INVALID || err->empty()) {
    return 1;
  }
  return rc;
}

template <class F>
static uint64_t edge_value() {  // one draw
  static const uint64_t edge[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 0xFFFFFull, 0x100000ull, 0x100001ull,
                                  0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x7FFFFFFFFFFFFFFFull,
                                  0x8000000000000000ull, 0xFFFFFFFFFFFFFFF0ull, 0xFFFFFFFFFFFFFFFFull};
  const size_t n_item = 6, first_item = 10, n_all = sizeof edge / sizeof edge[0];  // 63 .. 0x100001: kItemEdges only
  const size_t i = (size_t)(rnd() % (F::kItemEdges ? n_all : n_all - n_item));
  return edge[F::kItemEdges || i < first_item ? i : i + n_item];
}

template <class F>
static int run() {
  rng_state = 0x9E3779B97F4A7C15ull;
  uint64_t h_blobs = 0xCBF29CE484222325ull, h_outcomes = 0xCBF29CE484222325ull;
  // ---- valid blobs read back ----
  for (int round = 0; round < 200; ++round) {
    const uint32_t n = 1 + (uint32_t)(rnd() % 5), sw = (uint32_t)(rnd() % F::kSigWords), flags = (uint32_t)(rnd() & 1);
    const uint32_t aux = F::draw_aux(33);
    const uint64_t slot_bytes = 16 * (rnd() % 40);
    std::vector<typename F::Item> items;
    const std::vector<uint8_t> blob = make_blob<F>(n, sw, aux, slot_bytes, flags, &items);
    dsm_blob::Header h;
    std::string err;
    CHECK(F::read_header(blob.data(), blob.size(), &h, &err) == 0);
    CHECK(h.n_slots == n && h.sig_words == sw && h.flags == flags && h.aux == aux && h.slot_bytes == slot_bytes && h.total_bytes == blob.size());
    std::vector<typename F::Item> back;
    CHECK(F::read_host(blob.data(), h, &back, &err) == 0);
    CHECK(back.size() == items.size());
    for (size_t i = 0; i < items.size(); ++i) CHECK(F::same(back[i], items[i]));
    CHECK(parse_exact<F>(blob.data(), blob.size(), &err) == 0);
    h_blobs = fnv(h_blobs, blob.data(), blob.size());
  }
  // ---- mutations and truncations ----
  long accepted = 0, refused = 0;
  const int n_kinds = 6 + (F::kCountOffs ? 1 : 0);
  for (int round = 0; round < 60000; ++round) {
    const uint32_t n = 1 + (uint32_t)(rnd() % 4), sw = (uint32_t)(rnd() % 24);
    const uint32_t flags = (uint32_t)(rnd() & 1);  // in this order: the pins were taken with it
    const uint64_t slot_bytes = 16 * (rnd() % 12);
    const uint32_t aux = F::draw_aux(9);
    std::vector<uint8_t> blob = make_blob<F>(n, sw, aux, slot_bytes, flags, nullptr);
    const size_t front = 48 + (size_t)dsm_blob::align16(4ull * sw);
    const int kind = (int)(rnd() % n_kinds);
    size_t len = blob.size();
    if (kind == 0) {  // truncate anywhere
      len = (size_t)(rnd() % (blob.size() + 1));
    } else if (kind == 1) {  // a header field takes an edge value
      static const int off32[] = {0, 4, 8, 12, 16, 20};
      static const int off64[] = {24, 32, 40};
      if (rnd() & 1) { const uint32_t v = (uint32_t)edge_value<F>(); memcpy(&blob[(size_t)off32[rnd() % 6]], &v, 4); }
      else { const uint64_t v = edge_value<F>(); memcpy(&blob[(size_t)off64[rnd() % 3]], &v, 8); }
    } else if (kind == 2) {  // a 32-bit word of the host section takes an edge value
      const size_t words = (blob.size() - front) / 4;
      if (words) { const uint32_t v = (uint32_t)edge_value<F>(); memcpy(&blob[front + 4 * (size_t)(rnd() % words)], &v, 4); }
    } else if (kind == 3) {  // byte flips anywhere
      for (int f = 1 + (int)(rnd() % 8); f > 0; --f) blob[(size_t)(rnd() % blob.size())] ^= (uint8_t)(1u << (rnd() % 8));
    } else if (kind == 4) {  // header field and truncation together
      const uint64_t v = edge_value<F>();
      memcpy(&blob[24 + 8 * (size_t)(rnd() % 3)], &v, 8);
      len = (size_t)(rnd() % (blob.size() + 1));
    } else if (kind == 5 && F::kCountOffs) {  // a count of the first item takes an edge value
      const uint32_t v = (uint32_t)edge_value<F>();
      memcpy(&blob[front + (size_t)F::count_off[rnd() % (F::kCountOffs ? F::kCountOffs : 1)]], &v, 4);
    } else {  // sizes grown consistently, buffer not: total_bytes says more than there is
      uint64_t total;
      memcpy(&total, &blob[40], 8);
      total += 16 * (1 + rnd() % 4);
      memcpy(&blob[40], &total, 8);
    }
    std::string err;
    const int32_t rc = parse_exact<F>(blob.data(), len, &err);
    CHECK(rc == 0 || rc == DSM_ERR_INVALID);
    (rc == 0 ? accepted : refused) += 1;
    h_outcomes = fnv(fnv(h_outcomes, &rc, 4), err.c_str(), err.size() + 1);
  }
  CHECK(refused > 20000);   // most mutations break something the reader checks
  CHECK(accepted > 1000);   // and harmless ones (payload bytes, token values) still read
  printf("%s pins: blobs %016llx outcomes %016llx\n", F::name, (unsigned long long)h_blobs, (unsigned long long)h_outcomes);
  CHECK(h_blobs == F::kPinBlobs && h_outcomes == F::kPinOutcomes && refused == F::kPinRefused && accepted == F::kPinAccepted);
  printf("%s ok: %ld mutated blobs refused, %ld accepted\n", F::name, refused, accepted);
  return 0;
}

int main() { return run<SttFuzz>() || run<TtsFuzz>(); }
