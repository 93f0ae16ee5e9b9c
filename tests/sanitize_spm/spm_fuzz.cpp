// Stand-alone sanitizer harness of the native SentencePiece tokenizer (csrc/dsm_spm.h), built with AddressSanitizer + UBSan
// (Makefile).  Nothing but the header: no HIP, no Python.
//   1. the golden models load and replay tests/golden/spm/vectors.json byte for byte (the refused ones are refused);
//   2. 20 000 seeded mutations of every model's bytes — truncation, bit flips, edits of length fields — either fail to load
//      with a message or load and then encode and decode fixed input;
//   3. random byte strings as text through every golden model.
// Exit 0 and "spm_fuzz ok" when no check failed; a sanitizer report aborts the run.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_spm.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "spm_fuzz: check failed at line %d: %s\n", __LINE__, #c); exit(3); } } while (0)

namespace {

// ---- just enough JSON for vectors.json (objects, arrays, strings without escapes that matter, integers) ----
struct J {
  enum { NUL, NUM, STR, ARR, OBJ } t = NUL;
  long long num = 0;
  std::string s;
  std::vector<J> a;
  std::vector<std::pair<std::string, J>> o;
  const J& at(const char* key) const {
    for (const auto& kv : o) if (kv.first == key) return kv.second;
    fprintf(stderr, "spm_fuzz: vectors.json has no key %s\n", key);
    exit(3);
  }
};

struct JParser {
  const std::string& src;
  size_t o = 0;
  void ws() { while (o < src.size() && (src[o] == ' ' || src[o] == '\n' || src[o] == '\t' || src[o] == '\r')) ++o; }
  char peek() { ws(); REQUIRE(o < src.size()); return src[o]; }
  void expect(char c) { REQUIRE(peek() == c); ++o; }
  std::string str() {
    expect('"');
    std::string out;
    while (o < src.size() && src[o] != '"') {
      if (src[o] == '\\') { REQUIRE(o + 1 < src.size()); ++o; }
      out.push_back(src[o++]);
    }
    REQUIRE(o < src.size());
    ++o;
    return out;
  }
  J value(int depth = 0) {
    REQUIRE(depth < 16);
    J v;
    const char c = peek();
    if (c == '{') {
      v.t = J::OBJ; ++o;
      if (peek() == '}') { ++o; return v; }
      for (;;) {
        std::string k = str();
        expect(':');
        v.o.emplace_back(std::move(k), value(depth + 1));
        if (peek() == ',') { ++o; continue; }
        expect('}');
        return v;
      }
    }
    if (c == '[') {
      v.t = J::ARR; ++o;
      if (peek() == ']') { ++o; return v; }
      for (;;) {
        v.a.push_back(value(depth + 1));
        if (peek() == ',') { ++o; continue; }
        expect(']');
        return v;
      }
    }
    if (c == '"') { v.t = J::STR; v.s = str(); return v; }
    if (c == '-' || (c >= '0' && c <= '9')) {
      v.t = J::NUM;
      size_t used = 0;
      v.num = std::stoll(src.substr(o, 24), &used);
      o += used;
      return v;
    }
    for (const char* lit : {"true", "false", "null"})
      if (src.compare(o, strlen(lit), lit) == 0) { o += strlen(lit); return v; }
    REQUIRE(!"unexpected character in vectors.json");
    return v;
  }
};

std::string unhex(const std::string& h) {
  REQUIRE(h.size() % 2 == 0);
  std::string out;
  for (size_t i = 0; i < h.size(); i += 2) out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return out;
}

std::string read_file(const std::string& path) {
  std::vector<uint8_t> buf;
  std::string err;
  REQUIRE(dsm_spm_ns::load_file(path.c_str(), buf, err) == 0);
  return std::string(buf.begin(), buf.end());
}

std::vector<uint32_t> encode(const dsm_spm* t, const std::string& text) {
  const int64_t n = dsm_spm_encode(t, text.data(), text.size(), nullptr, 0);
  REQUIRE(n >= 0);
  std::vector<uint32_t> ids((size_t)n + 1, 0xdeadbeefu);
  REQUIRE(dsm_spm_encode(t, text.data(), text.size(), ids.data(), (size_t)n) == n);
  REQUIRE(ids[(size_t)n] == 0xdeadbeefu);  // nothing past cap
  ids.resize((size_t)n);
  return ids;
}

bool decode(const dsm_spm* t, const std::vector<uint32_t>& ids, std::string& out) {
  const int64_t n = dsm_spm_decode(t, ids.data(), ids.size(), nullptr, 0);
  if (n < 0) return false;
  out.assign((size_t)n + 1, '\x55');
  REQUIRE(dsm_spm_decode(t, ids.data(), ids.size(), &out[0], (size_t)n) == n);
  REQUIRE(out[(size_t)n] == '\x55');
  out.resize((size_t)n);
  return true;
}

// offsets of the length varints of the top-level fields and of the fields one level down
std::vector<size_t> length_fields(const std::string& blob) {
  std::vector<size_t> at;
  struct Range { size_t lo, hi; int depth; };
  std::vector<Range> todo{{0, blob.size(), 0}};
  while (!todo.empty()) {
    const Range r = todo.back();
    todo.pop_back();
    dsm_spm_ns::Pb p{(const uint8_t*)blob.data() + r.lo, r.hi - r.lo};
    while (!p.done()) {
      uint32_t f; int wt;
      if (!p.key(f, wt)) break;
      if (wt == 2) {
        const size_t len_at = r.lo + p.o;
        const uint8_t* q; size_t n;
        if (!p.bytes(q, n)) break;
        at.push_back(len_at);
        if (r.depth == 0 && at.size() < 4096) todo.push_back(Range{(size_t)(q - (const uint8_t*)blob.data()), (size_t)(q - (const uint8_t*)blob.data()) + n, 1});
      } else if (!p.skip(wt)) break;
    }
  }
  return at;
}

const char kFixedText[] = "  Hello  w\xc3\xb6rld \xef\xbc\xa8\xef\xbd\x85 \xe2\x91\xa0\xc2\xbd caf\xc3\xa9 \xe6\x97\xa5\xe6\x9c\xac \xf0\x9f\x98\x80 \xff\xc3 tail  ";

void use(const dsm_spm* t, std::mt19937_64& rng) {
  const int vocab = dsm_spm_vocab_size(t);
  REQUIRE(vocab > 0);
  int unk, bos, eos, pad;
  REQUIRE(dsm_spm_special_ids(t, &unk, &bos, &eos, &pad) == 0 && unk >= 0 && unk < vocab);
  std::vector<uint32_t> ids = encode(t, std::string(kFixedText, sizeof kFixedText - 1));
  for (uint32_t id : ids) REQUIRE(id < (uint32_t)vocab);
  std::string text;
  REQUIRE(decode(t, ids, text));
  std::vector<uint32_t> fixed{0, 1, 2, 3, (uint32_t)(vocab - 1), (uint32_t)(vocab / 2), (uint32_t)(rng() % (uint64_t)vocab)};
  REQUIRE(decode(t, fixed, text));
  fixed.push_back((uint32_t)vocab);
  REQUIRE(!decode(t, fixed, text) && dsm_spm_last_error(t)[0]);
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "../golden/spm";
  const std::string vec_src = read_file(dir + "/vectors.json");
  JParser jp{vec_src};
  const J vectors = jp.value();
  size_t n_enc = 0, n_dec = 0, loaded = 0, refused = 0;

  // 1. golden models and recorded vectors
  std::vector<std::pair<std::string, std::string>> blobs;
  for (const auto& kv : vectors.at("models").o) {
    const J& rec = kv.second;
    const std::string path = dir + "/" + rec.at("file").s;
    dsm_spm* t = nullptr;
    REQUIRE(dsm_spm_load(path.c_str(), &t) == 0);
    REQUIRE((size_t)dsm_spm_vocab_size(t) == rec.at("pieces").a.size());
    for (const J& pair : rec.at("encode").a) {
      std::vector<uint32_t> want;
      for (const J& v : pair.a[1].a) want.push_back((uint32_t)v.num);
      REQUIRE(encode(t, unhex(pair.a[0].s)) == want);
      ++n_enc;
    }
    for (const J& pair : rec.at("decode").a) {
      std::vector<uint32_t> ids;
      for (const J& v : pair.a[0].a) ids.push_back((uint32_t)v.num);
      std::string got;
      REQUIRE(decode(t, ids, got) && got == unhex(pair.a[1].s));
      ++n_dec;
    }
    dsm_spm_free(t);
    blobs.emplace_back(kv.first, read_file(path));
  }
  REQUIRE(blobs.size() >= 3 && n_enc >= 600 && n_dec >= 600);
  for (const J& name : vectors.at("refused").a) {
    dsm_spm* t = nullptr;
    REQUIRE(dsm_spm_load((dir + "/" + name.s).c_str(), &t) == DSM_ERR_INVALID && !t && dsm_spm_last_error(nullptr)[0]);
  }

  // 2. mutations
  for (const auto& nb : blobs) {
    const std::string& blob = nb.second;
    const std::vector<size_t> lens = length_fields(blob);
    REQUIRE(!lens.empty());
    std::mt19937_64 rng(0x5eed0000 + blob.size());
    // the specs and the head of the charsmap sit behind the pieces: half of the flips go near the structure, half anywhere
    const size_t head = std::min(blob.size(), *std::max_element(lens.begin(), lens.end()) + 4096);
    for (int it = 0; it < 20000; ++it) {
      std::string m = blob;
      switch (rng() % 4) {
        case 0: m.resize(rng() % blob.size()); break;
        case 1: for (int k = 1 + (int)(rng() % 8); k > 0; --k) m[rng() % head] ^= (char)(1u << (rng() % 8)); break;
        case 2: for (int k = 1 + (int)(rng() % 8); k > 0; --k) m[rng() % m.size()] ^= (char)(1u << (rng() % 8)); break;
        default: {
          const size_t at = lens[rng() % lens.size()];
          switch (rng() % 4) {
            case 0: m[at] = (char)(rng() & 0xff); break;
            case 1: m[at] = (char)(m[at] + 1); break;
            case 2: m[at] = (char)(m[at] | 0x80); break;                              // the length grows a byte
            default: m.insert(at, std::string(1 + rng() % 10, '\xff')); break;        // an over-long varint
          }
        }
      }
      dsm_spm* t = nullptr;
      const int rc = dsm_spm_load_bytes((const uint8_t*)m.data(), m.size(), &t);
      if (rc) {
        REQUIRE((rc == DSM_ERR_IO || rc == DSM_ERR_INVALID) && !t && dsm_spm_last_error(nullptr)[0]);
        ++refused;
        continue;
      }
      ++loaded;
      use(t, rng);
      dsm_spm_free(t);
    }
  }
  REQUIRE(loaded > 1000 && refused > 1000);  // both outcomes are exercised

  // 3. random bytes as text
  size_t n_text = 0;
  for (const auto& nb : blobs) {
    dsm_spm* t = nullptr;
    REQUIRE(dsm_spm_load_bytes((const uint8_t*)nb.second.data(), nb.second.size(), &t) == 0);
    std::mt19937_64 rng(0xb17e5 + nb.second.size());
    for (int it = 0; it < 20000; ++it) {
      std::string text(rng() % 65, '\0');
      const bool ascii_heavy = rng() & 1;
      for (char& c : text) c = (char)(ascii_heavy && (rng() % 4) ? 0x20 + rng() % 0x5f : rng() & 0xff);
      const std::vector<uint32_t> ids = encode(t, text);
      std::string back;
      REQUIRE(decode(t, ids, back));
      ++n_text;
    }
    dsm_spm_free(t);
  }
  printf("spm_fuzz ok: %zu encode and %zu decode vectors, %zu mutated models loaded and used, %zu refused, %zu random texts\n", n_enc,
         n_dec, loaded, refused, n_text);
  return 0;
}
