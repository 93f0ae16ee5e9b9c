// bias_fuzz — the host code of the text bias (csrc/dsm_text_bias.h: the compiler of a bias set, the checked reader of its table
// and the host pick) under AddressSanitizer + UBSan.  A stand-alone program with its own main:
//   1  seeded random bias sets, valid and malformed (tokens outside the vocabulary, duplicates, +inf / NaN, empty and
//      over-long keywords, terminator pieces, bad boosts, too many token biases) go through compile(): each is accepted or
//      refused with a message; an accepted table passes check(), compiles to the same words from the permuted input, and every
//      keyword can be walked through it with dsm_bias_child;
//   2  valid tables mutated (words overwritten with edge values, truncated, extended), each copied into a heap buffer of exactly
//      its length, go through pick_host() with random nodes and rows: a clean token or a clean DSM_ERR_INVALID;
//   3  wholly random word arrays do the same.
// Every accepted pick is repeated on the unchecked serial definition and must agree with it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../delayed-streams-modeling_amd/csrc/dsm_text_bias.h"

static uint64_t rng_state = 0x5EEDB1A5ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
static float unit() { return (float)(rnd() >> 40) / 16777216.0f; }

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "bias_fuzz: %s failed (line %d)\n", #cond, __LINE__); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static const uint32_t kEdgeWords[] = {0u, 1u, 2u, 3u, 4u, 7u, 8u, 63u, 64u, 255u, 1024u, 1025u, 65535u, 65536u, 0x7FFFFFFFu,
                                      0x80000000u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x3F800000u, 0xBF800000u};

struct Set {
  std::vector<dsm_bias_token> tokens;
  std::vector<std::vector<uint32_t>> pieces;
  std::vector<float> boosts;
  std::vector<dsm_bias_keyword> kws() const {
    std::vector<dsm_bias_keyword> k(pieces.size());
    for (size_t i = 0; i < k.size(); ++i) k[i] = dsm_bias_keyword{pieces[i].empty() ? nullptr : pieces[i].data(), (int)pieces[i].size(), boosts[i]};
    return k;
  }
};

// a random set over V pieces; `fault` in 1 .. 10 plants one thing compile() must refuse, 0 none
static Set make_set(int V, int fault) {
  Set s;
  const uint32_t nt = below(40), nk = below(60);
  std::vector<char> used((size_t)V, 0);
  for (uint32_t i = 0; i < nt && i < (uint32_t)V; ++i) {
    uint32_t t;
    do t = below((uint32_t)V); while (used[t]);
    used[t] = 1;
    s.tokens.push_back(dsm_bias_token{t, below(5) == 0 ? -DSM_INF_F : (unit() - 0.5f) * 20.0f});
  }
  for (uint32_t i = 0; i < nk; ++i) {
    std::vector<uint32_t> p(1 + below(below(4) ? 4 : DSM_BIAS_MAX_KEYWORD_TOKENS));
    for (uint32_t& x : p) {
      do x = below((uint32_t)(V < 12 ? V : (below(3) ? 12 : V))); while (x == 0 || x == 3);  // a small alphabet shares prefixes
    }
    s.pieces.push_back(p);
    s.boosts.push_back(0.01f + unit() * 9.0f);
  }
  auto any_kw = [&]() -> size_t {
    if (s.pieces.empty()) { s.pieces.push_back({1}); s.boosts.push_back(1.0f); }
    return below((uint32_t)s.pieces.size());
  };
  auto any_tok = [&]() -> size_t {
    if (s.tokens.empty()) s.tokens.push_back(dsm_bias_token{1, 1.0f});
    return below((uint32_t)s.tokens.size());
  };
  switch (fault) {
    case 1: s.tokens[any_tok()].token = (uint32_t)V + below(3) * 0x40000000u; break;
    case 2: { const size_t i = any_tok(); s.tokens.push_back(s.tokens[i]); break; }
    case 3: s.tokens[any_tok()].bias = below(2) ? DSM_INF_F : dsm_u32_as_f32(0x7FC00001u); break;
    case 4: s.pieces[any_kw()].clear(); break;
    case 5: s.pieces[any_kw()].assign(DSM_BIAS_MAX_KEYWORD_TOKENS + 1 + below(5), 1u); break;
    case 6: { auto& p = s.pieces[any_kw()]; p[below((uint32_t)p.size())] = below(2) ? 0u : 3u; break; }
    case 7: { auto& p = s.pieces[any_kw()]; p[below((uint32_t)p.size())] = (uint32_t)V + below(2) * 0xF0000000u; break; }
    case 8: { const float bad[] = {0.0f, -0.0f, -1.0f, DSM_INF_F, -DSM_INF_F, dsm_u32_as_f32(0x7FC00000u)}; s.boosts[any_kw()] = bad[below(6)]; break; }
    case 9:
      s.tokens.clear();
      for (uint32_t t = 0; t <= DSM_BIAS_MAX_TOKENS; ++t) s.tokens.push_back(dsm_bias_token{t, 1.0f});  // (V is raised by the caller)
      break;
    default: break;
  }
  return s;
}

static std::vector<float> make_row(int V) {
  std::vector<float> r((size_t)V);
  const uint32_t kind = below(8);
  for (float& x : r) {
    x = (unit() - 0.5f) * 8.0f;
    if (kind == 0 && below(4) == 0) x = -DSM_INF_F;
    if (kind == 1 && below(6) == 0) x = dsm_u32_as_f32(0x7FC00000u);
    if (kind == 2) x = -DSM_INF_F;
    if (kind == 3) x = 0.0f;
  }
  return r;
}

// pick_host on a heap copy of exactly `words` words; an accept must equal the unchecked definition
static int pick_once(const std::vector<uint32_t>& table, int V, int* accepted) {
  std::unique_ptr<uint32_t[]> t(new uint32_t[table.size() ? table.size() : 1]);
  if (!table.empty()) memcpy(t.get(), table.data(), 4 * table.size());
  const std::vector<float> row = make_row(V);
  const uint32_t node = below(4) == 0 ? DSM_BIAS_DEAD : below(3) ? below(8) : (uint32_t)rnd();
  const float temp = below(3) == 0 ? 0.25f + unit() : below(2) ? 0.0f : 1.0f;
  uint32_t key[8];
  for (uint32_t& k : key) k = (uint32_t)rnd();
  const uint64_t pos = 16ull * below(1000) + (below(20) == 0 ? 8 : 0);
  uint32_t tok = 0xABCDu, nxt = 0xABCDu;
  std::string err;
  const int rc = dsm_text_bias::pick_host(table.empty() ? nullptr : t.get(), table.size(), node, row.data(), V, temp, below(10) ? key : nullptr, pos,
                                          &tok, &nxt, &err);
  CHECK(rc == 0 || (rc == DSM_ERR_INVALID && !err.empty()));
  if (rc) return 0;
  *accepted += 1;
  CHECK(tok < (uint32_t)V);
  CHECK(table.empty() ? nxt == node : (nxt == DSM_BIAS_DEAD || nxt < t[4]));
  std::vector<float> x((size_t)V);
  uint32_t tok2 = 0, nxt2 = 0;
  dsm_text_bias_pick_row(table.empty() ? nullptr : t.get(), node, row.data(), V, temp, key, pos, x.data(), &tok2, &nxt2);
  CHECK(tok2 == tok && nxt2 == nxt);
  return 0;
}

int main() {
  int compiled = 0, refused = 0, picks = 0, tries = 0;
  std::vector<std::vector<uint32_t>> good;
  std::vector<int> good_v;
  // ---- 1: the compiler ----
  for (int it = 0; it < 3000; ++it) {
    const int fault = below(3) == 0 ? 1 + (int)below(9) : 0;
    int V = below(4) == 0 ? 4 + (int)below(8) : 16 + (int)below(3000);
    const Set s = make_set(V, fault);
    if (fault == 9) V = 5000;
    const std::vector<dsm_bias_keyword> k = s.kws();
    std::vector<uint32_t> w;
    std::string err;
    const int rc = dsm_text_bias::compile(s.tokens.data(), (int)s.tokens.size(), k.data(), (int)k.size(), V, &w, &err);
    if (fault) {
      CHECK(rc == DSM_ERR_INVALID && !err.empty() && w.empty());
      ++refused;
      continue;
    }
    CHECK(rc == 0);
    ++compiled;
    long mx = -1;
    CHECK(dsm_text_bias::check(w.data(), w.size(), &err, &mx) == 0 && mx < V);
    CHECK(w[3] == s.tokens.size());
    // the permuted input gives the same words
    Set p = s;
    for (size_t i = p.pieces.size(); i > 1; --i) {
      const size_t j = below((uint32_t)i);
      std::swap(p.pieces[i - 1], p.pieces[j]);
      std::swap(p.boosts[i - 1], p.boosts[j]);
    }
    for (size_t i = p.tokens.size(); i > 1; --i) std::swap(p.tokens[i - 1], p.tokens[below((uint32_t)i)]);
    const std::vector<dsm_bias_keyword> pk = p.kws();
    std::vector<uint32_t> w2;
    CHECK(dsm_text_bias::compile(p.tokens.data(), (int)p.tokens.size(), pk.data(), (int)pk.size(), V, &w2, &err) == 0 && w2 == w);
    // every keyword walks the trie, and its last edge carries at least its boost
    const uint32_t* first = dsm_bias_first_of(w.data(), w[3]);
    const uint32_t* edges = dsm_bias_edges_of(w.data(), w[3], w[4]);
    for (size_t i = 0; i < s.pieces.size(); ++i) {
      uint32_t at = 0;
      for (uint32_t piece : s.pieces[i]) {
        at = dsm_bias_child(first, edges, at, piece);
        CHECK(at != DSM_BIAS_DEAD && at < w[4]);
      }
      CHECK(dsm_u32_as_f32(edges[3 * (at - 1) + 1]) >= s.boosts[i]);
    }
    if (good.size() < 200) { good.push_back(w); good_v.push_back(V); }
  }
  {  // NULL arguments and counts out of range
    std::vector<uint32_t> w;
    std::string err;
    const dsm_bias_token tk{1, 1.0f};
    CHECK(dsm_text_bias::compile(nullptr, 1, nullptr, 0, 64, &w, &err) == DSM_ERR_INVALID);
    CHECK(dsm_text_bias::compile(&tk, -1, nullptr, 0, 64, &w, &err) == DSM_ERR_INVALID);
    CHECK(dsm_text_bias::compile(&tk, 1, nullptr, 2, 64, &w, &err) == DSM_ERR_INVALID);
    CHECK(dsm_text_bias::compile(&tk, 1, nullptr, 0, 0, &w, &err) == DSM_ERR_INVALID);
    CHECK(dsm_text_bias::compile(nullptr, 0, nullptr, 0, 1, &w, &err) == 0 && w.size() == 10);
  }
  // ---- 2: mutated tables through the host pick ----
  for (int it = 0; it < 40000; ++it) {
    const size_t g = below((uint32_t)good.size());
    std::vector<uint32_t> t = good[g];
    const uint32_t kind = below(8);
    if (kind == 0) {
      // unchanged
    } else if (kind <= 4) {
      for (uint32_t n = 1 + below(3); n; --n) t[below(below(2) ? DSM_BIAS_HEADER_WORDS : (uint32_t)t.size())] = kEdgeWords[below(sizeof kEdgeWords / 4)];
    } else if (kind == 5) {
      t[below((uint32_t)t.size())] ^= 1u << below(32);
    } else if (kind == 6) {
      t.resize(below((uint32_t)t.size()));
    } else {
      t.resize(t.size() + 1 + below(8), 0u);
    }
    ++tries;
    if (pick_once(t, below(6) == 0 ? 1 + (int)below(4000) : good_v[g], &picks)) return 1;
  }
  // ---- 3: random words ----
  for (int it = 0; it < 20000; ++it) {
    std::vector<uint32_t> t(below(64));
    for (uint32_t& x : t) x = below(2) ? kEdgeWords[below(sizeof kEdgeWords / 4)] : below(40);
    if (t.size() >= 8 && below(2)) { t[0] = DSM_BIAS_MAGIC; t[1] = DSM_BIAS_VERSION; t[6] = (uint32_t)t.size(); t[7] = 0; }
    ++tries;
    if (pick_once(t, 1 + (int)below(300), &picks)) return 1;
  }
  CHECK(compiled > 1500 && refused > 500 && picks > 5000 && picks < tries);
  printf("bias_fuzz ok: %d sets compiled, %d refused, %d of %d picks accepted\n", compiled, refused, picks, tries);
  return 0;
}
