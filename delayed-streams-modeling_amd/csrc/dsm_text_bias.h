/*
 * dsm_text_bias.h — per-stream keyword boosting and token bias on the pick of the step's text token: the definition, once for
 * the HIP kernel (lm_pick_biased_kernel, dsm_kernels.h) and the host (dsm_text_bias_pick_host), and the compiler of a bias set
 * into its flat table (host only).  This project's own: the reference takes the arg-max or the Gumbel sample of the raw row and
 * stops (core/asr.rs:208-216).
 *
 * A BIAS SET is immutable.  It holds token biases — up to DSM_BIAS_MAX_TOKENS pairs (token < V, bias), each bias a finite f32
 * or -inf (a ban) — and keywords: each ONE word of 1 .. DSM_BIAS_MAX_KEYWORD_TOKENS piece ids below V, none of them 0 or 3 (the
 * two word terminators of core/asr.rs:229), with a finite boost > 0 in logit units.  The keywords compile into a trie: node 0 is
 * the root, nodes are numbered breadth first, a node's edges are sorted by token, and an edge's boost is the maximum over the
 * keywords that pass through it (duplicates allowed).  The table is a function of the SET of inputs, not of their order.
 *
 * The flat table, u32 words, little-endian when it is stored:
 *   word 0  magic        "DSBT" (0x54425344)
 *        1  version      1
 *        2  V            every token of the table is below it
 *        3  n_tokens     0 .. DSM_BIAS_MAX_TOKENS
 *        4  n_nodes      1 .. DSM_BIAS_MAX_NODES (the root always exists)
 *        5  n_edges      n_nodes - 1: every node but the root has exactly one edge leading to it
 *        6  total_words  8 + 2 n_tokens + (n_nodes + 1) + 3 n_edges
 *        7  reserved     0
 *        8  token biases n_tokens x (token, f32 bits of the bias), token strictly ascending
 *           first        n_nodes + 1 words: node i owns the edges first[i] .. first[i + 1] - 1; first[0] = 0, first[n_nodes] = n_edges
 *           edges        n_edges x (token, f32 bits of the boost, child), in node order, token strictly ascending inside a node.
 *                        Breadth-first numbering with sorted edges makes child = edge index + 1; the checked reader insists on it,
 *                        which also proves the table is a tree.
 *
 * PER-SLOT STATE: the attached set (0 = none) and a trie node u32 — 0 the root, DSM_BIAS_DEAD (0xFFFFFFFF) inside a word that has
 * left the trie, or at a position the engine cannot know (a set attached in mid-stream, an imported slot).
 *
 * THE PICK for one row l[0..V) of raw text logits, every add ONE f32 add, in this order:
 *   1  x = l
 *   2  for every token bias (t, v):                          x[t] = x[t] + v
 *   3  if node != DEAD, for every edge (t, boost, child):    x[t] = x[t] + boost      (after 2: the order of the two adds is fixed)
 *   4  temperature <= 0: the first maximum of x (an all -inf or all-NaN row gives 0, as block_argmax_first does);
 *      else the first maximum of dsm_gumbel_value(x[j], word pos + j of the slot's ChaCha12 stream, temperature), and the
 *      stream advances by V rounded up to 16 — the position rule of lm_gumbel_kernel.
 *   5  advance (active slots only; an inactive slot's state is frozen): token 0 or 3 -> root; else DEAD stays DEAD; else the
 *      child along the token, or DEAD if the node has none.
 * With no set or an empty set x == l, and the token is what lm_argmax_kernel / lm_gumbel_kernel pick, bit for bit.  Without a
 * set the node is not touched.
 *
 * KNOWN LIMIT: this is greedy shallow fusion.  A partial match that then fails is not taken back — the boosted pieces of the
 * failed prefix stay in the transcript — and a keyword is one word: multi-word phrases are out of scope.
 */
#ifndef DSM_TEXT_BIAS_H
#define DSM_TEXT_BIAS_H

#include <stdint.h>
#include "../../include/dsm.h"
#include "dsm_numerics.h"
#include "dsm_sampling.h"

#define DSM_BIAS_MAGIC 0x54425344u
#define DSM_BIAS_VERSION 1u
#define DSM_BIAS_HEADER_WORDS 8u

/* where the three lists of a table start, from its two counts (the kernel takes the counts from the engine's set descriptor) */
DSM_HD const uint32_t* dsm_bias_tokens_of(const uint32_t* table) { return table + DSM_BIAS_HEADER_WORDS; }
DSM_HD const uint32_t* dsm_bias_first_of(const uint32_t* table, uint32_t n_tokens) { return table + DSM_BIAS_HEADER_WORDS + 2u * n_tokens; }
DSM_HD const uint32_t* dsm_bias_edges_of(const uint32_t* table, uint32_t n_tokens, uint32_t n_nodes) {
  return table + DSM_BIAS_HEADER_WORDS + 2u * n_tokens + n_nodes + 1u;
}

/* the child of `node` (a live node) along `tok`, DSM_BIAS_DEAD if there is none: binary search on the sorted edges */
DSM_HD uint32_t dsm_bias_child(const uint32_t* first, const uint32_t* edges, uint32_t node, uint32_t tok) {
  uint32_t lo = first[node], hi = first[node + 1];
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint32_t t = edges[3u * mid];
    if (t == tok) return edges[3u * mid + 2u];
    if (t < tok) lo = mid + 1u; else hi = mid;
  }
  return DSM_BIAS_DEAD;
}

/* step 5 with the child already looked up (the kernel finds it with a thread-parallel compare) */
DSM_HD uint32_t dsm_bias_advance(uint32_t node, uint32_t tok, uint32_t child) {
  if (tok == 0u || tok == 3u) return 0u;
  if (node == DSM_BIAS_DEAD) return DSM_BIAS_DEAD;
  return child;
}

/* Steps 1 - 5 serially.  x: V floats of scratch.  table NULL: no set.  key: 8 words, read when temperature > 0. */
DSM_HD void dsm_text_bias_pick_row(const uint32_t* table, uint32_t node, const float* l, int V, float temperature, const uint32_t* key,
                                   uint64_t pos, float* x, uint32_t* token, uint32_t* node_out) {
  const uint32_t n_tokens = table ? table[3] : 0u, n_nodes = table ? table[4] : 0u;
  const uint32_t* tb = table ? dsm_bias_tokens_of(table) : 0;
  const uint32_t* first = table ? dsm_bias_first_of(table, n_tokens) : 0;
  const uint32_t* edges = table ? dsm_bias_edges_of(table, n_tokens, n_nodes) : 0;
  for (int j = 0; j < V; ++j) x[j] = l[j];
  for (uint32_t i = 0; i < n_tokens; ++i) x[tb[2u * i]] = x[tb[2u * i]] + dsm_u32_as_f32(tb[2u * i + 1u]);
  if (table && node != DSM_BIAS_DEAD)
    for (uint32_t e = first[node]; e < first[node + 1]; ++e) x[edges[3u * e]] = x[edges[3u * e]] + dsm_u32_as_f32(edges[3u * e + 1u]);
  float bv = -DSM_INF_F;
  int bi = 0x7FFFFFFF;
  if (temperature > 0.0f) {
    const int nblk = (V + 15) >> 4;
    for (int blk = 0; blk < nblk; ++blk) {
      uint32_t w[16];
      dsm_chacha_block(key, (pos >> 4) + (uint64_t)blk, 12, w);
      for (int i = 0; i < 16; ++i) {
        const int j = 16 * blk + i;
        if (j < V) {
          const float v = dsm_gumbel_value(x[j], w[i], temperature);
          if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
        }
      }
    }
  } else {
    for (int j = 0; j < V; ++j) {
      const float v = x[j];
      if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
    }
  }
  const uint32_t tok = bi == 0x7FFFFFFF ? 0u : (uint32_t)bi;
  *token = tok;
  if (!table) { *node_out = node; return; }
  *node_out = dsm_bias_advance(node, tok, node == DSM_BIAS_DEAD ? DSM_BIAS_DEAD : dsm_bias_child(first, edges, node, tok));
}

/* ---- host only from here: the checked reader and the compiler ---- */
#if defined(__cplusplus)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace dsm_text_bias {

inline bool finite_f32(float v) { return (dsm_f32_as_u32(v) & 0x7F800000u) != 0x7F800000u; }

inline int fail(std::string* err, const char* fmt, long a = 0, long b = 0) {
  if (err) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    *err = buf;
  }
  return DSM_ERR_INVALID;
}

/* Everything the pick relies on, so that no table — however it was made — is read out of bounds: the counts against `words`,
 * every token below the table's V, sorted lists, bias and boost values of the allowed kinds, child = edge index + 1.
 * *max_token (optional): the largest token the table names, -1 if none: a row must be longer than that. */
inline int check(const uint32_t* t, size_t words, std::string* err, long* max_token = nullptr) {
  if (!t || words < DSM_BIAS_HEADER_WORDS) return fail(err, "text bias table: %ld words, the header alone has 8", (long)words);
  if (t[0] != DSM_BIAS_MAGIC) return fail(err, "text bias table: bad magic");
  if (t[1] != DSM_BIAS_VERSION) return fail(err, "text bias table: version %ld, this reader knows 1", (long)t[1]);
  const uint32_t V = t[2], nt = t[3], nn = t[4], ne = t[5];
  if (V < 1 || V > 0x7FFFFFFFu) return fail(err, "text bias table: V = %ld", (long)V);
  if (nt > DSM_BIAS_MAX_TOKENS) return fail(err, "text bias table: %ld token biases, at most %ld", (long)nt, (long)DSM_BIAS_MAX_TOKENS);
  if (nn < 1 || nn > DSM_BIAS_MAX_NODES) return fail(err, "text bias table: %ld nodes, 1 .. %ld allowed", (long)nn, (long)DSM_BIAS_MAX_NODES);
  if (ne != nn - 1) return fail(err, "text bias table: %ld edges for %ld nodes", (long)ne, (long)nn);
  const uint64_t total = (uint64_t)DSM_BIAS_HEADER_WORDS + 2ull * nt + nn + 1ull + 3ull * ne;
  if (t[6] != total || (uint64_t)words != total) return fail(err, "text bias table: %ld words, its counts need %ld", (long)words, (long)total);
  if (t[7] != 0) return fail(err, "text bias table: reserved word is not 0");
  long mx = -1;
  const uint32_t* tb = dsm_bias_tokens_of(t);
  for (uint32_t i = 0; i < nt; ++i) {
    if (tb[2 * i] >= V) return fail(err, "text bias table: token bias %ld names token %ld outside the vocabulary", (long)i, (long)tb[2 * i]);
    if (i && tb[2 * i] <= tb[2 * i - 2]) return fail(err, "text bias table: token biases not strictly ascending at %ld", (long)i);
    const float v = dsm_u32_as_f32(tb[2 * i + 1]);
    if (!finite_f32(v) && tb[2 * i + 1] != 0xFF800000u) return fail(err, "text bias table: token bias %ld is +inf or NaN", (long)i);
    mx = std::max(mx, (long)tb[2 * i]);
  }
  const uint32_t* first = dsm_bias_first_of(t, nt);
  const uint32_t* ed = dsm_bias_edges_of(t, nt, nn);
  if (first[0] != 0 || first[nn] != ne) return fail(err, "text bias table: edge ranges do not cover the edge list");
  for (uint32_t n = 0; n < nn; ++n) {
    if (first[n + 1] < first[n] || first[n + 1] > ne) return fail(err, "text bias table: edge range of node %ld is malformed", (long)n);
    for (uint32_t e = first[n]; e < first[n + 1]; ++e) {
      const uint32_t tok = ed[3 * e];
      if (tok >= V || tok == 0 || tok == 3) return fail(err, "text bias table: edge %ld carries token %ld", (long)e, (long)tok);
      if (e > first[n] && tok <= ed[3 * e - 3]) return fail(err, "text bias table: edges of node %ld not strictly ascending", (long)n);
      const float b = dsm_u32_as_f32(ed[3 * e + 1]);
      if (!finite_f32(b) || !(b > 0.0f)) return fail(err, "text bias table: boost of edge %ld is not a finite value above 0", (long)e);
      if (ed[3 * e + 2] != e + 1) return fail(err, "text bias table: edge %ld leads to node %ld, breadth-first order wants its index + 1", (long)e, (long)ed[3 * e + 2]);
      if (e + 1 <= n) return fail(err, "text bias table: edge %ld leads backwards", (long)e);
      mx = std::max(mx, (long)tok);
    }
  }
  if (max_token) *max_token = mx;
  return 0;
}

/* tokens / keywords -> the table.  DSM_ERR_INVALID with *err naming the first fault; `out` is written only on success. */
inline int compile(const dsm_bias_token* tokens, int n_tokens, const dsm_bias_keyword* keywords, int n_keywords, int V,
                   std::vector<uint32_t>* out, std::string* err) {
  if (V < 1) return fail(err, "text bias: V = %ld", (long)V);
  if (n_tokens < 0 || n_tokens > DSM_BIAS_MAX_TOKENS || (n_tokens > 0 && !tokens))
    return fail(err, "text bias: %ld token biases, 0 .. %ld allowed", (long)n_tokens, (long)DSM_BIAS_MAX_TOKENS);
  if (n_keywords < 0 || (n_keywords > 0 && !keywords)) return fail(err, "text bias: %ld keywords", (long)n_keywords);
  std::vector<std::pair<uint32_t, uint32_t>> tb;
  for (int i = 0; i < n_tokens; ++i) {
    if (tokens[i].token >= (uint32_t)V) return fail(err, "text bias: token bias %ld names token %ld outside the vocabulary", (long)i, (long)tokens[i].token);
    const uint32_t bits = dsm_f32_as_u32(tokens[i].bias);
    if (!finite_f32(tokens[i].bias) && bits != 0xFF800000u) return fail(err, "text bias: token bias %ld is +inf or NaN (finite or -inf allowed)", (long)i);
    tb.emplace_back(tokens[i].token, bits);
  }
  std::sort(tb.begin(), tb.end());
  for (size_t i = 1; i < tb.size(); ++i)
    if (tb[i].first == tb[i - 1].first) return fail(err, "text bias: token %ld is listed twice", (long)tb[i].first);
  // the trie in insertion order: per node a sorted map token -> (boost, child)
  struct Edge { float boost; uint32_t child; };
  std::vector<std::map<uint32_t, Edge>> nodes(1);
  for (int k = 0; k < n_keywords; ++k) {
    const dsm_bias_keyword& kw = keywords[k];
    if (kw.n_tokens < 1 || kw.n_tokens > DSM_BIAS_MAX_KEYWORD_TOKENS || !kw.tokens)
      return fail(err, "text bias: keyword %ld has %ld pieces, 1 .. 32 allowed", (long)k, (long)kw.n_tokens);
    if (!finite_f32(kw.boost) || !(kw.boost > 0.0f)) return fail(err, "text bias: the boost of keyword %ld is not a finite value above 0", (long)k);
    for (int i = 0; i < kw.n_tokens; ++i)
      if (kw.tokens[i] >= (uint32_t)V || kw.tokens[i] == 0 || kw.tokens[i] == 3)
        return fail(err, "text bias: keyword %ld holds piece %ld (outside the vocabulary, or a word terminator 0 / 3)", (long)k, (long)kw.tokens[i]);
    uint32_t at = 0;
    for (int i = 0; i < kw.n_tokens; ++i) {
      auto it = nodes[at].find(kw.tokens[i]);
      if (it == nodes[at].end()) {
        if (nodes.size() >= DSM_BIAS_MAX_NODES) return fail(err, "text bias: the keywords need more than %ld trie nodes", (long)DSM_BIAS_MAX_NODES);
        const uint32_t child = (uint32_t)nodes.size();
        nodes.emplace_back();  // (invalidates `it`, which is not used again)
        nodes[at].emplace(kw.tokens[i], Edge{kw.boost, child});
        at = child;
      } else {
        if (kw.boost > it->second.boost) it->second.boost = kw.boost;
        at = it->second.child;
      }
    }
  }
  // breadth first: `order` lists the old ids in their new numbering; a sorted map walk appends children in token order
  std::vector<uint32_t> order{0};
  order.reserve(nodes.size());
  for (size_t i = 0; i < order.size(); ++i)
    for (const auto& kv : nodes[order[i]]) order.push_back(kv.second.child);
  const uint32_t nn = (uint32_t)nodes.size(), ne = nn - 1, nt = (uint32_t)tb.size();
  std::vector<uint32_t> w;
  w.reserve(DSM_BIAS_HEADER_WORDS + 2 * nt + nn + 1 + 3 * ne);
  w.insert(w.end(), {DSM_BIAS_MAGIC, DSM_BIAS_VERSION, (uint32_t)V, nt, nn, ne, 0u, 0u});
  for (const auto& p : tb) { w.push_back(p.first); w.push_back(p.second); }
  uint32_t e = 0;
  for (uint32_t i = 0; i < nn; ++i) { w.push_back(e); e += (uint32_t)nodes[order[i]].size(); }
  w.push_back(e);
  e = 0;
  for (uint32_t i = 0; i < nn; ++i)
    for (const auto& kv : nodes[order[i]]) {
      w.push_back(kv.first);
      w.push_back(dsm_f32_as_u32(kv.second.boost));
      w.push_back(++e);  // the child's new number: children are appended to `order` in exactly this sequence
    }
  w[6] = (uint32_t)w.size();
  *out = std::move(w);
  return 0;
}

/* dsm_text_bias_pick_host behind its argument checks */
inline int pick_host(const uint32_t* table, size_t words, uint32_t node, const float* logits, int V, float temperature, const uint32_t* key,
                     uint64_t pos, uint32_t* token, uint32_t* node_out, std::string* err) {
  if (!logits || !token || !node_out || V < 1) return fail(err, "text bias pick: a NULL pointer or V < 1");
  if (!(temperature <= 0.0f) && !(temperature > 0.0f)) return fail(err, "text bias pick: temperature is NaN");
  if (temperature > 0.0f && !key) return fail(err, "text bias pick: temperature > 0 needs the 8 key words");
  if (temperature > 0.0f && pos % 16) return fail(err, "text bias pick: stream position %ld is not a multiple of 16", (long)pos);
  if (!table && words) return fail(err, "text bias pick: NULL table of %ld words", (long)words);
  if (table) {
    long mx = -1;
    if (int rc = check(table, words, err, &mx)) return rc;
    if (mx >= (long)V) return fail(err, "text bias pick: the table names token %ld, the row has %ld entries", mx, (long)V);
    if (node != DSM_BIAS_DEAD && node >= table[4]) return fail(err, "text bias pick: node %ld of %ld", (long)node, (long)table[4]);
  }
  std::vector<float> x((size_t)V);
  dsm_text_bias_pick_row(table, node, logits, V, temperature, key, pos, x.data(), token, node_out);
  return 0;
}

}  // namespace dsm_text_bias
#endif /* host */

#endif /* DSM_TEXT_BIAS_H */
