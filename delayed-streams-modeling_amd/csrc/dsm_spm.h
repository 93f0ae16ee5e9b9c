/*
 * dsm_spm.h — host-only SentencePiece tokenizer: the subset the reference's servers use (`text_tokenizer.encode(word)`,
 * srv/tts.rs:485; `decode_piece_ids`, srv/batched_asr.rs:667, srv/tts.rs:598) for UNIGRAM models.  No HIP include: plain
 * C++17, like dsm_safetensors.h.  Included once per binary (it defines the dsm_spm_* entry points of include/dsm.h).
 *
 *   model file   a serialized ModelProto, read with a bounds-checked protobuf wire parser (varint, 64-bit, length-delimited,
 *                32-bit; unknown fields skipped).  The file is untrusted: every length is checked against the buffer, a
 *                failure is DSM_ERR_IO with a message, and nothing of the file is executed.
 *   normalizer   the precompiled charsmap (u32 trie size, a Darts double-array of u32 units, a pool of NUL-terminated
 *                replacements), longest prefix at each position, else one UTF-8 character (a malformed byte: U+FFFD, one
 *                byte consumed); then remove_extra_whitespaces, the dummy prefix, spaces -> U+2581.
 *   encode       the best unigram path as SentencePieceProcessor::Encode's optimized Viterbi computes it (same order of
 *                candidates, same comparisons, same float widths: ties break the same way), unknown characters at
 *                min_score - 10, consecutive unknowns merged, byte fallback.
 *   decode       DecodeIds: control pieces vanish, unk -> unk_surface, byte runs -> UTF-8 (invalid bytes -> U+FFFD),
 *                U+2581 -> space, the leading dummy-prefix space stripped, an id >= piece count is an error.
 * Refused (DSM_ERR_INVALID): BPE / WORD / CHAR models, USER_DEFINED pieces, treat_whitespace_as_suffix, a denormalizer
 * charsmap — see DESIGN.md.  A loaded model is immutable: any number of threads may encode and decode with it.
 */
#ifndef DSM_SPM_H
#define DSM_SPM_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dsm.h"

namespace dsm_spm_ns {

enum PieceType { NORMAL = 1, UNKNOWN = 2, CONTROL = 3, USER_DEFINED = 4, UNUSED = 5, BYTE = 6 };

// ---- protobuf wire format ----
struct Pb {
  const uint8_t* p;
  size_t n, o = 0;
  bool varint(uint64_t& v) {
    v = 0;
    for (int s = 0; s < 70; s += 7) {
      if (o >= n) return false;
      const uint8_t b = p[o++];
      if (s < 64) v |= (uint64_t)(b & 0x7f) << s;
      if (!(b & 0x80)) return true;
    }
    return false;  // longer than ten bytes
  }
  bool fixed(int k, uint64_t& v) {
    if ((size_t)k > n - o) return false;
    v = 0;
    for (int i = 0; i < k; ++i) v |= (uint64_t)p[o + i] << (8 * i);
    o += (size_t)k;
    return true;
  }
  bool bytes(const uint8_t*& q, size_t& len) {
    uint64_t l;
    if (!varint(l) || l > n - o) return false;
    q = p + o;
    len = (size_t)l;
    o += len;
    return true;
  }
  bool key(uint32_t& field, int& wt) {
    uint64_t k;
    if (!varint(k) || (k >> 3) == 0 || (k >> 3) > 0x1fffffffu) return false;
    field = (uint32_t)(k >> 3);
    wt = (int)(k & 7);
    return true;
  }
  bool skip(int wt) {
    uint64_t v;
    const uint8_t* q;
    size_t len;
    switch (wt) {
      case 0: return varint(v);
      case 1: return fixed(8, v);
      case 2: return bytes(q, len);
      case 5: return fixed(4, v);
      default: return false;  // groups are not part of this schema
    }
  }
  bool done() const { return o >= n; }
};

struct Piece {
  std::string s;
  float score = 0.0f;
  int type = NORMAL;
};

struct Model {
  std::vector<Piece> pieces;
  // trainer_spec / normalizer_spec: field numbers and defaults of sentencepiece_model.proto
  int model_type = 1;
  bool byte_fallback = false, ws_suffix = false;
  int unk_id = 0, bos_id = 1, eos_id = 2, pad_id = -1;
  std::string unk_surface = " \xE2\x81\x87 ";
  bool add_dummy_prefix = true, remove_extra_ws = true, escape_ws = true;
  std::string charsmap;
  bool denorm_charsmap = false;
  // derived at load
  int unk = -1;  // the piece of type UNKNOWN
  float min_score = 0.0f;
  int byte_id[256];
  std::vector<uint32_t> nt;  // normalizer double-array
  std::string pool;          // replacement strings
  // piece trie over bytes: node k owns edges [first[k], first[k + 1]) sorted by label
  std::vector<int32_t> node_id;
  std::vector<uint32_t> first, target;
  std::vector<uint8_t> label;
};

inline bool parse_piece(Pb r, Piece& out) {
  while (!r.done()) {
    uint32_t f; int wt; uint64_t v; const uint8_t* q; size_t len;
    if (!r.key(f, wt)) return false;
    if (f == 1 && wt == 2) { if (!r.bytes(q, len)) return false; out.s.assign((const char*)q, len); }
    else if (f == 2 && wt == 5) { if (!r.fixed(4, v)) return false; const uint32_t u = (uint32_t)v; memcpy(&out.score, &u, 4); }
    else if (f == 3 && wt == 0) { if (!r.varint(v)) return false; out.type = (int)(int64_t)v; }
    else if (!r.skip(wt)) return false;
  }
  return true;
}

inline bool parse_trainer(Pb r, Model& m) {
  while (!r.done()) {
    uint32_t f; int wt; uint64_t v; const uint8_t* q; size_t len;
    if (!r.key(f, wt)) return false;
    if (wt == 0 && (f == 3 || f == 24 || f == 35 || (f >= 40 && f <= 43))) {
      if (!r.varint(v)) return false;
      const int iv = (int)(int64_t)v;  // int32 fields travel sign-extended to 64 bits
      switch (f) {
        case 3: m.model_type = iv; break;
        case 24: m.ws_suffix = v != 0; break;
        case 35: m.byte_fallback = v != 0; break;
        case 40: m.unk_id = iv; break;
        case 41: m.bos_id = iv; break;
        case 42: m.eos_id = iv; break;
        default: m.pad_id = iv; break;
      }
    } else if (f == 44 && wt == 2) { if (!r.bytes(q, len)) return false; m.unk_surface.assign((const char*)q, len); }
    else if (!r.skip(wt)) return false;
  }
  return true;
}

inline bool parse_normalizer(Pb r, Model& m, bool denorm) {
  while (!r.done()) {
    uint32_t f; int wt; uint64_t v; const uint8_t* q; size_t len;
    if (!r.key(f, wt)) return false;
    if (f == 2 && wt == 2) {
      if (!r.bytes(q, len)) return false;
      if (denorm) m.denorm_charsmap = len > 0; else m.charsmap.assign((const char*)q, len);
    } else if (wt == 0 && f >= 3 && f <= 5) {
      if (!r.varint(v)) return false;
      if (denorm) continue;
      if (f == 3) m.add_dummy_prefix = v != 0; else if (f == 4) m.remove_extra_ws = v != 0; else m.escape_ws = v != 0;
    } else if (!r.skip(wt)) return false;
  }
  return true;
}

inline int byte_of_piece(const std::string& s) {  // "<0xNN>", upper-case hex as ByteToPiece writes it
  if (s.size() != 6 || s[0] != '<' || s[1] != '0' || s[2] != 'x' || s[5] != '>') return -1;
  int v = 0;
  for (int i = 3; i < 5; ++i) {
    const char c = s[i];
    if (c >= '0' && c <= '9') v = v * 16 + (c - '0'); else if (c >= 'A' && c <= 'F') v = v * 16 + (c - 'A' + 10); else return -1;
  }
  return v;
}

inline void build_trie(Model& m) {
  std::vector<std::pair<std::string, int>> keys;
  for (size_t i = 0; i < m.pieces.size(); ++i)
    if (m.pieces[i].type == NORMAL || m.pieces[i].type == UNUSED) keys.emplace_back(m.pieces[i].s, (int)i);
  std::sort(keys.begin(), keys.end());
  struct Span { size_t lo, hi, depth; };
  std::vector<Span> q;
  q.push_back(Span{0, keys.size(), 0});
  for (size_t k = 0; k < q.size(); ++k) {  // breadth first: node index = position in q
    Span sp = q[k];
    int32_t id = -1;
    if (sp.lo < sp.hi && keys[sp.lo].first.size() == sp.depth) id = keys[sp.lo++].second;
    m.node_id.push_back(id);
    m.first.push_back((uint32_t)m.label.size());
    for (size_t i = sp.lo; i < sp.hi;) {
      const uint8_t c = (uint8_t)keys[i].first[sp.depth];
      size_t j = i;
      while (j < sp.hi && (uint8_t)keys[j].first[sp.depth] == c) ++j;
      m.label.push_back(c);
      m.target.push_back((uint32_t)q.size());
      q.push_back(Span{i, j, sp.depth + 1});
      i = j;
    }
  }
  m.first.push_back((uint32_t)m.label.size());
}

inline const char* model_type_name(int t) { return t == 2 ? "BPE" : t == 3 ? "WORD" : t == 4 ? "CHAR" : "unknown"; }

// 0, or DSM_ERR_IO (malformed) / DSM_ERR_INVALID (well-formed but outside the supported subset) with a message
inline int load(const uint8_t* data, size_t len, Model& m, std::string& err) {
  Pb r{data, len};
  bool have_trainer = false, have_norm = false;
  while (!r.done()) {
    uint32_t f; int wt; const uint8_t* q; size_t n;
    if (!r.key(f, wt)) { err = "model file: truncated or malformed field key at byte " + std::to_string(r.o); return DSM_ERR_IO; }
    if (wt == 2 && (f == 1 || f == 2 || f == 3 || f == 5)) {
      if (!r.bytes(q, n)) { err = "model file: field " + std::to_string(f) + " runs past the end of the file"; return DSM_ERR_IO; }
      bool ok;
      if (f == 1) { m.pieces.emplace_back(); ok = parse_piece(Pb{q, n}, m.pieces.back()); }
      else if (f == 2) { ok = parse_trainer(Pb{q, n}, m); have_trainer = true; }
      else { ok = parse_normalizer(Pb{q, n}, m, f == 5); have_norm = have_norm || f == 3; }
      if (!ok) { err = "model file: malformed sub-message in field " + std::to_string(f); return DSM_ERR_IO; }
    } else if (!r.skip(wt)) { err = "model file: malformed field " + std::to_string(f) + " at byte " + std::to_string(r.o); return DSM_ERR_IO; }
  }
  if (m.pieces.empty()) { err = "model file: no pieces (not a SentencePiece model, or truncated)"; return DSM_ERR_IO; }
  // the trainer writes both specs into every model file, behind the pieces: a file without them was cut short
  if (!have_trainer || !have_norm) { err = std::string("model file: no ") + (have_trainer ? "normalizer_spec" : "trainer_spec") + " (truncated?)"; return DSM_ERR_IO; }
  if (m.model_type != 1) { err = std::string("model type ") + model_type_name(m.model_type) + " is not supported: UNIGRAM only"; return DSM_ERR_INVALID; }
  if (m.ws_suffix) { err = "treat_whitespace_as_suffix models are not supported"; return DSM_ERR_INVALID; }
  if (m.denorm_charsmap) { err = "models with a denormalizer charsmap are not supported"; return DSM_ERR_INVALID; }
  bool byte_found[256] = {false};
  for (int b = 0; b < 256; ++b) m.byte_id[b] = -1;
  bool have_normal = false;
  for (size_t i = 0; i < m.pieces.size(); ++i) {
    const Piece& p = m.pieces[i];
    if (p.s.empty()) { err = "piece " + std::to_string(i) + " is empty"; return DSM_ERR_IO; }
    switch (p.type) {
      case NORMAL: m.min_score = have_normal ? std::min(m.min_score, p.score) : p.score; have_normal = true; break;
      case UNKNOWN: if (m.unk >= 0) { err = "the model defines two unknown pieces"; return DSM_ERR_IO; } m.unk = (int)i; break;
      case CONTROL: case UNUSED: break;
      case USER_DEFINED: err = "models with USER_DEFINED pieces are not supported (piece " + std::to_string(i) + ")"; return DSM_ERR_INVALID;
      case BYTE: {
        const int b = byte_of_piece(p.s);
        if (!m.byte_fallback || b < 0) { err = "byte piece " + std::to_string(i) + " is invalid"; return DSM_ERR_IO; }
        byte_found[b] = true; m.byte_id[b] = (int)i; break;
      }
      default: err = "piece " + std::to_string(i) + " has unknown type " + std::to_string(p.type); return DSM_ERR_IO;
    }
  }
  if (m.unk < 0) { err = "the model defines no unknown piece"; return DSM_ERR_IO; }
  if (m.byte_fallback)
    for (int b = 0; b < 256; ++b) if (!byte_found[b]) { err = "byte_fallback is set but the model lacks byte pieces"; return DSM_ERR_IO; }
  {  // a piece string names one id (ModelInterface::InitializePieces refuses duplicates)
    std::vector<const std::string*> v;
    for (const Piece& p : m.pieces) v.push_back(&p.s);
    std::sort(v.begin(), v.end(), [](const std::string* a, const std::string* b) { return *a < *b; });
    for (size_t i = 1; i < v.size(); ++i) if (*v[i] == *v[i - 1]) { err = "piece \"" + *v[i] + "\" is defined twice"; return DSM_ERR_IO; }
  }
  if (!m.charsmap.empty()) {
    const size_t n = m.charsmap.size();
    uint32_t tsz = 0;
    if (n > 4) memcpy(&tsz, m.charsmap.data(), 4);  // little-endian, as the hosts this library builds for
    if (n <= 4 || tsz < 4 || tsz % 4 != 0 || tsz >= n - 4) { err = "the precompiled charsmap is broken"; return DSM_ERR_IO; }
    m.nt.resize(tsz / 4);
    memcpy(m.nt.data(), m.charsmap.data() + 4, tsz);
    m.pool.assign(m.charsmap.data() + 4 + tsz, n - 4 - tsz);
    m.charsmap.clear();
    m.charsmap.shrink_to_fit();
  }
  build_trie(m);
  return 0;
}

// ---- normalizer ----
// string_util::DecodeUTF8 + IsValidDecodeUTF8: the length of the well-formed character at p, or 0
inline size_t valid_char_len(const uint8_t* p, size_t n) {
  auto trail = [](uint8_t c) { return (c & 0xc0) == 0x80; };
  auto scalar = [](uint32_t c) { return c < 0xd800 || (c >= 0xe000 && c <= 0x10ffff); };
  if (n == 0) return 0;
  if (p[0] < 0x80) return 1;
  if (n >= 2 && (p[0] & 0xe0) == 0xc0) {
    const uint32_t c = ((uint32_t)(p[0] & 0x1f) << 6) | (p[1] & 0x3f);
    return trail(p[1]) && c >= 0x80 ? 2 : 0;
  }
  if (n >= 3 && (p[0] & 0xf0) == 0xe0) {
    const uint32_t c = ((uint32_t)(p[0] & 0x0f) << 12) | ((uint32_t)(p[1] & 0x3f) << 6) | (p[2] & 0x3f);
    return trail(p[1]) && trail(p[2]) && c >= 0x800 && scalar(c) ? 3 : 0;
  }
  if (n >= 4 && (p[0] & 0xf8) == 0xf0) {
    const uint32_t c = ((uint32_t)(p[0] & 0x07) << 18) | ((uint32_t)(p[1] & 0x3f) << 12) | ((uint32_t)(p[2] & 0x3f) << 6) | (p[3] & 0x3f);
    return trail(p[1]) && trail(p[2]) && trail(p[3]) && c >= 0x10000 && scalar(c) ? 4 : 0;
  }
  return 0;
}

// Normalizer::NormalizePrefix: the replacement for the longest charsmap key that is a prefix of [p, p + n), else one character
inline void normalize_prefix(const Model& m, const uint8_t* p, size_t n, const char*& out, size_t& out_len, size_t& consumed) {
  size_t longest = 0;
  uint32_t value = 0;
  if (!m.nt.empty()) {  // Darts::DoubleArray::commonPrefixSearch, every index checked against the array
    const size_t units = m.nt.size();
    auto offset = [](uint32_t u) { return (size_t)((u >> 10) << ((u & (1u << 9)) >> 6)); };
    size_t pos = 0;
    uint32_t u = m.nt[0];
    pos ^= offset(u);
    for (size_t i = 0; i < n; ++i) {
      pos ^= p[i];
      if (pos >= units) break;
      u = m.nt[pos];
      if ((u & ((1u << 31) | 0xff)) != p[i]) break;
      pos ^= offset(u);
      if (pos >= units) break;
      if ((u >> 8) & 1) { longest = i + 1; value = m.nt[pos] & ((1u << 31) - 1); }
    }
  }
  if (longest == 0) {
    const size_t k = valid_char_len(p, n);
    if (k == 0) { out = "\xEF\xBF\xBD"; out_len = 3; consumed = 1; }
    else { out = (const char*)p; out_len = k; consumed = k; }
    return;
  }
  consumed = longest;
  if (value >= m.pool.size()) { out = ""; out_len = 0; return; }  // a hostile file: the real ones point into the pool
  out = m.pool.c_str() + value;  // NUL-terminated: std::string ends the pool with one
  out_len = strlen(out);
}

inline void normalize(const Model& m, const uint8_t* p, size_t n, std::string& out) {  // Normalizer::Normalize
  out.clear();
  const char* s; size_t sl, used;
  if (m.remove_extra_ws)
    while (n > 0) {
      normalize_prefix(m, p, n, s, sl, used);
      if (!(sl == 1 && s[0] == ' ')) break;
      p += used; n -= used;
    }
  if (n == 0) return;
  static const char kSpace[] = "\xE2\x96\x81";
  auto add_ws = [&] { if (m.escape_ws) out.append(kSpace, 3); else out.push_back(' '); };
  if (m.add_dummy_prefix) add_ws();
  bool prev_space = m.remove_extra_ws;
  while (n > 0) {
    normalize_prefix(m, p, n, s, sl, used);
    while (prev_space && sl > 0 && s[0] == ' ') { ++s; --sl; }
    if (sl > 0) {
      for (size_t i = 0; i < sl; ++i) {
        if (m.escape_ws && s[i] == ' ') out.append(kSpace, 3); else out.push_back(s[i]);
      }
      prev_space = s[sl - 1] == ' ';
    }
    p += used; n -= used;
    if (!m.remove_extra_ws) prev_space = false;
  }
  if (m.remove_extra_ws) {
    const char* sp = m.escape_ws ? kSpace : " ";
    const size_t k = m.escape_ws ? 3 : 1;
    while (out.size() >= k && memcmp(out.data() + out.size() - k, sp, k) == 0) out.resize(out.size() - k);
  }
}

// ---- encode: unigram::Model::EncodeOptimized + SentencePieceProcessor::PopulateSentencePieceText ----
inline void encode(const Model& m, const uint8_t* text, size_t len, std::vector<uint32_t>& ids) {
  ids.clear();
  std::string norm;
  normalize(m, text, len, norm);
  if (norm.empty()) return;
  struct Best { int id = -1; float score = 0.0f; int start = -1; };
  const int size = (int)norm.size();
  const uint8_t* z = (const uint8_t*)norm.data();
  const float unk_score = m.min_score - 10.0f;
  std::vector<Best> best((size_t)size + 1);
  static const uint8_t kLen[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 4};
  int at = 0;
  while (at < size) {
    const float here = best[at].score;
    const int mblen = std::min<int>(kLen[z[at] >> 4], size - at);
    bool single = false;
    uint32_t node = 0;
    for (int key = at; key < size;) {
      const uint8_t c = z[key];
      const uint8_t* lo = m.label.data() + m.first[node];
      const uint8_t* hi = m.label.data() + m.first[node + 1];
      const uint8_t* e = std::lower_bound(lo, hi, c);
      if (e == hi || *e != c) break;
      node = m.target[(size_t)(e - m.label.data())];
      ++key;
      const int id = m.node_id[node];
      if (id < 0 || m.pieces[id].type == UNUSED) continue;
      Best& t = best[key];
      const float cand = m.pieces[id].score + here;  // f32 sums; a later candidate wins only when strictly better
      if (t.start == -1 || cand > t.score) { t.score = cand; t.start = at; t.id = id; }
      if (!single && key - at == mblen) single = true;
    }
    if (!single) {
      Best& t = best[at + mblen];
      const float cand = unk_score + here;
      if (t.start == -1 || cand > t.score) { t.score = cand; t.start = at; t.id = m.unk; }
    }
    at += mblen;
  }
  std::vector<std::pair<int, int>> path;  // (start, id), last piece first
  for (int end = size; end > 0;) {
    const Best& b = best[end];
    if (b.start < 0 || b.start >= end) { ids.clear(); return; }  // cannot happen: every character boundary is reached
    path.emplace_back(b.start, b.id);
    end = b.start;
  }
  bool prev_unk = false;
  int end = 0;
  for (size_t k = path.size(); k-- > 0;) {
    const int start = path[k].first, id = path[k].second;
    end = k > 0 ? path[k - 1].first : size;
    const bool is_unk = id == m.unk;
    if (is_unk && m.byte_fallback) {
      for (int i = start; i < end; ++i) ids.push_back((uint32_t)m.byte_id[z[i]]);
    } else if (!(prev_unk && is_unk)) {
      ids.push_back((uint32_t)id);
    }
    prev_unk = is_unk;
  }
}

// ---- decode: SentencePieceProcessor::Decode over IdToPiece of every id ----
inline int decode(const Model& m, const uint32_t* ids, size_t n, std::string& out, std::string& err) {
  out.clear();
  for (size_t i = 0; i < n; ++i)
    if (ids[i] >= m.pieces.size()) {
      err = "piece id " + std::to_string(ids[i]) + " is out of range (the model has " + std::to_string(m.pieces.size()) + " pieces)";
      return DSM_ERR_INVALID;
    }
  static const char kSpace[] = "\xE2\x96\x81";
  std::string bytes;
  auto flush_bytes = [&] {
    for (size_t o = 0; o < bytes.size();) {
      const size_t k = valid_char_len((const uint8_t*)bytes.data() + o, bytes.size() - o);
      if (k == 0) { out += "\xEF\xBF\xBD"; o += 1; }
      else { out.append(bytes, o, k); o += k; }
    }
    bytes.clear();
  };
  bool ws_taken = false;  // the dummy prefix was consumed (models that keep extra whitespace strip one U+2581 only)
  for (size_t i = 0; i < n; ++i) {
    const Piece& p = m.pieces[ids[i]];
    if (p.type == BYTE) { bytes.push_back((char)byte_of_piece(p.s)); continue; }
    flush_bytes();
    if (p.type == CONTROL) continue;
    if (p.type == UNKNOWN) { out += m.unk_surface; continue; }
    const char* s = p.s.data();
    size_t sl = p.s.size();
    bool seen = false;
    if (!ws_taken && out.empty() && (m.add_dummy_prefix || m.remove_extra_ws)) {  // nothing decoded yet, byte pieces included
      if (sl >= 3 && memcmp(s, kSpace, 3) == 0) { s += 3; sl -= 3; seen = true; }
      if (m.remove_extra_ws) seen = false;  // keep stripping until text appears
    }
    for (size_t k = 0; k < sl;) {
      if (sl - k >= 3 && memcmp(s + k, kSpace, 3) == 0) { out.push_back(' '); k += 3; }
      else out.push_back(s[k++]);
    }
    if (seen) ws_taken = true;
  }
  flush_bytes();
  return 0;
}

}  // namespace dsm_spm_ns

struct dsm_spm {
  dsm_spm_ns::Model m;
};

namespace dsm_spm_ns {
inline std::string& load_error() {  // dsm_spm_last_error(NULL): the calling thread's last failed load
  static thread_local std::string e;
  return e;
}
inline std::string& use_error() {  // a failed dsm_spm_decode of this thread: the tokenizer itself stays immutable
  static thread_local std::string e;
  return e;
}
inline int load_file(const char* path, std::vector<uint8_t>& buf, std::string& err) {
  FILE* f = fopen(path, "rb");
  if (!f) { err = std::string("cannot open ") + path; return DSM_ERR_IO; }
  uint8_t tmp[1 << 16];
  size_t k;
  while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) {
    buf.insert(buf.end(), tmp, tmp + k);
    if (buf.size() > ((size_t)1 << 30)) { fclose(f); err = std::string(path) + " is larger than 1 GiB: not a tokenizer model"; return DSM_ERR_IO; }
  }
  fclose(f);
  return 0;
}
}  // namespace dsm_spm_ns

extern "C" {

int dsm_spm_load_bytes(const uint8_t* bytes, size_t len, dsm_spm** out) {
  if (!out || (!bytes && len)) return DSM_ERR_INVALID;
  *out = nullptr;
  dsm_spm* t = new dsm_spm();
  const int rc = dsm_spm_ns::load(bytes, len, t->m, dsm_spm_ns::load_error());
  if (rc) { delete t; return rc; }
  *out = t;
  return 0;
}

int dsm_spm_load(const char* path, dsm_spm** out) {
  if (!path || !out) return DSM_ERR_INVALID;
  *out = nullptr;
  std::vector<uint8_t> buf;
  if (int rc = dsm_spm_ns::load_file(path, buf, dsm_spm_ns::load_error())) return rc;
  return dsm_spm_load_bytes(buf.data(), buf.size(), out);
}

void dsm_spm_free(dsm_spm* t) { delete t; }

const char* dsm_spm_last_error(const dsm_spm* t) { return t ? dsm_spm_ns::use_error().c_str() : dsm_spm_ns::load_error().c_str(); }

int dsm_spm_vocab_size(const dsm_spm* t) { return t ? (int)t->m.pieces.size() : DSM_ERR_INVALID; }

int dsm_spm_special_ids(const dsm_spm* t, int* unk, int* bos, int* eos, int* pad) {
  if (!t) return DSM_ERR_INVALID;
  const dsm_spm_ns::Model& m = t->m;
  auto control = [&](int id) { return id >= 0 && (size_t)id < m.pieces.size() && m.pieces[id].type == dsm_spm_ns::CONTROL ? id : -1; };
  if (unk) *unk = m.unk;
  if (bos) *bos = control(m.bos_id);
  if (eos) *eos = control(m.eos_id);
  if (pad) *pad = control(m.pad_id);
  return 0;
}

int64_t dsm_spm_encode(const dsm_spm* t, const char* utf8, size_t len, uint32_t* ids_out, size_t cap) {
  if (!t || (!utf8 && len)) return DSM_ERR_INVALID;
  std::vector<uint32_t> ids;
  dsm_spm_ns::encode(t->m, (const uint8_t*)utf8, len, ids);
  if (ids_out && ids.size() <= cap && !ids.empty()) memcpy(ids_out, ids.data(), sizeof(uint32_t) * ids.size());
  return (int64_t)ids.size();
}

int64_t dsm_spm_decode(const dsm_spm* t, const uint32_t* ids, size_t n, char* out, size_t cap) {
  if (!t || (!ids && n)) return DSM_ERR_INVALID;
  std::string s;
  if (int rc = dsm_spm_ns::decode(t->m, ids, n, s, dsm_spm_ns::use_error())) return rc;
  if (out && s.size() <= cap && !s.empty()) memcpy(out, s.data(), s.size());
  return (int64_t)s.size();
}

}  // extern "C"

#endif  // DSM_SPM_H
