// dsm_text_bias.inc — the engine half of the text-bias section of include/dsm.h (included by dsm_engine.hip behind
// dsm_slot_state.inc): bias sets as device-resident objects that slots attach to by reference — the pattern of the TTS voices —
// the per-slot attachment and trie node, the engine-wide switch, the two host functions and the kernel's test aid.  The
// definition, the table format and its compiler are csrc/dsm_text_bias.h; the kernel is lm_pick_biased_kernel (dsm_kernels.h);
// lm_group_body launches it, dsm_asr_reset_slot and the slot importer reposition the node (bias_put_node).

namespace {

// The section's device buffers, once per engine.  Allocations take the exclusive side of api_mu (never beside a capture), so
// this runs BEFORE the caller takes its shared hold.
int bias_ensure(dsm_engine* e) {
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  if (e->bias_slot_node) return 0;
  const size_t B = (size_t)e->B;
  if (!e->bias_sets_d)
    if (int rc = e->dalloc(&e->bias_sets_d, (size_t)DSM_BIAS_MAX_SETS)) return rc;  // zeroed: every entry "no table"
  if (!e->bias_slot_set)
    if (int rc = e->dalloc(&e->bias_slot_set, B)) return rc;
  e->bias_slot_handle.assign(B, 0);
  uint32_t* nodes = nullptr;
  if (int rc = e->dalloc(&nodes, B)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));  // the fills ran on the null stream, which the engine's streams are not ordered against
  e->bias_slot_node = nodes;  // last: the test above and bias_put_node read it
  return 0;
}

// model stream and every group stream: what a step of the LM has in flight (the encoder stream does not touch the section)
int bias_sync_model(dsm_engine* e) {
  HIPCHK(hipStreamSynchronize(e->s_model));
  for (hipStream_t gs : e->s_grp)
    if (gs) HIPCHK(hipStreamSynchronize(gs));
  return 0;
}

// where a slot's node stands when the engine cannot have followed it: the root before the stream's first step, else DEAD
uint32_t bias_unknown_node(const dsm_engine* e, int slot) { return e->items[(size_t)slot].step_idx == 0 ? 0u : DSM_BIAS_DEAD; }

int bias_find(dsm_engine* e, int set, dsm_engine::BiasSet** out) {
  auto it = e->bias_sets.find(set);
  if (set <= 0 || it == e->bias_sets.end()) {
    e->set_error("text bias: no set %d (never created, or destroyed)", set);
    return DSM_ERR_INVALID;
  }
  *out = &it->second;
  return 0;
}

// compiled words -> a set of the engine.  A failure leaves the engine as it was.
int bias_install(dsm_engine* e, std::vector<uint32_t>&& words, int* set_out) {
  if (int rc = bias_ensure(e)) return rc;
  uint32_t* d_table = nullptr;
  {
    std::unique_lock<std::shared_mutex> alone(e->api_mu);  // allocates: never beside a capture
    if (int rc = e->dalloc(&d_table, words.size(), false)) return rc;
  }
  ApiShared api(e);  // lock order of the section: api_mu, then bias_mu
  std::lock_guard<std::mutex> host(e->bias_mu);
  std::vector<char> used((size_t)DSM_BIAS_MAX_SETS, 0);
  for (const auto& kv : e->bias_sets) used[(size_t)kv.second.index] = 1;
  int index = 0;
  for (int i = 1; i < DSM_BIAS_MAX_SETS && !index; ++i)
    if (!used[(size_t)i]) index = i;
  if (!index) {
    e->dfree(d_table);
    e->set_error("text bias: %d sets exist, no room for another (destroy one)", DSM_BIAS_MAX_SETS - 1);
    return DSM_ERR_STATE;
  }
  BiasSetDesc d{d_table, words[3], words[4], words[5], 0u};
  // entry `index` is referenced by no slot, so no step in flight reads it: plain blocking copies
  hipError_t he = hipMemcpy(d_table, words.data(), sizeof(uint32_t) * words.size(), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(e->bias_sets_d + index, &d, sizeof d, hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    e->dfree(d_table);
    e->set_error("text bias: upload failed: %s", hipGetErrorString(he));
    return DSM_ERR_DEVICE;
  }
  const int handle = e->bias_next_handle++;
  dsm_engine::BiasSet& s = e->bias_sets[handle];
  s.index = index;
  s.words = std::move(words);
  s.d_table = d_table;
  *set_out = handle;
  return 0;
}

}  // namespace

extern "C" {

int dsm_text_bias_compile(const dsm_bias_token* tokens, int n_tokens, const dsm_bias_keyword* keywords, int n_keywords, int V,
                          uint32_t* words_out, size_t cap, size_t* needed) {
  std::vector<uint32_t> w;
  std::string err;
  if (int rc = dsm_text_bias::compile(tokens, n_tokens, keywords, n_keywords, V, &w, &err)) { g_create_error = err; return rc; }
  if (needed) *needed = w.size();
  if (!words_out) return 0;
  if (cap < w.size()) {
    g_create_error = "text bias: buffer of " + std::to_string(cap) + " words, the table needs " + std::to_string(w.size());
    return DSM_ERR_INVALID;
  }
  memcpy(words_out, w.data(), sizeof(uint32_t) * w.size());
  return 0;
}

int dsm_text_bias_pick_host(const uint32_t* table, size_t table_words, uint32_t node, const float* logits, int V, float temperature,
                            const uint32_t* rng_key, uint64_t rng_pos, uint32_t* token, uint32_t* node_out) {
  std::string err;
  const int rc = dsm_text_bias::pick_host(table, table_words, node, logits, V, temperature, rng_key, rng_pos, token, node_out, &err);
  if (rc) g_create_error = err;
  return rc;
}

int dsm_asr_set_text_bias(dsm_engine* e, int on) {
  if (!e) return DSM_ERR_INVALID;
  const int V = e->cfg.text_out_vocab_size;
  if (on && (V > DSM_SCORES_STAGE_MAX || V < 4)) {
    e->set_error("text bias: text_out_vocab_size %d is outside 4 .. %d (the pick stages the row in LDS)", V, DSM_SCORES_STAGE_MAX);
    return DSM_ERR_INVALID;
  }
  if (!on) {  // nothing to prepare: an engine that never used the section allocates nothing for it
    std::unique_lock<std::shared_mutex> alone(e->api_mu);  // between steps: waits for calls in progress
    e->bias_on = false;
    return 0;
  }
  if (int rc = bias_ensure(e)) return rc;
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // no step can be enqueued between the node upload and the switch
  if (e->bias_on) return 0;
  // the pick kernels of the "off" steps did not move the nodes: every attached slot starts where the engine knows it stands
  std::lock_guard<std::mutex> host(e->bias_mu);
  if (int rc = bias_sync_model(e)) return rc;
  std::vector<uint32_t> nodes((size_t)e->B);
  for (int b = 0; b < e->B; ++b) nodes[(size_t)b] = bias_unknown_node(e, b);
  HIPCHK(hipMemcpy(e->bias_slot_node, nodes.data(), sizeof(uint32_t) * nodes.size(), hipMemcpyHostToDevice));
  e->bias_on = true;
  return 0;
}

int dsm_asr_bias_create(dsm_engine* e, const dsm_bias_token* tokens, int n_tokens, const dsm_bias_keyword* keywords, int n_keywords,
                        int* set_out) {
  if (!e || !set_out) return DSM_ERR_INVALID;
  std::vector<uint32_t> w;
  std::string err;
  if (int rc = dsm_text_bias::compile(tokens, n_tokens, keywords, n_keywords, e->cfg.text_out_vocab_size, &w, &err)) {
    e->set_error("%s", err.c_str());
    return rc;
  }
  return bias_install(e, std::move(w), set_out);
}

int dsm_asr_bias_create_text(dsm_engine* e, const dsm_spm* spm, const char* const* words, const float* boosts, int n_words,
                             const dsm_bias_token* tokens, int n_tokens, int* set_out) {
  if (!e || !set_out || n_words < 0 || (n_words > 0 && (!spm || !words || !boosts))) return DSM_ERR_INVALID;
  const uint32_t V = (uint32_t)e->cfg.text_out_vocab_size;
  std::vector<std::vector<uint32_t>> pieces((size_t)n_words);
  std::vector<dsm_bias_keyword> kws((size_t)n_words);
  for (int i = 0; i < n_words; ++i) {
    const char* w = words[i];
    if (!w) { e->set_error("text bias: word %d is NULL", i); return DSM_ERR_INVALID; }
    const size_t len = strlen(w);
    for (size_t k = 0; k < len; ++k) {
      const unsigned char ch = (unsigned char)w[k];
      // ASCII whitespace, and the two Unicode spaces a transcript is likely to hold: U+00A0 (C2 A0) and U+3000 (E3 80 80)
      const bool ws = ch == ' ' || (ch >= '\t' && ch <= '\r') || (ch == 0xC2 && (unsigned char)w[k + 1] == 0xA0) ||
                      (ch == 0xE3 && (unsigned char)w[k + 1] == 0x80 && (unsigned char)w[k + 2] == 0x80);
      if (ws) { e->set_error("text bias: word %d contains whitespace: a keyword is one word", i); return DSM_ERR_INVALID; }
    }
    std::vector<uint32_t>& p = pieces[(size_t)i];
    p.resize(DSM_BIAS_MAX_KEYWORD_TOKENS);
    const int64_t n = dsm_spm_encode(spm, w, len, p.data(), p.size());
    if (n < 0) { e->set_error("text bias: word %d: %s", i, dsm_spm_last_error(spm)); return DSM_ERR_INVALID; }
    if (n == 0) { e->set_error("text bias: word %d encodes to nothing", i); return DSM_ERR_INVALID; }
    if (n > DSM_BIAS_MAX_KEYWORD_TOKENS) { e->set_error("text bias: word %d encodes to %lld pieces, at most %d", i, (long long)n, DSM_BIAS_MAX_KEYWORD_TOKENS); return DSM_ERR_INVALID; }
    p.resize((size_t)n);
    for (uint32_t id : p)
      if (id >= V || id == 0 || id == 3) {
        e->set_error("text bias: word %d yields piece %u (outside text_out_vocab_size %u, or a word terminator 0 / 3)", i, id, V);
        return DSM_ERR_INVALID;
      }
    kws[(size_t)i] = dsm_bias_keyword{p.data(), (int)n, boosts[i]};
  }
  return dsm_asr_bias_create(e, tokens, n_tokens, kws.data(), n_words, set_out);
}

int dsm_asr_bias_destroy(dsm_engine* e, int set) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  std::lock_guard<std::mutex> host(e->bias_mu);
  dsm_engine::BiasSet* s = nullptr;
  if (int rc = bias_find(e, set, &s)) return rc;
  if (s->refs > 0) { e->set_error("text bias: set %d is in use by %d slots", set, s->refs); return DSM_ERR_STATE; }
  if (int rc = bias_sync_model(e)) return rc;  // a step enqueued while a slot was still attached may be in flight
  const BiasSetDesc none{nullptr, 0u, 0u, 0u, 0u};
  HIPCHK(hipMemcpy(e->bias_sets_d + s->index, &none, sizeof none, hipMemcpyHostToDevice));
  e->dfree(s->d_table);
  e->bias_sets.erase(set);
  return 0;
}

int dsm_asr_bias_info(dsm_engine* e, int set, int* nodes, int* edges, int* tokens, int* refs, size_t* device_bytes) {
  if (!e) return DSM_ERR_INVALID;
  std::lock_guard<std::mutex> host(e->bias_mu);
  dsm_engine::BiasSet* s = nullptr;
  if (int rc = bias_find(e, set, &s)) return rc;
  if (nodes) *nodes = (int)s->words[4];
  if (edges) *edges = (int)s->words[5];
  if (tokens) *tokens = (int)s->words[3];
  if (refs) *refs = s->refs;
  if (device_bytes) *device_bytes = sizeof(uint32_t) * s->words.size();
  return 0;
}

int dsm_asr_set_bias(dsm_engine* e, int slot, int set) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  if (set < 0) { e->set_error("text bias: no set %d", set); return DSM_ERR_INVALID; }
  if (int rc = bias_ensure(e)) return rc;
  ApiShared api(e);
  std::lock_guard<std::mutex> host(e->bias_mu);
  dsm_engine::BiasSet* s = nullptr;
  if (set)
    if (int rc = bias_find(e, set, &s)) return rc;
  if (int rc = bias_sync_model(e)) return rc;
  const uint32_t index = s ? (uint32_t)s->index : 0u, node = s ? bias_unknown_node(e, slot) : DSM_BIAS_DEAD;
  HIPCHK(hipMemcpy(e->bias_slot_set + slot, &index, sizeof index, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->bias_slot_node + slot, &node, sizeof node, hipMemcpyHostToDevice));
  int& cur = e->bias_slot_handle[(size_t)slot];
  if (cur) e->bias_sets[cur].refs -= 1;
  if (s) s->refs += 1;
  cur = set;
  return 0;
}

int dsm_asr_bias_state(dsm_engine* e, int slot, int* set, uint32_t* node) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  std::lock_guard<std::mutex> host(e->bias_mu);
  const int cur = e->bias_slot_node ? e->bias_slot_handle[(size_t)slot] : 0;
  if (set) *set = cur;
  if (node) {
    *node = DSM_BIAS_DEAD;
    if (cur) {
      if (int rc = bias_sync_model(e)) return rc;
      HIPCHK(hipMemcpy(node, e->bias_slot_node + slot, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

int dsm_debug_text_pick(dsm_engine* e, int set, const float* logits, int n, int V, const uint32_t* nodes_in, float temperature,
                        const uint32_t* rng_keys, const uint64_t* rng_pos, uint32_t* tokens_out, uint32_t* nodes_out) {
  if (!e || !logits || !nodes_in || !tokens_out || !nodes_out || n < 1 || set < 0) return DSM_ERR_INVALID;
  if (V < 4 || V > DSM_SCORES_STAGE_MAX) { e->set_error("text pick: V = %d is outside 4 .. %d", V, DSM_SCORES_STAGE_MAX); return DSM_ERR_INVALID; }
  const bool gumbel = temperature > 0.0f;
  if (!(temperature <= 0.0f) && !gumbel) { e->set_error("text pick: temperature is NaN"); return DSM_ERR_INVALID; }
  if (gumbel && (!rng_keys || !rng_pos)) { e->set_error("text pick: temperature > 0 needs rng_keys and rng_pos"); return DSM_ERR_INVALID; }
  for (int i = 0; gumbel && i < n; ++i)
    if (rng_pos[i] % 16) { e->set_error("text pick: stream position of row %d is not a multiple of 16", i); return DSM_ERR_INVALID; }
  if (int rc = bias_ensure(e)) return rc;
  // allocates: never beside a capture.  Held from the set's lookup to the end of the launch, so that no dsm_asr_bias_destroy
  // (which holds the shared side) can take the set away in between.
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  uint32_t index = 0;
  {
    std::lock_guard<std::mutex> host(e->bias_mu);
    if (set) {
      dsm_engine::BiasSet* s = nullptr;
      if (int rc = bias_find(e, set, &s)) return rc;
      long mx = -1;
      std::string err;
      if (int rc = dsm_text_bias::check(s->words.data(), s->words.size(), &err, &mx)) { e->set_error("%s", err.c_str()); return rc; }
      if (mx >= (long)V) { e->set_error("text pick: set %d names token %ld, the rows have %d entries", set, mx, V); return DSM_ERR_INVALID; }
      for (int i = 0; i < n; ++i)
        if (nodes_in[i] != DSM_BIAS_DEAD && nodes_in[i] >= s->words[4]) {
          e->set_error("text pick: node %u of row %d, the set has %u", nodes_in[i], i, s->words[4]);
          return DSM_ERR_INVALID;
        }
      index = (uint32_t)s->index;
    }
  }
  const size_t rows = (size_t)n;
  float* d_logits = nullptr;
  uint32_t *d_key = nullptr, *d_set = nullptr, *d_node = nullptr, *d_out = nullptr, *d_tt = nullptr;
  unsigned long long* d_pos = nullptr;
  uint8_t *d_first = nullptr, *d_active = nullptr;
  int rc = e->dalloc(&d_logits, rows * (size_t)V, false);
  if (!rc) rc = e->dalloc(&d_key, rows * 8);
  if (!rc) rc = e->dalloc(&d_pos, rows);
  if (!rc) rc = e->dalloc(&d_set, rows, false);
  if (!rc) rc = e->dalloc(&d_node, rows, false);
  if (!rc) rc = e->dalloc(&d_out, rows, false);
  if (!rc) rc = e->dalloc(&d_tt, rows, false);
  if (!rc) rc = e->dalloc(&d_first, rows, false);
  if (!rc) rc = e->dalloc(&d_active, rows, false);
  hipStream_t st = e->s_model;
  const std::vector<uint32_t> sets(rows, index);
  const std::vector<uint8_t> ones(rows, 1);
  std::vector<unsigned long long> pos(rows, 0);
  for (size_t i = 0; gumbel && i < rows; ++i) pos[i] = (unsigned long long)rng_pos[i];
  auto run = [&]() -> int {
    HIPCHK(hipStreamSynchronize(nullptr));  // the zero fills of dalloc ran on the null stream
    HIPCHK(hipMemcpyAsync(d_logits, logits, sizeof(float) * rows * (size_t)V, hipMemcpyHostToDevice, st));
    if (gumbel) {
      HIPCHK(hipMemcpyAsync(d_key, rng_keys, sizeof(uint32_t) * rows * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_pos, pos.data(), sizeof(unsigned long long) * rows, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(d_set, sets.data(), sizeof(uint32_t) * rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_node, nodes_in, sizeof(uint32_t) * rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_active, ones.data(), rows, hipMemcpyHostToDevice, st));
    if (int lrc = launch_pick_biased(e, st, n, d_logits, V, temperature, d_key, d_pos, e->bias_sets_d, d_set, d_node, d_out, d_tt, d_first, d_active))
      return lrc;
    HIPCHK(hipMemcpyAsync(tokens_out, d_out, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(nodes_out, d_node, sizeof(uint32_t) * rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  if (!rc) rc = run();
  for (void* p : {(void*)d_logits, (void*)d_key, (void*)d_pos, (void*)d_set, (void*)d_node, (void*)d_out, (void*)d_tt, (void*)d_first, (void*)d_active})
    e->dfree(p);
  return rc;
}

}  // extern "C"
