// dsm_tts_voice.inc — voices: a cross-attention source projected once into device memory of its own, which any number of slots
// attach to by reference (included by dsm_engine.hip behind dsm_tts.inc).
//
// dsm_tts_set_ca_src projects a request's rows through in_proj_kv of every main-LM layer into the batch row's private block, for
// every request again.  A voice is that projection kept: dsm_tts_voice_create runs tts_project_ca_row — the same GEMM, the same
// scatter kernel — with the voice's memory as the destination, and dsm_tts_set_voice only rewrites the batch row's entries of
// the per-layer pointer tables the cross-attention launches read (CaState::src), its `last` and the slot's guidance.  Rows that
// share a voice read the same addresses.

extern "C" {

int dsm_tts_voice_create(dsm_tts* t, const float* ca_src, int n, int* voice_out) {
  if (!t || !voice_out) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  *voice_out = 0;
  if (!c.cross_attention) { e->set_error("this engine was created without cross_attention"); return DSM_ERR_STATE; }
  if (!ca_src || n < 1 || n > c.ca_max_len) {
    e->set_error("a voice needs 1..ca_max_len = %d rows of ca_src (got %d%s)", c.ca_max_len, n, ca_src ? "" : ", NULL rows");
    return DSM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  dsm_tts::Voice v;
  v.rows = n;
  v.bytes = (size_t)2 * c.lm.num_layers * c.lm.d_model * t->ca.smax * (c.kv_bf16 ? 2 : 4);
  if (int rc = e->dalloc(&v.mem, v.bytes)) {  // zeroed like the private blocks; nothing else has changed yet
    (void)hipGetLastError();
    return rc;
  }
  int rc = with_kv_type(c.kv_bf16 != 0, [&](auto kv) { return tts_project_ca_row<decltype(kv)>(t, st, 0, &v, ca_src, n); });
  if (!rc && hipStreamSynchronize(st) != hipSuccess) {  // the staging buffers are free again; `ca_src` is the caller's memory
    e->set_error("dsm_tts_voice_create: the projection failed on the device");
    rc = DSM_ERR_DEVICE;
  }
  if (rc) {
    e->dfree(v.mem);
    return rc;
  }
  v.handle = t->next_voice++;
  t->voices.push_back(v);
  *voice_out = v.handle;
  return 0;
}

int dsm_tts_voice_destroy(dsm_tts* t, int voice) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  dsm_tts::Voice* v = tts_find_voice(t, voice);
  if (!v || voice <= 0) { e->set_error("no voice %d", voice); return DSM_ERR_INVALID; }
  if (v->refs > 0) { e->set_error("voice %d is in use by %d rows", voice, v->refs); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  HIPCHK(hipStreamSynchronize(e->s_model));  // steps that read it while it was attached are done
  e->dfree(v->mem);
  t->voices.erase(t->voices.begin() + (v - t->voices.data()));
  return 0;
}

int dsm_tts_voice_info(dsm_tts* t, int voice, int* rows, int* refs, size_t* device_bytes) {
  if (!t) return DSM_ERR_INVALID;
  const dsm_tts::Voice* v = tts_find_voice(t, voice);
  if (!v || voice <= 0) { t->set_error("no voice %d", voice); return DSM_ERR_INVALID; }
  if (rows) *rows = v->rows;
  if (refs) *refs = v->refs;
  if (device_bytes) *device_bytes = v->bytes;
  return 0;
}

int dsm_tts_set_voice(dsm_tts* t, int slot, int voice, int voice_uncond, double cfg_alpha) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  if (!c.cross_attention) { e->set_error("this engine was created without cross_attention"); return DSM_ERR_STATE; }
  dsm_tts::Voice* vs[2] = {tts_find_voice(t, voice), tts_find_voice(t, voice_uncond)};
  if ((voice != 0 && (voice < 0 || !vs[0])) || (voice_uncond != 0 && (voice_uncond < 0 || !vs[1]))) {
    e->set_error("no voice %d", (voice != 0 && (voice < 0 || !vs[0])) ? voice : voice_uncond);
    return DSM_ERR_INVALID;
  }
  if (voice_uncond != 0 && (t->rps != 2 || voice == 0)) {
    e->set_error("guidance needs an engine created with cfg_rows = 1 and a conditional source");
    return DSM_ERR_INVALID;
  }
  // as for dsm_tts_set_ca_src: only a fresh slot takes a source, clearing (voice = 0) is always allowed
  if ((voice != 0 || voice_uncond != 0) && t->items[slot].step_idx != 0) {
    e->set_error("slot %d is at step %zu: dsm_tts_set_voice needs a fresh slot (dsm_tts_reset_slot first)", slot, t->items[slot].step_idx);
    return DSM_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  uint32_t last[2] = {0u, 0u};  // every upload below is only enqueued; tts_upload_guidance ends with the one wait for all of them
  for (int j = 0; j < t->rps; ++j) {
    const int row = slot * t->rps + j, len = vs[j] ? vs[j]->rows : 0;
    if (int rc = tts_point_row(t, st, row, vs[j])) return rc;
    if (len == 0 && t->ca_len[row] > 0)  // as in dsm_tts_set_ca_src: the out_proj of a source-less row has to see zeros
      HIPCHK(hipMemsetAsync(t->ca.att + (size_t)row * c.lm.d_model, 0, sizeof(float) * (size_t)c.lm.d_model, st));
    last[j] = len > 0 ? (uint32_t)(len - 1) : 0u;
    t->ca_len[row] = len;
  }
  HIPCHK(hipMemcpyAsync(t->ca.last + (size_t)slot * t->rps, last, sizeof(uint32_t) * (size_t)t->rps, hipMemcpyHostToDevice, st));
  return tts_upload_guidance(t, st, slot, voice_uncond != 0, cfg_alpha);
}

}  // extern "C"
