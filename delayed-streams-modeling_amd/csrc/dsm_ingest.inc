// dsm_ingest.inc — the engine half of the ingest section of include/dsm.h (included by dsm_engine.hip behind
// dsm_text_bias.inc): the switch and its allocations, the per-slot format, the raw entry points — each its plain sibling with
// "upload 1920 floats per slot" replaced by "upload the raw rows, launch ingest_resample_kernel" — and the host functions.  The
// definition and the checked descriptor are csrc/dsm_ingest.h; the kernel is ingest_resample_kernel (dsm_kernels.h);
// reset_mimi_slot clears a side's history of a slot.

struct dsm_ingest_host_state {
  dsm_ingest::Host h;
};

namespace {

// The section's buffers, once per engine, under the exclusive side of api_mu (allocations never run beside a capture).
int ingest_ensure(dsm_engine* e) {
  if (e->ingest_ready) return 0;
  const size_t B = (size_t)e->B, rowb = DSM_INGEST_MAX_FRAME_BYTES;
  if (int rc = e->dalloc(&e->ingest_descs_d, dsm_engine::kIngestFormats)) return rc;
  if (int rc = e->dalloc(&e->ingest_coef_d, dsm_engine::kIngestCoefWords, false)) return rc;
  if (int rc = e->upload(&e->ingest_g711_d, dsm_ingest::g711_tables(), (size_t)512)) return rc;
  if (int rc = e->dalloc(&e->ingest_slot_desc_d, B)) return rc;  // zeroed: every slot on entry 0, the pass-through format
  for (int side = 0; side < 2; ++side) {
    if (int rc = e->dalloc(&e->ingest_hist[side], B * DSM_INGEST_MAX_TAPS)) return rc;
    if (int rc = e->dalloc(&e->ingest_started[side], B)) return rc;
    if (int rc = e->dalloc(&e->ingest_raw_d[side], B * rowb)) return rc;
    if (int rc = e->halloc(&e->ingest_raw_h[side], B * rowb)) return rc;
  }
  static_assert(dsm_engine::kPipe == 4, "ingest_pipe_raw_h");
  for (int i = 0; i < dsm_engine::kPipe; ++i)
    if (int rc = e->halloc(&e->ingest_pipe_raw_h[i], B * rowb)) return rc;
  dsm_ingest_desc d0;
  std::string err;
  if (dsm_ingest::describe(DSM_INGEST_OUT_RATE, DSM_PCM_F32, &d0, &err)) { e->set_error("%s", err.c_str()); return DSM_ERR_INVALID; }
  HIPCHK(hipMemcpy(e->ingest_descs_d, &d0, sizeof d0, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  e->ingest_descs_h.assign(1, d0);
  e->ingest_slot_desc_h.assign(B, 0u);
  e->ingest_coef_used = 0;
  e->ingest_ready = true;
  return 0;
}

// the entry of (rate, fmt), made if it is new: the rate's phase table appended to the arena, the descriptor to the table.  New
// entries are referenced by no slot, so no step in flight reads them: plain blocking copies.  Caller holds api_mu exclusively.
int ingest_format_entry(dsm_engine* e, int rate, int fmt, uint32_t* index) {
  dsm_ingest_desc d;
  std::string err;
  if (int rc = dsm_ingest::describe(rate, fmt, &d, &err)) { e->set_error("%s", err.c_str()); return rc; }
  bool have_table = d.table_words == 0;
  for (size_t i = 0; i < e->ingest_descs_h.size(); ++i) {
    const dsm_ingest_desc& o = e->ingest_descs_h[i];
    if (o.rate == d.rate && o.fmt == d.fmt) { *index = (uint32_t)i; return 0; }
    if (o.rate == d.rate && !have_table) { d.table_off = o.table_off; have_table = true; }
  }
  if (e->ingest_descs_h.size() >= dsm_engine::kIngestFormats) {
    e->set_error("input format: %d distinct formats are in use, no room for another", (int)dsm_engine::kIngestFormats);
    return DSM_ERR_STATE;
  }
  if (!have_table) {
    std::vector<float> ph;
    if (dsm_ingest::phase_table(rate, DSM_INGEST_OUT_RATE, nullptr, nullptr, nullptr, &ph) || ph.size() != d.table_words) {
      e->set_error("input format: no phase table for %d Hz", rate);
      return DSM_ERR_INVALID;
    }
    if (e->ingest_coef_used + ph.size() > dsm_engine::kIngestCoefWords) {
      e->set_error("input format: the coefficient arena is full (%zu of %zu words), no room for %d Hz", e->ingest_coef_used,
                   dsm_engine::kIngestCoefWords, rate);
      return DSM_ERR_STATE;
    }
    d.table_off = (uint32_t)e->ingest_coef_used;
    HIPCHK(hipMemcpy(e->ingest_coef_d + d.table_off, ph.data(), sizeof(float) * ph.size(), hipMemcpyHostToDevice));
    e->ingest_coef_used += ph.size();
  }
  if (int rc = dsm_ingest::check(&d, e->ingest_coef_used, &err)) { e->set_error("%s", err.c_str()); return rc; }
  const size_t at = e->ingest_descs_h.size();
  HIPCHK(hipMemcpy(e->ingest_descs_d + at, &d, sizeof d, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  e->ingest_descs_h.push_back(d);
  *index = (uint32_t)at;
  return 0;
}

// a raw call's arguments against the slots' formats.  mask NULL: every slot counts (the mask is on the device)
int ingest_check_call(dsm_engine* e, size_t pitch, const uint8_t* mask) {
  if (!e->ingest_on) {
    e->set_error("ingest is off: dsm_asr_set_ingest(engine, 1) comes before the raw calls");
    return DSM_ERR_STATE;
  }
  if (pitch == 0 || pitch % 16 != 0 || pitch > DSM_INGEST_MAX_FRAME_BYTES) {
    e->set_error("raw frames: a pitch of %zu bytes (a multiple of 16, at most %u)", pitch, DSM_INGEST_MAX_FRAME_BYTES);
    return DSM_ERR_INVALID;
  }
  std::lock_guard<std::mutex> host(e->ingest_mu);
  for (int b = 0; b < e->B; ++b) {
    if (mask && !mask[b]) continue;
    const dsm_ingest_desc& d = e->ingest_descs_h[e->ingest_slot_desc_h[(size_t)b]];
    if (d.frame_bytes > pitch) {
      e->set_error("raw frames: slot %d's frame has %u bytes, the pitch is %zu", b, d.frame_bytes, pitch);
      return DSM_ERR_INVALID;
    }
  }
  return 0;
}

// d_raw [B][pitch] and d_mask [B] on the device -> the side's frames in MimiState::pcm and its histories
int ingest_launch(dsm_engine* e, int side, hipStream_t st, const uint8_t* d_raw, size_t pitch, const uint8_t* d_mask) {
  const ConvGeom& c = e->mimi_w.init_conv;
  if (c.in_c != 1 || c.T_in != DSM_FRAME_SIZE) {
    e->set_error("ingest: the Mimi front end takes %d x %d samples a frame, not 1 x %d", c.in_c, c.T_in, DSM_FRAME_SIZE);
    return DSM_ERR_STATE;
  }
  IngestArgs a;
  a.raw = d_raw;
  a.pitch = pitch;
  a.mask = d_mask;
  a.slot_desc = e->ingest_slot_desc_d;
  a.descs = e->ingest_descs_d;
  a.coef = e->ingest_coef_d;
  a.g711 = e->ingest_g711_d;
  a.hist = e->ingest_hist[side];
  a.started = e->ingest_started[side];
  a.pcm = e->mimi[side].pcm;
  a.pcm_pitch = (long)(c.S + c.T_in) * c.in_c;  // upload_pcm's dpitch
  hipLaunchKernelGGL(ingest_resample_kernel, dim3((unsigned)e->B), dim3(256), ingest_lds(), st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// encode_host with raw rows: `stage` is the call's pinned staging [B][pitch]
int ingest_encode_host(dsm_engine* e, int side, hipStream_t st, uint8_t* stage, const void* raw, size_t pitch, const uint8_t* mask) {
  MimiState& s = e->mimi[side];
  const size_t bytes = (size_t)e->B * pitch;
  memcpy(stage, raw, bytes);
  HIPCHK(hipMemcpyAsync(e->ingest_raw_d[side], stage, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.mask, mask, (size_t)e->B, hipMemcpyHostToDevice, st));
  if (int rc = ingest_launch(e, side, st, e->ingest_raw_d[side], pitch, s.mask)) return rc;
  return mimi_encode(e, side, st);
}

}  // namespace

extern "C" {

dsm_ingest_host_state* dsm_ingest_host_new(int sample_rate_hz, int sample_format) {
  dsm_ingest_host_state* s = new (std::nothrow) dsm_ingest_host_state();
  if (!s) return nullptr;
  std::string err;
  if (dsm_ingest::host_new(sample_rate_hz, sample_format, &s->h, &err)) {
    g_create_error = err;
    delete s;
    return nullptr;
  }
  return s;
}

void dsm_ingest_host_free(dsm_ingest_host_state* s) { delete s; }

int dsm_ingest_host(dsm_ingest_host_state* s, const void* raw_frame, float* out1920) {
  if (!s) return DSM_ERR_INVALID;
  std::string err;
  const int rc = dsm_ingest::host_step(&s->h, raw_frame, s->h.d.frame_bytes, out1920, &err);
  if (rc) g_create_error = err;
  return rc;
}

int dsm_ingest_describe(int sample_rate_hz, int sample_format, uint32_t* words12) {
  if (!words12) return DSM_ERR_INVALID;
  dsm_ingest_desc d;
  std::string err;
  if (int rc = dsm_ingest::describe(sample_rate_hz, sample_format, &d, &err)) { g_create_error = err; return rc; }
  static_assert(sizeof d == sizeof(uint32_t) * DSM_INGEST_DESC_WORDS, "descriptor words");
  memcpy(words12, &d, sizeof d);
  return 0;
}

int dsm_ingest_g711_table(int sample_format, int16_t* out256) {
  if (!out256 || (sample_format != DSM_PCM_MULAW && sample_format != DSM_PCM_ALAW)) return DSM_ERR_INVALID;
  for (uint32_t b = 0; b < 256u; ++b)
    out256[b] = (int16_t)(sample_format == DSM_PCM_MULAW ? dsm_g711_ulaw_to_s16(b) : dsm_g711_alaw_to_s16(b));
  return 0;
}

int dsm_asr_set_ingest(dsm_engine* e, int on) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // between steps: waits for calls in progress
  if (!on) { e->ingest_on = false; return 0; }
  if (int rc = ingest_ensure(e)) return rc;
  e->ingest_on = true;
  return 0;
}

int dsm_asr_set_input_format(dsm_engine* e, int slot, int sample_rate_hz, int sample_format) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  if (!e->ingest_on) { e->set_error("ingest is off: dsm_asr_set_ingest(engine, 1) comes first"); return DSM_ERR_STATE; }
  std::lock_guard<std::mutex> host(e->ingest_mu);
  uint32_t index = 0;
  if (int rc = ingest_format_entry(e, sample_rate_hz, sample_format, &index)) return rc;
  // frames in flight read the slot's words: both streams drain before they change
  HIPCHK(hipStreamSynchronize(e->s_enc));
  HIPCHK(hipStreamSynchronize(e->s_model));
  const uint32_t zero = 0;
  HIPCHK(hipMemcpy(e->ingest_slot_desc_d + slot, &index, sizeof index, hipMemcpyHostToDevice));
  for (int side = 0; side < 2; ++side) HIPCHK(hipMemcpy(e->ingest_started[side] + slot, &zero, sizeof zero, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  e->ingest_slot_desc_h[(size_t)slot] = index;
  return 0;
}

int dsm_asr_input_format(dsm_engine* e, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples_24k) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  ApiShared api(e);
  std::lock_guard<std::mutex> host(e->ingest_mu);
  dsm_ingest_desc d;
  if (e->ingest_ready) d = e->ingest_descs_h[e->ingest_slot_desc_h[(size_t)slot]];
  else {
    std::string err;
    if (int rc = dsm_ingest::describe(DSM_INGEST_OUT_RATE, DSM_PCM_F32, &d, &err)) return rc;
  }
  if (rate) *rate = (int)d.rate;
  if (fmt) *fmt = (int)d.fmt;
  if (frame_samples) *frame_samples = (int)d.F_in;
  if (frame_bytes) *frame_bytes = (int)d.frame_bytes;
  if (latency_samples_24k) *latency_samples_24k = (int)d.D;
  return 0;
}

int dsm_mimi_encode_step_raw(dsm_engine* e, const void* raw, size_t pitch_bytes, const uint8_t* mask, uint32_t* codes_out, int* produced) {
  if (!e || !raw || !mask) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = ingest_check_call(e, pitch_bytes, mask)) return rc;
  HIPCHK(hipEventRecord(e->ev_a, e->s_enc));
  std::vector<uint8_t> m(mask, mask + e->B);
  if (int rc = ingest_encode_host(e, 0, e->s_enc, e->ingest_raw_h[0], raw, pitch_bytes, m.data())) return rc;
  HIPCHK(hipEventRecord(e->ev_b, e->s_enc));
  if (codes_out)
    HIPCHK(hipMemcpyAsync(codes_out, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToHost, e->s_enc));
  HIPCHK(hipStreamSynchronize(e->s_enc));
  float ms = 0;
  if (hipEventElapsedTime(&ms, e->ev_a, e->ev_b) == hipSuccess) e->metrics.last_encode_us = ms * 1000.0;
  e->metrics.steps_encode += 1;
  if (produced) *produced = 1;
  return 0;
}

int dsm_asr_step_raw(dsm_engine* e, const void* raw, size_t pitch_bytes, const uint8_t* mask, uint32_t* codes_out,
                     uint32_t* text_tokens_out, float* vad_prs_out) {
  if (!e || !raw || !mask) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  {  // a refused call changes nothing: the check comes before the model side's Mimi is made
    ApiShared api(e);
    if (int rc = ingest_check_call(e, pitch_bytes, mask)) return rc;
  }
  if (int rc = ensure_model_side_mimi(e)) return rc;
  ApiShared api(e);
  if (int rc = ingest_check_call(e, pitch_bytes, mask)) return rc;
  if (int rc = wait_group_inputs(e)) return rc;
  std::vector<uint8_t> m(mask, mask + e->B);
  if (int rc = ingest_encode_host(e, 1, e->s_model, e->ingest_raw_h[1], raw, pitch_bytes, m.data())) return rc;
  if (codes_out)
    HIPCHK(hipMemcpyAsync(codes_out, e->mimi[1].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToHost, e->s_model));
  return step_tokens_host(e, e->mimi[1].codes, m.data(), text_tokens_out, vad_prs_out);
}

int dsm_mimi_encode_step_raw_async(dsm_engine* e, const void* raw, size_t pitch_bytes, const uint8_t* mask, int* ticket) {
  if (!e || !raw || !mask || !ticket) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);  // as dsm_mimi_encode_step_async: no capture of the model thread is in progress from here to the return
  if (int rc = ingest_check_call(e, pitch_bytes, mask)) return rc;
  int slot;
  {
    std::lock_guard<std::mutex> lk(e->pipe_mu);
    if (int rc = pipe_init(e)) return rc;
    slot = e->pipe_next;
    if (e->pipe[slot].in_flight) {
      e->set_error("encode pipeline full: %d frames wait for dsm_asr_step_tokens_ticket", dsm_engine::kPipe);
      return DSM_ERR_STATE;
    }
    e->pipe[slot].in_flight = true;
    e->pipe_next = (slot + 1) % dsm_engine::kPipe;
  }
  dsm_engine::PipeSlot& ps = e->pipe[slot];
  struct Rollback {  // any failure below hands the ring entry back, as in dsm_mimi_encode_step_async
    dsm_engine* e; int slot; bool armed = true;
    ~Rollback() {
      if (!armed) return;
      std::lock_guard<std::mutex> lk(e->pipe_mu);
      e->pipe[slot].in_flight = false;
      e->pipe_next = slot;
    }
  } rollback{e, slot};
  HIPCHK(hipEventSynchronize(ps.ev_consumed));  // also orders the reuse of the entry's pinned staging
  memcpy(ps.h_mask, mask, (size_t)e->B);
  hipStream_t st = e->s_enc;
  if (int rc = ingest_encode_host(e, 0, st, e->ingest_pipe_raw_h[slot], raw, pitch_bytes, ps.h_mask)) return rc;
  HIPCHK(hipMemcpyAsync(ps.d_codes, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                        hipMemcpyDeviceToDevice, st));
  HIPCHK(hipEventRecord(ps.ev_done, st));
  rollback.armed = false;
  e->metrics.steps_encode += 1;
  *ticket = slot;
  return 0;
}

int dsm_mimi_encode_step_raw_dev(dsm_engine* e, const void* d_raw, size_t pitch_bytes, const uint8_t* d_mask, uint32_t* d_codes_out) {
  if (!e || !d_raw || !d_mask) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = ingest_check_call(e, pitch_bytes, nullptr)) return rc;
  if (((uintptr_t)d_raw & 15u) != 0) { e->set_error("raw frames: the device pointer is not 16-byte aligned"); return DSM_ERR_INVALID; }
  if (e->codes_consumed_valid) HIPCHK(hipStreamWaitEvent(e->s_enc, e->ev_codes_consumed, 0));
  HIPCHK(hipMemcpyAsync(e->mimi[0].mask, d_mask, (size_t)e->B, hipMemcpyDeviceToDevice, e->s_enc));
  if (int rc = ingest_launch(e, 0, e->s_enc, (const uint8_t*)d_raw, pitch_bytes, e->mimi[0].mask)) return rc;
  if (int rc = mimi_encode(e, 0, e->s_enc)) return rc;
  if (d_codes_out)
    HIPCHK(hipMemcpyAsync(d_codes_out, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToDevice, e->s_enc));
  HIPCHK(hipEventRecord(e->ev_join, e->s_enc));
  e->metrics.steps_encode += 1;
  return 0;
}

int dsm_debug_ingest_read(dsm_engine* e, int side, float* out) {
  if (!e || !out || side < 0 || side > 1) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (side == 1 && !e->mimi1_ready.load(std::memory_order_acquire)) { e->set_error("the model side's Mimi has not run yet"); return DSM_ERR_STATE; }
  hipStream_t st = side == 0 ? e->s_enc : e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  const ConvGeom& c = e->mimi_w.init_conv;
  const size_t spitch = sizeof(float) * (size_t)(c.S + c.T_in) * c.in_c, width = sizeof(float) * (size_t)c.T_in * c.in_c;
  HIPCHK(hipMemcpy2D(out, width, e->mimi[side].pcm, spitch, width, (size_t)e->B, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
