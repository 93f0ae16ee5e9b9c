// dsm_ingest.inc — the engine half of the ingest section of include/dsm.h (included by dsm_engine.hip behind
// dsm_text_bias.inc): the switch and its allocations, the per-slot format, the raw entry points — each its plain sibling with
// "upload 1920 floats per slot" replaced by "upload the raw rows, launch ingest_resample_kernel" — and the host functions.  The
// definition and the checked descriptor are csrc/dsm_pcm_format.h (DSM_PCM_IN); the slots' formats are a PcmFormatTable
// (dsm_pcm_table.inc); the kernel is ingest_resample_kernel (dsm_kernels.h); reset_mimi_slot clears a side's history of a slot.

struct dsm_ingest_host_state {
  dsm_pcm::Host h;
};

namespace {

// The section's buffers, once per engine, under the exclusive side of api_mu (allocations never run beside a capture).  The
// format table comes last: its `ready` says that all of this is there.
int ingest_ensure(dsm_engine* e) {
  if (e->ingest_fmt.ready) return 0;
  const size_t B = (size_t)e->B, rowb = DSM_PCM_MAX_FRAME_BYTES;
  if (int rc = e->upload(&e->ingest_g711_d, dsm_pcm::g711_tables(), (size_t)512)) return rc;
  for (int side = 0; side < 2; ++side) {
    if (int rc = e->dalloc(&e->ingest_hist[side], B * DSM_PCM_MAX_TAPS_IN)) return rc;
    if (int rc = e->dalloc(&e->ingest_started[side], B)) return rc;
    if (int rc = e->dalloc(&e->ingest_raw_d[side], B * rowb)) return rc;
    if (int rc = e->halloc(&e->ingest_raw_h[side], B * rowb)) return rc;
  }
  static_assert(dsm_engine::kPipe == 4, "ingest_pipe_raw_h");
  for (int i = 0; i < dsm_engine::kPipe; ++i)
    if (int rc = e->halloc(&e->ingest_pipe_raw_h[i], B * rowb)) return rc;
  return e->ingest_fmt.ensure(e, B);
}

// a raw call's arguments against the slots' formats.  mask NULL: every slot counts (the mask is on the device)
int ingest_check_call(dsm_engine* e, size_t pitch, const uint8_t* mask) {
  if (!e->ingest_on) {
    e->set_error("ingest is off: dsm_asr_set_ingest(engine, 1) comes before the raw calls");
    return DSM_ERR_STATE;
  }
  std::lock_guard<std::mutex> host(e->ingest_mu);
  return e->ingest_fmt.check_pitch(e, pitch, mask, mask == nullptr);
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
  a.slot_desc = e->ingest_fmt.slot_desc_d;
  a.descs = e->ingest_fmt.descs_d;
  a.coef = e->ingest_fmt.coef_d;
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
  if (dsm_pcm::host_new(DSM_PCM_IN, sample_rate_hz, sample_format, &s->h, &err)) {
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
  const int rc = dsm_pcm::host_step_in(&s->h, raw_frame, s->h.d.frame_bytes, out1920, &err);
  if (rc) g_create_error = err;
  return rc;
}

int dsm_ingest_describe(int sample_rate_hz, int sample_format, uint32_t* words12) {
  if (!words12) return DSM_ERR_INVALID;
  dsm_pcm_desc d;
  std::string err;
  if (int rc = dsm_pcm::describe(DSM_PCM_IN, sample_rate_hz, sample_format, &d, &err)) { g_create_error = err; return rc; }
  static_assert(sizeof d == sizeof(uint32_t) * DSM_PCM_DESC_WORDS, "descriptor words");
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
  if (int rc = e->clip_guard_slots(&slot, 1, "set_input_format")) return rc;
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  if (!e->ingest_on) { e->set_error("ingest is off: dsm_asr_set_ingest(engine, 1) comes first"); return DSM_ERR_STATE; }
  std::lock_guard<std::mutex> host(e->ingest_mu);
  uint32_t index = 0;
  if (int rc = e->ingest_fmt.entry(e, sample_rate_hz, sample_format, &index)) return rc;
  // frames in flight read the slot's words: both streams drain before they change
  HIPCHK(hipStreamSynchronize(e->s_enc));
  HIPCHK(hipStreamSynchronize(e->s_model));
  if (int rc = e->ingest_fmt.set_slot(e, slot, index)) return rc;
  const uint32_t zero = 0;
  for (int side = 0; side < 2; ++side) HIPCHK(hipMemcpy(e->ingest_started[side] + slot, &zero, sizeof zero, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  return 0;
}

int dsm_asr_input_format(dsm_engine* e, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples_24k) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  ApiShared api(e);
  std::lock_guard<std::mutex> host(e->ingest_mu);
  return e->ingest_fmt.get(slot, rate, fmt, frame_samples, frame_bytes, latency_samples_24k);
}

int dsm_mimi_encode_step_raw(dsm_engine* e, const void* raw, size_t pitch_bytes, const uint8_t* mask, uint32_t* codes_out, int* produced) {
  if (!e || !raw || !mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
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
  if (int rc = e->clip_guard(mask)) return rc;
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
  if (int rc = e->clip_guard(mask)) return rc;
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
  if (int rc = e->clip_guard(nullptr)) return rc;
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
