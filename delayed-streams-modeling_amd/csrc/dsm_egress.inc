// dsm_egress.inc — the engine half of the egress section of include/dsm.h (included by dsm_engine.hip behind
// dsm_tts_request.inc): the switch and its allocations, the per-slot output format, the raw calls — each its plain sibling with
// "download 1920 floats per slot" replaced by "launch egress_resample_kernel, download the raw rows" — and the host functions.
// The definition and the checked descriptor are csrc/dsm_pcm_format.h (DSM_PCM_OUT); the slots' formats are a PcmFormatTable
// (dsm_pcm_table.inc), which also holds the raw calls' pitch rule — where a call marks no slot only the pitch itself is checked:
// the entry's own check follows its download; the kernel is egress_resample_kernel (dsm_kernels.h); the hooks in dsm_tts.inc
// are tts_enqueue_decode (the launch), dsm_tts_reset_slot (the history) and the refusals of the f32 calls.

struct dsm_egress_host_state {
  dsm_pcm::Host h;
};

namespace {

// The section's buffers, once per engine, under the exclusive side of api_mu (allocations never run beside a capture).  The
// format table comes last: its `ready` says that all of this is there.
int egress_ensure(dsm_tts* t) {
  DsmDevice* e = t;
  if (t->egress_fmt.ready) return 0;
  const size_t B = (size_t)t->B, rowb = DSM_PCM_MAX_FRAME_BYTES;
  if (int rc = e->dalloc(&t->egress_hist, B * DSM_PCM_MAX_TAPS_OUT)) return rc;
  if (int rc = e->dalloc(&t->egress_started, B)) return rc;
  if (int rc = e->dalloc(&t->egress_raw_d, B * rowb)) return rc;
  if (int rc = e->dalloc(&t->egress_dbg_pcm, B * DSM_FRAME_SIZE)) return rc;
  if (int rc = e->dalloc(&t->egress_dbg_valid, B)) return rc;
  for (dsm_tts::PcmEntry& en : t->pcm_q)
    if (int rc = e->halloc(&en.h_raw, B * rowb)) return rc;
  for (dsm_tts::PcmEntry& en : t->blk_pcm)
    if (int rc = e->halloc(&en.h_raw, B * rowb)) return rc;
  if (int rc = t->egress_fmt.ensure(e, B)) return rc;
  t->egress_pitch = t->egress_fmt.slot(0).frame_bytes;
  return 0;
}

// pcm [B][1920] and valid [B] on the device -> the staging rows at egress_pitch, the histories
int egress_launch(dsm_tts* t, hipStream_t st, const float* d_pcm, const uint8_t* d_valid) {
  DsmDevice* e = t;
  EgressArgs a;
  a.pcm = d_pcm;
  a.valid = d_valid;
  a.slot_desc = t->egress_fmt.slot_desc_d;
  a.descs = t->egress_fmt.descs_d;
  a.coef = t->egress_fmt.coef_d;
  a.hist = t->egress_hist;
  a.started = t->egress_started;
  a.raw = t->egress_raw_d;
  a.pitch = t->egress_pitch;
  hipLaunchKernelGGL(egress_resample_kernel, dim3((unsigned)t->B), dim3(256), egress_lds(), st, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// tts_enqueue_decode with the section on: behind mimi_decode on the decode stream, the kernel and the download of the rows
int egress_enqueue(dsm_tts* t, hipStream_t sd, dsm_tts::PcmEntry& en) {
  DsmDevice* e = t;
  if (int rc = egress_launch(t, sd, t->dec.pcm, t->dec.mask)) return rc;
  en.raw_pitch = t->egress_pitch;
  en.fb.resize((size_t)t->B);
  for (int b = 0; b < t->B; ++b) en.fb[(size_t)b] = t->egress_fmt.slot(b).frame_bytes;
  HIPCHK(hipMemcpyAsync(en.h_raw, t->egress_raw_d, (size_t)t->B * en.raw_pitch, hipMemcpyDeviceToHost, sd));
  return 0;
}

// the oldest pending entry: wait for it, hand it out.  A pitch below an emitted frame: DSM_ERR_INVALID, the entry stays queued.
int egress_deliver(dsm_tts* t, uint8_t* raw_out, size_t pitch, uint8_t* valid_out) {
  DsmDevice* e = t;
  dsm_tts::PcmEntry& en = t->pcm_q[(t->pcm_seq - (uint64_t)t->pcm_pending) & 1];
  if (en.launched) HIPCHK(hipEventSynchronize(en.ev));
  for (int b = 0; raw_out && en.launched && b < t->B; ++b)
    if (en.h_valid[b] && en.fb[(size_t)b] > pitch) {
      e->set_error("raw frames: slot %d's frame has %u bytes, the pitch is %zu", b, en.fb[(size_t)b], pitch);
      return DSM_ERR_INVALID;
    }
  for (int b = 0; b < t->B; ++b) {
    const bool v = en.launched && en.h_valid[b];
    if (valid_out) valid_out[b] = v ? 1 : 0;
    if (raw_out && v) memcpy(raw_out + (size_t)b * pitch, en.h_raw + (size_t)b * en.raw_pitch, en.fb[(size_t)b]);
  }
  t->pcm_pending -= 1;
  return 0;
}

int egress_need_on(dsm_tts* t, const char* call) {
  if (t->egress_on) return 0;
  t->set_error("egress is off: dsm_tts_set_egress(engine, 1) comes before %s", call);
  return DSM_ERR_STATE;
}

}  // namespace

extern "C" {

dsm_egress_host_state* dsm_egress_host_new(int sample_rate_hz, int sample_format) {
  dsm_egress_host_state* s = new (std::nothrow) dsm_egress_host_state();
  if (!s) return nullptr;
  std::string err;
  if (dsm_pcm::host_new(DSM_PCM_OUT, sample_rate_hz, sample_format, &s->h, &err)) {
    g_create_error = err;
    delete s;
    return nullptr;
  }
  return s;
}

void dsm_egress_host_free(dsm_egress_host_state* s) { delete s; }

int dsm_egress_host(dsm_egress_host_state* s, const float* frame1920, void* raw_out) {
  if (!s) return DSM_ERR_INVALID;
  std::string err;
  const int rc = dsm_pcm::host_step_out(&s->h, frame1920, raw_out, &err);
  if (rc) g_create_error = err;
  return rc;
}

int dsm_egress_describe(int sample_rate_hz, int sample_format, uint32_t* words12) {
  if (!words12) return DSM_ERR_INVALID;
  dsm_pcm_desc d;
  std::string err;
  if (int rc = dsm_pcm::describe(DSM_PCM_OUT, sample_rate_hz, sample_format, &d, &err)) { g_create_error = err; return rc; }
  static_assert(sizeof d == sizeof(uint32_t) * DSM_PCM_DESC_WORDS, "descriptor words");
  memcpy(words12, &d, sizeof d);
  return 0;
}

int dsm_egress_encode_sample(int sample_format, float v, void* out) {
  if (!out || sample_format < DSM_PCM_F32 || sample_format > DSM_PCM_ALAW) return DSM_ERR_INVALID;
  dsm_pcm_store((uint32_t)sample_format, out, 0, v);
  return 0;
}

int dsm_tts_set_egress(dsm_tts* t, int on) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->mimi) { e->set_error("dsm_tts_set_egress needs dsm_tts_attach_mimi first"); return DSM_ERR_STATE; }
  if (t->pcm_pending > 0) { e->set_error("%d deferred step(s) wait to be received", t->pcm_pending); return DSM_ERR_STATE; }
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // between steps: allocations must not run beside a capture
  if (!on) { t->egress_on = false; return 0; }
  if (int rc = egress_ensure(t)) return rc;
  t->egress_on = true;
  return 0;
}

int dsm_tts_set_output_format(dsm_tts* t, int slot, int sample_rate_hz, int sample_format) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (slot < 0 || slot >= t->B) { e->set_error("batch index out of range: %d >= %d", slot, t->B); return DSM_ERR_INVALID; }
  if (int rc = egress_need_on(t, "dsm_tts_set_output_format")) return rc;
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  uint32_t index = 0;
  if (int rc = t->egress_fmt.entry(e, sample_rate_hz, sample_format, &index)) return rc;
  // frames in flight read the slot's words and write at the pitch: both streams drain before they change
  HIPCHK(hipStreamSynchronize(e->s_model));
  HIPCHK(hipStreamSynchronize(e->s_enc));
  if (int rc = t->egress_fmt.set_slot(e, slot, index)) return rc;
  const uint32_t zero = 0;
  HIPCHK(hipMemcpy(t->egress_started + slot, &zero, sizeof zero, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  size_t widest = 0;
  for (int b = 0; b < t->B; ++b) widest = std::max(widest, (size_t)t->egress_fmt.slot(b).frame_bytes);
  t->egress_pitch = (widest + 15) & ~(size_t)15;
  return 0;
}

int dsm_tts_output_format(dsm_tts* t, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (slot < 0 || slot >= t->B) { e->set_error("batch index out of range: %d >= %d", slot, t->B); return DSM_ERR_INVALID; }
  ApiShared api(e);
  return t->egress_fmt.get(slot, rate, fmt, frame_samples, frame_bytes, latency_samples);
}

int dsm_tts_step_raw(dsm_tts* t, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                     uint32_t* text_token_out, uint32_t* audio_out, void* raw_out, size_t pitch_bytes, uint8_t* valid_out) {
  if (!t || !prev_text_token || !allowed || !mask) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->mimi) { e->set_error("dsm_tts_step_raw needs dsm_tts_attach_mimi first"); return DSM_ERR_STATE; }
  if (int rc = egress_need_on(t, "dsm_tts_step_raw")) return rc;
  if (raw_out)
    if (int rc = t->egress_fmt.check_pitch(e, pitch_bytes, mask, false)) return rc;
  if (raw_out && t->pcm_pending > 0) {
    e->set_error("%d deferred step(s) wait for dsm_tts_recv_raw: a serial step would deliver out of order", t->pcm_pending);
    return DSM_ERR_STATE;
  }
  if (t->pcm_pending >= 2) { e->set_error("two deferred steps wait for dsm_tts_recv_raw"); return DSM_ERR_STATE; }
  const uint64_t seq = t->pcm_seq;
  const int rc = tts_step_impl(t, prev_text_token, allowed, mask, text_token_out, audio_out, true);
  if (raw_out && t->pcm_seq != seq) {  // serial: the entry this call queued is delivered at once
    ApiShared api(e);
    if (int rd = egress_deliver(t, (uint8_t*)raw_out, pitch_bytes, valid_out)) return rd;
  }
  return rc;
}

int dsm_tts_recv_raw(dsm_tts* t, void* raw_out, size_t pitch_bytes, uint8_t* valid_out) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (int rc = egress_need_on(t, "dsm_tts_recv_raw")) return rc;
  if (raw_out)
    if (int rc = t->egress_fmt.check_pitch(e, pitch_bytes, nullptr, false)) return rc;
  if (t->pcm_pending == 0) return 0;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = egress_deliver(t, (uint8_t*)raw_out, pitch_bytes, valid_out)) return rc;
  return 1;
}

int dsm_tts_collect_raw(dsm_tts* t, dsm_tts_block* out, void* raw, size_t pitch_bytes) {
  if (!t || !out) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (int rc = egress_need_on(t, "dsm_tts_collect_raw")) return rc;
  if (out->pcm) { e->set_error("dsm_tts_collect_raw: out->pcm must be NULL, the frames go to the raw rows"); return DSM_ERR_INVALID; }
  if (!t->blk_pending) { e->set_error("no block waits: dsm_tts_run first"); return DSM_ERR_STATE; }
  if (raw)
    if (int rc = t->egress_fmt.check_pitch(e, pitch_bytes, nullptr, false)) return rc;
  return tts_collect_impl(t, out, (uint8_t*)raw, pitch_bytes);
}

int dsm_tts_debug_egress(dsm_tts* t, const float* pcm, const uint8_t* valid, void* raw_out, size_t pitch_bytes) {
  if (!t || !pcm || !valid || !raw_out) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (int rc = egress_need_on(t, "dsm_tts_debug_egress")) return rc;
  if (t->pcm_pending > 0 || t->blk_pending) { e->set_error("frames wait to be received: the staging rows are theirs"); return DSM_ERR_STATE; }
  if (int rc = t->egress_fmt.check_pitch(e, pitch_bytes, valid, false)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  const size_t B = (size_t)t->B;
  hipStream_t sd = e->s_enc;
  std::vector<uint8_t> rows(B * t->egress_pitch);
  HIPCHK(hipMemcpyAsync(t->egress_dbg_pcm, pcm, sizeof(float) * B * DSM_FRAME_SIZE, hipMemcpyHostToDevice, sd));
  HIPCHK(hipMemcpyAsync(t->egress_dbg_valid, valid, B, hipMemcpyHostToDevice, sd));
  if (int rc = egress_launch(t, sd, t->egress_dbg_pcm, t->egress_dbg_valid)) return rc;
  HIPCHK(hipMemcpyAsync(rows.data(), t->egress_raw_d, rows.size(), hipMemcpyDeviceToHost, sd));
  HIPCHK(hipStreamSynchronize(sd));
  for (size_t b = 0; b < B; ++b)
    if (valid[b]) memcpy((uint8_t*)raw_out + b * pitch_bytes, rows.data() + b * t->egress_pitch, t->egress_fmt.slot((int)b).frame_bytes);
  return 0;
}

}  // extern "C"
