// dsm_egress.inc — the engine half of the egress section of include/dsm.h (included by dsm_engine.hip behind
// dsm_tts_request.inc): the switch and its allocations, the per-slot output format, the raw calls — each its plain sibling with
// "download 1920 floats per slot" replaced by "launch egress_resample_kernel, download the raw rows" — and the host functions.
// The definition and the checked descriptor are csrc/dsm_egress.h; the kernel is egress_resample_kernel (dsm_kernels.h); the
// hooks in dsm_tts.inc are tts_enqueue_decode (the launch), dsm_tts_reset_slot (the history) and the refusals of the f32 calls.

struct dsm_egress_host_state {
  dsm_egress::Host h;
};

namespace {

// The section's buffers, once per engine, under the exclusive side of api_mu (allocations never run beside a capture).
int egress_ensure(dsm_tts* t) {
  DsmDevice* e = t;
  if (t->egress_ready) return 0;
  const size_t B = (size_t)t->B, rowb = DSM_EGRESS_MAX_FRAME_BYTES;
  if (int rc = e->dalloc(&t->egress_descs_d, dsm_tts::kEgressFormats)) return rc;
  if (int rc = e->dalloc(&t->egress_coef_d, dsm_tts::kEgressCoefWords, false)) return rc;
  if (int rc = e->dalloc(&t->egress_slot_desc_d, B)) return rc;  // zeroed: every slot on entry 0, the pass-through format
  if (int rc = e->dalloc(&t->egress_hist, B * DSM_EGRESS_MAX_TAPS)) return rc;
  if (int rc = e->dalloc(&t->egress_started, B)) return rc;
  if (int rc = e->dalloc(&t->egress_raw_d, B * rowb)) return rc;
  if (int rc = e->dalloc(&t->egress_dbg_pcm, B * DSM_FRAME_SIZE)) return rc;
  if (int rc = e->dalloc(&t->egress_dbg_valid, B)) return rc;
  for (dsm_tts::PcmEntry& en : t->pcm_q)
    if (int rc = e->halloc(&en.h_raw, B * rowb)) return rc;
  for (dsm_tts::PcmEntry& en : t->blk_pcm)
    if (int rc = e->halloc(&en.h_raw, B * rowb)) return rc;
  dsm_egress_desc d0;
  std::string err;
  if (dsm_egress::describe(DSM_EGRESS_IN_RATE, DSM_PCM_F32, &d0, &err)) { e->set_error("%s", err.c_str()); return DSM_ERR_INVALID; }
  HIPCHK(hipMemcpy(t->egress_descs_d, &d0, sizeof d0, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  t->egress_descs_h.assign(1, d0);
  t->egress_slot_desc_h.assign(B, 0u);
  t->egress_coef_used = 0;
  t->egress_pitch = d0.frame_bytes;
  t->egress_ready = true;
  return 0;
}

// the entry of (rate, fmt), made if it is new: the rate's phase table appended to the arena, the descriptor to the table.  New
// entries are referenced by no slot, so no step in flight reads them: plain blocking copies.  Caller holds api_mu exclusively.
int egress_format_entry(dsm_tts* t, int rate, int fmt, uint32_t* index) {
  DsmDevice* e = t;
  dsm_egress_desc d;
  std::string err;
  if (int rc = dsm_egress::describe(rate, fmt, &d, &err)) { e->set_error("%s", err.c_str()); return rc; }
  bool have_table = d.table_words == 0;
  for (size_t i = 0; i < t->egress_descs_h.size(); ++i) {
    const dsm_egress_desc& o = t->egress_descs_h[i];
    if (o.rate == d.rate && o.fmt == d.fmt) { *index = (uint32_t)i; return 0; }
    if (o.rate == d.rate && !have_table) { d.table_off = o.table_off; have_table = true; }
  }
  if (t->egress_descs_h.size() >= dsm_tts::kEgressFormats) {
    e->set_error("output format: %d distinct formats are in use, no room for another", (int)dsm_tts::kEgressFormats);
    return DSM_ERR_STATE;
  }
  if (!have_table) {
    std::vector<float> ph;
    if (dsm_ingest::phase_table(DSM_EGRESS_IN_RATE, rate, nullptr, nullptr, nullptr, &ph) || ph.size() != d.table_words) {
      e->set_error("output format: no phase table for %d Hz", rate);
      return DSM_ERR_INVALID;
    }
    if (t->egress_coef_used + ph.size() > dsm_tts::kEgressCoefWords) {
      e->set_error("output format: the coefficient arena is full (%zu of %zu words), no room for %d Hz", t->egress_coef_used,
                   dsm_tts::kEgressCoefWords, rate);
      return DSM_ERR_STATE;
    }
    d.table_off = (uint32_t)t->egress_coef_used;
    HIPCHK(hipMemcpy(t->egress_coef_d + d.table_off, ph.data(), sizeof(float) * ph.size(), hipMemcpyHostToDevice));
    t->egress_coef_used += ph.size();
  }
  if (int rc = dsm_egress::check(&d, t->egress_coef_used, &err)) { e->set_error("%s", err.c_str()); return rc; }
  const size_t at = t->egress_descs_h.size();
  HIPCHK(hipMemcpy(t->egress_descs_d + at, &d, sizeof d, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  t->egress_descs_h.push_back(d);
  *index = (uint32_t)at;
  return 0;
}

const dsm_egress_desc& egress_slot_desc(const dsm_tts* t, int b) { return t->egress_descs_h[t->egress_slot_desc_h[(size_t)b]]; }

// a raw call's pitch against the formats of the slots `act` marks (NULL: none; the entry's own check follows its download)
int egress_check_pitch(dsm_tts* t, size_t pitch, const uint8_t* act) {
  DsmDevice* e = t;
  if (pitch == 0 || pitch % 16 != 0 || pitch > DSM_EGRESS_MAX_FRAME_BYTES) {
    e->set_error("raw frames: a pitch of %zu bytes (a multiple of 16, at most %u)", pitch, DSM_EGRESS_MAX_FRAME_BYTES);
    return DSM_ERR_INVALID;
  }
  for (int b = 0; act && b < t->B; ++b) {
    if (!act[b]) continue;
    const dsm_egress_desc& d = egress_slot_desc(t, b);
    if (d.frame_bytes > pitch) {
      e->set_error("raw frames: slot %d's frame has %u bytes, the pitch is %zu", b, d.frame_bytes, pitch);
      return DSM_ERR_INVALID;
    }
  }
  return 0;
}

// pcm [B][1920] and valid [B] on the device -> the staging rows at egress_pitch, the histories
int egress_launch(dsm_tts* t, hipStream_t st, const float* d_pcm, const uint8_t* d_valid) {
  DsmDevice* e = t;
  EgressArgs a;
  a.pcm = d_pcm;
  a.valid = d_valid;
  a.slot_desc = t->egress_slot_desc_d;
  a.descs = t->egress_descs_d;
  a.coef = t->egress_coef_d;
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
  for (int b = 0; b < t->B; ++b) en.fb[(size_t)b] = egress_slot_desc(t, b).frame_bytes;
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
  if (dsm_egress::host_new(sample_rate_hz, sample_format, &s->h, &err)) {
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
  const int rc = dsm_egress::host_step(&s->h, frame1920, raw_out, &err);
  if (rc) g_create_error = err;
  return rc;
}

int dsm_egress_describe(int sample_rate_hz, int sample_format, uint32_t* words12) {
  if (!words12) return DSM_ERR_INVALID;
  dsm_egress_desc d;
  std::string err;
  if (int rc = dsm_egress::describe(sample_rate_hz, sample_format, &d, &err)) { g_create_error = err; return rc; }
  static_assert(sizeof d == sizeof(uint32_t) * DSM_EGRESS_DESC_WORDS, "descriptor words");
  memcpy(words12, &d, sizeof d);
  return 0;
}

int dsm_egress_encode_sample(int sample_format, float v, void* out) {
  if (!out || sample_format < DSM_PCM_F32 || sample_format > DSM_PCM_ALAW) return DSM_ERR_INVALID;
  dsm_egress_store((uint32_t)sample_format, out, 0, v);
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
  if (int rc = egress_format_entry(t, sample_rate_hz, sample_format, &index)) return rc;
  // frames in flight read the slot's words and write at the pitch: both streams drain before they change
  HIPCHK(hipStreamSynchronize(e->s_model));
  HIPCHK(hipStreamSynchronize(e->s_enc));
  const uint32_t zero = 0;
  HIPCHK(hipMemcpy(t->egress_slot_desc_d + slot, &index, sizeof index, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->egress_started + slot, &zero, sizeof zero, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(nullptr));
  t->egress_slot_desc_h[(size_t)slot] = index;
  size_t widest = 0;
  for (int b = 0; b < t->B; ++b) widest = std::max(widest, (size_t)egress_slot_desc(t, b).frame_bytes);
  t->egress_pitch = (widest + 15) & ~(size_t)15;
  return 0;
}

int dsm_tts_output_format(dsm_tts* t, int slot, int* rate, int* fmt, int* frame_samples, int* frame_bytes, int* latency_samples) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (slot < 0 || slot >= t->B) { e->set_error("batch index out of range: %d >= %d", slot, t->B); return DSM_ERR_INVALID; }
  ApiShared api(e);
  dsm_egress_desc d;
  if (t->egress_ready) d = egress_slot_desc(t, slot);
  else {
    std::string err;
    if (int rc = dsm_egress::describe(DSM_EGRESS_IN_RATE, DSM_PCM_F32, &d, &err)) return rc;
  }
  if (rate) *rate = (int)d.rate;
  if (fmt) *fmt = (int)d.fmt;
  if (frame_samples) *frame_samples = (int)d.F_out;
  if (frame_bytes) *frame_bytes = (int)d.frame_bytes;
  if (latency_samples) *latency_samples = (int)d.D;
  return 0;
}

int dsm_tts_step_raw(dsm_tts* t, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                     uint32_t* text_token_out, uint32_t* audio_out, void* raw_out, size_t pitch_bytes, uint8_t* valid_out) {
  if (!t || !prev_text_token || !allowed || !mask) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->mimi) { e->set_error("dsm_tts_step_raw needs dsm_tts_attach_mimi first"); return DSM_ERR_STATE; }
  if (int rc = egress_need_on(t, "dsm_tts_step_raw")) return rc;
  if (raw_out)
    if (int rc = egress_check_pitch(t, pitch_bytes, mask)) return rc;
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
    if (int rc = egress_check_pitch(t, pitch_bytes, nullptr)) return rc;
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
    if (int rc = egress_check_pitch(t, pitch_bytes, nullptr)) return rc;
  return tts_collect_impl(t, out, (uint8_t*)raw, pitch_bytes);
}

int dsm_tts_debug_egress(dsm_tts* t, const float* pcm, const uint8_t* valid, void* raw_out, size_t pitch_bytes) {
  if (!t || !pcm || !valid || !raw_out) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (int rc = egress_need_on(t, "dsm_tts_debug_egress")) return rc;
  if (t->pcm_pending > 0 || t->blk_pending) { e->set_error("frames wait to be received: the staging rows are theirs"); return DSM_ERR_STATE; }
  if (int rc = egress_check_pitch(t, pitch_bytes, valid)) return rc;
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
    if (valid[b]) memcpy((uint8_t*)raw_out + b * pitch_bytes, rows.data() + b * t->egress_pitch, egress_slot_desc(t, (int)b).frame_bytes);
  return 0;
}

}  // extern "C"
