// dsm_asr_clip.inc — the engine half of the clips section of include/dsm.h (included by dsm_engine.hip behind dsm_ingest.inc):
// the switch and its allocations, a slot's clip (begin / push / close), the block call dsm_asr_run — the bodies of
// dsm_mimi_encode_step_raw_dev and dsm_asr_step_tokens_dev(codes = NULL) enqueued n times over engine-owned buffers, with
// asr_clip_frame_kernel in front of each encode and asr_clip_record_kernel behind each group's step — and dsm_asr_collect.  The
// definition (the cut, the schedule, the records' layout) is csrc/dsm_asr_clip.h; the kernels are in dsm_kernels.h.
//
// Three things the enqueue order below exists for:
//   * the mask of step k travels with its codes.  The encoder stream runs a step ahead of the model stream, so MimiState::mask
//     already holds step k + 1's mask when the LM's head of step k copies "the mask": the model stream takes mask and codes in
//     ONE hand-off — behind ev_join, in front of the record of ev_codes_consumed, which is what lets the next cut overwrite both.
//   * the clip kernels stay outside the captured graphs, k is a launch argument, and every pointer the graphs see (the raw
//     staging, MimiState::mask, lm.codes_in, lm.mask, lm.text_out, lm.prs) is the engine's: the capture keys of the encode and of
//     lm_group_rest are those of the per-step calls with NULL outputs, so a block adds no graph and nothing settles again.
//   * groups are not joined at the end of a step, so the record launch of a group goes on THAT GROUP'S stream, behind its step
//     (lm_step_then); the model stream joins them once, at the end of the block, in front of the records' download.

struct dsm_asr_clip_host_state {
  std::vector<dsm_asr_clip::Slot> slots;
  uint64_t cap = 0;
};

namespace {

constexpr uint64_t kClipMaxBytes = (uint64_t)1 << 31;

// a block's table, device and pinned alike: AsrClipSlot [B], frame [DSM_ASR_RUN_MAX][B], mask [DSM_ASR_RUN_MAX][B]
size_t clip_tab_frame_off(size_t B) { return sizeof(AsrClipSlot) * B; }
size_t clip_tab_mask_off(size_t B) { return clip_tab_frame_off(B) + sizeof(uint32_t) * DSM_ASR_RUN_MAX * B; }
size_t clip_tab_bytes(size_t B) { return clip_tab_mask_off(B) + (size_t)DSM_ASR_RUN_MAX * B; }

// (rate, fmt) -> the format's frame_bytes, or DSM_ERR_INVALID with the message in *err
int clip_frame_bytes(int rate, int fmt, uint32_t* frame_bytes, std::string* err) {
  dsm_pcm_desc d;
  if (int rc = dsm_pcm::describe(DSM_PCM_IN, rate, fmt, &d, err)) return rc;
  *frame_bytes = d.frame_bytes;
  return 0;
}

int clips_are_on(dsm_engine* e) {
  if (e->clips_on.load(std::memory_order_acquire)) return 0;
  e->set_error("clips are off: dsm_asr_set_clips(engine, 1, max_clip_bytes_per_slot) comes first");
  return DSM_ERR_STATE;
}

bool clip_ticket_outstanding(dsm_engine* e) {
  std::lock_guard<std::mutex> lk(e->pipe_mu);
  for (const dsm_engine::PipeSlot& ps : e->pipe)
    if (ps.in_flight) return true;
  return false;
}

// the section's buffers, once per engine, under the exclusive side of api_mu
int clips_ensure(dsm_engine* e, size_t cap16) {
  const size_t B = (size_t)e->B, rec = sizeof(uint32_t) * DSM_ASR_RUN_MAX * dsm_asr_clip::record_words(e->B, e->cfg.extra_heads_num);
  if (int rc = e->halloc(&e->clip_h, B * cap16)) return rc;
  if (int rc = e->dalloc(&e->clip_tab_d, clip_tab_bytes(B))) return rc;
  if (int rc = e->halloc(&e->clip_tab_h, clip_tab_bytes(B))) return rc;
  if (int rc = e->dalloc(&e->clip_rec_d, rec / sizeof(uint32_t))) return rc;
  if (int rc = e->halloc(&e->clip_rec_h, rec / sizeof(uint32_t))) return rc;
  memset(e->clip_tab_h, 0, clip_tab_bytes(B));
  e->clip_slots.assign(B, dsm_asr_clip::Slot());
  return e->dalloc(&e->clip_d, B * cap16);  // last: its presence says that all of this is there
}

}  // namespace

extern "C" {

int dsm_asr_clip_frame_host(const void* clip, size_t clip_bytes, int sample_rate_hz, int sample_format, uint64_t frame_index,
                            void* frame_out) {
  uint32_t fb = 0;
  std::string err;
  if (!frame_out || (!clip && clip_bytes)) { g_create_error = "clip frame: a NULL pointer"; return DSM_ERR_INVALID; }
  if (int rc = clip_frame_bytes(sample_rate_hz, sample_format, &fb, &err)) { g_create_error = err; return rc; }
  dsm_asr_clip::cut(clip, clip_bytes, fb, dsm_asr_clip::silence_byte((uint32_t)sample_format), frame_index, frame_out);
  return (int)fb;
}

dsm_asr_clip_host_state* dsm_asr_clip_host_new(int batch_size, size_t max_clip_bytes_per_slot) {
  if (batch_size < 1 || max_clip_bytes_per_slot < 1 || max_clip_bytes_per_slot > kClipMaxBytes) return nullptr;
  dsm_asr_clip_host_state* s = new (std::nothrow) dsm_asr_clip_host_state();
  if (!s) return nullptr;
  s->slots.assign((size_t)batch_size, dsm_asr_clip::Slot());
  s->cap = max_clip_bytes_per_slot;
  return s;
}

void dsm_asr_clip_host_free(dsm_asr_clip_host_state* s) { delete s; }

int dsm_asr_clip_host_begin(dsm_asr_clip_host_state* s, int slot, int sample_rate_hz, int sample_format, int flush_frames) {
  if (!s || slot < 0 || slot >= (int)s->slots.size() || flush_frames < 0) return DSM_ERR_INVALID;
  uint32_t fb = 0;
  std::string err;
  if (int rc = clip_frame_bytes(sample_rate_hz, sample_format, &fb, &err)) { g_create_error = err; return rc; }
  if (s->slots[(size_t)slot].status != DSM_ASR_CLIP_IDLE) return DSM_ERR_STATE;
  dsm_asr_clip::begin(&s->slots[(size_t)slot], fb, (uint64_t)flush_frames);
  return 0;
}

int dsm_asr_clip_host_push(dsm_asr_clip_host_state* s, int slot, size_t n) {
  if (!s || slot < 0 || slot >= (int)s->slots.size()) return DSM_ERR_INVALID;
  return dsm_asr_clip::push(&s->slots[(size_t)slot], n, s->cap) ? 0 : DSM_ERR_STATE;
}

int dsm_asr_clip_host_close(dsm_asr_clip_host_state* s, int slot) {
  if (!s || slot < 0 || slot >= (int)s->slots.size()) return DSM_ERR_INVALID;
  return dsm_asr_clip::close(&s->slots[(size_t)slot]) ? 0 : DSM_ERR_STATE;
}

int dsm_asr_clip_host_reset(dsm_asr_clip_host_state* s, int slot) {
  if (!s || slot < 0 || slot >= (int)s->slots.size()) return DSM_ERR_INVALID;
  s->slots[(size_t)slot] = dsm_asr_clip::Slot();
  return 0;
}

int dsm_asr_clip_host_status(dsm_asr_clip_host_state* s, int slot) {
  if (!s || slot < 0 || slot >= (int)s->slots.size()) return DSM_ERR_INVALID;
  return s->slots[(size_t)slot].status;
}

int dsm_asr_clip_host_run(dsm_asr_clip_host_state* s, int n_steps, uint32_t* frame, uint8_t* mask) {
  if (!s || !frame || !mask || n_steps < 1 || n_steps > DSM_ASR_RUN_MAX) return DSM_ERR_INVALID;
  dsm_asr_clip::plan(s->slots.data(), (int)s->slots.size(), n_steps, frame, mask);
  return 0;
}

int dsm_asr_set_clips(dsm_engine* e, int on, size_t max_clip_bytes_per_slot) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> lk(e->clip_mu);
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // between steps: waits for calls in progress; allocations never run beside a capture
  if (e->clip_blk_pending) { e->set_error("a block of %d steps waits for dsm_asr_collect", e->clip_blk_pending); return DSM_ERR_STATE; }
  for (size_t b = 0; b < e->clip_slots.size(); ++b)
    if (e->clip_slots[b].status != DSM_ASR_CLIP_IDLE) {
      e->set_error("dsm_asr_set_clips: slot %d has a clip (dsm_asr_reset_slot ends it)", (int)b);
      return DSM_ERR_STATE;
    }
  if (!on) { e->clips_on.store(false, std::memory_order_release); return 0; }
  if (max_clip_bytes_per_slot < 1 || (uint64_t)max_clip_bytes_per_slot > kClipMaxBytes) {
    e->set_error("dsm_asr_set_clips: max_clip_bytes_per_slot %zu is outside 1 .. 2^31", max_clip_bytes_per_slot);
    return DSM_ERR_INVALID;
  }
  const size_t cap16 = (max_clip_bytes_per_slot + 15) & ~(size_t)15;
  if (e->clip_d && cap16 != ((e->clip_cap + 15) & ~(size_t)15)) {
    e->set_error("dsm_asr_set_clips: the engine's clips hold %zu bytes a slot, not %zu", e->clip_cap, max_clip_bytes_per_slot);
    return DSM_ERR_STATE;
  }
  if (int rc = ingest_ensure(e)) return rc;
  e->ingest_on = true;
  if (!e->clip_d)
    if (int rc = clips_ensure(e, cap16)) return rc;
  e->clip_cap = max_clip_bytes_per_slot;
  e->clips_on.store(true, std::memory_order_release);
  return 0;
}

int dsm_asr_clip_begin(dsm_engine* e, int slot, int sample_rate_hz, int sample_format, int flush_frames) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  if (flush_frames < 0) { e->set_error("dsm_asr_clip_begin: flush_frames %d is negative", flush_frames); return DSM_ERR_INVALID; }
  uint32_t fb = 0;
  std::string err;
  if (int rc = clip_frame_bytes(sample_rate_hz, sample_format, &fb, &err)) { e->set_error("%s", err.c_str()); return rc; }
  if (int rc = clips_are_on(e)) return rc;
  if (int rc = e->clip_guard_slots(&slot, 1, "dsm_asr_clip_begin")) return rc;  // a block waits, or the slot has a clip already
  if (clip_ticket_outstanding(e)) {
    e->set_error("dsm_asr_clip_begin: an encode ticket is outstanding (dsm_asr_step_tokens_ticket it first)");
    return DSM_ERR_STATE;
  }
  if (int rc = dsm_asr_reset_slot(e, slot)) return rc;
  if (int rc = dsm_mimi_reset_slot(e, slot)) return rc;
  if (int rc = dsm_asr_set_input_format(e, slot, sample_rate_hz, sample_format)) return rc;
  std::lock_guard<std::mutex> lk(e->clip_mu);
  dsm_asr_clip::begin(&e->clip_slots[(size_t)slot], fb, (uint64_t)flush_frames);
  return 0;
}

int dsm_asr_clip_push(dsm_engine* e, int slot, const void* bytes, size_t n) {
  if (!e || (!bytes && n)) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  if (int rc = clips_are_on(e)) return rc;
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> lk(e->clip_mu);  // clip_mu before the API lock, everywhere
  ApiShared api(e);
  if (e->clip_blk_pending) { e->set_error("a block of %d steps waits for dsm_asr_collect", e->clip_blk_pending); return DSM_ERR_STATE; }
  dsm_asr_clip::Slot s = e->clip_slots[(size_t)slot];
  const uint64_t at = s.bytes;
  if (!dsm_asr_clip::push(&s, n, e->clip_cap)) {
    if (s.status == DSM_ASR_CLIP_IDLE) e->set_error("slot %d: no clip (dsm_asr_clip_begin first)", slot);
    else if (s.closed) e->set_error("slot %d: the clip was closed", slot);
    else e->set_error("slot %d: the clip holds %llu bytes, %zu more pass the %zu a slot holds", slot, (unsigned long long)at, n, e->clip_cap);
    return DSM_ERR_STATE;
  }
  if (n) {
    // the pinned mirror is append-only within a clip, so the copy may read it whenever the encoder stream gets there; a block
    // enqueued later cuts behind it
    const size_t off = (size_t)slot * ((e->clip_cap + 15) & ~(size_t)15) + (size_t)at;
    memcpy(e->clip_h + off, bytes, n);
    HIPCHK(hipMemcpyAsync(e->clip_d + off, e->clip_h + off, n, hipMemcpyHostToDevice, e->s_enc));
  }
  e->clip_slots[(size_t)slot] = s;
  return 0;
}

int dsm_asr_clip_close(dsm_engine* e, int slot) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  if (int rc = clips_are_on(e)) return rc;
  std::lock_guard<std::mutex> lk(e->clip_mu);
  if (e->clip_blk_pending) { e->set_error("a block of %d steps waits for dsm_asr_collect", e->clip_blk_pending); return DSM_ERR_STATE; }
  if (!dsm_asr_clip::close(&e->clip_slots[(size_t)slot])) { e->set_error("slot %d: no clip (dsm_asr_clip_begin first)", slot); return DSM_ERR_STATE; }
  return 0;
}

int dsm_asr_clip_status(dsm_engine* e, int slot) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) { e->set_error("batch index out of range: %d >= %d", slot, e->B); return DSM_ERR_INVALID; }
  if (!e->clips_on.load(std::memory_order_acquire)) return DSM_ASR_CLIP_IDLE;
  std::lock_guard<std::mutex> lk(e->clip_mu);
  return e->clip_slots[(size_t)slot].status;
}

int dsm_asr_run(dsm_engine* e, int n_steps) {
  if (!e) return DSM_ERR_INVALID;
  if (int rc = clips_are_on(e)) return rc;
  if (!e->ingest_on) { e->set_error("ingest is off: the clips' frames go through it (dsm_asr_set_ingest(engine, 1))"); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> lk(e->clip_mu);  // clip_mu before the API lock, everywhere
  ApiShared api(e);
  if (e->clip_blk_pending) { e->set_error("a block of %d steps waits for dsm_asr_collect", e->clip_blk_pending); return DSM_ERR_STATE; }
  if (n_steps < 1 || n_steps > DSM_ASR_RUN_MAX) { e->set_error("dsm_asr_run: n_steps %d outside 1..%d", n_steps, DSM_ASR_RUN_MAX); return DSM_ERR_STATE; }
  if (clip_ticket_outstanding(e)) {
    e->set_error("dsm_asr_run: an encode ticket is outstanding (dsm_asr_step_tokens_ticket it first)");
    return DSM_ERR_STATE;
  }
  const size_t B = (size_t)e->B, cap16 = (e->clip_cap + 15) & ~(size_t)15;
  const int heads = e->cfg.extra_heads_num;
  const size_t pitch = DSM_PCM_MAX_FRAME_BYTES;
  // the block's table: the clips as they are now, then every slot's frame index and mask for the n steps (the slots advance)
  AsrClipSlot* ts = reinterpret_cast<AsrClipSlot*>(e->clip_tab_h);
  for (size_t b = 0; b < B; ++b) {
    const dsm_asr_clip::Slot& s = e->clip_slots[b];
    const dsm_pcm_desc& d = e->ingest_fmt.slot((int)b);
    ts[b] = AsrClipSlot{(uint32_t)s.bytes, s.frame_bytes, dsm_asr_clip::silence_byte(d.fmt), 0u};
    if (s.status != DSM_ASR_CLIP_IDLE && (s.frame_bytes != d.frame_bytes || s.bytes > e->clip_cap)) {
      e->set_error("slot %d: its clip's frame has %u bytes, its input format's %u", (int)b, s.frame_bytes, d.frame_bytes);
      return DSM_ERR_STATE;
    }
  }
  dsm_asr_clip::plan(e->clip_slots.data(), e->B, n_steps, reinterpret_cast<uint32_t*>(e->clip_tab_h + clip_tab_frame_off(B)),
                     e->clip_tab_h + clip_tab_mask_off(B));
  hipStream_t enc = e->s_enc, mod = e->s_model;
  HIPCHK(hipMemcpyAsync(e->clip_tab_d, e->clip_tab_h, clip_tab_bytes(B), hipMemcpyHostToDevice, enc));
  AsrClipArgs ca;
  ca.clips = e->clip_d;
  ca.cap = cap16;
  ca.slots = reinterpret_cast<const AsrClipSlot*>(e->clip_tab_d);
  ca.frame = reinterpret_cast<const uint32_t*>(e->clip_tab_d + clip_tab_frame_off(B));
  ca.step_mask = e->clip_tab_d + clip_tab_mask_off(B);
  ca.raw = e->ingest_raw_d[0];
  ca.pitch = pitch;
  ca.mask = e->mimi[0].mask;
  ca.B = e->B;
  LmState& lm = e->lm;
  const size_t code_bytes = sizeof(uint32_t) * B * (size_t)e->cfg.audio_codebooks;
  for (int k = 0; k < n_steps; ++k) {
    // encoder stream: dsm_mimi_encode_step_raw_dev's body behind the cut.  The step before's codes and mask must have been
    // picked up by the model stream before the cut overwrites the mask and the encode the codes.
    if (e->codes_consumed_valid) HIPCHK(hipStreamWaitEvent(enc, e->ev_codes_consumed, 0));
    hipLaunchKernelGGL(asr_clip_frame_kernel, dim3((unsigned)B), dim3(256), 0, enc, ca, k);
    HIPCHK(hipGetLastError());
    if (int rc = ingest_launch(e, 0, enc, e->ingest_raw_d[0], pitch, e->mimi[0].mask)) return rc;
    if (int rc = mimi_encode(e, 0, enc)) return rc;
    HIPCHK(hipEventRecord(e->ev_join, enc));
    // model stream: dsm_asr_step_tokens_dev(codes = NULL)'s body, the mask taken in the same hand-off as the codes
    if (int rc = wait_group_inputs(e)) return rc;
    HIPCHK(hipStreamWaitEvent(mod, e->ev_join, 0));
    HIPCHK(hipMemcpyAsync(lm.codes_in, e->mimi[0].codes, code_bytes, hipMemcpyDeviceToDevice, mod));
    HIPCHK(hipMemcpyAsync(lm.mask, e->mimi[0].mask, B, hipMemcpyDeviceToDevice, mod));
    HIPCHK(hipEventRecord(e->ev_codes_consumed, mod));
    e->codes_consumed_valid = true;
    const int rc = lm_step_then(e, mod, lm.codes_in, lm.mask, lm.text_out, heads > 0 ? lm.prs : nullptr, [&](int g, hipStream_t gs) -> int {
      const LmState::Group& grp = lm.groups[(size_t)g];
      const int n = grp.nb * (2 + heads);
      hipLaunchKernelGGL(asr_clip_record_kernel, dim3((unsigned)(n + 255) / 256), dim3(256), 0, gs, e->clip_rec_d, k, lm.text_out,
                         e->scores_top_n >= 0 ? e->scores_lp : nullptr, lm.prs, grp.b0, grp.nb, e->B, heads);
      HIPCHK(hipGetLastError());
      return 0;
    });
    if (rc) return rc;
  }
  if (int rc = join_groups(e)) return rc;
  HIPCHK(hipMemcpyAsync(e->clip_rec_h, e->clip_rec_d, sizeof(uint32_t) * (size_t)n_steps * dsm_asr_clip::record_words(e->B, heads),
                        hipMemcpyDeviceToHost, mod));
  e->metrics.steps_encode += (uint64_t)n_steps;
  e->metrics.steps_lm += (uint64_t)n_steps;
  e->clip_blk_pending = n_steps;
  return 0;
}

int dsm_asr_collect(dsm_engine* e, dsm_asr_block* out) {
  if (!e || !out) return DSM_ERR_INVALID;
  if (int rc = clips_are_on(e)) return rc;
  if ((out->msgs_cap > 0 && (!out->msgs || !out->msg_step)) || out->msgs_cap < 0 || out->tokens_cap < 0 ||
      (out->tokens_cap > 0 && (!out->msg_tokens || !out->msg_logprobs))) {
    e->set_error("dsm_asr_collect: a message or token capacity without its arrays");
    return DSM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(e->device));
  std::lock_guard<std::mutex> lk(e->clip_mu);  // clip_mu before the API lock, everywhere
  ApiShared api(e);
  if (!e->clip_blk_pending) { e->set_error("no block waits: dsm_asr_run first"); return DSM_ERR_STATE; }
  HIPCHK(hipStreamSynchronize(e->s_model));  // the block's one synchronise: the records' download is the model stream's last
  const int n = e->clip_blk_pending, B = e->B, heads = e->cfg.extra_heads_num;
  const size_t words = (size_t)n * dsm_asr_clip::record_words(B, heads);
  const uint8_t* mask = e->clip_tab_h + clip_tab_mask_off((size_t)B);
  e->clip_blk_pending = 0;
  if (!dsm_asr_clip::unpack(e->clip_rec_h, words, mask, n, B, heads, out->stepped, out->text_token, out->vad_prs, out->logprob)) {
    e->set_error("dsm_asr_collect: the block's records do not hold %d steps", n);
    return DSM_ERR_STATE;
  }
  out->n_steps = n;
  out->n_msgs = 0;
  out->n_tokens = 0;
  // word assembly, once per step over the records: HostItem, model_step_idx and the word scores end as after the per-step calls
  for (int k = 0; k < n; ++k) {
    const uint32_t *text = nullptr, *lp = nullptr, *prs = nullptr;
    dsm_asr_clip::record_row(e->clip_rec_h, words, n, B, heads, k, &text, &lp, &prs);
    assemble_words(e, text, mask + (size_t)k * B, reinterpret_cast<const float*>(lp));
    dsm_asr_clip::append_step(out, k, e->msgs.data(), e->msgs.size(), e->msg_tokens.data(), e->msg_logprobs.data(), e->msg_tokens.size());
  }
  for (int b = 0; b < B && out->status; ++b) out->status[b] = e->clip_slots[(size_t)b].status;
  return 0;
}

}  // extern "C"
