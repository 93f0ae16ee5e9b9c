// dsm_slot_state.inc — slot snapshots: dsm_asr_export_slots / dsm_asr_import_slots / dsm_asr_move_slots (included by
// dsm_engine.hip behind dsm_engine_api.inc).  This file is what is STT about them: which sections a slot's state is, the
// signature, the host items, the payload's index checks and the three calls.  The blob format is csrc/dsm_slot_blob.h; the
// section table, staging and the pack / unpack launch are csrc/dsm_slot_xfer.inc; DESIGN.md has the table of state.
//
// Where a slot's state lives is what reset_transformer_slot, reset_mimi_slot and dsm_asr_reset_slot already enumerate, plus what
// they leave alone because a fresh value is never read (the ring rows behind pos, the shifted codes behind first_step, the
// Gumbel stream).  One call at a time per engine (SlotXfer::mu); every call ends with the streams it used drained, so the
// staging buffers are free again and both host threads' streams see what an import wrote.

namespace {

// Sections of one Mimi side, in blob order: ring position, ring index, K and V rows per layer, the carried conv states in
// ConvStateDesc order.  s null: the side does not exist yet — same sizes (taken from mimi[0]'s table), null bases.
void slot_mimi_sections(const dsm_engine* e, const MimiState* s, std::vector<SlotSection>* out) {
  const dsm_transformer_config& t = e->cfg.mimi.transformer;
  auto add = [&](void* base, size_t stride, size_t bytes) {
    SlotSection x{};
    x.base = reinterpret_cast<char*>(base);
    x.stride = (long)stride;
    x.bytes = (long)bytes;
    out->push_back(x);
  };
  add(s ? s->tr.pos : nullptr, 4, 4);
  add(s ? s->tr.idx : nullptr, 4, 4);
  const size_t ring = (size_t)t.d_model * t.context * sizeof(float);  // [H][ctx][hd] of one slot
  for (int l = 0; l < t.num_layers; ++l) {
    add(s ? s->tr.k[l] : nullptr, ring, ring);
    add(s ? s->tr.v[l] : nullptr, ring, ring);
  }
  for (size_t i = 0; i < e->mimi[0].h_descs.size(); ++i) {
    const ConvStateDesc& d = e->mimi[0].h_descs[i];
    add(s ? s->h_descs[i].cat : nullptr, (size_t)d.bstride * sizeof(float), (size_t)d.S * d.C * sizeof(float));
  }
}

// The section list (its offsets and piece counts: slot_layout_finish) and the signature: host work only, once per engine.
void slot_layout_build(dsm_engine* e) {
  SlotXfer& x = e->xfer;
  if (!x.secs.empty()) return;
  const dsm_asr_config& c = e->cfg;
  LmState& s = e->lm;
  std::vector<SlotSection> v;
  auto add = [&](void* base, size_t stride, size_t bytes) {
    SlotSection sec{};
    sec.base = reinterpret_cast<char*>(base);
    sec.stride = (long)stride;
    sec.bytes = (long)bytes;
    v.push_back(sec);
    return (int)v.size() - 1;
  };
  add(s.tr.pos, 4, 4);
  e->xsec.lm_idx = add(s.tr.idx, 4, 4);
  e->xsec.text_token = add(s.text_token, 4, 4);
  e->xsec.first_step = add(s.first_step, 1, 1);
  e->xsec.rng_pos = add(s.rng_pos, 8, 8);
  add(s.rng_key, 32, 32);
  e->xsec.next_cb = add(s.next_cb, (size_t)c.audio_codebooks * 4, (size_t)c.audio_codebooks * 4);
  const size_t ring = (size_t)c.lm.d_model * c.lm.context * (c.kv_bf16 ? 2 : 4);
  for (int l = 0; l < c.lm.num_layers; ++l) {
    add(s.tr.k[l], ring, ring);
    add(s.tr.v[l], ring, ring);
  }
  e->xsec.mimi_idx = (int)v.size() + 1;
  slot_mimi_sections(e, &e->mimi[0], &v);
  const int nsec_base = (int)v.size();
  slot_mimi_sections(e, nullptr, &v);
  const dsm_transformer_config& mt = c.mimi.transformer;
  x.sig = {(uint32_t)c.lm.num_layers, (uint32_t)c.lm.num_heads, (uint32_t)(c.lm.d_model / c.lm.num_heads), (uint32_t)c.lm.context,
           (uint32_t)(c.kv_bf16 ? 1 : 0), (uint32_t)mt.num_layers, (uint32_t)mt.num_heads, (uint32_t)(mt.d_model / mt.num_heads),
           (uint32_t)mt.context, (uint32_t)c.audio_codebooks, (uint32_t)c.text_in_vocab_size, (uint32_t)c.text_out_vocab_size,
           (uint32_t)c.audio_vocab_size, (uint32_t)c.asr_delay_in_tokens, (uint32_t)e->mimi[0].h_descs.size()};
  for (const ConvStateDesc& d : e->mimi[0].h_descs) {
    x.sig.push_back((uint32_t)d.S);
    x.sig.push_back((uint32_t)d.C);
  }
  slot_layout_finish(x, std::move(v), nsec_base);
}

const char* slot_sig_name(size_t i) {
  static const char* const names[] = {"lm.num_layers", "lm.num_heads", "lm head dim", "lm.context", "kv_bf16", "mimi.transformer.num_layers",
                                      "mimi.transformer.num_heads", "mimi transformer head dim", "mimi.transformer.context",
                                      "audio_codebooks (n_q)", "text_in_vocab_size", "text_out_vocab_size", "audio_vocab_size",
                                      "asr_delay_in_tokens", "number of carried conv states"};
  return i < sizeof names / sizeof names[0] ? names[i] : "carried conv state (S, C) list";
}

// Staging for n slots (slot_stage_ensure), behind what only this engine can do first: the model-side Mimi where the caller
// wants it; with keep: the per-slot keep bytes of every Mimi side whose first call has not run.  Called with SlotXfer::mu
// held and BEFORE the API's shared lock is taken: allocations take the exclusive side, for the reason ensure_model_side_mimi gives.
int slot_xfer_ensure(dsm_engine* e, int n, bool host, bool want_mimi1, bool keep) {
  SlotXfer& x = e->xfer;
  HIPCHK(hipSetDevice(e->device));
  if (want_mimi1)
    if (int rc = ensure_model_side_mimi(e)) return rc;
  const bool has1 = e->mimi1_ready.load(std::memory_order_acquire);
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  if (keep)
    for (int side = 0; side < (has1 ? 2 : 1); ++side) {
      MimiState& s = e->mimi[side];
      if (!s.first_call || s.keep) continue;
      s.keep_h.assign((size_t)e->B, 0);
      if (int rc = e->dalloc(&s.keep, (size_t)e->B)) return rc;
    }
  std::vector<SlotSection> side1;  // mimi[1] came into being since the table went to the device: its bases
  if (has1 && !x.d_has_opt) slot_mimi_sections(e, &e->mimi[1], &side1);
  return slot_stage_ensure(e, x, n, host, has1, side1);
}

// The host half of the listed slots, with the per-side "first call has not run and nothing was imported" flags.
void slot_gather_items(dsm_engine* e, const int* slots, int n, bool has1, std::vector<dsm_slot_blob::HostItem>* out) {
  out->resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const HostItem& it = e->items[(size_t)slots[i]];
    dsm_slot_blob::HostItem& o = (*out)[(size_t)i];
    o.step_idx = (uint64_t)it.step_idx;
    o.last_stop_time = it.last_stop_time;
    o.unended_word = it.unended_word ? 1 : 0;
    o.word_tokens = it.word_tokens;
    o.side_flags = 0;
    for (int side = 0; side < (has1 ? 2 : 1); ++side) {
      const MimiState& s = e->mimi[side];
      if (s.first_call && !(s.keep && s.keep_h[(size_t)slots[i]])) o.side_flags |= DSM_SLOT_SIDE_PRISTINE0 << side;
    }
  }
}

// What an import does besides the unpack launch, on `st`: the host items, the keep bytes of sides that have not run their first
// call (an imported slot is kept unless it was fresh where it came from), and the reset of a model-side Mimi the blob lacks.
int slot_apply_items(dsm_engine* e, hipStream_t st, const int* slots, int n, bool has1, const std::vector<dsm_slot_blob::HostItem>& items) {
  const bool dst1 = e->mimi1_ready.load(std::memory_order_acquire);
  for (int i = 0; i < n; ++i) {
    const dsm_slot_blob::HostItem& in = items[(size_t)i];
    HostItem& it = e->items[(size_t)slots[i]];
    it.step_idx = (size_t)in.step_idx;
    it.last_stop_time = in.last_stop_time;
    it.unended_word = in.unended_word != 0;
    it.word_tokens = in.word_tokens;
    it.word_logprobs.assign(in.word_tokens.size(), dsm_u32_as_f32(0x7FC00000u));  // a snapshot carries no scores: not recorded
    // text bias: the slot keeps its own attachment; where the imported stream stands inside a word is not known
    if (int rc = bias_put_node(e, st, slots[i], in.step_idx == 0 ? 0u : DSM_BIAS_DEAD)) return rc;
    for (int side = 0; side < (has1 ? 2 : 1); ++side) {
      MimiState& s = e->mimi[side];
      if (s.first_call && s.keep) s.keep_h[(size_t)slots[i]] = (in.side_flags & (DSM_SLOT_SIDE_PRISTINE0 << side)) ? 0 : 1;
    }
    if (!has1 && dst1)
      if (int rc = reset_mimi_slot(e, 1, st, slots[i])) return rc;
  }
  for (int side = 0; side < (has1 ? 2 : 1); ++side) {
    MimiState& s = e->mimi[side];
    if (s.first_call && s.keep) HIPCHK(hipMemcpyAsync(s.keep, s.keep_h.data(), (size_t)e->B, hipMemcpyHostToDevice, st));
  }
  return 0;
}

// Index-valued fields of a payload, against this engine's configuration: an unchecked ring index is the next step's
// out-of-bounds store, an unchecked token an out-of-bounds embedding row.
int slot_payload_check(dsm_engine* e, const uint8_t* payload, int n, bool has1) {
  const SlotXfer& x = e->xfer;
  const dsm_asr_config& c = e->cfg;
  const size_t sb = slot_bytes_of(x, has1);
  using dsm_slot_blob::rd32;
  using dsm_slot_blob::rd64;
  for (int i = 0; i < n; ++i) {
    const uint8_t* p = payload + (size_t)i * sb;
    auto at = [&](int sec) { return p + x.secs[(size_t)sec].off; };
    const uint32_t idx = rd32(at(e->xsec.lm_idx));
    if (idx >= (uint32_t)c.lm.context) { e->set_error("slot blob: slot %d: LM ring index %u >= context %d", i, idx, c.lm.context); return DSM_ERR_INVALID; }
    const uint32_t tt = rd32(at(e->xsec.text_token));
    if (tt >= (uint32_t)c.text_in_vocab_size) { e->set_error("slot blob: slot %d: text token %u >= text_in_vocab_size %d", i, tt, c.text_in_vocab_size); return DSM_ERR_INVALID; }
    if (*at(e->xsec.first_step) > 1) { e->set_error("slot blob: slot %d: first_step is not 0 or 1", i); return DSM_ERR_INVALID; }
    const uint64_t rp = rd64(at(e->xsec.rng_pos));
    if (rp % 16) { e->set_error("slot blob: slot %d: Gumbel stream position %llu is not a multiple of 16", i, (unsigned long long)rp); return DSM_ERR_INVALID; }
    for (int q = 0; q < c.audio_codebooks; ++q) {
      const uint32_t code = rd32(at(e->xsec.next_cb) + 4 * q);
      if (code >= (uint32_t)c.audio_vocab_size) { e->set_error("slot blob: slot %d: carried audio code %u >= audio_vocab_size %d", i, code, c.audio_vocab_size); return DSM_ERR_INVALID; }
    }
    for (int side = 0; side < (has1 ? 2 : 1); ++side) {
      const uint32_t mi = rd32(at(e->xsec.mimi_idx + side * x.nsec_opt));
      if (mi >= (uint32_t)c.mimi.transformer.context) {
        e->set_error("slot blob: slot %d: Mimi side %d ring index %u >= context %d", i, side, mi, c.mimi.transformer.context);
        return DSM_ERR_INVALID;
      }
    }
  }
  return 0;
}

bool slot_ticket_outstanding(dsm_engine* e) {
  std::lock_guard<std::mutex> lk(e->pipe_mu);
  for (const auto& ps : e->pipe)
    if (ps.in_flight) return true;
  return false;
}

// Source half of a move: everything enqueued on `e` done, the slots packed into e's staging buffer on the model stream, the
// event behind the launch recorded.  The model stream is NOT drained: the destination waits for the event.
int slot_move_pack(dsm_engine* e, const int* slots, int n, bool has1, std::vector<dsm_slot_blob::HostItem>* items) {
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (!slot_xfer_fits(e->xfer, n, false, has1) || has1 != e->mimi1_ready.load(std::memory_order_acquire)) {
    e->set_error("move_slots: the engine's model-side Mimi came into being during the call; call again");
    return DSM_ERR_STATE;
  }
  if (slot_ticket_outstanding(e)) { e->set_error("move_slots: an encode ticket is outstanding (dsm_asr_step_tokens_ticket it first)"); return DSM_ERR_STATE; }
  if (int rc = dsm_sync(e)) return rc;
  slot_gather_items(e, slots, n, has1, items);
  SlotXfer& x = e->xfer;
  HIPCHK(hipMemcpyAsync(x.d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, e->s_model));
  if (int rc = slot_launch(e, x, e->s_model, true, n, has1, x.d_stage)) return rc;
  HIPCHK(hipEventRecord(x.ev_packed, e->s_model));
  return 0;
}

// Destination half: behind `packed`, scatter `stage` (n slots of the source's layout, with or without mimi[1]) into `slots`.
int slot_move_unpack(dsm_engine* e, const int* slots, int n, bool has1, char* stage, hipEvent_t packed,
                     const std::vector<dsm_slot_blob::HostItem>& items) {
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (!slot_xfer_fits(e->xfer, n, false, has1)) { e->set_error("move_slots: destination staging not ready"); return DSM_ERR_STATE; }
  if (int rc = dsm_sync(e)) return rc;
  SlotXfer& x = e->xfer;
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamWaitEvent(st, packed, 0));
  HIPCHK(hipMemcpyAsync(x.d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  if (int rc = slot_launch(e, x, st, false, n, has1, stage)) return rc;
  if (int rc = slot_apply_items(e, st, slots, n, has1, items)) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

}  // namespace

extern "C" {

int dsm_slot_blob_info(const void* buf, size_t len, struct dsm_slot_blob_info* out) {
  std::string err;
  const int rc = dsm_slot_blob::info(buf, len, out, &err);
  if (rc) g_create_error = err;  // no engine is involved: dsm_last_error(NULL), like a failed create
  return rc;
}

int dsm_asr_export_slots(dsm_engine* e, const int* slots, int n, void* buf, size_t cap, size_t* needed) {
  if (!e) return DSM_ERR_INVALID;
  if (int rc = slot_check_list(e, e->B, slots, n, false, "export_slots")) return rc;
  if (int rc = e->clip_guard_slots(slots, n, "export_slots")) return rc;
  SlotXfer& x = e->xfer;
  std::lock_guard<std::mutex> one(x.mu);
  slot_layout_build(e);
  if (buf)
    if (int rc = slot_xfer_ensure(e, n, true, false, false)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  const bool has1 = e->mimi1_ready.load(std::memory_order_acquire);
  const size_t sb = slot_bytes_of(x, has1);
  if (slot_ticket_outstanding(e)) {
    e->set_error("export_slots: an encode ticket is outstanding (dsm_asr_step_tokens_ticket it first)");
    return DSM_ERR_STATE;
  }
  std::vector<dsm_slot_blob::HostItem> items;
  slot_gather_items(e, slots, n, has1, &items);
  std::vector<uint8_t> front;
  dsm_slot_blob::write_front(front, has1 ? DSM_SLOT_BLOB_HAS_MODEL_MIMI : 0u, x.sig, items, sb);
  const size_t total = front.size() + (size_t)n * sb;
  if (needed) *needed = total;
  if (!buf) return 0;
  if (cap < total) { e->set_error("export_slots: buffer of %zu bytes, the blob needs %zu", cap, total); return DSM_ERR_INVALID; }
  if (!slot_xfer_fits(e->xfer, n, true, has1)) {
    e->set_error("export_slots: the engine's model-side Mimi came into being during the call; call again");
    return DSM_ERR_STATE;
  }
  if (int rc = dsm_sync(e)) return rc;  // both streams and every group: the state is what the last finished step left
  hipStream_t st = e->s_model;
  HIPCHK(hipMemcpyAsync(x.d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  if (int rc = slot_launch(e, x, st, true, n, has1, x.d_stage)) return rc;
  HIPCHK(hipMemcpyAsync(x.h_stage, x.d_stage, (size_t)n * sb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  uint8_t* out = static_cast<uint8_t*>(buf);
  memcpy(out, front.data(), front.size());
  uint8_t* payload = out + front.size();
  memcpy(payload, x.h_stage, (size_t)n * sb);
  slot_zero_gaps(x, payload, n, has1);
  return 0;
}

int dsm_asr_import_slots(dsm_engine* e, const int* slots, int n, const void* buf, size_t len) {
  if (!e) return DSM_ERR_INVALID;
  if (int rc = slot_check_list(e, e->B, slots, n, true, "import_slots")) return rc;
  if (int rc = e->clip_guard_slots(slots, n, "import_slots")) return rc;
  SlotXfer& x = e->xfer;
  std::lock_guard<std::mutex> one(x.mu);
  slot_layout_build(e);
  // ---- everything that can refuse the blob, before anything of the engine changes ----
  dsm_slot_blob::Header h;
  std::string err;
  if (int rc = dsm_slot_blob::read_header(buf, len, &h, &err)) { e->set_error("%s", err.c_str()); return rc; }
  if ((int)h.n_slots != n) { e->set_error("import_slots: the blob holds %u slots, %d were listed", h.n_slots, n); return DSM_ERR_INVALID; }
  const uint8_t* p = static_cast<const uint8_t*>(buf);
  {
    std::vector<uint32_t> theirs(h.sig_words);
    if (h.sig_words) memcpy(theirs.data(), p + h.sig_offset(), 4 * (size_t)h.sig_words);
    const std::string diff = slot_sig_mismatch(theirs.data(), theirs.size(), x.sig, slot_sig_name);
    if (!diff.empty()) { e->set_error("import_slots: the blob is of another configuration: %s", diff.c_str()); return DSM_ERR_INVALID; }
  }
  std::vector<dsm_slot_blob::HostItem> items;
  if (int rc = dsm_slot_blob::read_host(buf, h, &items, &err)) { e->set_error("%s", err.c_str()); return rc; }
  const bool has1 = (h.flags & DSM_SLOT_BLOB_HAS_MODEL_MIMI) != 0;
  const size_t sb = slot_bytes_of(x, has1);  // this engine's own figure; the blob's must agree
  if (h.slot_bytes != (uint64_t)sb) {
    e->set_error("import_slots: the blob has %llu payload bytes per slot, this configuration %zu", (unsigned long long)h.slot_bytes, sb);
    return DSM_ERR_INVALID;
  }
  const uint8_t* payload = p + h.payload_offset();
  if (int rc = slot_payload_check(e, payload, n, has1)) return rc;
  // ---- accepted ----
  if (int rc = slot_xfer_ensure(e, n, true, has1, true)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (!slot_xfer_fits(e->xfer, n, true, has1)) { e->set_error("import_slots: staging not ready"); return DSM_ERR_STATE; }
  if (int rc = dsm_sync(e)) return rc;
  hipStream_t st = e->s_model;
  memcpy(x.h_stage, payload, (size_t)n * sb);
  HIPCHK(hipMemcpyAsync(x.d_stage, x.h_stage, (size_t)n * sb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(x.d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  if (int rc = slot_launch(e, x, st, false, n, has1, x.d_stage)) return rc;
  if (int rc = slot_apply_items(e, st, slots, n, has1, items)) return rc;
  HIPCHK(hipStreamSynchronize(st));  // the encoder stream and the groups start behind this
  return 0;
}

int dsm_asr_move_slots(dsm_engine* src, const int* src_slots, dsm_engine* dst, const int* dst_slots, int n) {
  if (!src || !dst) return DSM_ERR_INVALID;
  if (int rc = slot_check_list(src, src->B, src_slots, n, false, "move_slots (source)")) return rc;
  if (int rc = slot_check_list(dst, dst->B, dst_slots, n, true, "move_slots (destination)")) { src->set_error("%s", dst->err.c_str()); return rc; }
  if (int rc = src->clip_guard_slots(src_slots, n, "move_slots (source)")) return rc;
  if (int rc = dst->clip_guard_slots(dst_slots, n, "move_slots (destination)")) { src->set_error("%s", dst->err.c_str()); return rc; }
  if (src == dst)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        if (src_slots[i] == dst_slots[j]) {
          src->set_error("move_slots: slot %d is both a source and a destination of a move within one engine", src_slots[i]);
          return DSM_ERR_INVALID;
        }
  if (src->device != dst->device) {
    src->set_error("move_slots: the engines are on devices %d and %d: export_slots then import_slots", src->device, dst->device);
    return DSM_ERR_DEVICE;
  }
  std::unique_lock<std::mutex> l1(src->xfer.mu, std::defer_lock), l2(dst->xfer.mu, std::defer_lock);
  if (src == dst) l1.lock(); else std::lock(l1, l2);
  slot_layout_build(src);
  slot_layout_build(dst);
  {
    const std::string diff = slot_sig_mismatch(src->xfer.sig.data(), src->xfer.sig.size(), dst->xfer.sig, slot_sig_name);
    if (!diff.empty()) { src->set_error("move_slots: the engines differ in configuration: %s", diff.c_str()); return DSM_ERR_INVALID; }
  }
  const bool has1 = src->mimi1_ready.load(std::memory_order_acquire);
  if (int rc = slot_xfer_ensure(src, n, false, false, false)) return rc;
  if (int rc = slot_xfer_ensure(dst, n, false, has1, true)) { src->set_error("%s", dst->err.c_str()); return rc; }
  std::vector<dsm_slot_blob::HostItem> items;
  if (int rc = slot_move_pack(src, src_slots, n, has1, &items)) return rc;
  if (int rc = slot_move_unpack(dst, dst_slots, n, has1, src->xfer.d_stage, src->xfer.ev_packed, items)) {
    if (src != dst) src->set_error("%s", dst->err.c_str());
    (void)hipStreamSynchronize(src->s_model);
    return rc;
  }
  return 0;
}

}  // extern "C"
