// dsm_tts_request.inc — a request's text schedule on the device, K steps per visit (part of the library's one translation
// unit, behind dsm_tts.inc).  The reference's inference loop (srv/tts.rs:574-621 streaming, :852-907 over a whole prompt) decides
// prev_text_token and `allowed` of every step from the previous step's text token; with that decision on the host every step is
// a round trip (download, host loop over B slots, three uploads).  Here the loop's state lives in HBM (TtsReqState, the word
// queue), tts_sched_kernel writes every buffer dsm_tts_step uploads and tts_commit_kernel does the loop body behind the samplers,
// so dsm_tts_run enqueues K steps back to back and dsm_tts_collect waits once.
//
// The two kernels are launched on the model stream OUTSIDE the groups' graphs: the step of the block (record row, frame buffer)
// is a launch argument, and the graphs stay the ones dsm_tts_step replays.  The host picks a group's graph variant (with /
// without the depformer) from an upper bound of its slots' step indices — the index at the last collect plus the steps enqueued
// since; a slot that sat a step out or is done only has a smaller index, and its row flags keep the depformer off it: a depformer
// pass whose rows are all inactive writes the per-step scratch (x, xn, start_pos, widx of dep_head_row) and nothing that
// outlives the step — pos / idx are zeroed per step, the samplers return before `lat`, `last_tok` and the generators, and
// transformer_forward's rows are masked by d_rrun.  Mixed batches of dsm_tts_step rely on the same flags.
//
// Audio-token history: input assembly reads audio_tokens[step - 1][0] and audio_tokens[step - acoustic_delay - 1][k >= 1]
// (core/tts_streaming.rs:138,148).  Both are the slot's previous samples — d_lat, which only a step of the slot itself rewrites —
// except row 0's codebooks >= 1, which tts_frame_kernel already keeps in d_row0.  d_ring (codebook 0 of the last
// acoustic_delay + 1 steps) is what the FRAME needs, not the input; no further table is kept on the device, and the host's
// items[b] is rebuilt from the block's records with the write-back of dsm_tts_step.

namespace {

int tts_request_end(dsm_tts* t, int slot) {
  DsmDevice* e = t;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipLaunchKernelGGL(tts_req_init_kernel, dim3(1), dim3(1), 0, e->s_model, t->d_req + slot, TtsReqState{});
  HIPCHK(hipGetLastError());
  t->reqs[slot] = dsm_tts::ReqHost{};
  return 0;
}

// the groups of one step; run_dep per group from the host's upper bound of the slots' step indices
int tts_run_step_groups(dsm_tts* t, hipStream_t st, const std::vector<size_t>& ub) {
  DsmDevice* e = t;
  const size_t Gn = t->groups.size(), tad = (size_t)t->cfg.text_audio_delay_in_tokens;
  if (int rc = fork_groups(e, st, Gn)) return rc;
  if (int rc = run_groups(e, st, Gn, false, [&](size_t g, hipStream_t gs) {
        dsm_tts::Grp& grp = t->groups[g];
        bool run_dep = false;
        for (int b = grp.b0; b < grp.b0 + grp.nb; ++b) run_dep = run_dep || (ub[b] != SIZE_MAX && ub[b] >= tad);
        return run_captured(e, *t->g_ttsg[g][run_dep ? 1 : 0], gs, (run_dep ? 1 : 0) | (tts_any_sampling(t) ? 2 : 0),
                            [&] { return tts_group_body(t, gs, grp, run_dep); });
      }))
    return rc;
  return join_groups(e, st, Gn);
}

int tts_run_impl(dsm_tts* t, int n_steps, bool decode) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int B = t->B, R = t->R, S = c.dep_num_slices;
  hipStream_t st = e->s_model;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  for (int r = 0; r < R; ++r) t->h_ca_has[r] = t->ca_len[r] > 0 ? 1 : 0;
  HIPCHK(hipMemcpyAsync(t->d_ca_has, t->h_ca_has, (size_t)R, hipMemcpyHostToDevice, st));
  // upper bound of every stepping slot's index before step s of the block: SIZE_MAX = the slot cannot step
  std::vector<size_t> ub(B, SIZE_MAX);
  for (int b = 0; b < B; ++b) {
    const dsm_tts::ReqHost& rq = t->reqs[b];
    if (rq.active && rq.status != DSM_TTS_REQ_DONE && rq.status != DSM_TTS_REQ_DONE_LIMIT) ub[b] = t->items[b].step_idx;
  }
  TtsSchedArgs sa;
  sa.req = t->d_req; sa.q_tok = t->d_qtok; sa.q_end = t->d_qend; sa.qcap = t->qcap;
  sa.rec_ld = t->rec_ld;
  sa.tokens = t->d_tokens; sa.allowed = t->d_allowed;
  sa.mask = t->d_mask; sa.force = t->d_force_eop; sa.run = t->d_run; sa.forced = t->d_forced;
  sa.rmask = t->d_rmask; sa.rrun = t->d_rrun; sa.ca_act = t->d_ca_act; sa.fsel = t->d_fsel; sa.step = t->d_step;
  sa.lat = t->d_lat; sa.row0 = t->d_row0; sa.cfg_on = t->d_cfg_on; sa.ca_has = t->d_ca_has;
  sa.B = B; sa.rps = t->rps; sa.nc = c.audio_codebooks; sa.S = S; sa.ad = c.acoustic_delay; sa.tad = c.text_audio_delay_in_tokens;
  sa.max_cpads = c.max_consecutive_pads; sa.text_in_vocab = c.text_in_vocab_size; sa.n_steps = (int)t->n_steps;
  sa.pad = (uint32_t)c.audio_vocab_size - 1;
  TtsCommitArgs ca;
  ca.req = t->d_req; ca.rec_ld = t->rec_ld; ca.mask = t->d_mask; ca.run = t->d_run; ca.text_token = t->d_text_token; ca.lat = t->d_lat;
  ca.B = B; ca.S = S; ca.text_pad = (uint32_t)c.text_pad_token; ca.text_eop = (uint32_t)c.text_eop_token;
  const dim3 grid((B + 63) / 64), block(64);
  for (int s = 0; s < n_steps; ++s) {
    int32_t* rec = t->d_blk + (size_t)s * B * t->rec_ld;
    sa.rec = rec;
    sa.sel = decode ? 3 + s : 2;  // a frame buffer per step of the block; the spare one when nothing decodes
    hipLaunchKernelGGL(tts_sched_kernel, grid, block, 0, st, sa);
    HIPCHK(hipGetLastError());
    if (int rc = tts_run_step_groups(t, st, ub)) return rc;
    ca.rec = rec;
    hipLaunchKernelGGL(tts_commit_kernel, grid, block, 0, st, ca);
    HIPCHK(hipGetLastError());
    if (decode) {
      dsm_tts::PcmEntry& en = t->blk_pcm[s];
      en.launched = false;
      bool any = false;
      for (int b = 0; b < B; ++b)
        any = any || (ub[b] != SIZE_MAX && ub[b] >= (size_t)(c.text_audio_delay_in_tokens + c.acoustic_delay));
      if (any)
        if (int rc = tts_enqueue_decode(t, 3 + s, en)) return rc;
    }
    for (int b = 0; b < B; ++b)
      if (ub[b] != SIZE_MAX) ub[b] += 1;
  }
  HIPCHK(hipMemcpyAsync(t->h_blk, t->d_blk, sizeof(int32_t) * (size_t)n_steps * B * t->rec_ld, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(t->h_req, t->d_req, sizeof(TtsReqState) * (size_t)B, hipMemcpyDeviceToHost, st));
  t->blk_pending = n_steps;
  t->blk_decode = decode;
  return 0;
}

// raw (dsm_tts_collect_raw, egress on): [n][B][pitch] rows in the place of out->pcm, which is NULL then
int tts_collect_impl(dsm_tts* t, dsm_tts_block* out, uint8_t* raw = nullptr, size_t pitch = 0) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int B = t->B, S = c.dep_num_slices, n = t->blk_pending, ld = t->rec_ld;
  const uint32_t pad = (uint32_t)c.audio_vocab_size - 1, UNG = DSM_TTS_UNGENERATED;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  HIPCHK(hipStreamSynchronize(e->s_model));
  if (t->blk_decode)
    for (int s = 0; s < n; ++s)
      if (t->blk_pcm[s].launched) HIPCHK(hipEventSynchronize(t->blk_pcm[s].ev));
  if (raw && t->blk_decode)  // a pitch below an emitted frame is refused before anything is consumed
    for (int s = 0; s < n; ++s) {
      const dsm_tts::PcmEntry& en = t->blk_pcm[s];
      for (int b = 0; en.launched && b < B; ++b)
        if (en.h_valid[b] && en.fb[(size_t)b] > pitch) {
          e->set_error("raw frames: slot %d's frame has %u bytes, the pitch is %zu", b, en.fb[(size_t)b], pitch);
          return DSM_ERR_INVALID;
        }
    }
  out->n_steps = n;
  out->n_events = 0;
  for (int s = 0; s < n; ++s)
    for (int b = 0; b < B; ++b) {
      const int32_t* rec = t->h_blk + ((size_t)s * B + b) * ld;
      const size_t at_sb = (size_t)s * B + b;
      dsm_tts::Item& it = t->items[b];
      const bool stepped = rec[TTS_REC_STEPPED] != 0, run = rec[TTS_REC_RUN] != 0;
      const uint32_t text_token = (uint32_t)rec[TTS_REC_TEXT];
      if (out->stepped) out->stepped[at_sb] = stepped ? 1 : 0;
      if (out->text_token) out->text_token[at_sb] = stepped ? text_token : 0;
      if (out->audio)
        for (int k = 0; k < S; ++k) out->audio[at_sb * S + k] = (uint32_t)rec[TTS_REC_HDR + k];
      if (out->pcm_valid || out->pcm || raw) {
        const dsm_tts::PcmEntry& en = t->blk_pcm[s];
        const bool v = t->blk_decode && en.launched && en.h_valid[b];
        if (out->pcm_valid) out->pcm_valid[at_sb] = v ? 1 : 0;
        if (raw && v) memcpy(raw + at_sb * pitch, en.h_raw + (size_t)b * en.raw_pitch, en.fb[(size_t)b]);
        if (out->pcm && v)
          memcpy(out->pcm + at_sb * DSM_FRAME_SIZE, en.h_pcm + (size_t)b * DSM_FRAME_SIZE, sizeof(float) * DSM_FRAME_SIZE);
      }
      // overwrite_last_text_token(pad) decided in front of this step (the close arrived while the slot was WAITING)
      if ((rec[TTS_REC_OVW] & 1) && it.step_idx > 0) it.text_tokens[it.step_idx - 1] = (uint32_t)c.text_pad_token;
      if (!stepped) continue;
      // State::step's bookkeeping, as dsm_tts_step does it behind its download
      if (text_token == (uint32_t)c.text_pad_token) it.consecutive_pads += 1; else it.consecutive_pads = 0;
      it.text_tokens[it.step_idx] = text_token;
      for (int k = 0; k < S; ++k) {  // delayed write-back — core/tts_streaming.rs:220-236
        const size_t delay = k == 0 ? 0 : (size_t)c.acoustic_delay;
        const size_t at = it.step_idx >= delay ? it.step_idx - delay : 0;
        uint32_t& pos = it.audio_tokens[at * S + k];
        if (pos == UNG) pos = run ? (uint32_t)rec[TTS_REC_HDR + k] : pad;
      }
      it.step_idx += 1;
      if (rec[TTS_REC_OVW] & 2) it.text_tokens[it.step_idx - 1] = (uint32_t)c.text_pad_token;  // srv/tts.rs:607-610
      if (rec[TTS_REC_EV]) {
        if (out->events && out->n_events < out->events_cap)
          out->events[out->n_events] = dsm_tts_word_event{b, rec[TTS_REC_EV_WORD], rec[TTS_REC_EV_START], rec[TTS_REC_EV_STOP]};
        out->n_events += 1;
      }
    }
  for (int b = 0; b < B; ++b) {
    if (t->reqs[b].active) t->reqs[b].status = t->h_req[b].status;
    if (out->status) out->status[b] = t->reqs[b].status;
  }
  t->blk_pending = 0;
  return 0;
}

}  // namespace

extern "C" {

int dsm_tts_request_begin(dsm_tts* t, int slot, int max_seq_len, int extra_steps) {
  if (!t || slot < 0 || slot >= t->B || max_seq_len < 1 || extra_steps < 0) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  if (t->reqs[slot].active) { e->set_error("slot %d has a request already (dsm_tts_reset_slot ends it)", slot); return DSM_ERR_STATE; }
  if (t->items[slot].step_idx != 0) {
    e->set_error("slot %d is at step %zu: dsm_tts_request_begin needs a fresh slot (dsm_tts_reset_slot first)", slot, t->items[slot].step_idx);
    return DSM_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  TtsReqState r{};
  r.status = TTS_REQ_RUNNING;
  r.cur_word = -1;  // Some(vec![]): the empty word that triggers the first bos — srv/tts.rs:577
  r.has_word = 1;
  r.last_text = (uint32_t)t->cfg.text_start_token;
  r.max_seq_len = max_seq_len;
  r.extra_steps = extra_steps;
  hipLaunchKernelGGL(tts_req_init_kernel, dim3(1), dim3(1), 0, e->s_model, t->d_req + slot, r);
  HIPCHK(hipGetLastError());
  dsm_tts::ReqHost& rq = t->reqs[slot];
  rq = dsm_tts::ReqHost{};
  rq.active = true;
  rq.status = DSM_TTS_REQ_RUNNING;
  return 0;
}

int dsm_tts_request_push_words(dsm_tts* t, int slot, const uint32_t* tokens, const int* word_len, int n_words) {
  if (!t || slot < 0 || slot >= t->B || n_words < 0 || (n_words > 0 && !word_len)) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  long n_tok = 0;
  for (int w = 0; w < n_words; ++w) {
    if (word_len[w] < 0) return DSM_ERR_INVALID;
    n_tok += word_len[w];
  }
  if (n_tok > 0 && !tokens) return DSM_ERR_INVALID;
  dsm_tts::ReqHost& rq = t->reqs[slot];
  if (!rq.active || rq.closed) { e->set_error("slot %d: %s", slot, rq.active ? "the request was closed" : "no request (dsm_tts_request_begin first)"); return DSM_ERR_STATE; }
  if (rq.n_tok + n_tok > t->qcap || rq.n_words + n_words > t->qcap) {
    e->set_error("slot %d: the word queue holds %d tokens and %d words per request", slot, t->qcap, t->qcap);
    return DSM_ERR_STATE;
  }
  if (n_words == 0) return 0;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  // The pinned mirrors are append-only within a request, so the copies may read them whenever the stream gets there; the word
  // count travels in a launch behind them: no step sees a word before its tokens.
  const size_t q0 = (size_t)slot * t->qcap;
  int end = rq.n_tok;
  if (n_tok > 0) memcpy(t->h_qtok + q0 + rq.n_tok, tokens, sizeof(uint32_t) * (size_t)n_tok);
  for (int w = 0; w < n_words; ++w) {
    end += word_len[w];
    t->h_qend[q0 + rq.n_words + w] = end;
  }
  if (n_tok > 0)
    HIPCHK(hipMemcpyAsync(t->d_qtok + q0 + rq.n_tok, t->h_qtok + q0 + rq.n_tok, sizeof(uint32_t) * (size_t)n_tok, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_qend + q0 + rq.n_words, t->h_qend + q0 + rq.n_words, sizeof(int32_t) * (size_t)n_words, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(tts_req_store_kernel, dim3(1), dim3(1), 0, st, &t->d_req[slot].n_words, (int32_t)(rq.n_words + n_words));
  HIPCHK(hipGetLastError());
  rq.n_tok += (int)n_tok;
  rq.n_words += n_words;
  rq.bos_done = true;
  return 0;
}

int dsm_tts_attach_tokenizer(dsm_tts* t, const char* path) {
  if (!t || !path) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (t->tok) { e->set_error("a tokenizer is attached already"); return DSM_ERR_STATE; }
  dsm_spm* tok = nullptr;
  if (int rc = dsm_spm_load(path, &tok)) { e->set_error("tokenizer %s: %s", path, dsm_spm_last_error(nullptr)); return rc; }
  if (dsm_spm_vocab_size(tok) > t->cfg.text_out_vocab_size) {
    e->set_error("tokenizer %s has %d pieces, the model's text_out_vocab_size is %d", path, dsm_spm_vocab_size(tok), t->cfg.text_out_vocab_size);
    dsm_spm_free(tok);
    return DSM_ERR_INVALID;
  }
  t->tok.reset(tok);
  return 0;
}

// recv_loop's body for one text message — srv/tts.rs:480-494.  Host work only: the words go through the upload of
// dsm_tts_request_push_words, which checks everything before it touches the queue, so a refusal leaves the request as it was.
int dsm_tts_request_push_text(dsm_tts* t, int slot, const char* utf8, size_t len, int* n_words_out) {
  if (!t || slot < 0 || slot >= t->B || (!utf8 && len)) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->tok) { e->set_error("dsm_tts_request_push_text needs dsm_tts_attach_tokenizer first"); return DSM_ERR_STATE; }
  const dsm_tts::ReqHost& rq = t->reqs[slot];
  std::vector<uint32_t> tokens, ids;
  std::vector<int> word_len;
  for (size_t at = 0; at <= len;) {  // msg.split(' '): U+0020 only
    size_t end = at;
    while (end < len && utf8[end] != ' ') ++end;
    if (end > at) {  // empty words are skipped; a word that normalizes to nothing is sent as an empty word, like upstream
      dsm_spm_ns::encode(t->tok->m, (const uint8_t*)utf8 + at, end - at, ids);
      const bool bos = !rq.bos_done && word_len.empty();  // inserted_bos
      if (bos) tokens.push_back((uint32_t)t->cfg.text_bos_token);
      tokens.insert(tokens.end(), ids.begin(), ids.end());
      word_len.push_back((int)ids.size() + (bos ? 1 : 0));
    }
    at = end + 1;
  }
  if (n_words_out) *n_words_out = 0;
  // zero words (a message of spaces) still goes through the checks: a slot that cannot take words refuses the message
  if (int rc = dsm_tts_request_push_words(t, slot, tokens.data(), word_len.data(), (int)word_len.size())) return rc;
  if (n_words_out) *n_words_out = (int)word_len.size();
  return 0;
}

int64_t dsm_tts_word_text(dsm_tts* t, int slot, int word, char* out, size_t cap) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->tok) { e->set_error("dsm_tts_word_text needs dsm_tts_attach_tokenizer first"); return DSM_ERR_STATE; }
  const dsm_tts::ReqHost& rq = t->reqs[slot];
  if (!rq.active) { e->set_error("slot %d: no request (its word tokens are kept until dsm_tts_reset_slot)", slot); return DSM_ERR_STATE; }
  if (word < -1 || word >= rq.n_words) { e->set_error("slot %d: no word %d (the request has received %d)", slot, word, rq.n_words); return DSM_ERR_INVALID; }
  if (word == -1) return 0;  // Some(vec![]): the initial empty word — srv/tts.rs:577
  const size_t q0 = (size_t)slot * t->qcap;
  const int begin = word > 0 ? t->h_qend[q0 + word - 1] : 0, end = t->h_qend[q0 + word];
  std::string text, err;
  if (int rc = dsm_spm_ns::decode(t->tok->m, t->h_qtok + q0 + begin, (size_t)(end - begin), text, err)) {
    e->set_error("slot %d word %d: %s", slot, word, err.c_str());
    return rc;
  }
  if (out && text.size() <= cap && !text.empty()) memcpy(out, text.data(), text.size());
  return (int64_t)text.size();
}

int dsm_tts_request_close(dsm_tts* t, int slot) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  dsm_tts::ReqHost& rq = t->reqs[slot];
  if (!rq.active) { e->set_error("slot %d: no request (dsm_tts_request_begin first)", slot); return DSM_ERR_STATE; }
  if (rq.closed) return 0;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipLaunchKernelGGL(tts_req_store_kernel, dim3(1), dim3(1), 0, e->s_model, &t->d_req[slot].closed, (int32_t)1);
  HIPCHK(hipGetLastError());
  rq.closed = true;
  return 0;
}

int dsm_tts_run(dsm_tts* t, int n_steps, int decode) {
  if (!t) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  if (n_steps < 1 || n_steps > DSM_TTS_RUN_MAX) { e->set_error("dsm_tts_run: n_steps %d outside 1..%d", n_steps, DSM_TTS_RUN_MAX); return DSM_ERR_STATE; }
  if (decode && !t->mimi) { e->set_error("dsm_tts_run with decode needs dsm_tts_attach_mimi first"); return DSM_ERR_STATE; }
  if (decode && t->pcm_pending > 0) { e->set_error("%d deferred step(s) wait for dsm_tts_recv_pcm", t->pcm_pending); return DSM_ERR_STATE; }
  return tts_run_impl(t, n_steps, decode != 0);
}

int dsm_tts_collect(dsm_tts* t, dsm_tts_block* out) {
  if (!t || !out) return DSM_ERR_INVALID;
  if (!t->blk_pending) { t->set_error("no block waits: dsm_tts_run first"); return DSM_ERR_STATE; }
  if (t->egress_on && t->blk_decode && out->pcm) { t->set_error("egress is on: dsm_tts_collect_raw delivers the frames"); return DSM_ERR_STATE; }
  return tts_collect_impl(t, out);
}

int dsm_tts_request_status(dsm_tts* t, int slot) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  return t->reqs[slot].status;
}

}  // extern "C"
