// dsm_tts.inc — TTS step (BASELINE.json configs[4]): tts_streaming::State::step over B independent generations (part of the
// library's one translation unit).  Device work: input embedding sum, main LM (RoPE at the pre-append position, like the
// non-batched transformer the TTS worker builds: srv/tts.rs:345), text-token rule, then the DepFormer — num_slices
// sequential passes of one shared transformer whose KV sequence is the slice axis (core/lm.rs:640-684).  The per-slot
// delayed-streams bookkeeping (core/tts_streaming.rs:117-242) is integer work on the host, one upload and one
// download per step.  The engine is a DsmDevice (dsm_device.h) plus the TTS model: it shares the context type, the loaders,
// transformer_forward and the Mimi decoder with the STT engine, and none of that engine's state.  With a Mimi attached
// (dsm_tts_attach_mimi) dsm_tts_step_pcm also decodes the frame each step completes, on the context's second stream (the
// audio_processing_loop of srv/tts.rs:528-544): the frame is assembled on the device (tts_frame_kernel) and the decode of
// step n overlaps the LM of step n + 1.

namespace {

struct DepW {
  Linear in_all;                       // depformer_in.{0..G-1} stacked [G*D][d]: one GEMM per step instead of one per slice (r03)
  std::vector<float*> emb;             // [S] full tables [vocab][D] f32 (low-rank product folded in at load)
  std::vector<Linear> out;             // [S] linears.{k}
  std::vector<TransformerW> tr;        // [G] shared attention/norm weights, per-group gating
};

// SpeakerEncoder (core/tts_streaming.rs:335-417) on the attached Mimi: weights, tables and the whole-clip scratch of
// dsm_speaker.inc.  None of it is shared with the step or the decode side.
struct SpkEnc {
  bool ready = false;
  int n_speakers = 0, cond_dim = 0;
  int max_r = 0;     // longest clip in Mimi frames: transformer.context / frames per step at the encoder rate
  int pos_rows = 0;  // rows of the position table
  Linear proj;       // output_proj [cond_dim][dimension] f32
  float *pad = nullptr, *pos = nullptr;  // learnt_padding [cond_dim], pos_emb [pos_rows][cond_dim]
  float *pcm = nullptr, *stdev = nullptr;  // [n_speakers][clip], [n_speakers]
  SeanetEnc enc;                           // cat_init [n_speakers][S0 + clip]; everything behind it holds one clip
  ActScratch act;                          // [n_speakers * T] rows; q is not used (no ring): the projection lands in qkv
  float *qkv = nullptr, *rope_cs = nullptr;  // [n_speakers * T][3 d], [T][head_dim]
  float *cat_ds = nullptr, *latent = nullptr, *rows = nullptr;
  float *h_stdev = nullptr, *h_rows = nullptr;  // pinned
  hipEvent_t ev_a = nullptr, ev_b = nullptr;    // device time of the last encode
  size_t scratch_bytes = 0;
  int last_c = 0, last_r = 0;  // shape of the last encode ("spk.*" taps)
  float last_ms = 0.0f;
};

// ConditionProvider (core/conditioner.rs:119-176) once dsm_tts_attach_conditioners has loaded it (dsm_tts_cond.inc).  Every tensor
// is kept as f32 (the upcast of a BF16 checkpoint is exact).
struct TtsCond {
  struct One {
    std::string name;
    int type = 0, dim = 0;
    std::vector<std::string> values;  // LUT: value -> its position
    float scale_factor = 0.0f, max_period = 0.0f;
    float *embed = nullptr, *proj = nullptr, *pad = nullptr;  // [n_bins + 1][dim] (LUT), [d_model][dim], [d_model]
  };
  std::vector<One> list;
  float* d_in = nullptr;  // [largest dim] staging of a continuous conditioner's sin embedding
};

}  // namespace

struct dsm_tts : DsmDevice {
  dsm_tts_config cfg{};
  int B = 0;
  // batch rows: a slot owns rps consecutive rows of every activation and cache (2 with cfg_rows: the conditional and the
  // unconditional row of classifier-free guidance, core/tts_streaming.rs:122); R = B * rps
  int rps = 1, R = 0;
  LmW lm;
  DepW dep;
  // device state
  ActScratch act, dact;  // main LM, depformer
  float *hidden = nullptr, *logits = nullptr, *dproj = nullptr, *dlogits = nullptr;
  int32_t *d_tokens = nullptr, *d_allowed = nullptr;
  uint8_t *d_mask = nullptr, *d_force_eop = nullptr, *d_run = nullptr, *d_forced = nullptr;  // per slot
  uint8_t *d_rmask = nullptr, *d_rrun = nullptr, *d_ca_act = nullptr;                        // per batch row
  // cross attention + guidance (r03): per-row projected sources, per-slot guidance
  CaState ca;                         // full-batch view (groups take row-offset copies)
  float *ca_src_dev = nullptr, *ca_kv_tmp = nullptr;  // staging of dsm_tts_set_ca_src: [smax][ca_dim], [smax][2d]
  std::vector<int> ca_len;            // [R] host mirror: rows of the batch row's source (0 = None), private or a voice's
  // Voices (dsm_tts_voice.inc): a source projected once into device memory of its own, [layer][K, V][H][smax][hd] in the cache
  // dtype, that any number of batch rows read by reference.  ca_src_tab [layer][R] (ca.src[l] points into it) is what every
  // cross-attention launch — captured or not — reads a row's K / V base from: the row's private block from create on, a
  // voice's while the row is attached.
  struct Voice {
    int handle = 0, rows = 0, refs = 0;  // refs: batch rows whose table entries point here
    uint8_t* mem = nullptr;
    size_t bytes = 0;
  };
  std::vector<Voice> voices;
  int next_voice = 1;                 // handles count up and are never reused
  std::vector<int> row_voice;         // [R] the voice a batch row reads (0: its private block)
  AttnRowSrc* ca_src_tab = nullptr;
  std::vector<AttnRowSrc> src_stage;  // [rps][layers] host side of a slot's table uploads (kept here: the copies are asynchronous)
  std::vector<uint8_t> cfg_on;        // [B]
  uint8_t* d_cfg_on = nullptr;
  float *d_cfg_fa = nullptr, *d_cfg_fb = nullptr, *mixed = nullptr, *dmixed = nullptr;  // [B], [B], [B][Vt], [B][V]
  uint32_t *d_text_token = nullptr, *d_last = nullptr, *d_lat = nullptr;
  // per-slot LogitsProcessor state (dsm_sampling.h): top_k (0 = ArgMax), 1/temperature, ChaCha key, words drawn by text_lp / audio_lp
  int32_t* d_samp_k = nullptr;
  float* d_samp_invt = nullptr;
  uint32_t *d_rng_key = nullptr, *d_rng_pos_text = nullptr, *d_rng_pos_audio = nullptr;
  std::vector<int> samp_k;  // host mirror: is any slot sampling? (selects the kernels' LDS size and the graph variant)
  TransformerState tr, dtr;
  // Stream groups (r03): slots [b0, b0 + nb) of group g run their whole step — main LM, text token, the 32 depformer slices —
  // on their own HIP stream with their own split-K workspace and their own hipGraph.  The step is a chain of ~1 400 dependent
  // launches of a few microseconds each (launch ramp + one L2 round trip + a sliver of MFMA work on a corner of the chip), and
  // slots never interact, so two chains side by side serve twice the slots in the time of one: the depformer's weights are
  // re-read per group, but they are L2 / Infinity-Cache resident (25 MB per slice).  DSM_TTS_GROUPS overrides (1..4).
  struct Grp {
    int b0 = 0, nb = 0;        // slots
    TransformerState tr, dtr;  // views with every per-row pointer advanced to row b0 * rps
    CaState ca;
  };
  std::vector<Grp> groups;
  GraphSlot* g_ttsg[kMaxGroups][2] = {};  // per group: the step without / with the depformer
  // pinned staging
  int32_t *h_tokens = nullptr, *h_allowed = nullptr;
  uint8_t* h_flags = nullptr;  // [4][B]: mask, force_eop, run, forced; [3][R] row flags; then (4-byte aligned) step_idx [B] i32, frame buffer u8
  uint32_t *h_text_token = nullptr, *h_lat = nullptr;
  // tts_streaming::State per slot
  struct Item {
    size_t step_idx = 0, consecutive_pads = 0;
    std::vector<uint32_t> audio_tokens, text_tokens;
  };
  std::vector<Item> items;
  size_t n_steps = 0;
  // ---- generated frames -> PCM (dsm_tts_attach_mimi / dsm_tts_step_pcm) ----
  // tts_frame_kernel ends every group's step body: it keeps the last acoustic_delay + 1 codebook-0 samples of every slot and
  // writes the decoder's codes / mask of frame buffer *d_fsel.  Buffers 0 and 1 alternate between consecutive step_pcm calls (the
  // decode of the previous step may still read the other one); buffer 2 takes the frames of token-only dsm_tts_step calls.
  size_t flags_bytes = 0, step_off = 0;  // the per-step upload: size, offset of the step indices (the buffer byte follows them)
  int32_t* d_step = nullptr;
  uint8_t* d_fsel = nullptr;
  uint32_t *d_ring = nullptr, *d_row0 = nullptr, *d_fcodes = nullptr;  // [B][ad + 1], [B][S], [kFrameBufs][B][S]
  uint8_t* d_fvalid = nullptr;                                          // [kFrameBufs][B]
  bool mimi = false;  // mimi_w and dec are loaded: dsm_tts_step_pcm is available
  MimiW mimi_w;
  MimiDecState dec;
  hipEvent_t ev_frames = nullptr;
  struct PcmEntry {  // one deferred step: its PCM / valid land in pinned memory behind `ev`
    hipEvent_t ev = nullptr;
    float* h_pcm = nullptr;     // [B][DSM_FRAME_SIZE]
    uint8_t* h_valid = nullptr; // [B]
    bool launched = false;      // false: no slot could emit, nothing was enqueued, valid is all zero
    // egress (dsm_egress.inc): with the section on the entry receives raw rows in the place of h_pcm
    uint8_t* h_raw = nullptr;   // [B][DSM_PCM_MAX_FRAME_BYTES] pinned, allocated by the first dsm_tts_set_egress(1)
    size_t raw_pitch = 0;       // the pitch the rows of this entry were written and downloaded at
    std::vector<uint32_t> fb;   // [B] every slot's frame_bytes when the entry was enqueued
  };
  PcmEntry pcm_q[2];
  uint64_t pcm_seq = 0;  // step_pcm calls so far: entry / frame buffer of call n is n & 1
  int pcm_pending = 0;   // entries queued and not yet delivered (the oldest is (pcm_seq - pcm_pending) & 1)
  SpkEnc spk;            // voice clips -> cross-attention rows (dsm_tts_attach_speaker_encoder, dsm_speaker.inc)
  // ---- per-slot Condition::AddToInput (dsm_tts_cond.inc) ----
  // Allocated at create and never moved: tts_input_kernel of every captured step body reads these two, so a condition set after
  // capture is seen on replay.  lm_in [R][d_model] keeps the rows that kernel wrote ("lm.input").
  TtsCond cond;
  float *d_cond = nullptr, *lm_in = nullptr;  // [B][d_model] f32, zero where no condition is set
  uint8_t* d_cond_on = nullptr;               // [B]
  std::vector<uint8_t> cond_on;               // host mirror
  // ---- a request's text schedule on the device, K steps per visit (dsm_tts_request.inc) ----
  // Frames of a block: every step of a block fills a frame buffer and a pinned PCM entry of its own (buffers 3 .. 3 +
  // DSM_TTS_RUN_MAX - 1 of d_fcodes / d_fvalid, blk_pcm[s]) — no event wait holds the model stream back for the decode stream.
  static constexpr int kFrameBufs = 3 + DSM_TTS_RUN_MAX;
  TtsReqState *d_req = nullptr, *h_req = nullptr;  // [B]; the pinned copy is what the last collect read
  int qcap = 0;                                    // tokens, and words, a request's queue holds: n_steps
  uint32_t *d_qtok = nullptr, *h_qtok = nullptr;   // [B][qcap]; the pinned mirror is append-only per request (uploads read it later)
  int32_t *d_qend = nullptr, *h_qend = nullptr;    // [B][qcap]
  struct ReqHost {
    bool active = false, closed = false;
    int n_words = 0, n_tok = 0;
    int status = 0;  // DSM_TTS_REQ_* as of the last collect
    bool bos_done = false;  // the request has received its first word (inserted_bos, srv/tts.rs:486-489)
  };
  std::vector<ReqHost> reqs;
  std::unique_ptr<dsm_spm> tok;                    // dsm_tts_attach_tokenizer: text in (push_text), text out (word_text); host only
  int rec_ld = 0;                                  // TTS_REC_HDR + S
  int32_t *d_blk = nullptr, *h_blk = nullptr;      // [DSM_TTS_RUN_MAX][B][rec_ld] the block's records
  uint8_t *d_ca_has = nullptr, *h_ca_has = nullptr;  // [R] ca_len > 0, uploaded per block
  PcmEntry blk_pcm[DSM_TTS_RUN_MAX];
  int blk_pending = 0;    // steps of the block that waits for dsm_tts_collect (0: none)
  bool blk_decode = false;
  // ---- egress (dsm_tts_set_egress; dsm_pcm_format.h, dsm_egress.inc): a sample rate and a sample format per slot ----
  // What egress_resample_kernel reads: the slots' formats (PcmFormatTable, dsm_pcm_table.inc: descriptors, coefficient arena, each
  // slot's descriptor index, with their host mirrors), the history [B][204] and the "started" words [B]; what it writes: the
  // staging rows [B][15360], at egress_pitch — the largest frame_bytes of any slot, rounded up to 16 — which is also what a step
  // downloads.  All of it allocated by the first dsm_tts_set_egress(1), with a pinned raw buffer beside every PcmEntry, after
  // which egress_fmt.ready holds.
  bool egress_on = false;
  PcmFormatTable egress_fmt{DSM_PCM_OUT};
  float *egress_hist = nullptr, *egress_dbg_pcm = nullptr;
  uint32_t* egress_started = nullptr;
  uint8_t *egress_raw_d = nullptr, *egress_dbg_valid = nullptr;
  size_t egress_pitch = sizeof(float) * DSM_FRAME_SIZE;
};

namespace {

int tts_create_impl(dsm_tts* t, const dsm_tts_config* cfg, int device_id, int batch_size, const char* lm_path) {
  DsmDevice* e = t;
  t->cfg = *cfg;
  t->B = batch_size;
  const dsm_tts_config& c = t->cfg;
  const int B = batch_size, d = c.lm.d_model, D = c.depformer.d_model, S = c.dep_num_slices, G = c.dep_weight_groups;
  if (B <= 0) { e->set_error("batch_size must be positive"); return DSM_ERR_INVALID; }
  if (S <= 0 || G <= 0 || G > S || c.audio_codebooks > 64 || c.audio_codebooks < 1) {
    e->set_error("depformer slices/groups or audio_codebooks out of range");
    return DSM_ERR_INVALID;
  }
  if (c.depformer.context < S) { e->set_error("depformer context (%d) must cover num_slices (%d)", c.depformer.context, S); return DSM_ERR_INVALID; }
  if (c.depformer.positional_embedding != 0 || !c.depformer.gating || !c.lm.gating || c.lm.norm != 1 || c.depformer.norm != 1) {
    e->set_error("TTS path expects gated RMS-norm transformers and a depformer without positional embedding");
    return DSM_ERR_INVALID;
  }
  for (const dsm_transformer_config* tc : {&c.lm, &c.depformer})
    if (int rc = check_transformer_config(e, *tc)) return rc;
  if (c.acoustic_delay < 0 || c.text_audio_delay_in_tokens < 0) { e->set_error("negative delay"); return DSM_ERR_INVALID; }
  if (c.dep_low_rank % 4) { e->set_error("low_rank_embeddings must be a multiple of 4"); return DSM_ERR_INVALID; }
  if (c.cross_attention && (c.ca_max_len <= 0 || c.ca_dim < 0 || (c.ca_dim % 4) != 0)) {
    e->set_error("cross_attention needs ca_max_len > 0 and a ca_dim that is a multiple of 4 (0 = d_model)");
    return DSM_ERR_INVALID;
  }
  // the source length is the "ring" of the cross-attention launch: its scores live in LDS (4 (ca_max_len + 4 hd + 16) bytes)
  if (c.cross_attention && c.ca_max_len > 8192) { e->set_error("ca_max_len %d: at most 8192 (attention scores are staged in LDS)", c.ca_max_len); return DSM_ERR_INVALID; }
  if (c.cfg_rows && !c.cross_attention) { e->set_error("cfg_rows needs cross_attention (guidance contrasts two sources)"); return DSM_ERR_INVALID; }
  t->rps = c.cfg_rows ? 2 : 1;
  t->R = B * t->rps;
  if (c.dot_mode != 0 && c.dot_mode != 1) { e->set_error("dot_mode must be 0 or 1"); return DSM_ERR_INVALID; }
  if (int rc = e->open(device_id, c.dot_mode, false)) return rc;
  hipStream_t st = e->s_model;
  char err[512];
  dsm_st_file* f = dsm_st_open(lm_path, err, sizeof err);
  if (!f) { e->set_error("%s", err); return DSM_ERR_IO; }
  Loader ld{e, f};
  int rc = 0;
  do {
    if ((rc = load_lm_trunk(e, ld, &t->lm, c))) break;
    t->lm.tr.rope_pos_before = true;
    // a checkpoint with cross-attention tensors must not be run without them (ADVICE r03: the layers would be skipped silently)
    if (!c.cross_attention && (ld.has("transformer.layers.0.cross_attention.out_proj.weight") || ld.has("transformer.layers.0.norm_cross.weight") ||
                               ld.has("transformer.layers.0.norm_cross.alpha"))) {
      e->set_error("the checkpoint carries transformer.layers.N.cross_attention.* / norm_cross.* tensors but cfg.cross_attention is 0");
      rc = DSM_ERR_INVALID;
      break;
    }
    if (c.cross_attention) {  // StreamingMultiheadCrossAttention::new + norm_cross — core/transformer.rs:219-290,735-738
      const int kvd = c.ca_dim > 0 ? c.ca_dim : d;
      t->lm.tr.has_ca = true;
      t->lm.tr.ca_norm_rms = c.ca_norm == 1 ? 1 : 0;
      for (int l = 0; l < c.lm.num_layers && !rc; ++l) {
        TLayerW& L = t->lm.tr.layers[l];
        std::vector<float> wq, wkv;
        if (ld.has("transformer.layers.%d.cross_attention.in_proj_weight", l)) {  // "Case 1": rows q | k | v of one tensor
          if (kvd != d) { e->set_error("the single cross_attention.in_proj_weight layout needs ca_dim == d_model"); rc = DSM_ERR_INVALID; break; }
          auto w = ld.get((int64_t)3 * d * d, "transformer.layers.%d.cross_attention.in_proj_weight", l);
          wq.assign(w.begin(), w.begin() + (size_t)d * d);
          wkv.assign(w.begin() + (size_t)d * d, w.end());
        } else {
          wq = ld.get((int64_t)d * d, "transformer.layers.%d.cross_attention.in_proj_weight_q", l);
          wkv = ld.get((int64_t)2 * d * kvd, "transformer.layers.%d.cross_attention.in_proj_weight_kv", l);
        }
        auto wo = ld.get((int64_t)d * d, "transformer.layers.%d.cross_attention.out_proj.weight", l);
        std::vector<float> nw, nb;
        if (c.ca_norm == 1) {
          nw = ld.get(d, "transformer.layers.%d.norm_cross.alpha", l);
        } else {
          nb = ld.get(d, "transformer.layers.%d.norm_cross.bias", l);
          if (ld.has("transformer.layers.%d.norm_cross.alpha", l)) nw = ld.get(d, "transformer.layers.%d.norm_cross.alpha", l);
          else nw = ld.get(d, "transformer.layers.%d.norm_cross.weight", l);
        }
        if (ld.failed) { rc = DSM_ERR_IO; break; }
        if ((rc = pack_linear(e, &L.ca_q, wq.data(), d, d, true, nullptr))) break;
        if ((rc = pack_linear(e, &L.ca_kv, wkv.data(), 2 * d, kvd, true, nullptr))) break;
        if ((rc = pack_linear(e, &L.ca_out, wo.data(), d, d, true, nullptr))) break;
        if ((rc = e->upload(&L.ncw, nw.data(), nw.size()))) break;
        if (!nb.empty() && (rc = e->upload(&L.ncb, nb.data(), nb.size()))) break;
      }
      if (rc) break;
    }
    // ---- DepFormer ----
    DepW& w = t->dep;
    {  // the G input projections stacked row-wise (r03): depformer_in of every slice is a function of the main LM's output alone
      std::vector<float> all((size_t)G * D * d);
      for (int g = 0; g < G; ++g) {
        auto wi = ld.get((int64_t)D * d, "depformer_in.%d.weight", g);
        if (ld.failed) { rc = DSM_ERR_IO; break; }
        memcpy(all.data() + (size_t)g * D * d, wi.data(), sizeof(float) * (size_t)D * d);
      }
      if (!rc) rc = pack_linear(e, &w.in_all, all.data(), G * D, d, true, nullptr);
    }
    if (rc) break;
    w.out.resize(S);
    w.emb.assign(S, nullptr);
    const int lr = c.dep_low_rank;
    for (int k = 0; k < S && !rc; ++k) {
      auto wo = ld.get((int64_t)(c.audio_vocab_size - 1) * D, "linears.%d.weight", k);
      if (ld.failed) { rc = DSM_ERR_IO; break; }
      if ((rc = pack_linear(e, &w.out[k], wo.data(), c.audio_vocab_size - 1, D, true, nullptr))) break;
      const int vocab = k == 0 ? c.text_in_vocab_size : c.audio_vocab_size;
      char base[64];
      if (k == 0) snprintf(base, sizeof base, "depformer_text_emb");
      else snprintf(base, sizeof base, "depformer_emb.%d", k - 1);
      auto tab = ld.get((int64_t)vocab * (lr > 0 ? lr : D), "%s.weight", base);
      if (ld.failed) { rc = DSM_ERR_IO; break; }
      if (lr > 0) {  // fold LowRankEmbeddings' linear into the table: same GEMM, same summation order, run once
        auto lw = ld.get((int64_t)D * lr, "%s.low_rank.weight", base);
        if (ld.failed) { rc = DSM_ERR_IO; break; }
        Linear L;
        if ((rc = pack_linear(e, &L, lw.data(), D, lr, true, nullptr))) break;
        float* d_tab = nullptr;
        if ((rc = e->upload(&d_tab, tab.data(), tab.size()))) break;
        if ((rc = e->dalloc(&w.emb[k], (size_t)vocab * D))) break;
        GemmArgs a = base_args(L, d_tab, plain_map(vocab, lr), vocab);
        a.Y = w.emb[k]; a.ymap = plain_map(vocab, D);
        if ((rc = gemm_store<uint16_t>(e, st, a, lr % 32 == 0))) break;
      } else {
        if ((rc = e->upload(&w.emb[k], tab.data(), tab.size()))) break;
      }
    }
    if (rc) break;
    TransformerW base;
    dsm_transformer_config dc = c.depformer;
    base.cfg = dc;
    base.hidden = gating_hidden(dc);
    base.layers.resize(dc.num_layers);
    w.tr.assign(G, base);
    for (int l = 0; l < dc.num_layers && !rc; ++l) {
      TLayerW L;
      auto ip = ld.get((int64_t)3 * D * D, "depformer.layers.%d.self_attn.in_proj_weight", l);
      auto op = ld.get((int64_t)D * D, "depformer.layers.%d.self_attn.out_proj.weight", l);
      auto n1 = ld.get(D, "depformer.layers.%d.norm1.alpha", l);
      auto n2 = ld.get(D, "depformer.layers.%d.norm2.alpha", l);
      if (ld.failed) { rc = DSM_ERR_IO; break; }
      if ((rc = pack_linear(e, &L.in_proj, ip.data(), 3 * D, D, true, nullptr))) break;
      if ((rc = pack_linear(e, &L.out_proj, op.data(), D, D, true, nullptr))) break;
      if ((rc = e->upload(&L.n1w, n1.data(), n1.size()))) break;
      if ((rc = e->upload(&L.n2w, n2.data(), n2.size()))) break;
      for (int g = 0; g < G && !rc; ++g) {  // Mlp::new with gating_idx — core/transformer.rs:579-590
        TLayerW Lg = L;
        auto wi = ld.get((int64_t)2 * base.hidden * D, "depformer.layers.%d.gating.%d.linear_in.weight", l, g);
        auto wo = ld.get((int64_t)D * base.hidden, "depformer.layers.%d.gating.%d.linear_out.weight", l, g);
        if (ld.failed) { rc = DSM_ERR_IO; break; }
        if ((rc = pack_linear(e, &Lg.ff_in, wi.data(), 2 * base.hidden, D, true, nullptr, base.hidden))) break;
        if ((rc = pack_linear(e, &Lg.ff_out, wo.data(), D, base.hidden, true, nullptr))) break;
        w.tr[g].layers[l] = Lg;
      }
    }
  } while (0);
  dsm_st_close(f);
  if (rc) return rc;
  const int hid = gating_hidden(c.lm), dhid = gating_hidden(c.depformer), V = c.audio_vocab_size - 1;
  const int R = t->R, rps = t->rps;
  if ((rc = alloc_act(e, &t->act, R, d, hid))) return rc;
  if ((rc = e->dalloc(&t->hidden, (size_t)R * d))) return rc;
  if ((rc = e->dalloc(&t->logits, (size_t)R * c.text_out_vocab_size))) return rc;
  if ((rc = alloc_act(e, &t->dact, R, D, dhid))) return rc;
  if ((rc = e->dalloc(&t->dproj, (size_t)R * c.dep_weight_groups * D))) return rc;
  if ((rc = e->dalloc(&t->dlogits, (size_t)R * V))) return rc;
  if ((rc = e->dalloc(&t->d_tokens, (size_t)R * (1 + c.audio_codebooks)))) return rc;
  if ((rc = e->dalloc(&t->d_allowed, B))) return rc;
  // one upload per step: [mask | force_eop | run | forced] per slot, then [row mask | row run | row attends its source] per row
  t->step_off = ((size_t)4 * B + (size_t)3 * R + 3) & ~(size_t)3;
  t->flags_bytes = t->step_off + sizeof(int32_t) * (size_t)B + 4;
  if ((rc = e->dalloc(&t->d_mask, t->flags_bytes))) return rc;
  t->d_step = reinterpret_cast<int32_t*>(t->d_mask + t->step_off);
  t->d_fsel = t->d_mask + t->step_off + sizeof(int32_t) * (size_t)B;
  if ((rc = e->dalloc(&t->d_ring, (size_t)B * (c.acoustic_delay + 1)))) return rc;
  if ((rc = e->dalloc(&t->d_row0, (size_t)B * S))) return rc;
  if ((rc = e->dalloc(&t->d_fcodes, (size_t)dsm_tts::kFrameBufs * B * S))) return rc;
  if ((rc = e->dalloc(&t->d_fvalid, (size_t)dsm_tts::kFrameBufs * B))) return rc;
  t->d_force_eop = t->d_mask + B;
  t->d_run = t->d_mask + 2 * B;
  t->d_forced = t->d_mask + 3 * B;
  t->d_rmask = t->d_mask + 4 * B;
  t->d_rrun = t->d_rmask + R;
  t->d_ca_act = t->d_rrun + R;
  if ((rc = e->dalloc(&t->d_text_token, B))) return rc;
  if ((rc = e->dalloc(&t->d_last, B))) return rc;
  if ((rc = e->dalloc(&t->d_lat, (size_t)B * S))) return rc;
  if ((rc = e->dalloc(&t->d_samp_k, B))) return rc;
  if ((rc = e->dalloc(&t->d_samp_invt, B))) return rc;
  if ((rc = e->dalloc(&t->d_rng_key, (size_t)B * 8))) return rc;
  if ((rc = e->dalloc(&t->d_rng_pos_text, B))) return rc;
  if ((rc = e->dalloc(&t->d_rng_pos_audio, B))) return rc;
  t->samp_k.assign(B, 0);
  t->cfg_on.assign(B, 0);
  t->ca_len.assign(R, 0);
  if ((rc = e->dalloc(&t->d_cfg_on, B))) return rc;
  if ((rc = e->dalloc(&t->d_cfg_fa, B))) return rc;
  if ((rc = e->dalloc(&t->d_cfg_fb, B))) return rc;
  if (rps == 2) {
    if ((rc = e->dalloc(&t->mixed, (size_t)B * c.text_out_vocab_size))) return rc;
    if ((rc = e->dalloc(&t->dmixed, (size_t)B * V))) return rc;
  }
  if ((rc = alloc_transformer_state(e, &t->tr, c.lm, R, 1, c.kv_bf16 != 0))) return rc;
  if ((rc = alloc_transformer_state(e, &t->dtr, c.depformer, R, 1, false))) return rc;
  const size_t kv_elem = c.kv_bf16 ? 2 : 4;
  if (c.cross_attention) {  // per-row projected sources, [R][H][smax][hd] per layer in the cache dtype (zero = a defined "no source")
    const int smax = c.ca_max_len, kvd = c.ca_dim > 0 ? c.ca_dim : d;
    t->ca.smax = smax;
    t->ca.k.resize(c.lm.num_layers);
    t->ca.v.resize(c.lm.num_layers);
    for (int l = 0; l < c.lm.num_layers; ++l) {
      uint8_t *k = nullptr, *v = nullptr;
      if ((rc = e->dalloc(&k, (size_t)R * d * smax * kv_elem))) return rc;
      if ((rc = e->dalloc(&v, (size_t)R * d * smax * kv_elem))) return rc;
      t->ca.k[l] = k;
      t->ca.v[l] = v;
    }
    {  // every row starts on its private block (the identity table)
      const int L = c.lm.num_layers;
      const size_t blk = (size_t)d * smax * kv_elem;
      std::vector<AttnRowSrc> tab((size_t)L * R);
      for (int l = 0; l < L; ++l)
        for (int r = 0; r < R; ++r) {
          AttnRowSrc& s = tab[(size_t)l * R + r];
          s = AttnRowSrc{};
          s.k = (const uint8_t*)t->ca.k[l] + (size_t)r * blk;
          s.v = (const uint8_t*)t->ca.v[l] + (size_t)r * blk;
        }
      if ((rc = e->upload(&t->ca_src_tab, tab.data(), tab.size()))) return rc;
      t->ca.src.resize(L);
      for (int l = 0; l < L; ++l) t->ca.src[l] = t->ca_src_tab + (size_t)l * R;
      t->row_voice.assign(R, 0);
      t->src_stage.assign((size_t)rps * L, AttnRowSrc{});
    }
    if ((rc = e->dalloc(&t->ca.last, R))) return rc;
    if ((rc = e->dalloc(&t->ca.att, (size_t)R * d))) return rc;
    t->ca.act = t->d_ca_act;
    if ((rc = e->dalloc(&t->ca_src_dev, (size_t)smax * kvd))) return rc;
    if ((rc = e->dalloc(&t->ca_kv_tmp, (size_t)smax * 2 * d))) return rc;
  }
  {
    // Measured (r03, v202501 shapes): a step is as long as its chain of launches whatever the rows per launch, so groups buy
    // THROUGHPUT, not latency, and only once a launch has enough rows to be more than its floor — B = 32 as 1 / 2 groups:
    // 8.40 / 9.27 ms per step (three or four run as two rounds: 17.9 / 19.2 ms — the runtime kept two graphs in flight at a
    // time).  Default: one group below 96 slots, two from there on.
    int Gn = B >= 96 ? 2 : 1;  // measured (v202501, dot_mode 1): B = 32 8.4 vs 9.3 ms, 64 9.4 vs 10.1, 128 12.4 vs 11.7 (one vs two groups)
    Gn = dsm_env_int("DSM_TTS_GROUPS", Gn);
    if (Gn < 1) Gn = 1;
    if (Gn > DsmDevice::kMaxGroups) Gn = DsmDevice::kMaxGroups;
    if (Gn > B) Gn = B;
    t->groups.resize(Gn);
    int b0 = 0;
    for (int g = 0; g < Gn; ++g) {
      const int nb = B / Gn + (g < B % Gn ? 1 : 0);
      dsm_tts::Grp& grp = t->groups[g];
      grp.b0 = b0; grp.nb = nb;
      const int r0 = b0 * rps;
      grp.tr = group_view(t->tr, c.lm, kv_elem, r0);
      grp.dtr = group_view(t->dtr, c.depformer, 4, r0);
      if (c.cross_attention) grp.ca = group_view(t->ca, d, kv_elem, r0);
      b0 += nb;
      for (auto& gs : t->g_ttsg[g]) gs = e->graph_slot();
    }
    if ((rc = e->open_groups(Gn))) return rc;
  }
  if ((rc = e->halloc(&t->h_tokens, (size_t)R * (1 + c.audio_codebooks)))) return rc;
  if ((rc = e->halloc(&t->h_allowed, (size_t)B))) return rc;
  if ((rc = e->halloc(&t->h_flags, t->flags_bytes))) return rc;
  memset(t->h_flags, 0, t->flags_bytes);
  if ((rc = e->halloc(&t->h_text_token, (size_t)B))) return rc;
  if ((rc = e->halloc(&t->h_lat, (size_t)B * S))) return rc;
  t->n_steps = (size_t)c.max_steps + c.acoustic_delay;
  {  // the request loop's device state (dsm_tts_request.inc); zero = every slot IDLE
    t->qcap = (int)t->n_steps;
    t->rec_ld = TTS_REC_HDR + S;
    if ((rc = e->dalloc(&t->d_req, B))) return rc;
    if ((rc = e->halloc(&t->h_req, (size_t)B))) return rc;
    if ((rc = e->dalloc(&t->d_qtok, (size_t)B * t->qcap))) return rc;
    if ((rc = e->halloc(&t->h_qtok, (size_t)B * t->qcap))) return rc;
    if ((rc = e->dalloc(&t->d_qend, (size_t)B * t->qcap))) return rc;
    if ((rc = e->halloc(&t->h_qend, (size_t)B * t->qcap))) return rc;
    if ((rc = e->dalloc(&t->d_blk, (size_t)DSM_TTS_RUN_MAX * B * t->rec_ld))) return rc;
    if ((rc = e->halloc(&t->h_blk, (size_t)DSM_TTS_RUN_MAX * B * t->rec_ld))) return rc;
    if ((rc = e->dalloc(&t->d_ca_has, R))) return rc;
    if ((rc = e->halloc(&t->h_ca_has, (size_t)R))) return rc;
    t->reqs.assign(B, dsm_tts::ReqHost{});
  }
  // the conditioners' buffers (dsm_tts_cond.inc), behind every other allocation
  if ((rc = e->dalloc(&t->lm_in, (size_t)R * d))) return rc;
  if ((rc = e->dalloc(&t->d_cond, (size_t)B * d))) return rc;
  if ((rc = e->dalloc(&t->d_cond_on, B))) return rc;
  t->cond_on.assign(B, 0);
  t->items.resize(B);
  for (auto& it : t->items) {
    it.audio_tokens.assign(t->n_steps * S, DSM_TTS_UNGENERATED);
    it.text_tokens.assign(t->n_steps, DSM_TTS_UNGENERATED);
  }
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

bool tts_any_sampling(const dsm_tts* t) {
  for (int k : t->samp_k)
    if (k > 0) return true;
  return false;
}
int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
// dynamic LDS of the sampling kernels: the sort keys (u64 per padded vocabulary entry) + 9 floats; none when every slot is ArgMax
size_t sample_lds(const dsm_tts* t, int V) { return tts_any_sampling(t) ? (size_t)pow2_at_least(V) * 8 + 64 : 0; }
SampleArgs sample_args(const dsm_tts* t, int V, uint32_t* pos, int b0) {  // the per-slot arrays from slot b0 on
  SampleArgs sa;
  sa.top_k = tts_any_sampling(t) ? t->d_samp_k + b0 : nullptr;
  sa.inv_t = t->d_samp_invt + b0;
  sa.key = t->d_rng_key + (size_t)8 * b0;
  sa.pos = pos + b0;
  sa.vpad = pow2_at_least(V);
  return sa;
}

// DepFormer::sample — core/lm.rs:640-684 for the slots of one stream group, all slices enqueued back to back, tokens stay on
// the device
int tts_depformer(dsm_tts* t, hipStream_t st, dsm_tts::Grp& grp) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int d = c.lm.d_model, D = c.depformer.d_model, S = c.dep_num_slices, G = c.dep_weight_groups;
  const int V = c.audio_vocab_size - 1, dhid = gating_hidden(c.depformer);
  const int rps = t->rps, b0 = grp.b0, nslots = grp.nb, r0 = b0 * rps, B = nslots * rps;  // B: batch rows of this group from here on
  const ActScratch da = t->dact.from_row(r0, D, dhid);
  float* dlogits = t->dlogits + (size_t)r0 * V;
  const float* hidden = t->hidden + (size_t)r0 * d;
  // depformer_in.{g}(hidden) for every weight group in one GEMM (r03): the projection of slice k does not depend on the
  // tokens sampled before it, only its embedding does — 32 x (GEMM + reduce) per step become one pair
  float* dproj = t->dproj + (size_t)r0 * G * D;
  {
    GemmArgs a = base_args(t->dep.in_all, hidden, plain_map(B, d), B);
    a.Y = dproj; a.ymap = plain_map(B, G * D);
    if (int rc = gemm_store<uint16_t>(e, st, a)) return rc;
  }
  // slice 0 resets the KV state, slice k continues slice k-1's (:650-657): one sequence over the slice axis
  HIPCHK(hipMemsetAsync(grp.dtr.pos, 0, sizeof(uint32_t) * B, st));
  HIPCHK(hipMemsetAsync(grp.dtr.idx, 0, sizeof(uint32_t) * B, st));
  const dsm_transformer_config& dc = c.depformer;  // RMS-norm, gated, no positional embedding (checked at create)
  // the head of slice k: emb_k(token) + projection, the ring bookkeeping of the new position, norm1 of layer 0.  Slice 0's is
  // a launch of its own (dep_head_kernel); every later one runs in the tail of the previous slice's sampler launch (r04)
  auto head_args = [&](int k) {
    const int g = (k * G) / S;
    const TransformerW& tw = t->dep.tr[g];
    DepHeadArgs h;
    h.x = da.x; h.xn = da.xn; h.table = t->dep.emb[k];
    h.vocab = k == 0 ? c.text_in_vocab_size : c.audio_vocab_size;
    h.D = D; h.rps = rps;
    h.proj = dproj + (size_t)g * D; h.proj_ld = (long)G * D;
    h.pos = grp.dtr.pos; h.idx = grp.dtr.idx; h.active = t->d_rrun + r0;
    h.start_pos = grp.dtr.start_pos; h.widx = grp.dtr.widx;
    h.ctx = dc.context; h.nw = tw.layers[0].n1w; h.nb = tw.layers[0].n1b;
    h.eps = norm_eps(dc.norm); h.rms = dc.norm;
    return h;
  };
  for (int k = 0; k < S; ++k) {
    const int g = (k * G) / S;
    const TransformerW& tw = t->dep.tr[g];
    if (k == 0) {
      hipLaunchKernelGGL(dep_head_kernel, dim3(B), dim3(256), 0, st, head_args(0), t->d_last + b0);
      HIPCHK(hipGetLastError());
    }
    if (int rc = transformer_forward<uint16_t, float>(e, st, tw, grp.dtr, da, B, 1, t->d_rrun + r0, nullptr, plain_map(1, 1), nullptr,
                                                      nullptr, 0, nullptr, /*head_done=*/true))
      return rc;
    LogitSrc src{};
    {
      GemmArgs a = base_args(t->dep.out[k], da.x, plain_map(B, D), B);
      a.Y = dlogits; a.ymap = plain_map(B, V);
      // slabs left by the plan go to the sampler launch (one launch less per slice)
      Slabs sl;
      if (int rc = gemm_store<uint16_t>(e, st, a, true, &sl)) return rc;
      if (sl.ws) {
        src.ws = sl.ws; src.ld = sl.ld; src.cstride = sl.cstride; src.chunks = sl.chunks;
        src.store = dlogits;
      } else {
        src.rows = dlogits;
      }
    }
    // DepFormer::sample / sample_cfg (core/lm.rs:640-684,718-721): with two rows per slot the sampler mixes l0 * a - l1 * (a - 1)
    src.rps = rps;
    src.cfg_on = t->d_cfg_on + b0; src.fa = t->d_cfg_fa + b0; src.fb = t->d_cfg_fb + b0;
    const size_t row_off = (sample_lds(t, V) + 15) & ~(size_t)15;
    DepHeadArgs next{};
    if (k + 1 < S) next = head_args(k + 1);
    hipLaunchKernelGGL(dep_argmax_kernel, dim3(nslots), dim3(256), row_off + sizeof(float) * V, st, src, V, k, S,
                       t->d_lat + (size_t)b0 * S, t->d_last + b0, t->d_run + b0, t->d_forced + b0,
                       (uint32_t)c.audio_vocab_size - 1, sample_args(t, V, t->d_rng_pos_audio, b0), (int)row_off, next);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// The device side of State::step for one stream group: input embedding sum, main LM, text-token rule, depformer.
int tts_group_body(dsm_tts* t, hipStream_t st, dsm_tts::Grp& grp, bool run_dep) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int d = c.lm.d_model, nc = c.audio_codebooks, hid = gating_hidden(c.lm), Vt = c.text_out_vocab_size;
  const int rps = t->rps, b0 = grp.b0, nslots = grp.nb, r0 = b0 * rps, B = nslots * rps, sid = e->sid(st);  // B: batch rows of the group
  const ActScratch sc = t->act.from_row(r0, d, hid);
  float *hidden = t->hidden + (size_t)r0 * d, *logits = t->logits + (size_t)r0 * Vt;
  const CaState* ca = c.cross_attention ? &grp.ca : nullptr;
  e->tag_gemm[sid] = DSM_PROF_GEMM_LM;
  e->tag_attn[sid] = DSM_PROF_ATTN_LM;
  hipLaunchKernelGGL(tts_input_kernel, dim3(B, (d + 511) / 512), dim3(256), 0, st, sc.x, t->lm_in + (size_t)r0 * d, t->lm.text_emb,
                     t->lm.audio_emb, t->d_tokens + (size_t)r0 * (1 + nc), nc, d, c.audio_vocab_size, t->d_cond, t->d_cond_on, r0, rps);
  HIPCHK(hipGetLastError());
  int rc = with_kv_type(c.kv_bf16 != 0, [&](auto kv) {  // forward_cond, or forward_ca for rows that carry a source (core/lm.rs:957-1067)
    return transformer_forward<uint16_t, decltype(kv)>(e, st, t->lm.tr, grp.tr, sc, B, 1, t->d_rmask + r0, nullptr, plain_map(1, 1),
                                                       t->lm.out_norm, hidden, 0, ca);
  });
  if (rc) return rc;
  {
    GemmArgs a = base_args(t->lm.text_linear, hidden, plain_map(B, d), B);
    a.Y = logits; a.ymap = plain_map(B, Vt);
    if ((rc = gemm_store<uint16_t>(e, st, a))) return rc;
  }
  const float* slot_logits = logits;
  if (rps == 2) {  // text logits of a guided slot: l0 * a - l1 * (a - 1) — core/tts_streaming.rs:164-173
    float* mx = t->mixed + (size_t)b0 * Vt;
    hipLaunchKernelGGL(cfg_mix_kernel, dim3((Vt + 255) / 256, nslots), dim3(256), 0, st, mx, logits, Vt, t->d_cfg_on + b0,
                       t->d_cfg_fa + b0, t->d_cfg_fb + b0);
    slot_logits = mx;
  }
  hipLaunchKernelGGL(tts_text_token_kernel, dim3(nslots), dim3(256), sample_lds(t, Vt), st, slot_logits, Vt, t->d_allowed + b0,
                     t->d_force_eop + b0, (uint32_t)c.text_pad_token, (uint32_t)c.text_eop_token, t->d_text_token + b0,
                     t->d_last + b0, sample_args(t, Vt, t->d_rng_pos_text, b0), t->d_mask + b0);
  HIPCHK(hipGetLastError());
  e->tag_gemm[sid] = DSM_PROF_OTHER;
  e->tag_attn[sid] = DSM_PROF_OTHER;
  if (run_dep)
    if ((rc = tts_depformer(t, st, grp))) return rc;
  {  // the frame this step completes, for the decoder (behind the last sampler launch)
    const int S = c.dep_num_slices;
    TtsFrameArgs fa;
    fa.lat = t->d_lat + (size_t)b0 * S; fa.mask = t->d_mask + b0; fa.run = t->d_run + b0; fa.step = t->d_step + b0;
    fa.sel = t->d_fsel;
    fa.ring = t->d_ring + (size_t)b0 * (c.acoustic_delay + 1); fa.row0 = t->d_row0 + (size_t)b0 * S;
    fa.codes = t->d_fcodes + (size_t)b0 * S; fa.valid = t->d_fvalid + b0;
    fa.codes_stride = (long)t->B * S; fa.valid_stride = t->B;
    fa.nslots = nslots; fa.S = S; fa.ad = c.acoustic_delay; fa.tad = c.text_audio_delay_in_tokens;
    fa.pad = (uint32_t)c.audio_vocab_size - 1;
    hipLaunchKernelGGL(tts_frame_kernel, dim3((nslots + 63) / 64), dim3(64), 0, st, fa);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int egress_enqueue(dsm_tts* t, hipStream_t sd, dsm_tts::PcmEntry& en);  // dsm_egress.inc

// Mimi::decode_step of the frames buffer `sel` holds, on the decode stream behind the step's groups; PCM and valid flags go
// to the entry's pinned buffers, its event closes the sequence.
int tts_enqueue_decode(dsm_tts* t, int sel, dsm_tts::PcmEntry& en) {
  DsmDevice* e = t;
  const int B = t->B, S = t->cfg.dep_num_slices;
  hipStream_t sd = e->s_enc;
  MimiDecState& d = t->dec;
  HIPCHK(hipEventRecord(t->ev_frames, e->s_model));  // the model stream has joined every group
  HIPCHK(hipStreamWaitEvent(sd, t->ev_frames, 0));
  HIPCHK(hipMemcpyAsync(d.codes, t->d_fcodes + (size_t)sel * B * S, sizeof(uint32_t) * (size_t)B * S, hipMemcpyDeviceToDevice, sd));
  HIPCHK(hipMemcpyAsync(d.mask, t->d_fvalid + (size_t)sel * B, (size_t)B, hipMemcpyDeviceToDevice, sd));
  if (int rc = mimi_decode(e, t->mimi_w, d, B, sd)) return rc;
  if (t->egress_on) {  // the raw rows in the place of the f32 frames
    if (int rc = egress_enqueue(t, sd, en)) return rc;
  } else {
    HIPCHK(hipMemcpyAsync(en.h_pcm, d.pcm, sizeof(float) * (size_t)B * DSM_FRAME_SIZE, hipMemcpyDeviceToHost, sd));
  }
  HIPCHK(hipMemcpyAsync(en.h_valid, d.mask, (size_t)B, hipMemcpyDeviceToHost, sd));
  HIPCHK(hipEventRecord(en.ev, sd));
  en.launched = true;
  return 0;
}

// the oldest pending entry: wait for it, hand it out
int tts_deliver_pcm(dsm_tts* t, float* pcm_out, uint8_t* pcm_valid_out) {
  DsmDevice* e = t;
  dsm_tts::PcmEntry& en = t->pcm_q[(t->pcm_seq - (uint64_t)t->pcm_pending) & 1];
  if (en.launched) HIPCHK(hipEventSynchronize(en.ev));
  for (int b = 0; b < t->B; ++b) {
    const bool v = en.launched && en.h_valid[b];
    if (pcm_valid_out) pcm_valid_out[b] = v ? 1 : 0;
    if (pcm_out && v) memcpy(pcm_out + (size_t)b * DSM_FRAME_SIZE, en.h_pcm + (size_t)b * DSM_FRAME_SIZE, sizeof(float) * DSM_FRAME_SIZE);
  }
  t->pcm_pending -= 1;
  return 0;
}

}  // namespace

namespace {
int spk_debug_read(dsm_tts* t, const char* name, float* out, size_t cap);  // dsm_speaker.inc
int tts_request_end(dsm_tts* t, int slot);                                  // dsm_tts_request.inc
}

extern "C" {

void dsm_tts_config_v202501(dsm_tts_config* out) { dsm_preset_tts_v202501(out); }

const char* dsm_tts_last_error(const dsm_tts* t) { return t ? t->err.c_str() : g_create_error.c_str(); }

void dsm_tts_destroy(dsm_tts* t) { delete t; }  // ~DsmDevice releases what the engine was handed

int dsm_tts_create(const dsm_tts_config* cfg, int device_id, int batch_size, const char* lm_safetensors, dsm_tts** out) {
  if (!cfg || !out || !lm_safetensors) {
    g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  dsm_tts* t = new dsm_tts();
  return finish_create(t, tts_create_impl(t, cfg, device_id, batch_size, lm_safetensors), out);
}

}  // extern "C" (reopened below)

namespace {
// State::step.  decode: also queue the decode of the frame the step completes as the next entry of the PCM queue (the caller
// checked that the entry is free); otherwise the frame goes to the spare buffer and is dropped.
int tts_step_impl(dsm_tts* t, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                  uint32_t* text_token_out, uint32_t* audio_out, bool decode) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int B = t->B, S = c.dep_num_slices, nc = c.audio_codebooks;
  const uint32_t pad = (uint32_t)c.audio_vocab_size - 1, UNG = DSM_TTS_UNGENERATED;
  hipStream_t st = e->s_model;
  // the request loop (dsm_tts_request.inc) owns the step's device buffers while a block waits, and its slots' state always
  if (t->blk_pending) { e->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  for (int b = 0; b < B; ++b)
    if (mask[b] && t->reqs[b].active) { e->set_error("slot %d has a request: dsm_tts_run steps it", b); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  const int rps = t->rps, R = t->R;
  uint8_t *h_mask = t->h_flags, *h_force = t->h_flags + B, *h_run = t->h_flags + 2 * B, *h_forced = t->h_flags + 3 * B;
  uint8_t *h_rmask = t->h_flags + 4 * B, *h_rrun = h_rmask + R, *h_ca_act = h_rrun + R;
  int32_t* h_step = reinterpret_cast<int32_t*>(t->h_flags + t->step_off);
  const int fsel = decode ? (int)(t->pcm_seq & 1) : 2;
  t->h_flags[t->step_off + sizeof(int32_t) * (size_t)B] = (uint8_t)fsel;
  // A slot whose previous step returned "max step-idx reached" has step_idx == n_steps: the reference's next
  // `self.text_tokens[self.step_idx]` (core/tts_streaming.rs:199) is an out-of-bounds panic.  Here: refuse the whole
  // step before anything is touched, the caller resets the slot (or masks it out).
  for (int b = 0; b < B; ++b)
    if (mask[b] && t->items[b].step_idx >= t->n_steps) {
      e->set_error("slot %d: max step-idx reached (step_idx %zu of %zu): reset the slot", b, t->items[b].step_idx, t->n_steps);
      return DSM_ERR_STATE;
    }
  for (int b = 0; b < B; ++b) {  // input assembly — core/tts_streaming.rs:126-158
    const dsm_tts::Item& it = t->items[b];
    const size_t step = it.step_idx;
    int32_t* tk = t->h_tokens + (size_t)b * rps * (1 + nc);
    tk[0] = prev_text_token[b] < (uint32_t)c.text_in_vocab_size ? (int32_t)prev_text_token[b] : 0;
    for (int cb = 0; cb < nc; ++cb) tk[1 + cb] = -1;
    h_mask[b] = mask[b] ? 1 : 0;
    t->h_allowed[b] = allowed[b];
    h_force[b] = it.consecutive_pads > (size_t)c.max_consecutive_pads;
    h_run[b] = mask[b] && step >= (size_t)c.text_audio_delay_in_tokens;  // :203-205
    h_forced[b] = step < (size_t)c.acoustic_delay;
    h_step[b] = (int32_t)step;
    for (int j = 0; j < rps; ++j) {  // batch_size = if cfg_alpha.is_some() { 2 } else { 1 } — :122: the second row only runs when the slot is guided
      const int r = b * rps + j;
      h_rmask[r] = h_mask[b] && (j == 0 || t->cfg_on[b]);
      h_rrun[r] = h_run[b] && (j == 0 || t->cfg_on[b]);
      h_ca_act[r] = h_rmask[r] && t->ca_len[r] > 0;
    }
    if (mask[b]) {
      if (allowed[b] < DSM_TTS_ALLOW_PAD_OR_EPAD) { e->set_error("slot %d: bad allowed-token code %d", b, allowed[b]); return DSM_ERR_INVALID; }
      for (int cb = 0; cb < S && cb < nc; ++cb) {
        uint32_t tok;
        if (cb == 0) {
          if (step == 0) tok = pad;
          else if (step <= (size_t)c.text_audio_delay_in_tokens) continue;  // None
          else tok = it.audio_tokens[(step - 1) * S + cb];
        } else if (step <= (size_t)c.acoustic_delay) tok = pad;
        else if (step <= (size_t)(c.text_audio_delay_in_tokens + c.acoustic_delay)) continue;  // None
        else tok = it.audio_tokens[(step - c.acoustic_delay - 1) * S + cb];
        if (tok == UNG) { e->set_error("internal error, ungenerated %zu", step); return DSM_ERR_STATE; }
        tk[1 + cb] = (int32_t)tok;
      }
    }
    for (int j = 1; j < rps; ++j) memcpy(tk + (size_t)j * (1 + nc), tk, sizeof(int32_t) * (size_t)(1 + nc));  // vec![t; batch_size] — :150,157
  }
  HIPCHK(hipMemcpyAsync(t->d_tokens, t->h_tokens, sizeof(int32_t) * (size_t)R * (1 + nc), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_allowed, t->h_allowed, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_mask, t->h_flags, t->flags_bytes, hipMemcpyHostToDevice, st));
  // The whole device side of a group's step — ~45 launches for the main LM, ~44 per depformer slice — is one hipGraph per
  // group once its two variants (with / without the depformer) have each run twice: the step is launch-bound otherwise.
  // Groups fork from the model stream behind the uploads and join it again before the downloads.
  const size_t Gn = t->groups.size();
  if (int rc = fork_groups(e, st, Gn)) return rc;
  if (int rc = run_groups(e, st, Gn, false, [&](size_t g, hipStream_t gs) {
        dsm_tts::Grp& grp = t->groups[g];
        bool run_dep = false;
        for (int b = grp.b0; b < grp.b0 + grp.nb; ++b) run_dep = run_dep || h_run[b];
        // graph variants: with / without the depformer; the key also tells sampling launches (LDS, argument) from ArgMax ones
        return run_captured(e, *t->g_ttsg[g][run_dep ? 1 : 0], gs, (run_dep ? 1 : 0) | (tts_any_sampling(t) ? 2 : 0),
                            [&] { return tts_group_body(t, gs, grp, run_dep); });
      }))
    return rc;
  if (int rc = join_groups(e, st, Gn)) return rc;  // only after every group was launched
  if (decode) {  // the entry is queued whatever happens: a slot can emit from step text_audio_delay + acoustic_delay on
    dsm_tts::PcmEntry& en = t->pcm_q[fsel];
    en.launched = false;
    t->pcm_seq += 1;
    t->pcm_pending += 1;
    bool any = false;
    for (int b = 0; b < B; ++b)
      any = any || (mask[b] && t->items[b].step_idx >= (size_t)(c.text_audio_delay_in_tokens + c.acoustic_delay));
    if (any)
      if (int rc = tts_enqueue_decode(t, fsel, en)) return rc;
  }
  HIPCHK(hipMemcpyAsync(t->h_text_token, t->d_text_token, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
  bool any_run = false;
  for (int b = 0; b < B; ++b) any_run = any_run || h_run[b];
  if (any_run) HIPCHK(hipMemcpyAsync(t->h_lat, t->d_lat, sizeof(uint32_t) * (size_t)B * S, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int ret = 0;
  for (int b = 0; b < B; ++b) {
    if (text_token_out) text_token_out[b] = mask[b] ? t->h_text_token[b] : 0;
    for (int k = 0; k < S; ++k)
      if (audio_out) audio_out[(size_t)b * S + k] = h_run[b] ? t->h_lat[(size_t)b * S + k] : UNG;
    if (!mask[b]) continue;
    dsm_tts::Item& it = t->items[b];
    const uint32_t text_token = t->h_text_token[b];
    if (text_token == (uint32_t)c.text_pad_token) it.consecutive_pads += 1; else it.consecutive_pads = 0;
    it.text_tokens[it.step_idx] = text_token;
    for (int k = 0; k < S; ++k) {  // delayed write-back — :220-236
      const size_t delay = k == 0 ? 0 : (size_t)c.acoustic_delay;
      const size_t at = it.step_idx >= delay ? it.step_idx - delay : 0;
      uint32_t& pos = it.audio_tokens[at * S + k];
      if (pos == UNG) pos = h_run[b] ? t->h_lat[(size_t)b * S + k] : pad;
    }
    it.step_idx += 1;
    if (it.step_idx >= t->n_steps) { e->set_error("max step-idx reached"); ret = DSM_ERR_STATE; }
  }
  return ret;
}
}  // namespace

extern "C" {

int dsm_tts_step(dsm_tts* t, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                 uint32_t* text_token_out, uint32_t* audio_out) {
  if (!t || !prev_text_token || !allowed || !mask) return DSM_ERR_INVALID;
  return tts_step_impl(t, prev_text_token, allowed, mask, text_token_out, audio_out, false);
}

int dsm_tts_attach_mimi(dsm_tts* t, const dsm_mimi_config* mimi, const char* mimi_safetensors) {
  if (!t || !mimi || !mimi_safetensors) {
    if (!t) g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  if (t->mimi || t->dec.ready) { e->set_error("a Mimi is attached already"); return DSM_ERR_STATE; }  // (or got as far as its decode state)
  // srv/tts.rs:309-310: mimi::load(.., Some(audio_codebooks)); every generated token must be a codebook entry
  if (mimi->quantizer_n_q != c.dep_num_slices || mimi->quantizer_bins < c.audio_vocab_size - 1) {
    e->set_error("Mimi with n_q %d / %d bins does not decode frames of %d codebooks with tokens below %d", mimi->quantizer_n_q,
                 mimi->quantizer_bins, c.dep_num_slices, c.audio_vocab_size - 1);
    return DSM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // allocations (null-stream fills) must not run beside a capture
  HIPCHK(hipDeviceSynchronize());
  char err[512];
  dsm_st_file* f = dsm_st_open(mimi_safetensors, err, sizeof err);
  if (!f) { e->set_error("%s", err); return DSM_ERR_IO; }
  Loader ld{e, f};
  int rc = load_mimi(e, ld, &t->mimi_w, *mimi);
  dsm_st_close(f);
  if (rc) return rc;
  if (!t->mimi_w.has_decoder) { e->set_error("the Mimi checkpoint has no decoder.* tensors"); return DSM_ERR_STATE; }
  const int B = t->B;
  if ((rc = alloc_dec_state(e, t->mimi_w, t->dec, B))) return rc;
  if (t->dec.h_descs.empty()) { e->set_error("a decoder without streaming convolutions is not supported"); return DSM_ERR_INVALID; }
  if ((rc = e->dalloc(&t->dec.started, B))) return rc;
  if ((rc = e->new_event(&t->ev_frames))) return rc;
  for (dsm_tts::PcmEntry& en : t->pcm_q) {
    if ((rc = e->new_event(&en.ev))) return rc;
    if ((rc = e->halloc(&en.h_pcm, (size_t)B * DSM_FRAME_SIZE))) return rc;
    if ((rc = e->halloc(&en.h_valid, (size_t)B))) return rc;
  }
  for (dsm_tts::PcmEntry& en : t->blk_pcm) {  // one per step of a dsm_tts_run block
    if ((rc = e->new_event(&en.ev))) return rc;
    if ((rc = e->halloc(&en.h_pcm, (size_t)B * DSM_FRAME_SIZE))) return rc;
    if ((rc = e->halloc(&en.h_valid, (size_t)B))) return rc;
  }
  HIPCHK(hipDeviceSynchronize());
  t->mimi = true;
  return 0;
}

int dsm_tts_step_pcm(dsm_tts* t, const uint32_t* prev_text_token, const int32_t* allowed, const uint8_t* mask,
                     uint32_t* text_token_out, uint32_t* audio_out, float* pcm_out, uint8_t* pcm_valid_out) {
  if (!t || !prev_text_token || !allowed || !mask) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!t->mimi) { e->set_error("dsm_tts_step_pcm needs dsm_tts_attach_mimi first"); return DSM_ERR_STATE; }
  if (t->egress_on) { e->set_error("egress is on: dsm_tts_step_raw delivers the frames"); return DSM_ERR_STATE; }
  if (pcm_out && t->pcm_pending > 0) {
    e->set_error("%d deferred step(s) wait for dsm_tts_recv_pcm: a serial step would deliver out of order", t->pcm_pending);
    return DSM_ERR_STATE;
  }
  if (t->pcm_pending >= 2) { e->set_error("two deferred steps wait for dsm_tts_recv_pcm"); return DSM_ERR_STATE; }
  const uint64_t seq = t->pcm_seq;
  const int rc = tts_step_impl(t, prev_text_token, allowed, mask, text_token_out, audio_out, true);
  if (pcm_out && t->pcm_seq != seq) {  // serial: the entry this call queued is delivered at once
    ApiShared api(e);
    if (int rd = tts_deliver_pcm(t, pcm_out, pcm_valid_out)) return rd;
  }
  return rc;
}

int dsm_tts_recv_pcm(dsm_tts* t, float* pcm_out, uint8_t* pcm_valid_out) {
  if (!t) return DSM_ERR_INVALID;
  if (t->egress_on) { t->set_error("egress is on: dsm_tts_recv_raw delivers the frames"); return DSM_ERR_STATE; }
  if (t->pcm_pending == 0) return 0;
  DsmDevice* e = t;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = tts_deliver_pcm(t, pcm_out, pcm_valid_out)) return rc;
  return 1;
}

int dsm_tts_pcm_pending(dsm_tts* t) { return t ? t->pcm_pending : DSM_ERR_INVALID; }

int dsm_tts_get_metrics(dsm_tts* t, dsm_metrics* out) {
  if (!t || !out) return DSM_ERR_INVALID;
  memset(out, 0, sizeof *out);
  t->fill_graph_metrics(out);
  // algorithmic bytes of one step: every DISTINCT weight matrix the step multiplies by, once (main LM layers + text linear; the
  // stacked depformer input projections; the depformer's shared attention weights, the gating weights of each of its G weight
  // groups and the 32 output linears), bf16.  A weight group serves ~3 consecutive slices and fits the Infinity Cache, so one
  // pass from HBM per step is what the algorithm needs; embedding rows gathered per slot and the short KV reads are left out.
  std::set<const void*> seen;
  double bytes = 0;
  auto lin = [&](const Linear& L) {
    if (L.w && seen.insert(L.w).second) bytes += (double)L.N * (double)L.K * (L.bf16 ? 2.0 : 4.0);
  };
  auto trw = [&](const TransformerW& w) {
    for (const TLayerW& L : w.layers) {
      lin(L.in_proj); lin(L.out_proj); lin(L.ff_in); lin(L.ff_out);
      if (w.has_ca) { lin(L.ca_q); lin(L.ca_out); }
    }
  };
  trw(t->lm.tr);
  lin(t->lm.text_linear);
  lin(t->dep.in_all);
  for (const TransformerW& w : t->dep.tr) trw(w);
  for (const Linear& L : t->dep.out) lin(L);
  out->algorithmic_bytes_lm = bytes;
  return 0;
}

int dsm_tts_audio_tokens(dsm_tts* t, int slot, int step, uint32_t* out) {
  if (!t || !out || slot < 0 || slot >= t->B || step < 0 || (size_t)step >= t->n_steps) return DSM_ERR_INVALID;
  const int S = t->cfg.dep_num_slices;
  memcpy(out, &t->items[slot].audio_tokens[(size_t)step * S], sizeof(uint32_t) * S);
  return 0;
}

int dsm_tts_step_idx(dsm_tts* t, int slot) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  return (int)t->items[slot].step_idx;
}

int dsm_tts_set_sampling(dsm_tts* t, int slot, int top_k, float temperature, uint64_t seed) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  // srv/tts.rs:401-408: ArgMax unless temperature > 0 and top_k > 1
  const int32_t k = (temperature > 0.0f && top_k > 1) ? top_k : 0;
  const float invt = k ? (float)(1.0 / (double)temperature) : 1.0f;  // candle: logits / t == affine(1 / t, 0)
  uint32_t key[8];
  dsm_seed_from_u64(seed, key);
  const uint32_t zero = 0;
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpyAsync(t->d_samp_k + slot, &k, sizeof k, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_samp_invt + slot, &invt, sizeof invt, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_rng_key + (size_t)slot * 8, key, sizeof key, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_rng_pos_text + slot, &zero, sizeof zero, hipMemcpyHostToDevice, st));  // both processors start at
  HIPCHK(hipMemcpyAsync(t->d_rng_pos_audio + slot, &zero, sizeof zero, hipMemcpyHostToDevice, st)); // word 0 of the same stream
  HIPCHK(hipStreamSynchronize(st));  // the sources are stack variables
  t->samp_k[slot] = k;
  return 0;
}

}  // extern "C" (reopened below)

namespace {
// A voice's K (kv = 0) or V (kv = 1) block of layer l, [H][smax][hd] in the cache dtype
uint8_t* tts_voice_block(const dsm_tts* t, const dsm_tts::Voice& v, int l, int kv) {
  const size_t blk = (size_t)t->cfg.lm.d_model * t->ca.smax * (t->cfg.kv_bf16 ? 2 : 4);
  return v.mem + ((size_t)2 * l + kv) * blk;
}

// compute_kv(CaSrc::Tokens(src)) (core/transformer.rs:299-318) into every layer's [H][smax][hd] block of a voice, or (voice ==
// nullptr) of batch row `row`'s private part of the source cache: one code path, so that a voice holds a private row's bits
template <typename KVT>
int tts_project_ca_row(dsm_tts* t, hipStream_t st, int row, const dsm_tts::Voice* voice, const float* src, int n) {
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  const int d = c.lm.d_model, H = c.lm.num_heads, hd = d / H, kvd = c.ca_dim > 0 ? c.ca_dim : d, smax = t->ca.smax;
  HIPCHK(hipMemcpyAsync(t->ca_src_dev, src, sizeof(float) * (size_t)n * kvd, hipMemcpyHostToDevice, st));
  for (int l = 0; l < c.lm.num_layers; ++l) {
    GemmArgs a = base_args(t->lm.tr.layers[l].ca_kv, t->ca_src_dev, plain_map(n, kvd), n);
    a.Y = t->ca_kv_tmp; a.ymap = plain_map(n, 2 * d);
    if (int rc = gemm_store<uint16_t>(e, st, a, kvd % 32 == 0)) return rc;
    KVT* kc = voice ? reinterpret_cast<KVT*>(tts_voice_block(t, *voice, l, 0)) : reinterpret_cast<KVT*>(t->ca.k[l]) + (size_t)row * H * smax * hd;
    KVT* vc = voice ? reinterpret_cast<KVT*>(tts_voice_block(t, *voice, l, 1)) : reinterpret_cast<KVT*>(t->ca.v[l]) + (size_t)row * H * smax * hd;
    const long tot = (long)n * d;
    hipLaunchKernelGGL(ca_kv_scatter_kernel<KVT>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, t->ca_kv_tmp, kc, vc, n, d, hd, smax);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

dsm_tts::Voice* tts_find_voice(dsm_tts* t, int handle) {
  for (dsm_tts::Voice& v : t->voices)
    if (v.handle == handle) return &v;
  return nullptr;
}

// Batch row `row` reads `voice` from now on, or (nullptr) its private block again: its entry of every layer's table in one
// strided upload, and the reference counts.  Nothing else is copied.  Only enqueues (the entries wait in src_stage, one part per
// row of a slot): the caller synchronises the stream before it touches another slot.
int tts_point_row(dsm_tts* t, hipStream_t st, int row, dsm_tts::Voice* voice) {
  DsmDevice* e = t;
  const int have = t->row_voice[row], want = voice ? voice->handle : 0;
  if (have == want) return 0;
  const int L = t->cfg.lm.num_layers, R = t->R;
  const size_t blk = (size_t)t->cfg.lm.d_model * t->ca.smax * (t->cfg.kv_bf16 ? 2 : 4);
  AttnRowSrc* ent = t->src_stage.data() + (size_t)(row % t->rps) * L;
  for (int l = 0; l < L; ++l) {
    ent[l].k = voice ? tts_voice_block(t, *voice, l, 0) : (uint8_t*)t->ca.k[l] + (size_t)row * blk;
    ent[l].v = voice ? tts_voice_block(t, *voice, l, 1) : (uint8_t*)t->ca.v[l] + (size_t)row * blk;
  }
  HIPCHK(hipMemcpy2DAsync(t->ca_src_tab + row, sizeof(AttnRowSrc) * (size_t)R, ent, sizeof(AttnRowSrc), sizeof(AttnRowSrc), (size_t)L,
                          hipMemcpyHostToDevice, st));
  if (dsm_tts::Voice* old = tts_find_voice(t, have)) --old->refs;
  if (voice) ++voice->refs;
  t->row_voice[row] = want;
  return 0;
}

// The slot's guidance: Tensor * f64 = affine(mul as f32, 0.), the two factors of l0 * a - l1 * (a - 1.) in f32
int tts_upload_guidance(dsm_tts* t, hipStream_t st, int slot, bool guided, double cfg_alpha) {
  DsmDevice* e = t;
  const uint8_t on = guided ? 1 : 0;
  const float fa = (float)cfg_alpha, fb = (float)(cfg_alpha - 1.);
  HIPCHK(hipMemcpyAsync(t->d_cfg_on + slot, &on, 1, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_cfg_fa + slot, &fa, sizeof fa, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(t->d_cfg_fb + slot, &fb, sizeof fb, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  t->cfg_on[slot] = on;
  return 0;
}
}  // namespace

extern "C" {

int dsm_tts_set_ca_src(dsm_tts* t, int slot, const float* ca_src, int n, const float* ca_src_uncond, int n_uncond, double cfg_alpha) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  const dsm_tts_config& c = t->cfg;
  if (!c.cross_attention) { e->set_error("this engine was created without cross_attention"); return DSM_ERR_STATE; }
  if (n < 0 || n_uncond < 0 || n > c.ca_max_len || n_uncond > c.ca_max_len) {
    e->set_error("cross-attention source of %d / %d rows: at most ca_max_len = %d", n, n_uncond, c.ca_max_len);
    return DSM_ERR_INVALID;
  }
  if (!ca_src) n = 0;
  if (!ca_src_uncond) n_uncond = 0;
  if (n_uncond > 0 && (t->rps != 2 || n == 0)) {
    e->set_error("guidance needs an engine created with cfg_rows = 1 and a conditional source");
    return DSM_ERR_INVALID;
  }
  // The reference fixes ca_src and the batch size at State::new (core/tts_streaming.rs:100-115).  Giving a slot a source — or
  // switching guidance on — in the middle of a generation would mix rows whose self-attention histories differ in length (the
  // unconditional row of an unguided slot does not advance): only a fresh slot takes a source; clearing is always allowed.
  if ((n > 0 || n_uncond > 0) && t->items[slot].step_idx != 0) {
    e->set_error("slot %d is at step %zu: dsm_tts_set_ca_src needs a fresh slot (dsm_tts_reset_slot first)", slot, t->items[slot].step_idx);
    return DSM_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < t->rps; ++j) {
    const int row = slot * t->rps + j, len = j == 0 ? n : n_uncond;
    const float* src = j == 0 ? ca_src : ca_src_uncond;
    if (int rc = tts_point_row(t, st, row, nullptr)) return rc;  // a row on a voice (dsm_tts_set_voice) lets go of it first
    if (len > 0) {
      const int rc = with_kv_type(c.kv_bf16 != 0, [&](auto kv) { return tts_project_ca_row<decltype(kv)>(t, st, row, nullptr, src, len); });
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(st));  // the staging buffers are reused by the next row; `src` is the caller's memory
    } else if (t->ca_len[row] > 0) {
      // the row's last attention output must not outlive its source: the out_proj of a source-less row has to see zeros
      HIPCHK(hipMemsetAsync(t->ca.att + (size_t)row * c.lm.d_model, 0, sizeof(float) * (size_t)c.lm.d_model, st));
    }
    const uint32_t last = len > 0 ? (uint32_t)(len - 1) : 0u;
    HIPCHK(hipMemcpyAsync(t->ca.last + row, &last, sizeof last, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    t->ca_len[row] = len;
  }
  return tts_upload_guidance(t, st, slot, n_uncond > 0, cfg_alpha);
}

int dsm_tts_reset_slot(dsm_tts* t, int slot) {
  if (!t || slot < 0 || slot >= t->B) return DSM_ERR_INVALID;
  if (t->blk_pending) { t->set_error("a block of %d steps waits for dsm_tts_collect", t->blk_pending); return DSM_ERR_STATE; }
  if (t->reqs[slot].active)  // ends the slot's request: IDLE again
    if (int rc = tts_request_end(t, slot)) return rc;
  if (t->samp_k[slot] > 0)  // a fresh State has fresh (ArgMax) processors until the caller configures them again
    if (int rc = dsm_tts_set_sampling(t, slot, 0, 0.0f, 0)) return rc;
  if (t->cfg.cross_attention)  // ... and whatever ca_src / cfg_alpha its creator passes: none until dsm_tts_set_ca_src
    if (int rc = dsm_tts_set_ca_src(t, slot, nullptr, 0, nullptr, 0, 0.0)) return rc;
  if (t->cond_on[slot])  // ... and no Condition until dsm_tts_set_condition_*
    if (int rc = dsm_tts_clear_condition(t, slot)) return rc;
  DsmDevice* e = t;
  dsm_tts::Item& it = t->items[slot];
  it.step_idx = 0;
  it.consecutive_pads = 0;
  std::fill(it.audio_tokens.begin(), it.audio_tokens.end(), DSM_TTS_UNGENERATED);
  std::fill(it.text_tokens.begin(), it.text_tokens.end(), DSM_TTS_UNGENERATED);
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  for (int j = 0; j < t->rps; ++j)
    if (int rc = reset_transformer_slot(e, e->s_model, t->tr, slot * t->rps + j)) return rc;
  HIPCHK(hipStreamSynchronize(e->s_model));
  if (t->mimi) {
    // The slot's next generation decodes with a fresh Mimi (srv/tts.rs:499-500: clone() + reset_state()): conv states and carries
    // zero, not started, and — unlike Mimi::reset_batch_idx — the decoder transformer back at position 0.  On the decode stream,
    // i.e. behind the decodes already queued for the old generation.  Egress: the slot's history goes with it, its format stays.
    if (t->egress_fmt.ready) HIPCHK(hipMemsetAsync(t->egress_started + slot, 0, sizeof(uint32_t), e->s_enc));
    return reset_decoder_slot(e, t->mimi_w, t->dec, e->s_enc, slot, true);
  }
  return 0;
}

int dsm_tts_debug_read(dsm_tts* t, const char* name, float* out, size_t cap) {
  if (!t || !name || !out) return DSM_ERR_INVALID;
  DsmDevice* e = t;
  if (!strncmp(name, "spk.", 4)) return spk_debug_read(t, name, out, cap);
  const float* src = nullptr;
  size_t n = 0;
  if (!strcmp(name, "lm.hidden")) { src = t->hidden; n = (size_t)t->R * t->cfg.lm.d_model; }
  else if (!strcmp(name, "lm.logits")) { src = t->logits; n = (size_t)t->R * t->cfg.text_out_vocab_size; }
  else if (!strcmp(name, "dep.logits")) { src = t->dlogits; n = (size_t)t->R * (t->cfg.audio_vocab_size - 1); }
  else if (!strcmp(name, "lm.input")) { src = t->lm_in; n = (size_t)t->R * t->cfg.lm.d_model; }  // the rows tts_input_kernel wrote in the last step
  else if (!strcmp(name, "cond.row")) { src = t->d_cond; n = (size_t)t->B * t->cfg.lm.d_model; }  // [B][d_model], zeros without a condition
  if (!src) return DSM_ERR_INVALID;
  if (n > cap) n = cap;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  // the copy rides the model stream: a null-stream hipMemcpy queues behind whatever other engines of the process have enqueued on
  // the hardware queue it lands on (166 ms behind a B = 64 STT engine's queued steps, profiles/r11/packed_f32.txt)
  HIPCHK(hipMemcpyAsync(out, src, sizeof(float) * n, hipMemcpyDeviceToHost, e->s_model));
  HIPCHK(hipStreamSynchronize(e->s_model));
  return (int)n;
}

}  // extern "C"
