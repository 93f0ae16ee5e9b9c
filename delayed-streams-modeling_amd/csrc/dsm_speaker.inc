// dsm_speaker.inc — SpeakerEncoder (core/tts_streaming.rs:335-417): voice clips to the rows dsm_tts_set_ca_src takes (part of
// the library's one translation unit).  encode() is a whole-clip, NON-streaming Mimi encode (Mimi::encode_pre_quantize,
// core/mimi.rs:177-183): the SEANet convolutions over all r frames of a clip at once — the streaming geometries with T_in scaled
// by r over the same packed weights, a fresh state's zero / replicate left pad, nothing carried out — and the encoder
// transformer over T = 2 r positions with plain causal attention (spk_attn_kernel): T never exceeds the transformer's context, so
// the ring of the streaming path never wraps and both compute the same sums.  Then ConvDownsample1d, output_proj, learnt_padding for
// the speakers a request does not name and add_sin_embeddings (core/tts.rs:94-109).
//
// Tolerance-pinned, not bit-pinned: the oracle has only the streaming Mimi (DESIGN.md, "Speaker encoder").  The attention sums in
// its own fixed order; everything else uses the library's GEMMs and epilogues, whose sums do not depend on how many rows a launch has.
//
// Shared with the step path, each written once: the SEANet chain and its buffers (seanet_encode, alloc_seanet_enc — here one clip
// of r frames per call where the step path has B slots of one frame) and every transformer layer from out_proj onward
// (transformer_layer_tail).  This path's own: the normalisation of the clips, the RoPE table, the plain QKV store and
// spk_attn_kernel in place of the ring front, and everything from ConvDownsample1d on.
//
// Nothing of the step or the decode side is touched: the scratch below is the clip path's own, the work runs on the model stream
// between steps like dsm_tts_set_ca_src, and no graph slot is involved.

namespace {

int spk_frames_per_step(const MimiW& w) { return w.final_conv.T_out; }  // encoder-rate positions per 1920-sample frame

template <int HD>
int spk_launch_attn(DsmDevice* e, hipStream_t st, float* out, const float* qkv, const float* cs, int T, int H, int clips) {
  const size_t lds = spk_attn_lds<HD>(T);  // within the default 64 KB of dynamic LDS: checked at attach for T = context
  hipLaunchKernelGGL(spk_attn_kernel<HD>, dim3((T + SPK_QB - 1) / SPK_QB, H, clips), dim3(256), lds, st, out, qkv, cs, T, H);
  HIPCHK(hipGetLastError());
  return 0;
}

// The device side of one encode: c normalised clips of r frames in cat_init -> n_speakers * r rows in spk.rows.  Launches on
// `st` only (no copy to the host, no synchronisation), so a stream capture can count them ("spk.launches").
int spk_encode_body(dsm_tts* t, hipStream_t st, int c, int r) {
  DsmDevice* e = t;
  SpkEnc& s = t->spk;
  const MimiW& w = t->mimi_w;
  const dsm_transformer_config& tc = w.tr.cfg;
  const RowMap none = plain_map(1, 1);
  const int d = w.cfg.dimension, H = tc.num_heads, hd = d / H, T = spk_frames_per_step(w) * r, M = c * T;
  e->tag_gemm[e->sid(st)] = DSM_PROF_OTHER;
  e->tag_attn[e->sid(st)] = DSM_PROF_OTHER;
  // ---- SeaNetEncoder::forward, one clip at a time (layer 0 of a 10 s clip is 240 000 rows: a clip alone fills the chip, and the
  // scratch stays that of one clip whatever n_speakers is) ----
  const ConvGeom g0 = over_frames(w.init_conv, r);
  const long init_stride = (long)(g0.S + g0.T_in) * g0.in_c;
  for (int i = 0; i < c; ++i)
    if (int rc = seanet_encode(e, st, w, s.enc, s.enc.cat_init + (long)i * init_stride, 1, r, s.act.x + (long)i * T * d, plain_map(T, d)))
      return rc;
  // ---- ProjectedTransformer::forward over all clips' positions, M = c * T rows: the QKV projection a plain store (no ring, no
  // builder) and causal attention within each clip, then the layer tail of the step path; the last layer's output lands in the
  // downsample convolution's concat buffer ----
  const ConvGeom gd = over_frames(w.downsample, r);
  if (gd.S > 0 && !gd.replicate)  // a zero left pad: where it sits depends on the clip length of this call
    HIPCHK(hipMemsetAsync(s.cat_ds, 0, sizeof(float) * (size_t)c * (gd.S + gd.T_in) * gd.in_c, st));
  const float* rope = tc.positional_embedding == 1 ? s.rope_cs : nullptr;  // null: q and k are not rotated
  if (rope) {
    const int n = T * (hd / 2);
    hipLaunchKernelGGL(spk_rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, st, s.rope_cs, w.tr.inv_freq, T, hd / 2,
                       w.tr.rope_pos_before ? 0 : spk_frames_per_step(w));
    HIPCHK(hipGetLastError());
  }
  if (int rc = run_norm(e, st, s.act.xn, s.act.x, w.tr.layers[0].n1w, w.tr.layers[0].n1b, M, d, tc.norm)) return rc;
  for (int l = 0; l < tc.num_layers; ++l) {
    GemmArgs a = base_args(w.tr.layers[l].in_proj, s.act.xn, plain_map(M, d), M);
    a.Y = s.qkv; a.ymap = plain_map(M, 3 * d);
    if (int rc = gemm_store<float>(e, st, a)) return rc;
    if (int rc = hd == 32 ? spk_launch_attn<32>(e, st, s.act.att, s.qkv, rope, T, H, c)
                          : spk_launch_attn<64>(e, st, s.act.att, s.qkv, rope, T, H, c))
      return rc;
    if (int rc = transformer_layer_tail<float, float>(e, st, w.tr, l, s.act, c, T, s.cat_ds, cat_map(gd), nullptr, nullptr, nullptr)) return rc;
  }
  // ---- ConvDownsample1d::forward — core/conv.rs:527-547: the left pad of a clip repeats its first frame ----
  if (gd.S > 0) {
    if (gd.replicate) hipLaunchKernelGGL(conv_replicate_init_kernel, dim3(c), dim3(256), 0, st, conv_desc(s.cat_ds, gd), (const uint8_t*)nullptr);
    HIPCHK(hipGetLastError());
  }
  if (int rc = run_conv(e, st, gd, s.cat_ds, c, s.latent, plain_map(c * r, d), nullptr, none, nullptr, none)) return rc;
  // ---- output_proj, + pos_emb through the GEMM's residual input; learnt_padding + pos_emb for the speakers not named ----
  {
    GemmArgs a = base_args(s.proj, s.latent, plain_map(c * r, d), c * r);
    a.res = s.pos; a.rmap = plain_map(c * r, s.cond_dim);
    a.Y = s.rows; a.ymap = plain_map(c * r, s.cond_dim);
    if (int rc = gemm_store<float>(e, st, a)) return rc;
  }
  if (c < s.n_speakers) {
    const long n = (long)(s.n_speakers - c) * r * s.cond_dim;
    hipLaunchKernelGGL(spk_pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.rows, s.pad, s.pos, (long)c * r,
                       (long)(s.n_speakers - c) * r, s.cond_dim);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// Kernel launches of the last encode's device side ("spk.launches", a diagnostic for tools/voice_encode_timing.py, asked for once
// per shape): the kernel nodes of a stream capture of spk_encode_body that is thrown away (nothing runs; memset nodes are not
// counted).  The launches sit inside the shared GEMM helpers, so a counter of this file's own would miss most of them.
int spk_count_launches(dsm_tts* t, size_t* out) {
  DsmDevice* e = t;
  *out = 0;
  if (t->spk.last_c == 0) return 0;
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  ApiExclusive alone(e);
  HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
  e->capturing = true;
  e->capture_failed = false;
  const int rc = spk_encode_body(t, st, t->spk.last_c, t->spk.last_r);
  e->capturing = false;
  hipGraph_t g = nullptr;
  const hipError_t he = hipStreamEndCapture(st, &g);
  if (!rc && he == hipSuccess && g) {
    size_t n = 0;
    (void)hipGraphGetNodes(g, nullptr, &n);
    std::vector<hipGraphNode_t> nodes(n);
    if (n && hipGraphGetNodes(g, nodes.data(), &n) == hipSuccess)
      for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nodes[i], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel) *out += 1;
      }
  }
  if (g) (void)hipGraphDestroy(g);
  if (rc) return rc;
  HIPCHK(he);
  return 0;
}

int spk_debug_read(dsm_tts* t, const char* name, float* out, size_t cap) {
  DsmDevice* e = t;
  SpkEnc& s = t->spk;
  if (!s.ready) { e->set_error("no speaker encoder attached"); return DSM_ERR_STATE; }
  const MimiW& w = t->mimi_w;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  HIPCHK(hipStreamSynchronize(e->s_model));
  if (!strcmp(name, "spk.stats")) {  // scratch MiB, milliseconds between the last encode's two events
    const float v[2] = {(float)((double)s.scratch_bytes / (1024.0 * 1024.0)), s.last_ms};
    const size_t n = cap < 2 ? cap : 2;
    memcpy(out, v, sizeof(float) * n);
    return (int)n;
  }
  if (!strcmp(name, "spk.launches")) {
    size_t nodes = 0;
    if (int rc = spk_count_launches(t, &nodes)) return rc;
    out[0] = (float)nodes;
    return cap ? 1 : 0;
  }
  const int c = s.last_c, r = s.last_r;
  if (!strcmp(name, "spk.pcm_norm")) {  // [c][clip_len]: the clips behind the first convolution's left pad
    const ConvGeom g0 = over_frames(w.init_conv, r);
    const size_t len = (size_t)g0.T_in * g0.in_c, stride = (size_t)(g0.S + g0.T_in) * g0.in_c;
    size_t n = 0;
    for (int i = 0; i < c && n + len <= cap; ++i, n += len)
      HIPCHK(hipMemcpy(out + n, s.enc.cat_init + (size_t)i * stride + (size_t)g0.S * g0.in_c, sizeof(float) * len, hipMemcpyDeviceToHost));
    return (int)n;
  }
  if (!strcmp(name, "spk.latent")) {  // [c * r][dimension]: encode_pre_quantize, transposed
    size_t n = (size_t)c * r * w.cfg.dimension;
    if (n > cap) n = cap;
    HIPCHK(hipMemcpy(out, s.latent, sizeof(float) * n, hipMemcpyDeviceToHost));
    return (int)n;
  }
  return DSM_ERR_INVALID;
}

// add_sin_embeddings' table — core/tts.rs:94-109, in its order of operations: powf, the f32 quotient and product, cosf / sinf,
// cosines first
void spk_pos_table(std::vector<float>& out, int rows, int dim) {
  const int half = dim / 2;
  out.assign((size_t)rows * dim, 0.0f);
  std::vector<float> inv((size_t)half);
  for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(10000.0f, (float)i / (float)(half - 1));
  for (int j = 0; j < rows; ++j)
    for (int i = 0; i < half; ++i) {
      const float f = (float)j * inv[i];
      out[(size_t)j * dim + i] = cosf(f);
      out[(size_t)j * dim + half + i] = sinf(f);
    }
}

int spk_attach_impl(dsm_tts* t, int n_speakers, const char* lm_path) {
  DsmDevice* e = t;
  SpkEnc& s = t->spk;
  const dsm_tts_config& c = t->cfg;
  const MimiW& w = t->mimi_w;
  const dsm_mimi_config& mc = w.cfg;
  const int cond = c.ca_dim > 0 ? c.ca_dim : c.lm.d_model, d = mc.dimension;
  const int fps = spk_frames_per_step(w), hd = d / mc.transformer.num_heads, ctx = mc.transformer.context;
  if (mc.channels != 1) { e->set_error("the speaker encoder takes mono clips (Mimi channels = %d)", mc.channels); return DSM_ERR_INVALID; }
  if (hd != 32 && hd != 64) { e->set_error("speaker encoder: Mimi head_dim %d unsupported (32, 64)", hd); return DSM_ERR_INVALID; }
  if (cond < 4 || cond % 2) { e->set_error("speaker encoder: cond_dim %d must be even and at least 4", cond); return DSM_ERR_INVALID; }
  const int max_r = ctx / fps;
  if (max_r < 1) { e->set_error("Mimi transformer context %d is shorter than one frame (%d positions)", ctx, fps); return DSM_ERR_INVALID; }
  if ((hd == 32 ? spk_attn_lds<32>(ctx) : spk_attn_lds<64>(ctx)) > (size_t)64 * 1024) {  // context above 700 (head_dim 64) / 860 (32)
    e->set_error("Mimi transformer context %d: the clip attention keeps a block's scores in 64 KB of LDS", ctx);
    return DSM_ERR_INVALID;
  }
  char err[512];
  dsm_st_file* f = dsm_st_open(lm_path, err, sizeof err);
  if (!f) { e->set_error("%s", err); return DSM_ERR_IO; }
  static const char* kProj = "condition_provider.conditioners.speaker_wavs.output_proj.weight";
  static const char* kPad = "condition_provider.conditioners.speaker_wavs.learnt_padding";
  std::vector<float> wp((size_t)cond * d), lp((size_t)cond);
  int rc = 0;
  const dsm_st_tensor* tp = dsm_st_find(f, kProj);
  if (tp && (tp->ndim != 2 || tp->shape[0] != cond || tp->shape[1] != d)) {
    e->set_error("shape mismatch for %s: expected [%d][%d]", kProj, cond, d);
    rc = DSM_ERR_IO;
  } else if (dsm_st_read_f32(f, kProj, (int64_t)cond * d, wp.data(), err, sizeof err) || dsm_st_read_f32(f, kPad, cond, lp.data(), err, sizeof err)) {
    e->set_error("%s", err);
    rc = DSM_ERR_IO;
  }
  dsm_st_close(f);
  if (rc) return rc;
  size_t floats = 0;
  auto alloc = [&](float** p, size_t count) {
    floats += count;
    return e->dalloc(p, count);
  };
  if ((rc = pack_linear(e, &s.proj, wp.data(), cond, d, false, nullptr))) return rc;
  if ((rc = e->upload(&s.pad, lp.data(), lp.size()))) return rc;
  s.pos_rows = n_speakers * (max_r > 125 ? max_r : 125);  // encode: n_speakers * r rows; empty: n_speakers * 125
  {
    std::vector<float> pos;
    spk_pos_table(pos, s.pos_rows, cond);
    if ((rc = e->upload(&s.pos, pos.data(), pos.size()))) return rc;
  }
  // scratch of the longest clip (max_r frames): one clip through the convolutions, n_speakers through the transformer
  const ConvGeom g0 = over_frames(w.init_conv, max_r), gd = over_frames(w.downsample, max_r);
  const size_t len = (size_t)g0.T_in * g0.in_c, T = (size_t)fps * max_r, rows = (size_t)n_speakers * T;
  if ((rc = alloc(&s.pcm, (size_t)n_speakers * len))) return rc;
  if ((rc = alloc(&s.stdev, (size_t)n_speakers))) return rc;
  if ((rc = alloc_seanet_enc(e, &s.enc, w, n_speakers, 1, max_r, nullptr, &floats))) return rc;
  // not alloc_act: its q would be a [rows][d] buffer this path never touches, on top of qkv
  if ((rc = alloc(&s.act.x, rows * d))) return rc;
  if ((rc = alloc(&s.act.xn, rows * d))) return rc;
  if ((rc = alloc(&s.qkv, rows * 3 * d))) return rc;
  if ((rc = alloc(&s.act.att, rows * d))) return rc;
  if ((rc = alloc(&s.act.g, rows * (size_t)w.tr.hidden))) return rc;
  if ((rc = alloc(&s.rope_cs, T * hd))) return rc;
  if ((rc = alloc(&s.cat_ds, (size_t)n_speakers * (gd.S + gd.T_in) * gd.in_c))) return rc;
  if ((rc = alloc(&s.latent, (size_t)n_speakers * max_r * d))) return rc;
  if ((rc = alloc(&s.rows, (size_t)s.pos_rows * cond))) return rc;
  if ((rc = e->halloc(&s.h_stdev, (size_t)n_speakers))) return rc;
  if ((rc = e->halloc(&s.h_rows, (size_t)s.pos_rows * cond))) return rc;
  if ((rc = e->new_event(&s.ev_a, hipEventDefault))) return rc;
  if ((rc = e->new_event(&s.ev_b, hipEventDefault))) return rc;
  s.scratch_bytes = floats * sizeof(float);
  s.n_speakers = n_speakers;
  s.cond_dim = cond;
  s.max_r = max_r;
  HIPCHK(hipDeviceSynchronize());
  s.ready = true;
  return 0;
}

}  // namespace

extern "C" {

int dsm_tts_attach_speaker_encoder(dsm_tts* t, int n_speakers, const char* lm_safetensors) {
  if (!t || !lm_safetensors) {
    if (!t) g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  DsmDevice* e = t;
  if (n_speakers < 1) { e->set_error("n_speakers must be at least 1 (got %d)", n_speakers); return DSM_ERR_INVALID; }
  if (!t->cfg.cross_attention) { e->set_error("the speaker encoder needs an engine created with cross_attention"); return DSM_ERR_STATE; }
  if (!t->mimi) { e->set_error("the speaker encoder needs dsm_tts_attach_mimi first (that Mimi is the speaker tokenizer)"); return DSM_ERR_STATE; }
  if (t->spk.ready || t->spk.pad) { e->set_error("a speaker encoder is attached already"); return DSM_ERR_STATE; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // allocations (null-stream fills) must not run beside a capture
  HIPCHK(hipDeviceSynchronize());
  return spk_attach_impl(t, n_speakers, lm_safetensors);
}

int dsm_tts_encode_voice(dsm_tts* t, const float* pcm, int n_clips, int clip_len, float* ca_src_out, int cap_rows, int* rows_out) {
  if (!t || !pcm || !ca_src_out || !rows_out) {
    if (!t) g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  DsmDevice* e = t;
  SpkEnc& s = t->spk;
  *rows_out = 0;
  if (!s.ready) { e->set_error("dsm_tts_encode_voice needs dsm_tts_attach_speaker_encoder first"); return DSM_ERR_STATE; }
  if (n_clips < 1) { e->set_error("empty speakers in encode"); return DSM_ERR_INVALID; }
  if (clip_len <= 0 || clip_len % DSM_FRAME_SIZE) {
    e->set_error("clip_len %d must be a positive multiple of %d samples", clip_len, DSM_FRAME_SIZE);
    return DSM_ERR_INVALID;
  }
  const int r = clip_len / DSM_FRAME_SIZE, c = n_clips < s.n_speakers ? n_clips : s.n_speakers;
  if (r > s.max_r) {
    e->set_error("a clip of %d frames is %d positions: more than the Mimi transformer's context of %d", r, r * spk_frames_per_step(t->mimi_w),
                 t->mimi_w.cfg.transformer.context);
    return DSM_ERR_INVALID;
  }
  const int rows = s.n_speakers * r;
  *rows_out = rows;
  if (cap_rows < rows) { e->set_error("the voice encodes to %d rows, ca_src_out holds %d", rows, cap_rows); return DSM_ERR_INVALID; }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  const ConvGeom g0 = over_frames(t->mimi_w.init_conv, r);
  const long stride = (long)(g0.S + g0.T_in) * g0.in_c;
  HIPCHK(hipEventRecord(s.ev_a, st));
  HIPCHK(hipMemcpyAsync(s.pcm, pcm, sizeof(float) * (size_t)c * clip_len, hipMemcpyHostToDevice, st));
  // the clips' zero left pads: where they sit depends on the clip length of this call
  HIPCHK(hipMemsetAsync(s.enc.cat_init, 0, sizeof(float) * (size_t)c * stride, st));
  hipLaunchKernelGGL(spk_normalize_kernel, dim3(c), dim3(1024), 0, st, s.pcm, clip_len, s.enc.cat_init + (long)g0.S * g0.in_c, stride, s.stdev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.h_stdev, s.stdev, sizeof(float) * (size_t)c, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  s.last_c = c;
  s.last_r = r;
  for (int i = 0; i < c; ++i)
    if (!(s.h_stdev[i] > 0.0f) || !std::isfinite(s.h_stdev[i])) {  // the reference would hand NaNs to the LM
      e->set_error("clip %d: standard deviation %g (a silent or non-finite clip cannot be normalised)", i, (double)s.h_stdev[i]);
      return DSM_ERR_INVALID;
    }
  if (int rc = spk_encode_body(t, st, c, r)) return rc;
  HIPCHK(hipMemcpyAsync(s.h_rows, s.rows, sizeof(float) * (size_t)rows * s.cond_dim, hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(s.ev_b, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&s.last_ms, s.ev_a, s.ev_b));
  memcpy(ca_src_out, s.h_rows, sizeof(float) * (size_t)rows * s.cond_dim);
  return 0;
}

int dsm_tts_speaker_empty(dsm_tts* t, float* ca_src_out, int cap_rows, int* rows_out) {
  if (!t || !ca_src_out || !rows_out) {
    if (!t) g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  DsmDevice* e = t;
  SpkEnc& s = t->spk;
  *rows_out = 0;
  if (!s.ready) { e->set_error("dsm_tts_speaker_empty needs dsm_tts_attach_speaker_encoder first"); return DSM_ERR_STATE; }
  const int rows = s.n_speakers * 125;  // the reference's literal, whatever the clip length
  *rows_out = rows;
  if (cap_rows < rows) { e->set_error("the empty voice is %d rows, ca_src_out holds %d", rows, cap_rows); return DSM_ERR_INVALID; }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  hipStream_t st = e->s_model;
  HIPCHK(hipStreamSynchronize(st));
  const long n = (long)rows * s.cond_dim;
  hipLaunchKernelGGL(spk_pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s.rows, s.pad, s.pos, 0L, (long)rows, s.cond_dim);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s.h_rows, s.rows, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  memcpy(ca_src_out, s.h_rows, sizeof(float) * (size_t)n);
  return 0;
}

}  // extern "C"
