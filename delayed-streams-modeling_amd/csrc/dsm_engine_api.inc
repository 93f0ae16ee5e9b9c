// dsm_engine_api.inc — step orchestration + the extern "C" entry points (included by dsm_engine.hip)

namespace {

template <typename KVT, int HD, int T>
int launch_attn_t(DsmDevice* e, hipStream_t st, float* out, const float* q, const void* k, const void* v,
                  const uint32_t* start_pos, const uint8_t* active, int B, int H, int ctx, int d, const AttnFused& fq) {
  // bf16 rings: eight keys per lane group and batch at head_dim 128 (126 VGPRs; 0.69 of the HBM peak alone at 32 slots, 0.88 at 1024),
  // four below (78 VGPRs: stt-2.6b's head_dim-64 launches 39.2 against 42.8 us).  Four at head_dim 128 buys the B = 64 step 0.6 %
  // through co-residency and costs the kernel itself 3-4 % (38.7 against 37.0 us alone): not taken.
  // (T = 2 on a bf16 ring — no shipped configuration — spills with eight: always four; so do the f32 rings)
  constexpr int UNR = (sizeof(KVT) == 2 && T == 1 && HD == 128) ? 8 : 4;
  size_t lds = sizeof(float) * ((size_t)T * ctx + 4 * T * HD + 16);
  // Large launches: two workgroups per CU already saturate HBM (isolated time unchanged), and the LDS padding that
  // enforces it leaves registers for the other streams' GEMM workgroups to run beside the attention instead of queueing
  // behind it: -4 % per step at B = 1024.
  // (only when a workgroup streams enough by itself — 384 KB for stt-1b; with stt-2.6b's 96 KB per (slot, head) two
  // workgroups per CU starve HBM: +5 %)
  if ((long)B * H >= 2048 && (size_t)2 * ctx * HD * sizeof(KVT) >= (size_t)256 * 1024) lds += e->attn_lds_pad;
  if (lds > 64 * 1024) {  // beyond the default dynamic-LDS limit (long rings, or the padding)
    static size_t allowed = 0;
    if (lds > allowed) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_kernel<KVT, HD, T, UNR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      allowed = lds;
    }
  }
  const int tag = e->tag_attn[e->sid(st)];
  if (T == 1 && HD == 64 && ctx <= 32) {  // short rings (the DepFormer's): one wave per (slot, head)
    const int ph = e->prof_begin(tag, st);
    hipLaunchKernelGGL((attn_small_kernel<KVT, 64>), dim3((B * H + 3) / 4), dim3(256), 0, st, out, q, reinterpret_cast<const KVT*>(k),
                       reinterpret_cast<const KVT*>(v), start_pos, active, B * H, H, ctx, d, fq);
    e->prof_end(ph, st);
    HIPCHK(hipGetLastError());
    return 0;
  }
  const int ph = e->prof_begin(tag, st);
  hipLaunchKernelGGL((attn_kernel<KVT, HD, T, UNR>), dim3(B * H), dim3(256), lds, st, out, q, reinterpret_cast<const KVT*>(k),
                     reinterpret_cast<const KVT*>(v), start_pos, active, H, ctx, d, e->dev_ts_slot(tag, e->sid(st), 0), fq);
  e->prof_end(ph, st);
  HIPCHK(hipGetLastError());
  return 0;
}

template <typename KVT>
int launch_attn(DsmDevice* e, hipStream_t st, float* out, const float* q, const void* k, const void* v,
                const uint32_t* start_pos, const uint8_t* active, int B, int H, int hd, int T, int ctx, int d,
                const AttnFused& fq) {
#define DSM_ATTN(HDv, Tv) \
  if (hd == HDv && T == Tv) return launch_attn_t<KVT, HDv, Tv>(e, st, out, q, k, v, start_pos, active, B, H, ctx, d, fq);
  DSM_ATTN(32, 1) DSM_ATTN(64, 1) DSM_ATTN(128, 1) DSM_ATTN(32, 2) DSM_ATTN(64, 2) DSM_ATTN(128, 2)
#undef DSM_ATTN
  e->set_error("unsupported attention shape head_dim=%d T=%d (head_dim must be 32, 64 or 128; T 1 or 2)", hd, T);
  return DSM_ERR_INVALID;
}

int run_norm(DsmDevice* e, hipStream_t st, float* y, const float* x, const float* w, const float* b, int rows, int d,
             int rms) {
  hipLaunchKernelGGL(row_norm_kernel, dim3(rows), dim3(256), 0, st, y, x, w, b, rows, d, norm_eps(rms), rms);
  HIPCHK(hipGetLastError());
  return 0;
}

// Layer l of a transformer stack from the point where its self-attention output sits in act.att, for M = B * T rows: out_proj
// (+ layer scale, residual) with norm2 — or norm_cross and the cross-attention block, then norm2 — the gated or plain FFN, and
// ff_out with the next layer's norm1.  The last layer's output may be redirected to (final_out, final_map) and followed by the
// model's output norm (post_norm_w / post_norm_out).  Every norm is fused behind the GEMM that produces its input (split-K reduce
// + residual + norm in one row-wise kernel).  Written once for both attention fronts: the ring of transformer_forward and the
// whole-clip attention of spk_encode_body (dsm_speaker.inc).
template <typename WT, typename KVT>
int transformer_layer_tail(DsmDevice* e, hipStream_t st, const TransformerW& w, int l, const ActScratch& act, int B, int T,
                           float* final_out, RowMap final_map, const float* post_norm_w, float* post_norm_out, const CaState* ca) {
  const dsm_transformer_config& c = w.cfg;
  const int d = c.d_model, H = c.num_heads, hd = d / H, M = B * T;
  const TLayerW& L = w.layers[l];
  const bool last = (l == c.num_layers - 1);
  {
    GemmArgs a = base_args(L.out_proj, act.att, plain_map(M, d), M);
    a.scale = L.ls1;
    a.res = act.x; a.rmap = plain_map(M, d);
    a.Y = act.x; a.ymap = plain_map(M, d);
    if (ca) set_norm(a, L.ncw, L.ncb, act.xn, w.ca_norm_rms);  // norm_cross follows instead of norm2 — core/transformer.rs:755-757
    else set_norm(a, L.n2w, L.n2b, act.xn, c.norm);            // norm2
    if (int rc = gemm_store<WT>(e, st, a)) return rc;
  }
  if (ca) {  // xs = residual + cross_attn.forward(norm_cross(xs), ca_src) — core/transformer.rs:753-760, :320-352
    AttnFused none{};
    none.nt = sizeof(KVT) == 2;  // as for the self-attention (transformer_forward)
    none.src = ca->src[l];       // each row's block: private, or a voice it shares (read from device memory at every replay);
                                 // the launch below passes no cache base, which is what sends the kernel to the table
    {
      GemmArgs a = base_args(L.ca_q, act.xn, plain_map(M, d), M);  // in_proj_q, (b, t, H, hd)
      a.Y = act.q; a.ymap = plain_map(M, d);
      // T = 1 and slabs left by the plan: the ordered slab sum of the query runs in the attention kernel's prologue (r04)
      Slabs sl;
      if (int rc = gemm_store<WT>(e, st, a, true, T == 1 && e->fuse_qkv ? &sl : nullptr)) return rc;
      if (sl.ws) {
        none.ws = sl.ws; none.ld = sl.ld; none.cstride = sl.cstride; none.chunks = sl.chunks;
        none.q_only = 1;
      }
    }
    // softmax(q k^T hd^-1/2) v over the row's source, no mask: the self-attention kernel on a "ring" that holds the
    // projected source, every row of it visible (canonical order as for the ring)
    if (int rc = launch_attn<KVT>(e, st, ca->att, act.q, nullptr, nullptr, ca->last, ca->act, B, H, hd, T, ca->smax, d, none)) return rc;
    GemmArgs a = base_args(L.ca_out, ca->att, plain_map(M, d), M);  // out_proj; gating = Normal
    a.res = act.x; a.rmap = plain_map(M, d);
    a.Y = act.x; a.ymap = plain_map(M, d);
    set_norm(a, L.n2w, L.n2b, act.xn, c.norm);  // norm2
    if (int rc = gemm_store<WT>(e, st, a)) return rc;
  }
  if (c.gating) {  // Mlp::Gating — core/batched_transformer.rs:170-176
    GemmArgs a = base_args(L.ff_in, act.xn, plain_map(M, d), M);
    a.N = w.hidden;
    a.nt_stride = w.hidden;
    a.Y = act.g; a.ymap = plain_map(M, w.hidden);
    if (int rc = launch_gemm<WT, KVT, EPI_GATE, 2>(e, st, a, true)) return rc;
  } else {  // Mlp::NoGating — :169
    GemmArgs a = base_args(L.ff_in, act.xn, plain_map(M, d), M);
    a.act = 1;
    a.Y = act.g; a.ymap = plain_map(M, w.hidden);
    if (int rc = gemm_store<WT>(e, st, a)) return rc;
  }
  GemmArgs a = base_args(L.ff_out, act.g, plain_map(M, w.hidden), M);
  a.scale = L.ls2;
  a.res = act.x; a.rmap = plain_map(M, d);
  if (last && final_out) {
    a.Y = final_out; a.ymap = final_map;
  } else {
    a.Y = act.x; a.ymap = plain_map(M, d);
  }
  if (!last) set_norm(a, w.layers[l + 1].n1w, w.layers[l + 1].n1b, act.xn, c.norm);  // the next layer's norm1
  else if (post_norm_out) set_norm(a, post_norm_w, nullptr, post_norm_out, c.norm);    // e.g. LmModel::out_norm — core/lm.rs:1002
  return gemm_store<WT>(e, st, a);
}

// batched_transformer::StreamingTransformer::forward_ca — core/batched_transformer.rs:425-459, the streaming stack
// act.x [B*T][d] is updated in place; the last layer's output may be redirected to (final_out, final_map).
// This function's own: the head (ring bookkeeping in kv_builder_kernel, the first norm) and per layer the ring front — the QKV
// projection that scatters into the ring and the attention over it.  The rest of each layer is transformer_layer_tail, shared
// with the whole-clip encoder.
// phase: 0 = the whole stack; 1 = only the head of it — ring bookkeeping, first norm, layer 0's QKV projection and attention
// (what a stream group runs before it lets the next group start: the staggered start of lm_step); 2 = everything after that.
template <typename WT, typename KVT>
int transformer_forward(DsmDevice* e, hipStream_t st, const TransformerW& w, TransformerState& s, const ActScratch& act, int B,
                        int T, const uint8_t* d_mask, float* final_out, RowMap final_map, const float* post_norm_w = nullptr,
                        float* post_norm_out = nullptr, int phase = 0, const CaState* ca = nullptr, bool head_done = false) {
  const dsm_transformer_config& c = w.cfg;
  const int d = c.d_model, H = c.num_heads, hd = d / H, M = B * T;
  if (phase != 2 && !head_done) {  // head_done: the caller's own kernel did the ring bookkeeping and norm1 of layer 0 (dep_head_kernel)
    hipLaunchKernelGGL(kv_builder_kernel, dim3(B), dim3(64), 0, st, s.pos, s.idx, d_mask, s.start_pos, s.widx,
                       c.positional_embedding == 1 ? s.rope_cs : (float*)nullptr, w.inv_freq, B, T, c.context, hd,
                       w.rope_pos_before ? 1 : 0);
    HIPCHK(hipGetLastError());
    if (int rc = run_norm(e, st, act.xn, act.x, w.layers[0].n1w, w.layers[0].n1b, M, d, c.norm)) return rc;
  }
  for (int l = 0; l < c.num_layers; ++l) {
    const TLayerW& L = w.layers[l];
    AttnFused fq{};
    // Non-temporal K / V loads for the bf16 rings (the LM's): a ring is read once per step and all of them together are far
    // larger than the Infinity Cache, so they should not evict the weights the other stream group reads next.  Measured:
    // LM attention 1410 -> 1336 us/step at B = 64 (38.0 -> 36.7 us per launch alone), 31.4 -> 29.3 ms at B = 2048 (6.9 TB/s),
    // stt-2.6b 4704 -> 4560 us; the f32 rings of Mimi (T = 2) get 6-13 % SLOWER with it and keep ordinary loads.
    fq.nt = sizeof(KVT) == 2;
    if (!(phase == 2 && l == 0)) {
      GemmArgs a = base_args(L.in_proj, act.xn, plain_map(M, d), M);
      a.Y = act.q;
      a.d = d; a.hd = hd; a.H = H; a.T = T; a.ctx = c.context;
      a.kcache = s.k[l]; a.vcache = s.v[l];
      a.widx = s.widx;
      a.rope_cs = c.positional_embedding == 1 ? s.rope_cs : nullptr;
      a.active = d_mask;
      // T = 1 and slabs left by the plan: the ordered reduce + RoPE + ring scatter run in the attention kernel's prologue
      Slabs sl;
      if (int rc = launch_gemm<WT, KVT, EPI_QKV, 1>(e, st, a, true, T == 1 && e->fuse_qkv ? &sl : nullptr)) return rc;
      if (sl.ws) {
        fq.ws = sl.ws; fq.ld = sl.ld; fq.cstride = sl.cstride; fq.chunks = sl.chunks;
        fq.rope_cs = a.rope_cs;
        fq.widx = s.widx;
      }
      if (int rc = launch_attn<KVT>(e, st, act.att, act.q, s.k[l], s.v[l], s.start_pos, d_mask, B, H, hd, T, c.context, d, fq)) return rc;
    }
    if (phase == 1) return 0;
    if (int rc = transformer_layer_tail<WT, KVT>(e, st, w, l, act, B, T, final_out, final_map, post_norm_w, post_norm_out, ca)) return rc;
  }
  return 0;
}

// The ring element type of an LM as a template argument: f(uint16_t{}) for bf16 rings (kv_bf16), f(float{}) for f32 ones.
template <typename F>
int with_kv_type(bool kv_bf16, F&& f) {
  return kv_bf16 ? f(uint16_t{}) : f(float{});
}

// Stream groups: group 0 runs on `st` (the model stream), group g > 0 on s_grp[g].  fork_groups lets the group streams start
// behind what `st` holds so far; run_groups launches body(g, stream) for the trailing groups first — `st` is the stream later
// work queues behind — and records each group's "done" event; join_groups makes `st` wait for them.
int fork_groups(DsmDevice* e, hipStream_t st, size_t G) {
  if (G > 1) {
    HIPCHK(hipEventRecord(e->ev_fork, st));
    for (size_t g = 1; g < G; ++g) HIPCHK(hipStreamWaitEvent(e->s_grp[g], e->ev_fork, 0));
  }
  return 0;
}
template <typename F>
int run_groups(DsmDevice* e, hipStream_t st, size_t G, bool serialize, F&& body) {
  for (size_t g = G; g-- > 0;) {
    hipStream_t gs = (g == 0 || serialize) ? st : e->s_grp[g];
    if (int rc = body(g, gs)) return rc;
    if (g > 0) HIPCHK(hipEventRecord(e->ev_grp_done[g], gs));
  }
  return 0;
}
int join_groups(DsmDevice* e, hipStream_t st, size_t G) {
  for (size_t g = 1; g < G; ++g) HIPCHK(hipStreamWaitEvent(st, e->ev_grp_done[g], 0));
  return 0;
}

// SeaNetEncoder — core/seanet.rs:292-302 — over B items of r frames each (the per-frame geometries with T scaled by r): init conv,
// per stage the residual block (ELU -> conv k3 -> ELU -> conv k1, + skip; :140-150) and the downsampling conv, then the final conv
// into (out, omap).  The one chain of both paths: the step path runs it for B slots of one frame, the clip path once per clip of
// r frames with cat_init pointing at that clip.  front_done: the caller's own kernel already ran the init conv and stage 0's
// residual block (seanet_front_kernel).
int seanet_encode(DsmDevice* e, hipStream_t st, const MimiW& w, SeanetEnc& s, const float* cat_init, int B, int r, float* out,
                  RowMap omap, bool front_done = false) {
  const RowMap none = plain_map(1, 1);
  const size_t n = w.stages.size();
  const ConvGeom g0 = over_frames(w.init_conv, r), gf = over_frames(w.final_conv, r);
  if (!front_done)
    if (int rc = run_conv(e, st, g0, cat_init, B, s.stages[0].y, plain_map(B * g0.T_out, g0.out_c), s.stages[0].cat_ra,
                          cat_map(over_frames(w.stages[0].ra, r)), nullptr, none))
      return rc;
  for (size_t i = 0; i < n; ++i) {
    const ConvGeom ra = over_frames(w.stages[i].ra, r), rb = over_frames(w.stages[i].rb, r), dn = over_frames(w.stages[i].down, r);
    SeanetEnc::Stage& ss = s.stages[i];
    if (!(i == 0 && front_done)) {
      if (int rc = run_conv(e, st, ra, ss.cat_ra, B, nullptr, none, ss.cat_rb, cat_map(rb), nullptr, none)) return rc;
      if (int rc = run_conv(e, st, rb, ss.cat_rb, B, nullptr, none, ss.cat_down, cat_map(dn), ss.y, plain_map(B * rb.T_out, rb.out_c)))
        return rc;
    }
    if (i + 1 < n) {
      if (int rc = run_conv(e, st, dn, ss.cat_down, B, s.stages[i + 1].y, plain_map(B * dn.T_out, dn.out_c), s.stages[i + 1].cat_ra,
                            cat_map(over_frames(w.stages[i + 1].ra, r)), nullptr, none))
        return rc;
    } else if (int rc = run_conv(e, st, dn, ss.cat_down, B, nullptr, none, s.cat_final, cat_map(gf), nullptr, none)) {
      return rc;
    }
  }
  return run_conv(e, st, gf, s.cat_final, B, out, omap, nullptr, none, nullptr, none);
}

int mimi_encode_body(dsm_engine* e, int side, hipStream_t st);
// Mimi::encode_step — core/mimi.rs:195-206.  PCM already sits in cat_init[:, S:, :], mask in s.mask.
int mimi_encode(dsm_engine* e, int side, hipStream_t st) {
  return run_captured(e, *e->g_enc[side], st, (uint64_t)e->sid(st), [&] { return mimi_encode_body(e, side, st); });
}
int mimi_encode_body(dsm_engine* e, int side, hipStream_t st) {
  const MimiW& w = e->mimi_w;
  MimiState& s = e->mimi[side];
  const int B = e->B;
  const RowMap none = plain_map(1, 1);
  e->tag_gemm[e->sid(st)] = DSM_PROF_GEMM_MIMI;
  e->tag_attn[e->sid(st)] = DSM_PROF_ATTN_MIMI;
  // The real Mimi front end (1 -> 64 k 7, residual block 64 -> 32 k 3 -> 64 k 1, f32, frames a multiple of 64) runs as one
  // kernel whose intermediates stay in LDS (seanet_front_kernel); any other geometry takes seanet_encode's three GEMM launches.
  bool fused_front = false;
  {
    const MimiW::Stage& s0 = w.stages[0];
    const ConvGeom& c = w.init_conv;
    fused_front = e->fuse_front && c.in_c == 1 && c.k == 7 && c.stride == 1 && c.out_c == 64 && c.S == 6 && !c.lin.bf16 &&
                  s0.ra.k == 3 && s0.ra.stride == 1 && s0.ra.in_c == 64 && s0.ra.out_c == 32 && s0.ra.S == 2 && !s0.ra.lin.bf16 &&
                  s0.rb.k == 1 && s0.rb.stride == 1 && s0.rb.in_c == 32 && s0.rb.out_c == 64 && !s0.rb.lin.bf16 &&
                  c.T_in % 64 == 0 && c.T_out == c.T_in && s0.ra.T_in == c.T_in && s0.rb.T_in == c.T_in && s0.down.in_c == 64 &&
                  s0.down.T_in == c.T_in && !c.replicate && !s0.ra.replicate;
    if (fused_front) {
      SeanetFrontArgs fa;
      fa.cat_init = s.enc.cat_init;
      fa.w0 = reinterpret_cast<const float*>(c.lin.w); fa.b0 = c.lin.bias; fa.ld0 = c.lin.Kpad;
      fa.w1 = reinterpret_cast<const float*>(s0.ra.lin.w); fa.b1 = s0.ra.lin.bias; fa.ld1 = s0.ra.lin.Kpad;
      fa.w2 = reinterpret_cast<const float*>(s0.rb.lin.w); fa.b2 = s0.rb.lin.bias; fa.ld2 = s0.rb.lin.Kpad;
      fa.cat_ra = s.enc.stages[0].cat_ra;
      fa.cat_down = s.enc.stages[0].cat_down;
      fa.T = c.T_in; fa.S0 = c.S; fa.Sd = s0.down.S;
      const int ph = e->prof_begin(e->tag_gemm[e->sid(st)], st);
      hipLaunchKernelGGL(seanet_front_kernel<64>, dim3(c.T_in / 64, B), dim3(256), seanet_front_lds<64>(), st, fa);  // 32-frame tiles: same time (14.85 vs 14.79 ms of encode at B = 2048)
      e->prof_end(ph, st);
      HIPCHK(hipGetLastError());
    }
  }
  const int Tt = w.final_conv.T_out, d = w.cfg.dimension;
  if (int rc = seanet_encode(e, st, w, s.enc, s.enc.cat_init, B, 1, s.act.x, plain_map(B * Tt, d), fused_front)) return rc;
  // ProjectedTransformer::step — core/batched_transformer.rs:584-602; its output lands in the downsample
  // conv's concat buffer
  if (int rc = transformer_forward<float, float>(e, st, w.tr, s.tr, s.act, B, Tt, s.mask, s.cat_ds, cat_map(w.downsample))) return rc;
  if (s.first_call && w.downsample.S > 0) {  // replicate left pad on the module's first call
    hipLaunchKernelGGL(conv_replicate_init_kernel, dim3(B), dim3(256), 0, st, s.h_descs[s.ds_desc], (const uint8_t*)s.keep);
    HIPCHK(hipGetLastError());
  }
  // ConvDownsample1d::step — core/conv.rs:552-554
  if (int rc = run_conv(e, st, w.downsample, s.cat_ds, B, s.latent, plain_map(B, d), nullptr, none, nullptr, none)) return rc;
  // SplitResidualVectorQuantizer::encode — core/quantization.rs:366-378
  const int n_q = w.cfg.quantizer_n_q, qd = w.cfg.quantizer_dim;
  e->tag_gemm[e->sid(st)] = DSM_PROF_RVQ;
  for (int which = 0; which < 2; ++which) {
    const RvqW& r = which == 0 ? w.rvq_first : w.rvq_rest;
    if (r.n_q == 0) continue;
    float* res = which == 0 ? s.res_first : s.res_rest;
    {
      GemmArgs a = base_args(r.input_proj, s.latent, plain_map(B, d), B);
      a.Y = res; a.ymap = plain_map(B, qd);
      if (int rc = gemm_store<float>(e, st, a)) return rc;
    }
    for (int i = 0; i < r.n_q; ++i) {
      const Linear& cb = r.codebooks[i];
      GemmArgs a = base_args(cb, res, plain_map(B, qd), B);
      a.pval = s.pval; a.pidx = s.pidx;
      if (int rc = launch_gemm<float, float, EPI_RVQ, 1>(e, st, a, true)) return rc;
      hipLaunchKernelGGL(rvq_select_kernel, dim3(B), dim3(256), 0, st, s.pval, s.pidx, (cb.N + 15) / 16, B, s.codes, n_q,
                         which == 0 ? 0 : 1 + i, res, reinterpret_cast<const float*>(cb.w), qd, cb.Kpad);
      HIPCHK(hipGetLastError());
    }
  }
  // carried conv state: masked in-place shift of every concat buffer (core/conv.rs:347-367)
  if (!s.h_descs.empty()) {
    // keep: null unless slots were imported before this side's first call (import_slots), and only looked at on that call
    hipLaunchKernelGGL(conv_state_shift_kernel, dim3(B, (unsigned)s.h_descs.size()), dim3(256), 0, st, s.descs, s.mask,
                       s.first_call ? 1 : 0, nullptr, (const uint8_t*)(s.first_call ? s.keep : nullptr));
    HIPCHK(hipGetLastError());
  }
  s.first_call = false;
  return 0;
}

// ---- decode side ---------------------------------------------------------------------------------------
int alloc_dec_state(DsmDevice* e, const MimiW& w, MimiDecState& s, int B) {  // on first use
  if (s.ready) return 0;
  const dsm_mimi_config& c = w.cfg;
  const int dim = c.dimension, T2 = w.dec_init.T_in;
  if (!w.has_decoder) {
    e->set_error("the Mimi checkpoint has no decoder.* tensors: decode_step is unavailable");
    return DSM_ERR_STATE;
  }
  if (int rc = e->dalloc(&s.codes, (size_t)B * c.quantizer_n_q)) return rc;
  if (int rc = e->dalloc(&s.mask, B)) return rc;
  if (int rc = e->dalloc(&s.q_first, (size_t)B * c.quantizer_dim)) return rc;
  if (int rc = e->dalloc(&s.q_rest, (size_t)B * c.quantizer_dim)) return rc;
  if (int rc = e->dalloc(&s.emb, (size_t)B * dim)) return rc;
  if (int rc = e->dalloc(&s.up_carry, (size_t)B * c.downsample_stride * dim)) return rc;
  if (int rc = alloc_act(e, &s.act, (size_t)B * T2, dim, c.transformer.dim_feedforward)) return rc;  // (hidden, or more with gating)
  if (int rc = alloc_transformer_state(e, &s.tr, c.transformer, B, T2, false)) return rc;
  auto add = [&](float* cat, const ConvGeom& g) { add_desc(s.h_descs, cat, g); };  // (no decoder conv pads by replication)
  if (int rc = alloc_cat(e, &s.cat_init, w.dec_init, B)) return rc;
  add(s.cat_init, w.dec_init);
  s.stages.resize(w.dec_stages.size());
  for (size_t i = 0; i < w.dec_stages.size(); ++i) {
    const MimiW::DecStage& st = w.dec_stages[i];
    MimiDecState::Stage& ss = s.stages[i];
    const int T_out = st.T_in * st.stride;
    if (int rc = e->dalloc(&ss.x, (size_t)B * st.T_in * st.in_c)) return rc;
    if (int rc = e->dalloc(&ss.z, (size_t)B * st.T_in * st.k * st.out_c)) return rc;
    if (int rc = e->dalloc(&ss.carry, (size_t)B * (st.k - st.stride) * st.out_c)) return rc;
    if (int rc = e->dalloc(&ss.y, (size_t)B * T_out * st.out_c)) return rc;
    if (int rc = alloc_cat(e, &ss.cat_ra, st.ra, B)) return rc;
    if (int rc = alloc_cat(e, &ss.cat_rb, st.rb, B)) return rc;
    add(ss.cat_ra, st.ra);
    add(ss.cat_rb, st.rb);
  }
  if (int rc = alloc_cat(e, &s.cat_final, w.dec_final, B)) return rc;
  add(s.cat_final, w.dec_final);
  if (int rc = e->dalloc(&s.pcm, (size_t)B * DSM_FRAME_SIZE * c.channels)) return rc;
  if (int rc = e->upload(&s.descs, s.h_descs.data(), s.h_descs.size())) return rc;
  if (int rc = e->halloc(&s.h_pcm_out, (size_t)B * DSM_FRAME_SIZE)) return rc;
  s.graph = e->graph_slot();
  s.ready = true;
  return 0;
}

int mimi_decode_body(DsmDevice* e, const MimiW& w, MimiDecState& s, int B, hipStream_t st);
// Mimi::decode_step — core/mimi.rs:217-225.  codes in s.codes, mask in s.mask; PCM lands in s.pcm.
int mimi_decode(DsmDevice* e, const MimiW& w, MimiDecState& s, int B, hipStream_t st) {
  return run_captured(e, *s.graph, st, (uint64_t)e->sid(st), [&] { return mimi_decode_body(e, w, s, B, st); });
}
int mimi_decode_body(DsmDevice* e, const MimiW& w, MimiDecState& s, int B, hipStream_t st) {
  const dsm_mimi_config& c = w.cfg;
  const int dim = c.dimension, qd = c.quantizer_dim, T2 = w.dec_init.T_in;
  const RowMap none = plain_map(1, 1);
  e->tag_gemm[e->sid(st)] = DSM_PROF_GEMM_MIMI;
  e->tag_attn[e->sid(st)] = DSM_PROF_ATTN_MIMI;
  // SplitResidualVectorQuantizer::decode — core/quantization.rs:380-390
  {
    RvqGatherArgs g;
    g.emb = w.emb_ptrs; g.n_q = c.quantizer_n_q; g.bins = c.quantizer_bins; g.dim = qd; g.ldE = w.rvq_first.codebooks[0].Kpad;
    hipLaunchKernelGGL(rvq_gather_sum_kernel, dim3(B), dim3(256), 0, st, g, s.codes, s.q_first, s.q_rest);
    HIPCHK(hipGetLastError());
    GemmArgs a = base_args(w.rvq_first.output_proj, s.q_first, plain_map(B, qd), B);
    a.Y = s.emb; a.ymap = plain_map(B, dim);
    if (int rc = gemm_store<float>(e, st, a)) return rc;
    if (c.quantizer_n_q > 1) {
      GemmArgs r = base_args(w.rvq_rest.output_proj, s.q_rest, plain_map(B, qd), B);
      r.res = s.emb; r.rmap = plain_map(B, dim);
      r.Y = s.emb; r.ymap = plain_map(B, dim);
      if (int rc = gemm_store<float>(e, st, r)) return rc;
    }
  }
  // ConvTrUpsample1d::step — core/conv.rs:603-605
  hipLaunchKernelGGL(upsample_dw_kernel, dim3(B), dim3(256), 0, st, s.emb, w.upsample_w, s.up_carry, s.act.x, s.mask, dim,
                     c.downsample_stride, 2 * c.downsample_stride, s.first_call ? 0 : 1, s.started);
  HIPCHK(hipGetLastError());
  // decoder_transformer.step; its output lands in the decoder's first conv buffer
  if (int rc = transformer_forward<float, float>(e, st, w.dec_tr, s.tr, s.act, B, T2, s.mask, s.cat_init, cat_map(w.dec_init))) return rc;
  // SeaNetDecoder::step — core/seanet.rs:452-467
  if (int rc = run_conv(e, st, w.dec_init, s.cat_init, B, nullptr, none, s.stages[0].x,
                        plain_map(B * T2, w.dec_init.out_c), nullptr, none))
    return rc;
  for (size_t i = 0; i < w.dec_stages.size(); ++i) {
    const MimiW::DecStage& sw = w.dec_stages[i];
    MimiDecState::Stage& ss = s.stages[i];
    const int M = B * sw.T_in, T_out = sw.T_in * sw.stride;
    {  // StreamableConvTranspose1d::step: GEMM then overlap-add with the carried tail
      GemmArgs a = base_args(sw.up, ss.x, plain_map(M, sw.in_c), M);
      a.Y = ss.z; a.ymap = plain_map(M, sw.k * sw.out_c);
      if (int rc = gemm_store<float>(e, st, a)) return rc;
      OverlapAddArgs o;
      o.z = ss.z; o.bias = sw.up_bias; o.carry = ss.carry; o.active = s.mask;
      o.T = sw.T_in; o.s = sw.stride; o.OC = sw.out_c; o.has_state = s.first_call ? 0 : 1;
      o.Y = ss.y; o.ymap = plain_map(B * T_out, sw.out_c);
      o.Y2 = ss.cat_ra; o.y2map = cat_map(sw.ra);
      o.started = s.started;
      const int per_b = T_out * (sw.out_c / 4);
      hipLaunchKernelGGL(convtr_overlap_add_kernel, dim3((per_b + 255) / 256 < 64 ? (per_b + 255) / 256 : 64, B), dim3(256), 0,
                         st, o);
      HIPCHK(hipGetLastError());
    }
    if (int rc = run_conv(e, st, sw.ra, ss.cat_ra, B, nullptr, none, ss.cat_rb, cat_map(sw.rb), nullptr, none)) return rc;
    if (i + 1 < w.dec_stages.size()) {
      if (int rc = run_conv(e, st, sw.rb, ss.cat_rb, B, nullptr, none, s.stages[i + 1].x, plain_map(B * T_out, sw.out_c), ss.y,
                            plain_map(B * T_out, sw.out_c)))
        return rc;
    } else {
      if (int rc = run_conv(e, st, sw.rb, ss.cat_rb, B, nullptr, none, s.cat_final, cat_map(w.dec_final), ss.y,
                            plain_map(B * T_out, sw.out_c)))
        return rc;
    }
  }
  if (int rc = run_conv(e, st, w.dec_final, s.cat_final, B, s.pcm, plain_map(B * DSM_FRAME_SIZE, c.channels), nullptr, none,
                        nullptr, none))
    return rc;
  if (!s.h_descs.empty()) {
    hipLaunchKernelGGL(conv_state_shift_kernel, dim3(B, (unsigned)s.h_descs.size()), dim3(256), 0, st, s.descs, s.mask,
                       s.first_call ? 1 : 0, s.started, (const uint8_t*)nullptr);
    HIPCHK(hipGetLastError());
  }
  s.first_call = false;
  return 0;
}

// lm_token_scores_kernel over `rows` rows of V logits: staged in LDS while a row fits, read from L2 pass by pass beyond that
int launch_token_scores(DsmDevice* e, hipStream_t st, int rows, const float* logits, int V, const uint32_t* tokens, int top_n, float* lp,
                        uint32_t* top_id, float* top_lp) {
  if (V <= DSM_SCORES_STAGE_MAX)
    hipLaunchKernelGGL(lm_token_scores_kernel<true>, dim3(rows), dim3(256), sizeof(float) * (size_t)V, st, logits, V, tokens, top_n, lp, top_id, top_lp);
  else
    hipLaunchKernelGGL(lm_token_scores_kernel<false>, dim3(rows), dim3(256), 0, st, logits, V, tokens, top_n, lp, top_id, top_lp);
  HIPCHK(hipGetLastError());
  return 0;
}

// Text bias: slot's trie node = `node`, on `st`.  Nothing to do until the section's buffers exist (a slot attached later
// takes its node from dsm_asr_set_bias).
int bias_put_node(dsm_engine* e, hipStream_t st, int slot, uint32_t node) {
  if (!e->bias_slot_node) return 0;
  hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(64), 0, st, e->bias_slot_node + slot, node, 1L);
  HIPCHK(hipGetLastError());
  return 0;
}

// lm_pick_biased_kernel over `rows` rows of V <= DSM_SCORES_STAGE_MAX logits (the callers check), staged in dynamic LDS
int launch_pick_biased(DsmDevice* e, hipStream_t st, int rows, const float* logits, int V, float temperature, const uint32_t* rng_key,
                       unsigned long long* rng_pos, const BiasSetDesc* sets, const uint32_t* slot_set, uint32_t* slot_node,
                       uint32_t* text_out, uint32_t* text_token, uint8_t* first_step, const uint8_t* active) {
  const size_t lds = sizeof(float) * (size_t)V;
  if (temperature > 0.0f)
    hipLaunchKernelGGL(lm_pick_biased_kernel<true>, dim3(rows), dim3(256), lds, st, logits, V, temperature, rng_key, rng_pos, sets, slot_set,
                       slot_node, text_out, text_token, first_step, active);
  else
    hipLaunchKernelGGL(lm_pick_biased_kernel<false>, dim3(rows), dim3(256), lds, st, logits, V, temperature, rng_key, rng_pos, sets, slot_set,
                       slot_node, text_out, text_token, first_step, active);
  HIPCHK(hipGetLastError());
  return 0;
}

// asr::State::step_tokens device part — core/asr.rs:165-217, for the slots [b0, b0+nb) of one stream group.
// Part 1 (eager, three launches): the group's private mask copy, token shift + pad select + embedding sum, next_codebooks
// update; it ends with the event that tells the model stream the step's shared inputs (codes, mask) are consumed.
// Part 2 (hipGraph once settled): transformer, out_norm, text linear, argmax, extra heads — every argument is an engine
// buffer or the caller's output pointers (part of the capture key).
int lm_group_body(dsm_engine* e, hipStream_t st, int g, uint32_t* d_text_out, float* d_prs_out, int phase) {
  const dsm_asr_config& c = e->cfg;
  LmState& s = e->lm;
  const LmW& w = e->lm_w;
  LmState::Group& grp = s.groups[g];
  const int B = e->B, d = c.lm.d_model, b0 = grp.b0, nb = grp.nb;
  e->tag_gemm[e->sid(st)] = DSM_PROF_GEMM_LM;
  e->tag_attn[e->sid(st)] = DSM_PROF_ATTN_LM;
  uint8_t* gmask = s.gmask + b0;
  const ActScratch sc = s.act.from_row(b0, d, w.tr.hidden);
  float* hidden = s.hidden + (size_t)b0 * d;
  int rc = with_kv_type(c.kv_bf16 != 0, [&](auto kv) {
    return transformer_forward<uint16_t, decltype(kv)>(e, st, w.tr, grp.view, sc, nb, 1, gmask, nullptr, plain_map(1, 1), w.out_norm, hidden, phase);
  });
  if (rc || phase == 1) return rc;  // hidden = out_norm(x) — core/lm.rs:1002 (fused behind the last layer's linear_out)
  float* logits = s.logits + (size_t)b0 * c.text_out_vocab_size;
  {
    GemmArgs a = base_args(w.text_linear, hidden, plain_map(nb, d), nb);
    a.Y = logits; a.ymap = plain_map(nb, c.text_out_vocab_size);
    if ((rc = gemm_store<uint16_t>(e, st, a))) return rc;
  }
  if (e->bias_on) {  // dsm_asr_set_text_bias: one launch in place of the two below
    if ((rc = launch_pick_biased(e, st, nb, logits, c.text_out_vocab_size, c.temperature, s.rng_key + (size_t)b0 * 8, s.rng_pos + b0,
                                 e->bias_sets_d, e->bias_slot_set + b0, e->bias_slot_node + b0, d_text_out + b0, s.text_token + b0,
                                 s.first_step + b0, gmask)))
      return rc;
  } else if (c.temperature > 0.0f)
    hipLaunchKernelGGL(lm_gumbel_kernel, dim3(nb), dim3(256), 0, st, logits, c.text_out_vocab_size, c.temperature,
                       s.rng_key + (size_t)b0 * 8, s.rng_pos + b0, d_text_out + b0, s.text_token + b0, s.first_step + b0, gmask);
  else
    hipLaunchKernelGGL(lm_argmax_kernel, dim3(nb), dim3(256), 0, st, logits, c.text_out_vocab_size, d_text_out + b0,
                       s.text_token + b0, s.first_step + b0, gmask);
  HIPCHK(hipGetLastError());
  if (e->scores_top_n >= 0) {  // dsm_asr_set_token_scores: always from the raw logits, whichever kernel picked the token
    if ((rc = launch_token_scores(e, st, nb, logits, c.text_out_vocab_size, d_text_out + b0, e->scores_top_n, e->scores_lp + b0,
                                  e->scores_top_id + (size_t)b0 * DSM_SCORES_MAX_TOP, e->scores_top_lp + (size_t)b0 * DSM_SCORES_MAX_TOP)))
      return rc;
  }
  if (c.extra_heads_num > 0 && d_prs_out) {
    const int ehw = c.extra_heads_num * c.extra_heads_dim;
    float* eh = s.eh + (size_t)b0 * ehw;
    GemmArgs a = base_args(w.extra_heads, hidden, plain_map(nb, d), nb);
    a.Y = eh; a.ymap = plain_map(nb, ehw);
    if ((rc = gemm_store<uint16_t>(e, st, a))) return rc;
    int n = nb * c.extra_heads_num;
    hipLaunchKernelGGL(extra_heads_kernel, dim3((n + 255) / 256), dim3(256), 0, st, eh, d_prs_out + b0, nb,
                       c.extra_heads_num, c.extra_heads_dim, B);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// Head of a group's step, launched eagerly: inputs, then (staggered start only) the transformer up to layer 0's attention.
int lm_group_head(dsm_engine* e, hipStream_t st, int g, const uint32_t* d_codes, const uint8_t* d_mask, bool with_prefix) {
  const dsm_asr_config& c = e->cfg;
  LmState& s = e->lm;
  const LmW& w = e->lm_w;
  LmState::Group& grp = s.groups[g];
  const int d = c.lm.d_model, b0 = grp.b0, nb = grp.nb, nc = c.audio_codebooks;
  uint8_t* gmask = s.gmask + b0;
  HIPCHK(hipMemcpyAsync(gmask, d_mask + b0, (size_t)nb, hipMemcpyDeviceToDevice, st));
  float* x = s.act.x + (size_t)b0 * d;
  hipLaunchKernelGGL(lm_input_kernel, dim3(nb, (d + 511) / 512), dim3(256), 0, st, x, w.text_emb, w.audio_emb,
                     d_codes + (size_t)b0 * nc, s.next_cb + (size_t)b0 * nc, s.text_token + b0, s.first_step + b0, gmask, nc, d,
                     c.audio_vocab_size, (uint32_t)c.audio_vocab_size - 1, (uint32_t)c.text_in_vocab_size - 1);
  hipLaunchKernelGGL(lm_next_codebooks_kernel, dim3((nb * nc + 255) / 256), dim3(256), 0, st, d_codes + (size_t)b0 * nc,
                     s.next_cb + (size_t)b0 * nc, gmask, nb, nc);
  HIPCHK(hipGetLastError());
  if (g > 0) HIPCHK(hipEventRecord(e->ev_grp_in[g], st));  // the step's shared inputs (codes, mask) are consumed
  if (with_prefix)
    if (int rc = lm_group_body(e, st, g, nullptr, nullptr, 1)) return rc;
  return 0;
}

// Rest of the group's step: one hipGraph once settled.  Capture key: the stream's workspace slot, the caller's output
// pointers (everything else is engine-owned), whether the head already ran the transformer's prefix, and the token-scores
// setting (off adds nothing to the key; each top_n is a body of its own, since it is a launch argument), and the text-bias
// switch (off adds nothing either; on is another pick kernel).
int lm_group_rest(dsm_engine* e, hipStream_t st, int g, uint32_t* d_text_out, float* d_prs_out, bool after_prefix) {
  const uint64_t key = (uint64_t)e->sid(st) ^ ((uint64_t)(uintptr_t)d_text_out << 3) ^ ((uint64_t)(uintptr_t)d_prs_out * 0x9E3779B97F4A7C15ull) ^
                       (after_prefix ? 0x8000000000000000ull : 0ull) ^ ((uint64_t)(e->scores_top_n + 1) * 0xD6E8FEB86659FD93ull) ^
                       (e->bias_on ? 0xA24BAED4963EE407ull : 0ull);
  return run_captured(e, *e->g_grp[g], st, key, [&] { return lm_group_body(e, st, g, d_text_out, d_prs_out, after_prefix ? 2 : 0); });
}

// Before the model stream overwrites anything a group reads at the start of its step (codes, mask), every group must
// have consumed the previous step's copy.
int wait_group_inputs(dsm_engine* e) {
  if (!e->grp_busy) return 0;
  for (size_t g = 1; g < e->lm.groups.size(); ++g) HIPCHK(hipStreamWaitEvent(e->s_model, e->ev_grp_in[g], 0));
  return 0;
}
// Model stream waits until every group finished its last step (slot resets, position edits).
int join_groups(dsm_engine* e) { return e->grp_busy ? join_groups(e, e->s_model, e->lm.groups.size()) : 0; }

// One LM step of the whole batch: group 0 on `st` (the model stream), the others forked onto their own streams.
// Groups are NOT joined at the end of the step: each consumes only its own slots' state, so they free-run and one
// group's attention (HBM-bound) overlaps another's GEMMs (MFMA-bound).  dsm_sync / the host-pointer entry points
// synchronise every group stream.
// after(g, stream): what a caller enqueues behind each group's step on that group's stream (dsm_asr_run's record launch).
template <typename After>
int lm_step_then(dsm_engine* e, hipStream_t st, const uint32_t* d_codes, const uint8_t* d_mask, uint32_t* d_text_out,
                 float* d_prs_out, After&& after) {
  const size_t G = e->lm.groups.size();
  if (int rc = fork_groups(e, st, G)) return rc;
  // Staggered start (r02).  Groups that begin a step together stay in phase through all the layers — their attention
  // launches run against each other (two HBM-bound kernels halving each other's bandwidth: 60 us live against 39 alone at
  // B = 64) and so do their GEMMs — which is the opposite of what the groups are for.  So group g starts only when group
  // g-1 has launched its layer-0 attention: from then on one group's attention runs beside the other's GEMMs.  The head of
  // each group's step (inputs + transformer prefix) is launched eagerly so that the event between the groups is an
  // ordinary stream event; the rest replays as a graph.  The delay costs each later group one QKV + attention per step.
  // Measured (experiments/large_batch_sweep.py, r02): -4 % per step at B = 1024, -3 % at 2048, -2 % at 512, nothing at
  // 400, +3 % at 64 (there the delay is not repaid): on from 256 slots per group.
  const bool stagger = G > 1 && !e->serialize_groups && e->lm.groups[0].nb >= 256;
  for (size_t g = 0; g < G; ++g) {
    hipStream_t gs = (g == 0 || e->serialize_groups) ? st : e->s_grp[g];
    if (stagger && g > 0) HIPCHK(hipStreamWaitEvent(gs, e->ev_stagger[g - 1], 0));
    if (int rc = lm_group_head(e, gs, (int)g, d_codes, d_mask, stagger)) return rc;
    if (stagger && g + 1 < G) HIPCHK(hipEventRecord(e->ev_stagger[g], gs));
  }
  if (int rc = run_groups(e, st, G, e->serialize_groups, [&](size_t g, hipStream_t gs) {
        if (int rc = lm_group_rest(e, gs, (int)g, d_text_out, d_prs_out, stagger)) return rc;
        return after((int)g, gs);
      }))
    return rc;
  if (G > 1) e->grp_busy = true;
  return 0;
}
int lm_step(dsm_engine* e, hipStream_t st, const uint32_t* d_codes, const uint8_t* d_mask, uint32_t* d_text_out,
            float* d_prs_out) {
  return lm_step_then(e, st, d_codes, d_mask, d_text_out, d_prs_out, [](int, hipStream_t) { return 0; });
}

int upload_pcm(dsm_engine* e, int side, hipStream_t st, const float* src, hipMemcpyKind kind) {
  const ConvGeom& c = e->mimi_w.init_conv;
  MimiState& s = e->mimi[side];
  size_t dpitch = sizeof(float) * (size_t)(c.S + c.T_in) * c.in_c;
  size_t width = sizeof(float) * (size_t)c.T_in * c.in_c;
  HIPCHK(hipMemcpy2DAsync(s.pcm, dpitch, src, width, width, e->B, kind, st));
  return 0;
}

void push_msg(dsm_engine* e, dsm_asr_msg m, const std::vector<uint32_t>* toks, const std::vector<float>* lps = nullptr) {
  if (m.kind == DSM_MSG_WORD && toks) {
    m.tokens_offset = (int)e->msg_tokens.size();
    m.n_tokens = (int)toks->size();
    e->msg_tokens.insert(e->msg_tokens.end(), toks->begin(), toks->end());
    e->msg_logprobs.insert(e->msg_logprobs.end(), lps->begin(), lps->end());
  }
  e->msgs.push_back(m);
}

// host half of step_tokens: word assembly — core/asr.rs:218-252
// logprobs: the step's token scores [B], or null while they are off (the tokens then carry NaN, "not recorded")
void assemble_words(dsm_engine* e, const uint32_t* text_tokens, const uint8_t* mask, const float* logprobs) {
  const dsm_asr_config& c = e->cfg;
  e->msgs.clear();
  e->msg_tokens.clear();
  e->msg_logprobs.clear();
  e->model_step_idx += 1;
  if (c.extra_heads_num > 0) {
    dsm_asr_msg m;
    memset(&m, 0, sizeof m);
    m.kind = DSM_MSG_STEP;
    m.step_idx = (int)e->model_step_idx;
    push_msg(e, m, nullptr);
  }
  for (int b = 0; b < e->B; ++b) {
    if (!mask[b]) continue;
    HostItem& it = e->items[b];
    const uint32_t text_token = text_tokens[b];
    it.step_idx += 1;
    if (it.step_idx >= (size_t)c.asr_delay_in_tokens) {
      if (text_token == 3 || text_token == 0) {
        if (!it.word_tokens.empty()) {
          dsm_asr_msg m;
          memset(&m, 0, sizeof m);
          m.kind = DSM_MSG_WORD;
          m.batch_idx = b;
          m.time = it.last_stop_time;
          push_msg(e, m, &it.word_tokens, &it.word_logprobs);
          it.word_tokens.clear();
          it.word_logprobs.clear();
          it.unended_word = true;
        }
      } else {
        it.word_tokens.push_back(text_token);
        it.word_logprobs.push_back(logprobs ? logprobs[b] : dsm_u32_as_f32(0x7FC00000u));
      }
      if (text_token == 0) {
        double stop_time = (double)(it.step_idx - (size_t)c.asr_delay_in_tokens) / 12.5;
        if (it.unended_word) {
          it.unended_word = false;
          dsm_asr_msg m;
          memset(&m, 0, sizeof m);
          m.kind = DSM_MSG_END_WORD;
          m.batch_idx = b;
          m.time = stop_time;
          push_msg(e, m, nullptr);
        }
        it.last_stop_time = stop_time;
      }
    }
  }
}

// The model-side Mimi state (asr::State's own clone, core/asr.rs:58) comes into being with the first step_pcm: a fresh state is a
// reset state, so resets and position jumps issued before that have nothing to do.  Called BEFORE the API's shared lock is taken:
// the allocation (hipMalloc + null-stream memset) must not run beside another thread's graph capture, so it takes the exclusive
// side like a capture does.
int ensure_model_side_mimi(dsm_engine* e) {
  if (e->mimi1_ready.load(std::memory_order_acquire)) return 0;
  std::lock_guard<std::mutex> one(e->mimi1_mu);
  if (e->mimi1_ready.load(std::memory_order_acquire)) return 0;
  std::unique_lock<std::shared_mutex> alone(e->api_mu);
  if (int rc = alloc_mimi_state(e, &e->mimi[1], e->mimi_w, e->B)) return rc;
  e->mimi1_ready.store(true, std::memory_order_release);
  return 0;
}

int reset_transformer_slot(DsmDevice* e, hipStream_t st, TransformerState& s, int slot) {
  HIPCHK(hipMemsetAsync(s.pos + slot, 0, sizeof(uint32_t), st));  // core/kv_cache.rs:111-117
  HIPCHK(hipMemsetAsync(s.idx + slot, 0, sizeof(uint32_t), st));
  return 0;
}

// One slot of the decode state: conv states, convtr carries and the upsampler's carry zeroed.  fresh: the slot's next frame is
// the first of a Mimi of its own (the TTS engine: srv/tts.rs:499-500 clone() + reset_state()) — not started, and the decoder
// transformer back at position 0.
int reset_decoder_slot(DsmDevice* e, const MimiW& w, MimiDecState& d, hipStream_t st, int slot, bool fresh) {
  hipLaunchKernelGGL(conv_state_reset_kernel, dim3((unsigned)d.h_descs.size()), dim3(256), 0, st, d.descs, slot);
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < w.dec_stages.size(); ++i) {
    const size_t n = (size_t)(w.dec_stages[i].k - w.dec_stages[i].stride) * w.dec_stages[i].out_c;
    HIPCHK(hipMemsetAsync(d.stages[i].carry + (size_t)slot * n, 0, n * sizeof(float), st));
  }
  const size_t n = (size_t)w.cfg.downsample_stride * w.cfg.dimension;
  HIPCHK(hipMemsetAsync(d.up_carry + (size_t)slot * n, 0, n * sizeof(float), st));
  if (!fresh) return 0;
  HIPCHK(hipMemsetAsync(d.started + slot, 0, 1, st));
  return reset_transformer_slot(e, st, d.tr, slot);
}

int reset_mimi_slot(dsm_engine* e, int side, hipStream_t st, int slot) {  // Mimi::reset_batch_idx — core/mimi.rs:236-244
  if (side == 1 && !e->mimi1_ready.load(std::memory_order_acquire)) return 0;  // not in being yet: born reset
  MimiState& s = e->mimi[side];
  if (int rc = reset_transformer_slot(e, st, s.tr, slot)) return rc;
  // ingest: the side's history of the slot is cleared (a slot that has not started reads zeros); its format stays
  if (e->ingest_fmt.ready) HIPCHK(hipMemsetAsync(e->ingest_started[side] + slot, 0, sizeof(uint32_t), st));
  if (!s.h_descs.empty()) {
    hipLaunchKernelGGL(conv_state_reset_kernel, dim3((unsigned)s.h_descs.size()), dim3(256), 0, st, s.descs, slot);
    HIPCHK(hipGetLastError());
  }
  if (s.keep && s.first_call && s.keep_h[slot]) {  // an imported slot reset before the side's first call is a fresh slot again
    s.keep_h[slot] = 0;
    HIPCHK(hipMemsetAsync(s.keep + slot, 0, 1, st));
  }
  // decode side of the same Mimi: the decoder transformer is NOT reset (the reference resets encoder_transformer twice
  // instead: core/mimi.rs:237-238)
  if (side == 0 && e->dec.ready) return reset_decoder_slot(e, e->mimi_w, e->dec, st, slot, false);
  return 0;
}

// BASELINE.md bytes_step(): weights once + per-stream KV / embedding / pcm traffic.  Uses full-context KV
// (steady state); the bench reports the exact fill it ran with.
double lm_algorithmic_bytes(const dsm_engine* e) {
  const dsm_asr_config& c = e->cfg;
  const double d = c.lm.d_model, L = c.lm.num_layers, hid = gating_hidden(c.lm);
  const double H = c.lm.num_heads, hd = d / H, ctx = c.lm.context;
  double w = 2.0 * (L * (3 * d * d + d * d + 2 * hid * d + hid * d + 2 * d) + c.text_out_vocab_size * d + d +
                    (double)c.extra_heads_num * c.extra_heads_dim * d);
  double kvb = c.kv_bf16 ? 2.0 : 4.0;
  double per = L * 2 * H * hd * ctx * kvb + L * 2 * H * hd * kvb + (c.audio_codebooks + 1) * d * 2.0;
  return w + e->B * per;
}

}  // namespace

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
// Mimi encode side of SURVEY.md §8(d)'s bytes_step: every encoder weight once (f32) + per stream the PCM frame and
// the full encoder-transformer ring (K and V, f32)
double mimi_enc_algorithmic_bytes(const dsm_engine* e) {
  const MimiW& w = e->mimi_w;
  double bytes = 0;
  auto add = [&](const Linear& L) { bytes += (double)L.N * L.K * (L.bf16 ? 2.0 : 4.0); };
  add(w.init_conv.lin); add(w.final_conv.lin); add(w.downsample.lin);
  for (const auto& st : w.stages) { add(st.ra.lin); add(st.rb.lin); add(st.down.lin); }
  for (const auto& L : w.tr.layers) { add(L.in_proj); add(L.out_proj); add(L.ff_in); add(L.ff_out); }
  for (const RvqW* r : {&w.rvq_first, &w.rvq_rest}) {
    add(r->input_proj);
    for (const auto& cb : r->codebooks) add(cb);
  }
  const dsm_transformer_config& t = w.cfg.transformer;
  const double kv = (double)t.num_layers * 2 * t.d_model * t.context * 4.0;
  return bytes + e->B * (DSM_FRAME_SIZE * 4.0 + kv);
}

extern "C" {

void dsm_mimi_config_v0_1(dsm_mimi_config* out, int num_codebooks) { dsm_preset_mimi_v0_1(out, num_codebooks); }
void dsm_asr_config_stt_1b_en_fr(dsm_asr_config* out) { dsm_preset_stt_1b_en_fr(out); }
void dsm_asr_config_stt_2_6b_en(dsm_asr_config* out) { dsm_preset_stt_2_6b_en(out); }

}  // extern "C" (reopened below)

// The end of every create function: a failed create leaves its message in g_create_error and no engine behind (the context's
// destructor releases whatever the partial create was handed).
template <typename E>
static int finish_create(E* e, int rc, E** out) {
  if (rc) {
    g_create_error = e->err;
    delete e;
    e = nullptr;
  }
  *out = e;
  return rc;
}

extern "C" {

const char* dsm_last_error(const dsm_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

void dsm_destroy(dsm_engine* e) { delete e; }  // ~DsmDevice releases what the engine was handed

// Mimi + LM weights through whatever weight mode the engine is in (dsm_engine::WeightMode); lm / mimi are null when attaching
static int load_all_weights(dsm_engine* e, dsm_st_file* lm, dsm_st_file* mimi) {
  const dsm_asr_config& c = e->cfg;
  const int d = c.lm.d_model;
  {
    Loader ld{e, mimi};
    int rc = load_mimi(e, ld, &e->mimi_w, c.mimi);
    if (rc) return rc;
    if (ld.failed) return DSM_ERR_IO;
  }
  Loader ld{e, lm};
  if (int rc = load_lm_trunk(e, ld, &e->lm_w, c)) return rc;
  if (c.extra_heads_num > 0) {
    std::vector<float> eh((size_t)c.extra_heads_num * c.extra_heads_dim * d);
    for (int i = 0; i < c.extra_heads_num && !ld.failed; ++i) {
      auto w = ld.get((int64_t)c.extra_heads_dim * d, "extra_heads.%d.weight", i);
      memcpy(&eh[(size_t)i * c.extra_heads_dim * d], w.data(), sizeof(float) * w.size());
    }
    if (ld.failed) return DSM_ERR_IO;
    if (int rc = pack_linear(e, &e->lm_w.extra_heads, eh.data(), c.extra_heads_num * c.extra_heads_dim, d, true, nullptr)) return rc;
  }
  return 0;
}

static int create_impl(dsm_engine* e, const dsm_asr_config* cfg, int device_id, int batch_size, const char* lm_path,
                       const char* mimi_path, const void* attach_arena = nullptr, size_t attach_bytes = 0,
                       const uint8_t* attach_manifest = nullptr, size_t attach_manifest_bytes = 0) {
  e->cfg = *cfg;
  e->B = batch_size;
  const dsm_asr_config& c = e->cfg;
  if (batch_size <= 0) { e->set_error("batch_size must be positive"); return DSM_ERR_INVALID; }
  if (c.audio_codebooks > 64 || c.audio_codebooks != c.mimi.quantizer_n_q) {
    e->set_error("audio_codebooks (%d) must equal the Mimi quantizer_n_q (%d) and be <= 64", c.audio_codebooks,
                 c.mimi.quantizer_n_q);
    return DSM_ERR_INVALID;
  }
  if (c.mimi.n_residual_layers != 1) {
    e->set_error("only n_residual_layers = 1 (dilation 1 residual blocks, Mimi v0_1) is supported");
    return DSM_ERR_INVALID;
  }
  if (c.extra_heads_num > DSM_MAX_EXTRA_HEADS) { e->set_error("too many extra heads"); return DSM_ERR_INVALID; }
  if (c.dot_mode != 0 && c.dot_mode != 1) { e->set_error("dot_mode must be 0 (f32 MFMA chain) or 1 (bx3)"); return DSM_ERR_INVALID; }
  for (const dsm_transformer_config* t : {&c.lm, &c.mimi.transformer})
    if (int rc = check_transformer_config(e, *t)) return rc;
  if (int rc = e->open(device_id, c.dot_mode, true)) return rc;
  for (hipEvent_t* ev : {&e->ev_join, &e->ev_codes_consumed})
    if (int rc = e->new_event(ev)) return rc;
  for (hipEvent_t* ev : {&e->ev_a, &e->ev_b, &e->ev_c, &e->ev_d})
    if (int rc = e->new_event(ev, hipEventDefault)) return rc;
  for (auto& gs : e->g_enc) gs = e->graph_slot();
  const int B = batch_size, d = c.lm.d_model;
  // ---- weights: Mimi (f32, core/mimi.rs:261-276) + LM (bf16, srv/batched_asr.rs:738-745) into one arena ----
  if (attach_arena) {
    e->arena = const_cast<char*>(reinterpret_cast<const char*>(attach_arena));
    e->arena_size = attach_bytes;
    e->arena_owned = false;
    e->manifest.assign(attach_manifest, attach_manifest + attach_manifest_bytes);
    e->manifest_pos = 0;
    e->arena_off = 0;
    e->wmode = dsm_engine::W_ATTACH;
    if (int rc = load_all_weights(e, nullptr, nullptr)) return rc;
    if (e->arena_off != e->arena_size || e->manifest_pos != e->manifest.size()) {
      e->set_error("received weight arena does not match this configuration (%zu of %zu bytes, %zu of %zu manifest entries used)",
                   e->arena_off, e->arena_size, e->manifest_pos, e->manifest.size());
      return DSM_ERR_INVALID;
    }
  } else {
    char err[512];
    dsm_st_file* fm = dsm_st_open(mimi_path, err, sizeof err);
    if (!fm) { e->set_error("%s", err); return DSM_ERR_IO; }
    dsm_st_file* fl = dsm_st_open(lm_path, err, sizeof err);
    if (!fl) { dsm_st_close(fm); e->set_error("%s", err); return DSM_ERR_IO; }
    e->wmode = dsm_engine::W_MEASURE;
    e->arena_off = 0;
    int rc = load_all_weights(e, fl, fm);
    if (rc == 0) {
      e->arena_size = e->arena_off;
      void* p = nullptr;
      hipError_t he = hipMalloc(&p, e->arena_size);
      if (he != hipSuccess) { e->set_error("hipMalloc of the %zu-byte weight arena failed: %s", e->arena_size, hipGetErrorString(he)); rc = DSM_ERR_DEVICE; }
      else {
        e->arena = reinterpret_cast<char*>(p);
        e->arena_owned = true;
        he = hipMemset(p, 0, e->arena_size);  // the padding between carves is part of what a broadcast ships: defined bytes
        if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
        if (he != hipSuccess) { e->set_error("clearing the weight arena failed: %s", hipGetErrorString(he)); rc = DSM_ERR_DEVICE; }
      }
    }
    if (rc == 0) {
      e->wmode = dsm_engine::W_LOAD;
      e->arena_off = 0;
      e->manifest.clear();
      rc = load_all_weights(e, fl, fm);
      if (rc == 0) HIPCHK(hipStreamSynchronize(nullptr));  // the uploads ran on the null stream; the engine's streams are not ordered against it
    }
    dsm_st_close(fl);
    dsm_st_close(fm);
    if (rc) return rc;
  }
  e->wmode = dsm_engine::W_PLAIN;
  if (int rc = alloc_mimi_state(e, &e->mimi[0], e->mimi_w, B)) return rc;  // mimi[1]: ensure_model_side_mimi, on first use
  LmState& s = e->lm;
  const int hid = c.lm.gating ? gating_hidden(c.lm) : c.lm.dim_feedforward;
  if (int rc = alloc_act(e, &s.act, B, d, hid)) return rc;
  if (int rc = e->dalloc(&s.hidden, (size_t)B * d)) return rc;
  if (int rc = e->dalloc(&s.logits, (size_t)B * c.text_out_vocab_size)) return rc;
  if (int rc = e->dalloc(&s.eh, (size_t)B * (c.extra_heads_num * c.extra_heads_dim + 1))) return rc;
  if (int rc = e->dalloc(&s.prs, (size_t)B * (c.extra_heads_num + 1))) return rc;
  if (int rc = e->dalloc(&s.next_cb, (size_t)B * c.audio_codebooks)) return rc;
  if (int rc = e->dalloc(&s.text_token, B)) return rc;
  if (int rc = e->dalloc(&s.text_out, B)) return rc;
  if (int rc = e->dalloc(&s.codes_in, (size_t)B * c.audio_codebooks)) return rc;
  if (int rc = e->dalloc(&s.first_step, B)) return rc;
  if (int rc = e->dalloc(&s.rng_key, (size_t)B * 8)) return rc;
  if (int rc = e->dalloc(&s.rng_pos, B)) return rc;
  {  // default seeds: slot b draws from seed_from_u64(0x5EED0000 + b) until dsm_asr_set_seed says otherwise
    std::vector<uint32_t> keys((size_t)B * 8);
    for (int b = 0; b < B; ++b) dsm_seed_from_u64(0x5EED0000ull + (uint64_t)b, &keys[(size_t)b * 8]);
    HIPCHK(hipMemcpy(s.rng_key, keys.data(), sizeof(uint32_t) * keys.size(), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  if (int rc = e->dalloc(&s.mask, B)) return rc;
  if (int rc = alloc_transformer_state(e, &s.tr, c.lm, B, 1, c.kv_bf16 != 0)) return rc;
  if (int rc = e->dalloc(&s.gmask, B)) return rc;
  {
    // stream groups (see LmState::Group).  Default: two groups once each still fills 16-row MFMA tiles twice over;
    // DSM_LM_GROUPS overrides (1..4) for experiments.
    int G = dsm_env_int("DSM_LM_GROUPS", B >= 32 ? 2 : 1);
    if (G < 1) G = 1;
    if (G > dsm_engine::kMaxGroups) G = dsm_engine::kMaxGroups;
    const int n16 = (B + 15) / 16;
    if (G > n16) G = n16;
    s.groups.resize(G);
    int b0 = 0;
    for (int g = 0; g < G; ++g) {
      int blocks = n16 / G + (g < n16 % G ? 1 : 0);
      int nb = std::min(blocks * 16, B - b0);
      LmState::Group& grp = s.groups[g];
      grp.b0 = b0;
      grp.nb = nb;
      grp.view = group_view(s.tr, c.lm, c.kv_bf16 ? 2 : 4, b0);
      b0 += nb;
      e->g_grp[g] = e->graph_slot();
      if (g > 0)
        if (int rc = e->new_event(&e->ev_grp_in[g])) return rc;
    }
    if (int rc = e->open_groups(G)) return rc;
    for (int g = 0; g + 1 < G; ++g)
      if (int rc = e->new_event(&e->ev_stagger[g])) return rc;
  }
  // State::new — core/asr.rs:65-88: next_codebooks = audio_pad_token, text_token = text_start_token, step_idx = 0
  {
    long n = (long)B * c.audio_codebooks;
    hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->s_model, s.next_cb,
                       (uint32_t)c.audio_vocab_size - 1, n);
    hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, e->s_model, s.text_token,
                       (uint32_t)c.text_in_vocab_size - 1, (long)B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(s.first_step, 1, B, e->s_model));
  }
  e->items.assign(B, HostItem());
  if (int rc = e->halloc(&e->h_pcm, (size_t)B * DSM_FRAME_SIZE)) return rc;
  if (int rc = e->halloc(&e->h_pcm1, (size_t)B * DSM_FRAME_SIZE)) return rc;
  if (int rc = e->halloc(&e->h_mask, (size_t)B)) return rc;
  if (int rc = e->halloc(&e->h_codes, (size_t)B * c.audio_codebooks)) return rc;
  if (int rc = e->halloc(&e->h_text, (size_t)B)) return rc;
  if (int rc = e->halloc(&e->h_prs, (size_t)B * (c.extra_heads_num + 1))) return rc;
  HIPCHK(hipDeviceSynchronize());
  e->metrics.algorithmic_bytes_lm = lm_algorithmic_bytes(e);
  e->metrics.algorithmic_bytes_encode = mimi_enc_algorithmic_bytes(e);
  return 0;
}

int dsm_asr_create(const dsm_asr_config* cfg, int device_id, int batch_size, const char* lm_safetensors,
                   const char* mimi_safetensors, dsm_engine** out) {
  if (!cfg || !out || !lm_safetensors || !mimi_safetensors) {
    g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  dsm_engine* e = new dsm_engine();
  return finish_create(e, create_impl(e, cfg, device_id, batch_size, lm_safetensors, mimi_safetensors), out);
}

int dsm_asr_weight_arena(dsm_engine* e, void** d_arena, size_t* arena_bytes, const uint8_t** manifest, size_t* manifest_bytes) {
  if (!e || !e->arena) return DSM_ERR_INVALID;
  if (d_arena) *d_arena = e->arena;
  if (arena_bytes) *arena_bytes = e->arena_size;
  if (manifest) *manifest = e->manifest.data();
  if (manifest_bytes) *manifest_bytes = e->manifest.size();
  return 0;
}

int dsm_asr_create_from_arena(const dsm_asr_config* cfg, int device_id, int batch_size, const void* d_arena, size_t arena_bytes,
                              const uint8_t* manifest, size_t manifest_bytes, dsm_engine** out) {
  if (!cfg || !out || !d_arena || (!manifest && manifest_bytes)) {
    g_create_error = "null argument";
    return DSM_ERR_INVALID;
  }
  dsm_engine* e = new dsm_engine();
  return finish_create(e, create_impl(e, cfg, device_id, batch_size, nullptr, nullptr, d_arena, arena_bytes, manifest, manifest_bytes), out);
}

// One process, several devices (r04; the reference is one process, srv/main.rs:317-327, and a Rust host has no torch.distributed):
// a second engine on `device_id` whose weights are a device-to-device copy of `src`'s packed arena — no file, no bf16 conversion, no
// packing, no host copy.  Across devices the copy goes over xGMI with hipMemcpyPeerAsync in 256 MB pieces (peer access enabled both
// ways when the devices allow it; the copy works without it, through the host, and says so in the error text only if it fails);
// on the same device it is a plain device copy (two engines, one process: the test of the path on a one-GPU box).  The new engine
// OWNS its arena.  `cfg` may differ from src's in everything that is not baked into the arena (batch size, kv_bf16, dot_mode).
int dsm_asr_create_replica(dsm_engine* src, const dsm_asr_config* cfg, int device_id, int batch_size, dsm_engine** out) {
  if (!src || !out || !src->arena) {
    g_create_error = "null argument (or a source engine without a weight arena)";
    return DSM_ERR_INVALID;
  }
  *out = nullptr;
  const dsm_asr_config c = cfg ? *cfg : src->cfg;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) {
    g_create_error = "no such device";
    return DSM_ERR_DEVICE;
  }
  void* copy = nullptr;
  hipStream_t st = nullptr;
  auto fail = [&](const char* what, hipError_t he) {
    g_create_error = std::string(what) + ": " + hipGetErrorString(he);
    if (st) (void)hipStreamDestroy(st);
    if (copy) (void)hipFree(copy);
    (void)hipGetLastError();
    return DSM_ERR_DEVICE;
  };
  {
    ApiShared api(src);  // nothing rewrites the arena after load, but the source must not be destroyed under the copy
    hipError_t he = hipSetDevice(src->device);
    if (he != hipSuccess) return fail("hipSetDevice(src)", he);
    if ((he = hipDeviceSynchronize()) != hipSuccess) return fail("hipDeviceSynchronize(src)", he);
    if (device_id != src->device) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, device_id, src->device) == hipSuccess && can) {
        (void)hipSetDevice(device_id);
        he = hipDeviceEnablePeerAccess(src->device, 0);
        if (he != hipSuccess && he != hipErrorPeerAccessAlreadyEnabled) return fail("hipDeviceEnablePeerAccess", he);
        (void)hipGetLastError();
      }
      if (hipDeviceCanAccessPeer(&can, src->device, device_id) == hipSuccess && can) {
        (void)hipSetDevice(src->device);
        he = hipDeviceEnablePeerAccess(device_id, 0);
        if (he != hipSuccess && he != hipErrorPeerAccessAlreadyEnabled) return fail("hipDeviceEnablePeerAccess", he);
        (void)hipGetLastError();
      }
    }
    if ((he = hipSetDevice(device_id)) != hipSuccess) return fail("hipSetDevice(dst)", he);
    if ((he = hipMalloc(&copy, src->arena_size)) != hipSuccess) return fail("hipMalloc(arena copy)", he);
    if ((he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", he);
    const size_t piece = (size_t)256 << 20;
    for (size_t o = 0; o < src->arena_size; o += piece) {
      const size_t n = std::min(piece, src->arena_size - o);
      he = device_id != src->device
               ? hipMemcpyPeerAsync((char*)copy + o, device_id, (const char*)src->arena + o, src->device, n, st)
               : hipMemcpyAsync((char*)copy + o, (const char*)src->arena + o, n, hipMemcpyDeviceToDevice, st);
      if (he != hipSuccess) return fail("arena copy", he);
    }
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return fail("arena copy (sync)", he);
    (void)hipStreamDestroy(st);
    st = nullptr;
  }
  dsm_engine* e = new dsm_engine();
  const int rc = create_impl(e, &c, device_id, batch_size, nullptr, nullptr, copy, src->arena_size, src->manifest.data(), src->manifest.size());
  if (rc) {
    g_create_error = e->err;
    dsm_destroy(e);
    (void)hipSetDevice(device_id);
    (void)hipFree(copy);
    return rc;
  }
  e->arena_owned = true;  // attach carved the weights out of `copy`: this engine frees it
  *out = e;
  return 0;
}

int dsm_batch_size(const dsm_engine* e) { return e ? e->B : DSM_ERR_INVALID; }
int dsm_n_q(const dsm_engine* e) { return e ? e->cfg.mimi.quantizer_n_q : DSM_ERR_INVALID; }

int dsm_sync(dsm_engine* e) {
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  HIPCHK(hipStreamSynchronize(e->s_enc));
  HIPCHK(hipStreamSynchronize(e->s_model));
  for (hipStream_t gs : e->s_grp)
    if (gs) HIPCHK(hipStreamSynchronize(gs));
  return 0;
}

int dsm_streams_join(dsm_engine* e) {
  ApiShared api(e);
  HIPCHK(hipEventRecord(e->ev_join, e->s_enc));
  HIPCHK(hipStreamWaitEvent(e->s_model, e->ev_join, 0));
  return 0;
}

static int encode_host(dsm_engine* e, int side, hipStream_t st, const float* pcm, const uint8_t* mask) {
  MimiState& s = e->mimi[side];
  float* stage = side == 0 ? e->h_pcm : e->h_pcm1;  // one pinned staging buffer per side / host thread
  memcpy(stage, pcm, sizeof(float) * (size_t)e->B * DSM_FRAME_SIZE);
  if (int rc = upload_pcm(e, side, st, stage, hipMemcpyHostToDevice)) return rc;
  HIPCHK(hipMemcpyAsync(s.mask, mask, (size_t)e->B, hipMemcpyHostToDevice, st));
  return mimi_encode(e, side, st);
}

int dsm_mimi_encode_step(dsm_engine* e, const float* pcm, const uint8_t* mask, uint32_t* codes_out, int* produced) {
  if (!e || !pcm || !mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  HIPCHK(hipEventRecord(e->ev_a, e->s_enc));
  // the mask must stay valid until the async copy ran: stage it
  static_assert(sizeof(uint8_t) == 1, "");
  std::vector<uint8_t> m(mask, mask + e->B);
  if (int rc = encode_host(e, 0, e->s_enc, pcm, m.data())) return rc;
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

static int step_tokens_host(dsm_engine* e, const uint32_t* d_codes, const uint8_t* mask, uint32_t* text_tokens_out,
                            float* vad_prs_out) {
  LmState& s = e->lm;
  const int nh = e->cfg.extra_heads_num;
  HIPCHK(hipMemcpyAsync(s.mask, mask, (size_t)e->B, hipMemcpyHostToDevice, e->s_model));
  HIPCHK(hipEventRecord(e->ev_c, e->s_model));
  if (int rc = lm_step(e, e->s_model, d_codes, s.mask, s.text_out, nh > 0 ? s.prs : nullptr)) return rc;
  if (int rc = join_groups(e)) return rc;
  HIPCHK(hipEventRecord(e->ev_d, e->s_model));
  HIPCHK(hipMemcpyAsync(e->h_text, s.text_out, sizeof(uint32_t) * (size_t)e->B, hipMemcpyDeviceToHost, e->s_model));
  if (nh > 0)
    HIPCHK(hipMemcpyAsync(e->h_prs, s.prs, sizeof(float) * (size_t)e->B * nh, hipMemcpyDeviceToHost, e->s_model));
  const int top_n = e->scores_top_n;
  if (top_n >= 0) {
    HIPCHK(hipMemcpyAsync(e->h_scores_lp, e->scores_lp, sizeof(float) * (size_t)e->B, hipMemcpyDeviceToHost, e->s_model));
    if (top_n > 0) {
      const size_t n = (size_t)e->B * DSM_SCORES_MAX_TOP;
      HIPCHK(hipMemcpyAsync(e->h_scores_top_id, e->scores_top_id, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, e->s_model));
      HIPCHK(hipMemcpyAsync(e->h_scores_top_lp, e->scores_top_lp, sizeof(float) * n, hipMemcpyDeviceToHost, e->s_model));
    }
  }
  HIPCHK(hipStreamSynchronize(e->s_model));
  if (top_n >= 0) e->scores_host_steps += 1;
  float ms = 0;
  if (hipEventElapsedTime(&ms, e->ev_c, e->ev_d) == hipSuccess) e->metrics.last_lm_us = ms * 1000.0;
  e->metrics.steps_lm += 1;
  if (text_tokens_out) memcpy(text_tokens_out, e->h_text, sizeof(uint32_t) * (size_t)e->B);
  if (vad_prs_out && nh > 0) memcpy(vad_prs_out, e->h_prs, sizeof(float) * (size_t)e->B * nh);
  assemble_words(e, e->h_text, mask, top_n >= 0 ? e->h_scores_lp : nullptr);
  return 0;
}

int dsm_asr_step_tokens(dsm_engine* e, const uint32_t* codes, const uint8_t* mask, uint32_t* text_tokens_out,
                        float* vad_prs_out) {
  if (!e || !mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = wait_group_inputs(e)) return rc;
  std::vector<uint8_t> m(mask, mask + e->B);
  const uint32_t* d_codes;
  if (codes) {
    memcpy(e->h_codes, codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.audio_codebooks);
    HIPCHK(hipMemcpyAsync(e->lm.codes_in, e->h_codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.audio_codebooks,
                          hipMemcpyHostToDevice, e->s_model));
    d_codes = e->lm.codes_in;
  } else {
    if (int rc = dsm_streams_join(e)) return rc;
    d_codes = e->mimi[0].codes;
  }
  return step_tokens_host(e, d_codes, m.data(), text_tokens_out, vad_prs_out);
}

int dsm_asr_step_pcm(dsm_engine* e, const float* pcm, const uint8_t* mask, uint32_t* codes_out,
                     uint32_t* text_tokens_out, float* vad_prs_out) {
  if (!e || !pcm || !mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = ensure_model_side_mimi(e)) return rc;
  ApiShared api(e);
  if (int rc = wait_group_inputs(e)) return rc;
  std::vector<uint8_t> m(mask, mask + e->B);
  if (int rc = encode_host(e, 1, e->s_model, pcm, m.data())) return rc;
  if (codes_out)
    HIPCHK(hipMemcpyAsync(codes_out, e->mimi[1].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToHost, e->s_model));
  return step_tokens_host(e, e->mimi[1].codes, m.data(), text_tokens_out, vad_prs_out);
}

// ---- run-ahead pipeline: encoder thread -> model thread (srv/batched_asr.rs:291,314-522) ----
static int pipe_init(dsm_engine* e) {
  if (e->pipe_ready) return 0;
  const size_t B = (size_t)e->B, nq = (size_t)e->cfg.mimi.quantizer_n_q;
  for (auto& ps : e->pipe) {
    if (int rc = e->halloc(&ps.h_pcm, B * DSM_FRAME_SIZE)) return rc;
    if (int rc = e->halloc(&ps.h_mask, B)) return rc;
    if (int rc = e->dalloc(&ps.d_codes, B * nq)) return rc;
    if (int rc = e->new_event(&ps.ev_done)) return rc;
    if (int rc = e->new_event(&ps.ev_consumed)) return rc;
  }
  e->pipe_ready = true;
  return 0;
}

int dsm_mimi_encode_step_async(dsm_engine* e, const float* pcm, const uint8_t* mask, int* ticket) {
  if (!e || !pcm || !mask || !ticket) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
  HIPCHK(hipSetDevice(e->device));
  // from here to the return no capture of the model thread is in progress (dsm_engine::api_mu): in particular not while
  // this thread waits on ev_consumed, an event last recorded on the stream that thread captures on
  ApiShared api(e);
  int slot;
  {
    std::lock_guard<std::mutex> lk(e->pipe_mu);
    if (int rc = pipe_init(e)) return rc;
    slot = e->pipe_next;
    if (e->pipe[slot].in_flight) {  // the ring is full: the bounded channel of the reference blocks its sender too; here the caller retries
      e->set_error("encode pipeline full: %d frames wait for dsm_asr_step_tokens_ticket", dsm_engine::kPipe);
      return DSM_ERR_STATE;
    }
    e->pipe[slot].in_flight = true;
    e->pipe_next = (slot + 1) % dsm_engine::kPipe;
  }
  dsm_engine::PipeSlot& ps = e->pipe[slot];
  // Any failure below hands the ring entry back (ADVICE r02): without this, four failed calls left four entries in_flight
  // for good and every later call reported "encode pipeline full".  The entry was the ring's newest, so pipe_next steps back.
  struct Rollback {
    dsm_engine* e; int slot; bool armed = true;
    ~Rollback() {
      if (!armed) return;
      std::lock_guard<std::mutex> lk(e->pipe_mu);
      e->pipe[slot].in_flight = false;
      e->pipe_next = slot;
    }
  } rollback{e, slot};
  // the entry was last read by the model stream one lap ago: its codes copy must have been consumed, which also orders
  // the reuse of the pinned staging (its upload ran before that encode)
  HIPCHK(hipEventSynchronize(ps.ev_consumed));
  memcpy(ps.h_pcm, pcm, sizeof(float) * (size_t)e->B * DSM_FRAME_SIZE);
  memcpy(ps.h_mask, mask, (size_t)e->B);
  hipStream_t st = e->s_enc;
  if (int rc = upload_pcm(e, 0, st, ps.h_pcm, hipMemcpyHostToDevice)) return rc;
  HIPCHK(hipMemcpyAsync(e->mimi[0].mask, ps.h_mask, (size_t)e->B, hipMemcpyHostToDevice, st));
  if (int rc = mimi_encode(e, 0, st)) return rc;
  HIPCHK(hipMemcpyAsync(ps.d_codes, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                        hipMemcpyDeviceToDevice, st));
  HIPCHK(hipEventRecord(ps.ev_done, st));
  rollback.armed = false;
  e->metrics.steps_encode += 1;
  *ticket = slot;
  return 0;
}

int dsm_asr_step_tokens_ticket(dsm_engine* e, int ticket, const uint8_t* mask, uint32_t* text_tokens_out, float* vad_prs_out) {
  if (!e || !mask || ticket < 0 || ticket >= dsm_engine::kPipe) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(mask)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  dsm_engine::PipeSlot& ps = e->pipe[ticket];
  {
    std::lock_guard<std::mutex> lk(e->pipe_mu);
    if (!e->pipe_ready || !ps.in_flight) { e->set_error("ticket %d holds no encoded frame", ticket); return DSM_ERR_STATE; }
  }
  // whatever happens below, the ticket is spent: the entry goes back to the encoder side on every exit (a failed step must
  // not leave it in_flight for good); ev_consumed is recorded after whatever part of the step was enqueued
  struct Release {
    dsm_engine* e; dsm_engine::PipeSlot* ps;
    ~Release() {
      (void)hipEventRecord(ps->ev_consumed, e->s_model);
      std::lock_guard<std::mutex> lk(e->pipe_mu);
      ps->in_flight = false;
    }
  } release{e, &ps};
  if (int rc = wait_group_inputs(e)) return rc;
  HIPCHK(hipStreamWaitEvent(e->s_model, ps.ev_done, 0));
  std::vector<uint8_t> m(mask, mask + e->B);
  return step_tokens_host(e, ps.d_codes, m.data(), text_tokens_out, vad_prs_out);  // synchronises the model stream
}

int dsm_mimi_decode_step(dsm_engine* e, const uint32_t* codes, const uint8_t* mask, float* pcm_out, int* produced) {
  if (!e || !codes || !mask) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = alloc_dec_state(e, e->mimi_w, e->dec, e->B)) return rc;
  MimiDecState& s = e->dec;
  hipStream_t st = e->s_enc;
  std::vector<uint8_t> m(mask, mask + e->B);
  HIPCHK(hipMemcpyAsync(s.codes, codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s.mask, m.data(), (size_t)e->B, hipMemcpyHostToDevice, st));
  if (int rc = mimi_decode(e, e->mimi_w, s, e->B, st)) return rc;
  HIPCHK(hipMemcpyAsync(s.h_pcm_out, s.pcm, sizeof(float) * (size_t)e->B * DSM_FRAME_SIZE, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (pcm_out) memcpy(pcm_out, s.h_pcm_out, sizeof(float) * (size_t)e->B * DSM_FRAME_SIZE);
  if (produced) *produced = DSM_FRAME_SIZE;
  return 0;
}

int dsm_mimi_decode_step_dev(dsm_engine* e, const uint32_t* d_codes, const uint8_t* d_mask, float* d_pcm_out) {
  if (!e || !d_codes || !d_mask) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = alloc_dec_state(e, e->mimi_w, e->dec, e->B)) return rc;
  MimiDecState& s = e->dec;
  hipStream_t st = e->s_enc;
  HIPCHK(hipMemcpyAsync(s.codes, d_codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(s.mask, d_mask, (size_t)e->B, hipMemcpyDeviceToDevice, st));
  if (int rc = mimi_decode(e, e->mimi_w, s, e->B, st)) return rc;
  if (d_pcm_out)
    HIPCHK(hipMemcpyAsync(d_pcm_out, s.pcm, sizeof(float) * (size_t)e->B * DSM_FRAME_SIZE, hipMemcpyDeviceToDevice, st));
  return 0;
}

int dsm_asr_poll_msgs(dsm_engine* e, dsm_asr_msg* msgs, int cap, uint32_t* tokens_out, int tokens_cap) {
  if (!e || (!msgs && cap > 0)) return DSM_ERR_INVALID;
  int n = (int)e->msgs.size() < cap ? (int)e->msgs.size() : cap;
  for (int i = 0; i < n; ++i) msgs[i] = e->msgs[i];
  int nt = (int)e->msg_tokens.size() < tokens_cap ? (int)e->msg_tokens.size() : tokens_cap;
  if (tokens_out && nt > 0) memcpy(tokens_out, e->msg_tokens.data(), sizeof(uint32_t) * (size_t)nt);
  return n;
}

// ---- token scores (dsm_token_scores.h) ----
int dsm_asr_set_token_scores(dsm_engine* e, int top_n) {
  if (!e) return DSM_ERR_INVALID;
  if (top_n < -1 || top_n > DSM_SCORES_MAX_TOP) {
    e->set_error("token scores: top_n must be -1 (off) or 0..%d, got %d", DSM_SCORES_MAX_TOP, top_n);
    return DSM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // between steps; the allocation (null-stream fill) must not run beside a capture
  if (top_n >= 0 && !e->scores_lp) {
    const size_t B = (size_t)e->B, n = B * DSM_SCORES_MAX_TOP;
    if (int rc = e->dalloc(&e->scores_top_id, n)) return rc;
    if (int rc = e->dalloc(&e->scores_top_lp, n)) return rc;
    if (int rc = e->halloc(&e->h_scores_lp, B)) return rc;
    if (int rc = e->halloc(&e->h_scores_top_id, n)) return rc;
    if (int rc = e->halloc(&e->h_scores_top_lp, n)) return rc;
    if (int rc = e->dalloc(&e->scores_lp, B)) return rc;  // last: the test above reads it
  }
  if (top_n != e->scores_top_n) e->scores_host_steps = 0;
  e->scores_top_n = top_n;
  return 0;
}

static int scores_on(dsm_engine* e) {
  if (e->scores_top_n >= 0) return 0;
  e->set_error("token scores are off: dsm_asr_set_token_scores turns them on");
  return DSM_ERR_STATE;
}

int dsm_asr_token_scores(dsm_engine* e, float* logprob_out, uint32_t* top_ids_out, float* top_logprobs_out) {
  if (!e || !logprob_out) return DSM_ERR_INVALID;
  if (int rc = scores_on(e)) return rc;
  if (e->scores_host_steps == 0) {
    e->set_error("token scores: no dsm_asr_step_tokens / _step_pcm / _step_tokens_ticket since the setting last changed");
    return DSM_ERR_STATE;
  }
  const int top_n = e->scores_top_n;
  memcpy(logprob_out, e->h_scores_lp, sizeof(float) * (size_t)e->B);
  for (int b = 0; b < e->B && top_n > 0; ++b) {
    if (top_ids_out) memcpy(top_ids_out + (size_t)b * top_n, e->h_scores_top_id + (size_t)b * DSM_SCORES_MAX_TOP, sizeof(uint32_t) * (size_t)top_n);
    if (top_logprobs_out) memcpy(top_logprobs_out + (size_t)b * top_n, e->h_scores_top_lp + (size_t)b * DSM_SCORES_MAX_TOP, sizeof(float) * (size_t)top_n);
  }
  return top_n;
}

int dsm_asr_token_scores_dev(dsm_engine* e, const float** d_logprob, const uint32_t** d_top_ids, const float** d_top_logprobs) {
  if (!e) return DSM_ERR_INVALID;
  if (int rc = scores_on(e)) return rc;
  if (d_logprob) *d_logprob = e->scores_lp;
  if (d_top_ids) *d_top_ids = e->scores_top_id;
  if (d_top_logprobs) *d_top_logprobs = e->scores_top_lp;
  return e->scores_top_n;
}

int dsm_asr_poll_word_scores(dsm_engine* e, float* logprobs_out, int cap) {
  if (!e || (!logprobs_out && cap > 0)) return DSM_ERR_INVALID;
  if (int rc = scores_on(e)) return rc;
  const int n = (int)e->msg_logprobs.size() < cap ? (int)e->msg_logprobs.size() : cap;
  if (n > 0) memcpy(logprobs_out, e->msg_logprobs.data(), sizeof(float) * (size_t)n);
  return n;
}

int dsm_token_scores_host(const float* logits, int V, uint32_t token, int top_n, float* logprob, uint32_t* top_ids, float* top_logprobs) {
  if (!logits || !logprob || V < 1 || token >= (uint32_t)V || top_n < 0 || top_n > DSM_SCORES_MAX_TOP ||
      (top_n > 0 && (!top_ids || !top_logprobs)))
    return DSM_ERR_INVALID;
  dsm_token_scores_row(logits, V, token, top_n, logprob, top_ids, top_logprobs);
  return 0;
}

int dsm_debug_token_scores(dsm_engine* e, const float* logits, int n, int V, const uint32_t* tokens, int top_n, float* logprob_out,
                           uint32_t* top_ids_out, float* top_logprobs_out) {
  if (!e || !logits || !tokens || !logprob_out || n < 1 || V < 1 || V > (1 << 30) || top_n < 0 || top_n > DSM_SCORES_MAX_TOP ||
      (top_n > 0 && (!top_ids_out || !top_logprobs_out)))
    return DSM_ERR_INVALID;  // (V beyond 2^30: the kernel's int indices walk a row 2048 entries at a time)
  for (int i = 0; i < n; ++i)
    if (tokens[i] >= (uint32_t)V) { e->set_error("token %u of row %d is outside the row (V = %d)", tokens[i], i, V); return DSM_ERR_INVALID; }
  HIPCHK(hipSetDevice(e->device));
  std::unique_lock<std::shared_mutex> alone(e->api_mu);  // allocates: never beside a capture
  float *d_logits = nullptr, *d_lp = nullptr, *d_top_lp = nullptr;
  uint32_t *d_tok = nullptr, *d_top_id = nullptr;
  const size_t rows = (size_t)n, top = rows * DSM_SCORES_MAX_TOP;
  int rc = e->dalloc(&d_logits, rows * (size_t)V, false);
  if (!rc) rc = e->dalloc(&d_tok, rows, false);
  if (!rc) rc = e->dalloc(&d_lp, rows, false);
  if (!rc) rc = e->dalloc(&d_top_id, top, false);
  if (!rc) rc = e->dalloc(&d_top_lp, top, false);
  std::vector<uint32_t> h_id(top);
  std::vector<float> h_lp(top);
  hipStream_t st = e->s_model;
  auto run = [&]() -> int {
    HIPCHK(hipMemcpyAsync(d_logits, logits, sizeof(float) * rows * (size_t)V, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tok, tokens, sizeof(uint32_t) * rows, hipMemcpyHostToDevice, st));
    if (int lrc = launch_token_scores(e, st, n, d_logits, V, d_tok, top_n, d_lp, d_top_id, d_top_lp)) return lrc;
    HIPCHK(hipMemcpyAsync(logprob_out, d_lp, sizeof(float) * rows, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_id.data(), d_top_id, sizeof(uint32_t) * top, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_lp.data(), d_top_lp, sizeof(float) * top, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  if (!rc) rc = run();
  for (void* p : {(void*)d_logits, (void*)d_tok, (void*)d_lp, (void*)d_top_id, (void*)d_top_lp}) e->dfree(p);
  if (rc) return rc;
  for (size_t i = 0; i < rows && top_n > 0; ++i) {
    memcpy(top_ids_out + i * (size_t)top_n, &h_id[i * DSM_SCORES_MAX_TOP], sizeof(uint32_t) * (size_t)top_n);
    memcpy(top_logprobs_out + i * (size_t)top_n, &h_lp[i * DSM_SCORES_MAX_TOP], sizeof(float) * (size_t)top_n);
  }
  return 0;
}

int dsm_asr_reset_slot(dsm_engine* e, int slot) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) {
    e->set_error("batch index out of range: %d >= %d", slot, e->B);  // core/asr.rs:258-260
    return DSM_ERR_INVALID;
  }
  if (int rc = e->clip_guard(nullptr)) return rc;
  if (e->clips_on.load(std::memory_order_acquire)) {  // a reset ends the slot's clip
    std::lock_guard<std::mutex> lk(e->clip_mu);
    e->clip_slots[(size_t)slot] = dsm_asr_clip::Slot();
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  e->items[slot] = HostItem();
  hipStream_t st = e->s_model;
  if (int rc = join_groups(e)) return rc;
  if (int rc = reset_transformer_slot(e, st, e->lm.tr, slot)) return rc;
  HIPCHK(hipMemsetAsync(e->lm.first_step + slot, 1, 1, st));
  hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(64), 0, st, e->lm.text_token + slot,
                     (uint32_t)e->cfg.text_in_vocab_size - 1, 1L);
  HIPCHK(hipGetLastError());
  if (int rc = bias_put_node(e, st, slot, 0u)) return rc;  // text bias: the attachment stays, the trie node returns to the root
  return reset_mimi_slot(e, 1, st, slot);
}

// temperature > 0 (core/asr.rs:211-215): the slot's Gumbel-noise stream = ChaCha12 keyed by seed_from_u64(seed), from word 0.
// The reference draws from the device's unseeded generator; a per-slot seed is this engine's (documented) restatement.
int dsm_asr_set_seed(dsm_engine* e, int slot, uint64_t seed) {
  if (!e || slot < 0 || slot >= e->B) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  uint32_t key[8];
  dsm_seed_from_u64(seed, key);
  const unsigned long long zero = 0;
  HIPCHK(hipMemcpy(e->lm.rng_key + (size_t)slot * 8, key, sizeof key, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(e->lm.rng_pos + slot, &zero, sizeof zero, hipMemcpyHostToDevice));
  return dsm_sync(e);
}

int dsm_mimi_reset_slot(dsm_engine* e, int slot) {
  if (!e) return DSM_ERR_INVALID;
  if (slot < 0 || slot >= e->B) {
    e->set_error("batch index out of range: %d >= %d", slot, e->B);
    return DSM_ERR_INVALID;
  }
  if (int rc = e->clip_guard(nullptr)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  return reset_mimi_slot(e, 0, e->s_enc, slot);
}

int dsm_get_metrics(dsm_engine* e, dsm_metrics* out) {
  if (!e || !out) return DSM_ERR_INVALID;
  *out = e->metrics;
  e->fill_graph_metrics(out);
  return 0;
}

int dsm_mimi_encode_step_dev(dsm_engine* e, const float* d_pcm, const uint8_t* d_mask, uint32_t* d_codes_out) {
  if (!e || !d_pcm || !d_mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(nullptr)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  // the previous frame's codes must have been picked up by the model stream before they are overwritten
  if (e->codes_consumed_valid) HIPCHK(hipStreamWaitEvent(e->s_enc, e->ev_codes_consumed, 0));
  if (int rc = upload_pcm(e, 0, e->s_enc, d_pcm, hipMemcpyDeviceToDevice)) return rc;
  HIPCHK(hipMemcpyAsync(e->mimi[0].mask, d_mask, (size_t)e->B, hipMemcpyDeviceToDevice, e->s_enc));
  if (int rc = mimi_encode(e, 0, e->s_enc)) return rc;
  if (d_codes_out)
    HIPCHK(hipMemcpyAsync(d_codes_out, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToDevice, e->s_enc));
  HIPCHK(hipEventRecord(e->ev_join, e->s_enc));
  e->metrics.steps_encode += 1;
  return 0;
}

int dsm_asr_step_tokens_dev(dsm_engine* e, const uint32_t* d_codes, const uint8_t* d_mask, uint32_t* d_text_tokens_out,
                            float* d_vad_prs_out) {
  if (!e || !d_mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(nullptr)) return rc;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = wait_group_inputs(e)) return rc;
  HIPCHK(hipMemcpyAsync(e->lm.mask, d_mask, (size_t)e->B, hipMemcpyDeviceToDevice, e->s_model));
  const uint32_t* codes = d_codes;
  if (!codes) {
    // encoder-thread -> model-thread hand-off (the reference's sync_channel, srv/batched_asr.rs:291): wait for the
    // encode enqueued last on the encoder stream, take a private copy of its codes, and let the next encode go
    HIPCHK(hipStreamWaitEvent(e->s_model, e->ev_join, 0));
    HIPCHK(hipMemcpyAsync(e->lm.codes_in, e->mimi[0].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.audio_codebooks,
                          hipMemcpyDeviceToDevice, e->s_model));
    HIPCHK(hipEventRecord(e->ev_codes_consumed, e->s_model));
    e->codes_consumed_valid = true;
    codes = e->lm.codes_in;
  }
  if (int rc = lm_step(e, e->s_model, codes, e->lm.mask, d_text_tokens_out ? d_text_tokens_out : e->lm.text_out,
                       e->cfg.extra_heads_num > 0 ? (d_vad_prs_out ? d_vad_prs_out : e->lm.prs) : nullptr))
    return rc;
  e->metrics.steps_lm += 1;
  e->model_step_idx += 1;
  return 0;
}

int dsm_asr_step_pcm_dev(dsm_engine* e, const float* d_pcm, const uint8_t* d_mask, uint32_t* d_codes_out,
                         uint32_t* d_text_tokens_out, float* d_vad_prs_out) {
  if (!e || !d_pcm || !d_mask) return DSM_ERR_INVALID;
  if (int rc = e->clip_guard(nullptr)) return rc;
  HIPCHK(hipSetDevice(e->device));
  if (int rc = ensure_model_side_mimi(e)) return rc;
  ApiShared api(e);
  hipStream_t st = e->s_model;
  if (int rc = wait_group_inputs(e)) return rc;
  if (int rc = upload_pcm(e, 1, st, d_pcm, hipMemcpyDeviceToDevice)) return rc;
  HIPCHK(hipMemcpyAsync(e->mimi[1].mask, d_mask, (size_t)e->B, hipMemcpyDeviceToDevice, st));
  if (int rc = mimi_encode(e, 1, st)) return rc;
  if (d_codes_out)
    HIPCHK(hipMemcpyAsync(d_codes_out, e->mimi[1].codes, sizeof(uint32_t) * (size_t)e->B * e->cfg.mimi.quantizer_n_q,
                          hipMemcpyDeviceToDevice, st));
  if (int rc = lm_step(e, st, e->mimi[1].codes, e->mimi[1].mask, d_text_tokens_out ? d_text_tokens_out : e->lm.text_out,
                       e->cfg.extra_heads_num > 0 ? (d_vad_prs_out ? d_vad_prs_out : e->lm.prs) : nullptr))
    return rc;
  e->metrics.steps_encode += 1;
  e->metrics.steps_lm += 1;
  e->model_step_idx += 1;
  return 0;
}

int dsm_prof_enable(dsm_engine* e, unsigned tag_mask) {
  if (!e) return DSM_ERR_INVALID;
  e->prof_mask = tag_mask;
  if (tag_mask && !e->dev_ts) {  // launch-bracket records for dsm_prof_read_device: (min start, max end) per launch
    HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
    if (int rc = e->dalloc(&e->dev_ts, 2 * dsm_engine::kDevTsCap, false)) return rc;
    std::vector<unsigned long long> init(2 * dsm_engine::kDevTsCap);
    for (size_t i = 0; i < dsm_engine::kDevTsCap; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0; }
    HIPCHK(hipMemcpy(e->dev_ts, init.data(), sizeof(unsigned long long) * init.size(), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));  // the engine's streams are not ordered against the null stream
  }
  return 0;
}

int dsm_prof_read(dsm_engine* e, double* total_us, uint64_t* launches) {
  if (!e) return DSM_ERR_INVALID;
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  for (auto& r : e->prof_recs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      e->prof_total_us[r.tag] += ms * 1000.0;
      e->prof_launches[r.tag] += 1;
    }
    e->prof_pool.push_back(r.a);
    e->prof_pool.push_back(r.b);
  }
  e->prof_recs.clear();
  for (int i = 0; i < DSM_PROF_NTAGS; ++i) {
    if (total_us) total_us[i] = e->prof_total_us[i];
    if (launches) launches[i] = e->prof_launches[i];
    e->prof_total_us[i] = 0;
    e->prof_launches[i] = 0;
  }
  return 0;
}

int dsm_lm_stream_groups(dsm_engine* e, int* first_slot, int* n_slots, int cap) {
  if (!e) return DSM_ERR_INVALID;
  const int G = (int)e->lm.groups.size();
  for (int g = 0; g < G && g < cap; ++g) {
    if (first_slot) first_slot[g] = e->lm.groups[g].b0;
    if (n_slots) n_slots[g] = e->lm.groups[g].nb;
  }
  return G;
}

int dsm_debug_serialize_groups(dsm_engine* e, int on) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  e->serialize_groups = on != 0;
  return 0;
}

int dsm_prof_read_device(dsm_engine* e, double* total_us, uint64_t* launches) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  for (int i = 0; i < DSM_PROF_NTAGS; ++i) {
    if (total_us) total_us[i] = 0;
    if (launches) launches[i] = 0;
  }
  const size_t n = e->dev_ts_tags.size();
  if (n) {
    std::vector<unsigned long long> h(2 * n);
    HIPCHK(hipMemcpy(h.data(), e->dev_ts, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost));
    int khz = 100000;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device);
    for (size_t i = 0; i < n; ++i) {
      if (h[2 * i + 1] < h[2 * i]) continue;  // never ran
      if (total_us) total_us[e->dev_ts_tags[i]] += (double)(h[2 * i + 1] - h[2 * i]) * 1000.0 / khz;
      if (launches) launches[e->dev_ts_tags[i]] += 1;
    }
    for (size_t i = 0; i < n; ++i) { h[2 * i] = ~0ull; h[2 * i + 1] = 0; }  // hand the records out again
    HIPCHK(hipMemcpy(e->dev_ts, h.data(), sizeof(unsigned long long) * 2 * n, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  e->dev_ts_tags.clear();
  e->dev_ts_info.clear();
  return 0;
}

// Timeline diagnostics: with `on`, GEMM launches (and their reduce launches) take device-clock brackets like the attention
// kernels do; dsm_prof_timeline_read returns every bracketed launch since the last read as (stream id, kind, tag, start us,
// end us) relative to the earliest start.  Needs dsm_prof_enable with the classes of interest; forces eager launches.
int dsm_prof_timeline(dsm_engine* e, int on) {
  if (!e) return DSM_ERR_INVALID;
  e->timeline = on != 0;
  return 0;
}

int dsm_prof_timeline_read(dsm_engine* e, int* sid, int* kind, int* tag, double* start_us, double* end_us, int cap) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  const size_t n = e->dev_ts_tags.size();
  int out = 0;
  if (n) {
    std::vector<unsigned long long> h(2 * n);
    HIPCHK(hipMemcpy(h.data(), e->dev_ts, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost));
    int khz = 100000;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device);
    unsigned long long t0 = ~0ull;
    for (size_t i = 0; i < n; ++i)
      if (h[2 * i + 1] >= h[2 * i] && h[2 * i] < t0) t0 = h[2 * i];
    for (size_t i = 0; i < n && out < cap; ++i) {
      if (h[2 * i + 1] < h[2 * i]) continue;  // never ran (e.g. a GEMM without a reduce launch)
      sid[out] = e->dev_ts_info[i] >> 8;
      kind[out] = e->dev_ts_info[i] & 0xff;
      tag[out] = e->dev_ts_tags[i];
      start_us[out] = (double)(h[2 * i] - t0) * 1000.0 / khz;
      end_us[out] = (double)(h[2 * i + 1] - t0) * 1000.0 / khz;
      ++out;
    }
    for (size_t i = 0; i < n; ++i) { h[2 * i] = ~0ull; h[2 * i + 1] = 0; }
    HIPCHK(hipMemcpy(e->dev_ts, h.data(), sizeof(unsigned long long) * 2 * n, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  e->dev_ts_tags.clear();
  e->dev_ts_info.clear();
  return out;
}

int dsm_debug_set_positions(dsm_engine* e, uint32_t lm_pos, uint32_t mimi_pos) {
  if (!e) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  auto fill = [&](TransformerState& s, uint32_t pos, int ctx) {
    unsigned g = (unsigned)((e->B + 255) / 256);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(g), dim3(256), 0, e->s_model, s.pos, pos, (long)e->B);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(g), dim3(256), 0, e->s_model, s.idx, pos % (uint32_t)ctx, (long)e->B);
  };
  fill(e->lm.tr, lm_pos, e->cfg.lm.context);
  for (int side = 0; side < 2; ++side)
    if (side == 0 || e->mimi1_ready.load(std::memory_order_acquire)) fill(e->mimi[side].tr, mimi_pos, e->cfg.mimi.transformer.context);
  HIPCHK(hipGetLastError());
  return dsm_sync(e);
}

int dsm_debug_set_text_tokens(dsm_engine* e, const uint32_t* tokens) {
  if (!e || !tokens) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  HIPCHK(hipMemcpy(e->lm.text_token, tokens, sizeof(uint32_t) * (size_t)e->B, hipMemcpyHostToDevice));
  return dsm_sync(e);
}

int dsm_debug_read(dsm_engine* e, const char* name, float* out, size_t cap) {
  if (!e || !name || !out) return DSM_ERR_INVALID;
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  if (int rc = dsm_sync(e)) return rc;
  const float* src = nullptr;
  size_t n = 0;
  const int B = e->B, dim = e->cfg.mimi.dimension;
  int side = 0;
  std::string nm(name);
  if (nm.rfind("mimi1.", 0) == 0) { side = 1; nm = nm.substr(6); }
  else if (nm.rfind("mimi.", 0) == 0) nm = nm.substr(5);
  if (nm == "lm.hidden") { src = e->lm.hidden; n = (size_t)B * e->cfg.lm.d_model; }
  else if (nm == "lm.logits") { src = e->lm.logits; n = (size_t)B * e->cfg.text_out_vocab_size; }
  else if (nm == "latent") { src = e->mimi[side].latent; n = (size_t)B * dim; }
  if (!src) { e->set_error("unknown debug tap %s", name); return DSM_ERR_INVALID; }
  if (n > cap) n = cap;
  HIPCHK(hipMemcpy(out, src, sizeof(float) * n, hipMemcpyDeviceToHost));
  return (int)n;
}

int dsm_debug_gemm_plan(int stt, int dot_mode, int weight_bf16, int epi, int nt, int M, int N, int K, int flags, char* buf, size_t cap) {
  const int knobs[5] = {dot_mode, -1, -1, -1, -1};  // the kind's own knobs in this mode: one query path for both entry points
  return dsm_debug_gemm_plan_knobs(stt, knobs, weight_bf16, epi, nt, M, N, K, flags, buf, cap);
}

}  // extern "C"

namespace {
// knobs[5] of the debug entry points over `base`: -1 keeps base's value; false when a value is none a DSM_* variable could set
bool debug_knobs(const int* knobs, GemmKnobs* k) {
  if (knobs[0] >= 0) k->dot_mode = knobs[0];
  if (knobs[1] >= 0) k->chunk_loop_min_tiles = knobs[1];
  if (knobs[2] >= 0) k->smallk_min_tiles = knobs[2];
  if (knobs[3] >= 0) k->smallk_mt = knobs[3];
  if (knobs[4] >= 0) k->loop_depth = knobs[4];
  return (k->dot_mode == 0 || k->dot_mode == 1) && (k->smallk_mt == 1 || k->smallk_mt == 2 || k->smallk_mt == 4) &&
         (k->loop_depth == 2 || k->loop_depth == 4);
}

// What a consumer of split-K slabs does (AttnFused, LogitSrc), as a plain store: Y[m][n..n+3] = the ordered slab sum.
__global__ __launch_bounds__(256) void debug_slab_sum_kernel(float* Y, RowMap ymap, Slabs s, int M, int N) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int n4 = N >> 2;
  if (i >= (long)M * n4) return;
  const int m = (int)(i / n4), n = (int)(i % n4) * 4;
  const f32x4 v = slab_sum(s.ws + (long)m * s.ld + n, s.cstride, s.chunks);
  float* y = Y + ymap.off(m) + n;
  y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
}

// A host buffer on the device for the length of one dsm_debug_gemm call (plain allocation, handed back by the destructor).
struct DebugBuf {
  DsmDevice* e;
  float* d = nullptr;
  explicit DebugBuf(DsmDevice* e_) : e(e_) {}
  ~DebugBuf() { e->dfree(d); }
  int put(const float* host, size_t n) {
    if (int rc = e->dalloc(&d, n, false)) return rc;
    HIPCHK(hipMemcpy(d, host, sizeof(float) * n, hipMemcpyHostToDevice));
    return 0;
  }
};

// one past the last element rows 0 .. M - 1 of `width` floats reach under a row map; 0 when the map is not one the aid takes
size_t debug_extent(const dsm_debug_rowmap& m, int M, int width) {
  if (m.bstride < 0 || m.rpb < 1 || m.ld < 0 || m.toff < 0) return 0;
  const RowMap r{(long)m.bstride, m.rpb, m.ld, m.toff};
  long hi = 0;
  for (int i = 0; i < M; ++i) hi = std::max(hi, r.off(i) + width);
  return (size_t)hi;
}
// output rows must not overlap each other (two workgroups would race for the shared elements)
bool debug_rows_disjoint(const dsm_debug_rowmap& m, int M, int N) {
  if (m.ld < N) return false;
  return m.bstride == 0 ? m.rpb >= M : m.bstride >= (int64_t)(m.rpb + m.toff) * m.ld;
}
RowMap debug_map(const dsm_debug_rowmap& m) { return RowMap{(long)m.bstride, m.rpb, m.ld, m.toff}; }
}  // namespace

extern "C" {

int dsm_debug_gemm_plan_knobs(int stt, const int* knobs, int weight_bf16, int epi, int nt, int M, int N, int K, int flags, char* buf, size_t cap) {
  if (!knobs || epi < EPI_STORE || epi > EPI_RVQ || (nt != 1 && nt != 2) || M < 1 || N < 1 || K < 1 || !buf || !cap) return DSM_ERR_INVALID;
  GemmKnobs k = gemm_default_knobs(stt != 0, knobs[0] < 0 ? 0 : knobs[0]);  // the defaults of the kind and mode, then the explicit entries
  if (!debug_knobs(knobs, &k)) return DSM_ERR_INVALID;
  GemmQuery q;
  q.weight_bf16 = weight_bf16 != 0;
  q.epi = epi;
  q.NT = nt;
  q.M = M; q.N = N; q.K = K;
  q.Kpad = round_up(K, 32);                // pack_linear
  q.nt_stride = epi == EPI_GATE ? N : 16;  // base_args; the gate's up rows sit `hidden` below its gate rows
  q.aligned = flags & DSM_GEMMQ_ALIGNED;
  q.has_Y = flags & DSM_GEMMQ_Y; q.has_Y2 = flags & DSM_GEMMQ_Y2; q.has_res = flags & DSM_GEMMQ_RES;
  q.has_bias = flags & DSM_GEMMQ_BIAS; q.has_norm = flags & DSM_GEMMQ_NORM;
  q.y_ok4 = flags & DSM_GEMMQ_Y_OK4; q.y2_ok4 = flags & DSM_GEMMQ_Y2_OK4; q.res_ok4 = flags & DSM_GEMMQ_RES_OK4;
  q.y_bstride0 = flags & DSM_GEMMQ_Y_PLAIN;
  q.may_defer = flags & DSM_GEMMQ_MAY_DEFER;
  return gemm_plan_line(plan_gemm(q, k), q.has_norm, buf, cap);
}

int dsm_debug_gemm(dsm_engine* e, dsm_debug_gemm_args* g, char* plan, size_t plan_cap) {
  if (!e) return DSM_ERR_INVALID;
  auto bad = [&](const char* what) { e->set_error("dsm_debug_gemm: %s", what); return DSM_ERR_INVALID; };
  if (!g || !plan || !plan_cap) return bad("null argument");
  const int M = g->M, N = g->N, K = g->K, epi = g->epi;
  if (M < 1 || N < 1 || K < 1 || M > (1 << 20) || N > (1 << 20) || K > (1 << 16)) return bad("M, N or K out of range");
  if (epi == EPI_RVQ) return bad("the RVQ epilogue is not offered (the model tests keep it)");
  if (epi != EPI_STORE && epi != EPI_QKV && epi != EPI_GATE) return bad("no such epilogue");
  if (!g->X || !g->W || !(g->Y || (epi == EPI_STORE && g->Y2))) return bad("X, W and Y (the store epilogue: Y or Y2) are required");
  const bool has_norm = g->norm_out != nullptr;
  if (has_norm && !g->Y) return bad("a row norm needs Y");
  if (epi != EPI_STORE && (g->bias || g->scale || g->res || g->Y2 || has_norm || g->act)) return bad("only the store epilogue has bias, act, scale, res, Y2 and a norm");
  if (epi == EPI_QKV && !g->may_defer) return bad("the direct QKV epilogue is not offered (the model tests keep it)");
  if (g->act != 0 && g->act != 1) return bad("act is 0 or 1");
  if (has_norm && (!g->norm_w || (!g->norm_rms && !g->norm_b) || N % 4 != 0 || g->ymap.bstride != 0 || g->ymap.toff != 0 || g->ymap.ld != N ||
                   g->norm_len < (uint64_t)M * N))
    return bad("a row norm needs its weights, N % 4 == 0, Y as a plain [M][N] matrix and norm_len >= M * N");
  // every row the kernels read or write lies inside the caller's buffers
  const size_t x_ext = debug_extent(g->xmap, M, K);
  if (!x_ext || x_ext > g->x_len) return bad("X rows reach outside x_len");
  if (g->Y) {
    const size_t ext = debug_extent(g->ymap, M, N);
    if (!ext || ext > g->y_len || !debug_rows_disjoint(g->ymap, M, N)) return bad("Y rows overlap or reach outside y_len");
  }
  if (g->Y2) {
    const size_t ext = debug_extent(g->y2map, M, N);
    if (!ext || ext > g->y2_len || !debug_rows_disjoint(g->y2map, M, N)) return bad("Y2 rows overlap or reach outside y2_len");
  }
  if (g->res) {
    const size_t ext = debug_extent(g->rmap, M, N);
    if (!ext || ext > g->res_len) return bad("res rows reach outside res_len");
  }
  HIPCHK(hipSetDevice(e->device));
  ApiShared api(e);
  ApiExclusive alone(e);  // the knobs below are the engine's: nobody else launches while they are changed
  if (int rc = dsm_sync(e)) return rc;

  // the knobs for this call; put back on every way out
  struct Restore {
    DsmDevice* e;
    GemmKnobs k;
    DsmDevice::WeightMode wmode;
    ~Restore() {
      e->dot_mode = k.dot_mode; e->chunk_loop_min_tiles = k.chunk_loop_min_tiles; e->smallk_min_tiles = k.smallk_min_tiles;
      e->smallk_mt = k.smallk_mt; e->loop_depth = k.loop_depth;
      e->wmode = wmode;
    }
  } restore{e, gemm_knobs(e), e->wmode};
  GemmKnobs k = restore.k;
  if (!debug_knobs(g->knobs, &k)) return bad("knobs: dot_mode 0 / 1, smallk_mt 1 / 2 / 4, loop_depth 2 / 4");
  e->dot_mode = k.dot_mode; e->chunk_loop_min_tiles = k.chunk_loop_min_tiles; e->smallk_min_tiles = k.smallk_min_tiles;
  e->smallk_mt = k.smallk_mt; e->loop_depth = k.loop_depth;

  // the weight, packed as load time packs it, in plain device memory of this call
  struct TmpLinear {
    DsmDevice* e;
    Linear L;
    ~TmpLinear() { e->dfree(L.w); e->dfree(L.bias); }
  } w{e, Linear{}};
  const bool gate = epi == EPI_GATE, bf16 = g->weight_bf16 != 0;
  e->wmode = DsmDevice::W_PLAIN;
  if (int rc = pack_linear(e, &w.L, g->W, gate ? 2 * N : N, K, bf16, g->bias, gate ? N : 0)) return rc;
  e->wmode = restore.wmode;
  const size_t w_bytes = (size_t)w.L.Npad * w.L.Kpad * (bf16 ? 2 : 4);
  std::vector<uint8_t> w_before(w_bytes), w_after(w_bytes);
  HIPCHK(hipMemcpy(w_before.data(), w.L.w, w_bytes, hipMemcpyDeviceToHost));

  DebugBuf X(e), Y(e), Y2(e), res(e), scale(e), nw(e), nb(e), nout(e);
  if (int rc = X.put(g->X, g->x_len)) return rc;
  if (g->Y) if (int rc = Y.put(g->Y, g->y_len)) return rc;
  if (g->Y2) if (int rc = Y2.put(g->Y2, g->y2_len)) return rc;
  if (g->res) if (int rc = res.put(g->res, g->res_len)) return rc;
  if (g->scale) if (int rc = scale.put(g->scale, N)) return rc;
  if (has_norm) {
    if (int rc = nw.put(g->norm_w, N)) return rc;
    if (!g->norm_rms) if (int rc = nb.put(g->norm_b, N)) return rc;
    if (int rc = nout.put(g->norm_out, g->norm_len)) return rc;
  }
  HIPCHK(hipStreamSynchronize(nullptr));  // the copies above ran on the null stream, which the engine's streams do not wait for

  GemmArgs a = base_args(w.L, X.d, debug_map(g->xmap), M);
  a.N = N;
  if (gate) a.nt_stride = N;
  a.scale = scale.d;
  a.act = g->act;
  a.res = res.d; a.rmap = debug_map(g->rmap);
  a.Y = Y.d; a.ymap = debug_map(g->ymap);
  a.Y2 = Y2.d; a.y2map = debug_map(g->y2map);
  if (has_norm) set_norm(a, nw.d, nb.d, nout.d, g->norm_rms ? 1 : 0);
  const bool aligned = g->xmap.ld % 4 == 0 && g->xmap.bstride % 4 == 0;

  // launch_gemm's own question, asked first: the plan line to hand back, and whether the plan ends in an epilogue the aid offers
  const GemmPlan p = plan_gemm(gemm_query(a, bf16, epi, gate ? 2 : 1, aligned, g->may_defer != 0), k);
  gemm_plan_line(p, has_norm, plan, plan_cap);
  if (p.form == GEMM_NO_FIT) return bad("chunk partials do not fit in LDS");
  // The generic kernel's chunk partials may plan up to 160 KB of dynamic LDS (K > 16384 at MT = 1), but launch_gemm does not raise the
  // kernel's dynamic-LDS limit above the 64 KB every kernel starts with (only the attention launch does), and no engine has a product
  // that large on the generic kernel: what such a launch does has never been run, so the aid does not offer it.
  if (p.lds > 64 * 1024) return bad("a plan with more than 64 KB of dynamic LDS is not offered (launch_gemm never raises the kernel's limit)");
  if (epi == EPI_QKV && p.reduce != GEMM_RED_CONSUMER) return bad("the direct QKV epilogue is not offered (the model tests keep it)");

  hipStream_t st = e->s_model;
  Slabs slabs;
  Slabs* sp = g->may_defer ? &slabs : nullptr;
  int rc;
  if (epi == EPI_QKV) rc = bf16 ? launch_gemm<uint16_t, float, EPI_QKV, 1>(e, st, a, aligned, sp) : launch_gemm<float, float, EPI_QKV, 1>(e, st, a, aligned, sp);
  else if (gate) rc = bf16 ? launch_gemm<uint16_t, float, EPI_GATE, 2>(e, st, a, aligned, sp) : launch_gemm<float, float, EPI_GATE, 2>(e, st, a, aligned, sp);
  else rc = bf16 ? launch_gemm<uint16_t, float, EPI_STORE, 1>(e, st, a, aligned, sp) : launch_gemm<float, float, EPI_STORE, 1>(e, st, a, aligned, sp);
  if (rc) return rc;
  if (slabs.ws) {
    const long n = (long)M * (N >> 2);
    hipLaunchKernelGGL(debug_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Y.d, a.ymap, slabs, M, N);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));

  if (g->Y) HIPCHK(hipMemcpy(g->Y, Y.d, sizeof(float) * g->y_len, hipMemcpyDeviceToHost));
  if (g->Y2) HIPCHK(hipMemcpy(g->Y2, Y2.d, sizeof(float) * g->y2_len, hipMemcpyDeviceToHost));
  if (has_norm) HIPCHK(hipMemcpy(g->norm_out, nout.d, sizeof(float) * g->norm_len, hipMemcpyDeviceToHost));
  if (g->x_back) HIPCHK(hipMemcpy(g->x_back, X.d, sizeof(float) * g->x_len, hipMemcpyDeviceToHost));
  if (g->res && g->res_back) HIPCHK(hipMemcpy(g->res_back, res.d, sizeof(float) * g->res_len, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(w_after.data(), w.L.w, w_bytes, hipMemcpyDeviceToHost));
  g->w_changed = w_before != w_after;
  return 0;
}

}  // extern "C"
