// dsm_gemm_plan.h — which kernel a matrix product gets: the whole decision of the GEMM launcher as one pure function.
//
// plan_gemm(query, knobs) -> plan.  No HIP type and no DsmDevice: the header compiles with a host compiler alone, so which
// shapes reach which kernel form can be read off on the CPU (dsm_debug_gemm_plan, tests/test_gemm_plan_cpu.py).  launch_gemm
// (dsm_engine.hip) fills a query from its GemmArgs, runs plan_gemm and executes the plan; it decides nothing itself.
#ifndef DSM_GEMM_PLAN_H
#define DSM_GEMM_PLAN_H
#include <stddef.h>
#include <stdio.h>

#include "dsm_numerics.h"  // DSM_KC: the K-chunk of the ordered reduction

enum { GEMM_EPI_STORE = 0, GEMM_EPI_QKV = 1, GEMM_EPI_GATE = 2, GEMM_EPI_RVQ = 3 };  // == EPI_* of dsm_kernels.h (asserted in launch_gemm)

// The five numbers of the device context the decision reads, and what they start from with no DSM_* variable set.
struct GemmKnobs {
  int dot_mode = 0;                // 1: every bf16-weight GEMM on the bf16 matrix pipe ("bx3")
  int chunk_loop_min_tiles = 384;  // DSM_CHUNK_LOOP_MIN: whole-K workgroups from this many (n, m) tiles on (swept at B = 512 / 1024: 384 best)
  int smallk_min_tiles = 1024;     // DSM_SMALLK_MIN: one-chunk GEMMs (K <= 256) move to gemm_loop_kernel from this many 64-row tiles on
  int smallk_mt = 4;               // DSM_SMALLK_MT: 16-row tiles per workgroup of those launches
  int loop_depth = 4;              // DSM_LOOP_DEPTH=2: two-block rolling window (fewer registers, three waves per SIMD) where four is the default
};
// dot_mode 1, STT engine only: the bx3 loop is cheaper per tile, so whole-K workgroups pay from 192 (n, m) tiles on (r03 sweep,
// profiles/r03/experiments/chunk_loop_min_mode1.txt: B = 400 13.2 -> 12.0 ms, B = 1024 27.9 -> 26.7).  The TTS engine has always
// kept 384 in both modes; the difference is kept on purpose: dropping it would change which kernels a TTS step launches.
inline GemmKnobs gemm_default_knobs(bool stt, int dot_mode) {
  GemmKnobs k;
  k.dot_mode = dot_mode;
  if (stt && dot_mode == 1) k.chunk_loop_min_tiles = 192;
  return k;
}

// What the decision depends on, and nothing else.
struct GemmQuery {
  bool weight_bf16 = false;
  int epi = GEMM_EPI_STORE;
  int NT = 1;  // n-tiles per wave: 2 for the gate (its gate and up rows), else 1
  int M = 0, N = 0, K = 0, Kpad = 0;
  int nt_stride = 16;    // as the caller set it (16, or the hidden width for the gate)
  bool aligned = false;  // every activation row starts on a multiple of 4 floats
  bool has_Y = false, has_Y2 = false, has_res = false, has_bias = false, has_norm = false;
  bool y_ok4 = false, y2_ok4 = false, res_ok4 = false;  // the row map's ld and bstride are multiples of 4 floats
  bool y_bstride0 = false;                              // ymap.bstride == 0: Y is one plain [M][ld] matrix
  bool may_defer = false;                               // the caller can sum split-K slabs itself (AttnFused, LogitSrc)
};

// One value per launch expression of launch_gemm.  MT (and, for the generic kernel, k_aligned) is the plan's.
enum GemmForm {
  GEMM_MFMA,          // gemm_mfma_kernel<WT, KVT, MT, NT, EPI, AL>: the generic kernel, any K and any row alignment
  GEMM_MFMA_BX3,      // gemm_mfma_kernel<WT, KVT, MT, NT, EPI, AL, true>
  GEMM_TILE,          // gemm_tile_kernel<WT, KVT, MT, NT, EPI>: one K-chunk per workgroup, all loads up front
  GEMM_LOOP2,         // gemm_loop_kernel<WT, KVT, MT, NT, EPI, 2>: whole K in the workgroup, two-block load window
  GEMM_LOOP_DEEP,     // gemm_loop_kernel<WT, KVT, MT, NT, EPI, LoopDepth<WT, NT>::MAX>: four-block window
  GEMM_BX3_LOOP,      // gemm_bx3_kernel<KVT, MT, NT, EPI, true>: whole K in the workgroup
  GEMM_BX3_LOOP_NT2,  // gemm_bx3_kernel<KVT, 4, 2, EPI, true> on 128 weight rows per workgroup: the two-n-tile form
  GEMM_BX3_SPLIT,     // gemm_bx3_kernel<KVT, 4, NT, EPI, false>: split-K, 64-row tiles
  GEMM_BX3U_1,        // gemm_bx3u_kernel<KVT, 1, NT, EPI, 8>: split-K at M <= 16, every load of the chunk up front, 24 KB of LDS
  GEMM_BX3U_2,        // gemm_bx3u_kernel<KVT, 2, NT, EPI, 8, 0, 4>: split-K at 32-row tiles, 48 KB of LDS
  GEMM_WK,            // gemm_wk_kernel<KVT, 1, 2, EPI_GATE, 1, 4, 2, true, 4>: the gate with the whole K in the workgroup
  GEMM_NO_FIT,        // error: the generic kernel's chunk partials do not fit in LDS
};
enum GemmReduce {
  GEMM_RED_NONE,      // nothing to sum: one chunk per workgroup column, or the chunks were summed in the workgroup
  GEMM_RED_CONSUMER,  // the slabs are left to the caller's next kernel
  GEMM_RED_ROWS1,     // gemm_reduce_rows_kernel<1|2|4>: slab sum + epilogue + row norm, one workgroup per row
  GEMM_RED_ROWS2,
  GEMM_RED_ROWS4,
  GEMM_RED_TILES,     // gemm_reduce_kernel<KVT, EPI>: slab sum + epilogue
};

struct GemmPlan {
  GemmForm form = GEMM_NO_FIT;
  bool tiled = false;      // one of the tiled kernels (everything but gemm_mfma_kernel): the launch takes a timeline record
  bool k_aligned = false;  // gemm_mfma_kernel's AL.  Always false today: an aligned product with K % 32 == 0 never reaches that kernel
  int MT = 1;              // 16-row tiles per workgroup
  unsigned gx = 1, gy = 1, gz = 1, block = 256;
  size_t lds = 0;      // dynamic LDS bytes
  int chunks = 1;      // K-chunks across workgroups (grid.y of the tiled kernels): > 1 leaves slabs in the workspace
  int chunk_loop = 0;  // > 1: K-chunks one workgroup walks itself (GemmArgs::chunk_loop)
  int wg_cols = 0, nt_stride = 16, ws_ntiles = 0, vec = 0;  // the GemmArgs fields of the same names
  size_t ws_bytes = 0;  // split-K workspace needed: chunks x M padded to 16 x ws_ntiles * 16 floats, 0 without slabs
  GemmReduce reduce = GEMM_RED_NONE;
  bool row_norm = false;  // row_norm_kernel follows as a launch of its own (the norm could not be fused behind the reduce)
};

inline GemmPlan plan_gemm(const GemmQuery& q, const GemmKnobs& k) {
  GemmPlan p;
  const int kchunks = (q.Kpad + DSM_KC - 1) / DSM_KC;
  // 16-byte epilogue accesses need every row offset to be a multiple of 4 floats
  p.vec = (q.N % 4 == 0) && (!q.has_Y || q.y_ok4) && (!q.has_Y2 || q.y2_ok4) && (!q.has_res || q.res_ok4);
  p.nt_stride = q.nt_stride;

  if (!(q.aligned && q.K % 32 == 0)) {
    // ---- the generic kernel: the tiled ones have no K-tail handling and load activations 16 bytes at a time.  A workgroup
    // holds every K-chunk, one wave each (or several chunks per wave beyond 16), and sums the partials in LDS.
    const int rounds = (kchunks + 15) / 16;            // chunks per wave when there are more than 16
    const int S = (kchunks + rounds - 1) / rounds;     // waves per workgroup
    const int tiles16 = (q.N + 15) / 16;  // for the gate N is the hidden width: one (gate, up) tile pair per block
    const int nx = (q.epi == GEMM_EPI_GATE) ? tiles16 : (tiles16 + q.NT - 1) / q.NT;
    // M-tiles per wave: as many as possible (weights are re-read once per m-group) while the grid still covers
    // the 256 CUs at least twice and the chunk partials fit in LDS
    int MT = (q.NT == 2) ? 2 : 4;  // NT=2 x MT=4 would need > 128 VGPRs (spills under the 1024-thread cap)
    while (MT > 1 && (q.M <= 16 * (MT / 2) || (long)nx * ((q.M + 16 * MT - 1) / (16 * MT)) * S < 2048 ||
                      (kchunks > 1 && (size_t)kchunks * q.NT * MT * 1024 > 64 * 1024)))
      MT /= 2;
    if (kchunks > 1 && (size_t)kchunks * q.NT * MT * 1024 > 160 * 1024) return p;  // GEMM_NO_FIT
    p.form = (k.dot_mode == 1 && q.weight_bf16 && q.epi != GEMM_EPI_RVQ) ? GEMM_MFMA_BX3 : GEMM_MFMA;
    p.k_aligned = q.aligned && (q.K % 32 == 0);  // the fast kernel has no K-tail handling
    p.MT = MT;
    p.gx = nx;
    p.gy = (q.M + 16 * MT - 1) / (16 * MT);
    p.block = 64 * S;
    p.lds = kchunks > 1 ? (size_t)kchunks * q.NT * MT * 1024 : 0;
    p.row_norm = q.has_norm;
    return p;
  }

  p.tiled = true;
  int chunks = kchunks;
  const int gx = (q.N + 63) / 64;
  const bool bx3 = k.dot_mode == 1 && q.weight_bf16;  // dot_mode 1: every bf16-weight GEMM on the bf16 matrix pipe
  // ---- chunk loop.  Enough (n, m) tiles to fill the chip (large batches; the Mimi convs, whose M is B x frames): no
  // split-K across workgroups — each walks the chunks itself and sums them in order in registers, so the slabs
  // (chunks x M x N floats written, then read back by a reduce launch) disappear.
  if (chunks > 1 && (long)gx * ((q.M + 63) / 64) >= k.chunk_loop_min_tiles) {
    p.chunk_loop = chunks;
    chunks = 1;
  }
  // ---- whole-K gate (dsm_gemm_wk.h): dot_mode 1, bf16 weights, at most four K-chunks, M <= 64.  r04: short reductions (the
  // DepFormer's: K = 1024) keep the whole K inside the workgroup — four waves, one chunk each, 16 rows x one (gate, up) tile
  // pair per workgroup, the epilogue behind the ordered LDS sum: no slabs, no reduce launch.  experiments/gemm_wk_probe: gate
  // 7.5 us against 13.4 (10.9 with gemm_bx3u_kernel) at M = 32; at K = 2048 the activation re-read (every workgroup reads
  // 16 x K x 4 bytes from L2) makes it lose (27 against 20 us).
  if (q.epi == GEMM_EPI_GATE && q.NT == 2) {
    const bool wk_applicable = q.weight_bf16 && k.dot_mode == 1 && q.K % 32 == 0 && q.Kpad == q.K && kchunks <= 4 && q.M <= 64;
    if (wk_applicable && chunks > 1 && q.N % 16 == 0) {
      p.form = GEMM_WK;
      p.gx = q.N / 16;
      p.gz = (q.M + 15) / 16;
      p.lds = (size_t)chunks * 2 * 1024;
      return p;
    }
  }
  // ---- MT: 16-row tiles per workgroup
  int MT = q.M > 32 ? 4 : (q.M > 16 ? 2 : 1);
  while (MT > 1 && (long)gx * chunks * ((q.M + 16 * MT - 1) / (16 * MT)) < 256) MT /= 2;  // cover the 256 CUs
  // 33..64 rows, dot_mode 1, a launch of at most 256 workgroups (out_proj of a 2048-wide model): two 32-row z-tiles on
  // gemm_bx3u_kernel instead of one 64-row tile on gemm_bx3_kernel — 12.8 against 15.4 us with its reduce (experiments/gemm_wk_probe 3,
  // form 5); the wider launches (QKV, gate, ff_out) tie or lose that way and keep MT = 4.
  if (MT == 4 && bx3 && chunks > 1 && q.M <= 64 && (long)gx * chunks <= 256 && q.epi == GEMM_EPI_STORE) MT = 2;
  // one K-chunk and thousands of m-tiles (the first SEANet layers at large batches: K = 32..192, M = B x 1920): a
  // workgroup is one short dependent chain — loads, one to six MFMA blocks, residual load, store — so what counts is how
  // many of them a CU holds; gemm_tile_kernel's up-front window of eight blocks costs 200-230 VGPRs (two workgroups per CU),
  // gemm_loop_kernel's two-block window 150 (three).  Mimi encode alone at B = 2048: 17.7 -> 16.6 ms; 8-row tiles no better.
  const bool smallk = chunks == 1 && p.chunk_loop == 0 && (long)gx * ((q.M + 63) / 64) >= k.smallk_min_tiles && !bx3;
  if (smallk && k.smallk_mt < MT) MT = k.smallk_mt;
  // ---- split-K workspace
  p.ws_ntiles = (((q.NT - 1) * q.nt_stride) >> 4) + gx * 4;
  if (chunks > 1) p.ws_bytes = (size_t)chunks * ((q.M + 15) / 16) * p.ws_ntiles * 256 * sizeof(float);
  // ---- the launch
  p.MT = MT;
  p.chunks = chunks;
  p.gx = gx;
  p.gy = chunks;
  p.gz = (q.M + 16 * MT - 1) / (16 * MT);
  // dot_mode 1, whole-K form, plain epilogues, from 256 workgroups on: two n-tiles per wave (128 weight rows per workgroup).  With
  // one n-tile a wave reads 12 LDS fragments (12 KB) per block for 12 MFMAs and the LDS, not the matrix pipe, bounds the loop; the
  // gate has always run two.
  const bool nt2 = q.NT == 1 && bx3 && p.chunk_loop > 1 && MT == 4 && (q.epi == GEMM_EPI_STORE || q.epi == GEMM_EPI_QKV) &&
                   q.N % 128 == 0 && (long)(q.N / 128) * p.gz >= 256;
  const bool roll = p.chunk_loop > 1 || smallk;  // whole K in the workgroup with a rolling load window
  const bool deep = !(q.NT == 2 || !q.weight_bf16) && k.loop_depth == 4 && !smallk;  // LoopDepth<WT, NT>::MAX == 4
  if (nt2) {
    p.form = GEMM_BX3_LOOP_NT2;
    p.gx = q.N / 128;
    p.wg_cols = 128;
    p.nt_stride = 64;
  } else if (bx3 && q.epi != GEMM_EPI_RVQ) {
    // whole K in the workgroup -> gemm_bx3_kernel<.., true>; split-K at M <= 32 -> gemm_bx3u_kernel, which issues every load of
    // its chunk up front (r04; 48 KB of LDS at MT = 2, 24 KB at MT = 1); split-K at MT = 4 -> gemm_bx3_kernel<.., false>
    if (p.chunk_loop > 1) p.form = GEMM_BX3_LOOP;
    else if (MT == 4) p.form = GEMM_BX3_SPLIT;
    else if (MT == 2) { p.form = GEMM_BX3U_2; p.lds = 8 * 3 * 32 * 32 * 2; }
    else { p.form = GEMM_BX3U_1; p.lds = 8 * 3 * 16 * 32 * 2; }
  } else {
    // whole K (roll) -> gemm_loop_kernel with a four- or two-block load window; split-K -> gemm_tile_kernel
    p.form = roll && deep ? GEMM_LOOP_DEEP : (roll ? GEMM_LOOP2 : GEMM_TILE);
  }
  // ---- the reduce.  Slabs are left to the consumer (the attention prologue's ordered sum + RoPE + ring scatter, the sampler's
  // logits) when it asked for them and the product is split-K across workgroups with a plain epilogue: no bias to add, rows of
  // whole float4 groups.  This is the one place that predicate lives; a call site adds only conditions of its own.
  const bool rows_ok = (q.epi == GEMM_EPI_STORE) && q.has_norm && p.vec && !q.has_Y2 && q.has_Y && q.N <= 4096 && q.y_bstride0;
  const bool defer = q.may_defer && chunks > 1 && q.Kpad > DSM_KC && q.K % 32 == 0 && !q.has_bias && q.N % 4 == 0 &&
                     (q.epi == GEMM_EPI_STORE || q.epi == GEMM_EPI_QKV);
  if (chunks > 1) {
    if (defer) p.reduce = GEMM_RED_CONSUMER;
    else if (rows_ok) p.reduce = q.N <= 1024 ? GEMM_RED_ROWS1 : (q.N <= 2048 ? GEMM_RED_ROWS2 : GEMM_RED_ROWS4);
    else p.reduce = GEMM_RED_TILES;
  }
  p.row_norm = q.has_norm && !(chunks > 1 && rows_ok);  // the norm could not be fused: it runs on the stored rows
  return p;
}

// The plan as one line, e.g. "bx3u<2> grid=32x4x2 wg=256 lds=49152 chunks=4 loop=0 reduce=rows2 norm=fused ..." (dsm_debug_gemm_plan)
inline int gemm_plan_line(const GemmPlan& p, bool has_norm, char* buf, size_t cap) {
  char form[32];
  switch (p.form) {
    case GEMM_MFMA: snprintf(form, sizeof form, "mfma<%d,al=%d>", p.MT, p.k_aligned ? 1 : 0); break;
    case GEMM_MFMA_BX3: snprintf(form, sizeof form, "mfma_bx3<%d,al=%d>", p.MT, p.k_aligned ? 1 : 0); break;
    case GEMM_TILE: snprintf(form, sizeof form, "tile<%d>", p.MT); break;
    case GEMM_LOOP2: snprintf(form, sizeof form, "loop2<%d>", p.MT); break;
    case GEMM_LOOP_DEEP: snprintf(form, sizeof form, "loop4<%d>", p.MT); break;
    case GEMM_BX3_LOOP: snprintf(form, sizeof form, "bx3_loop<%d>", p.MT); break;
    case GEMM_BX3_LOOP_NT2: snprintf(form, sizeof form, "bx3_loop_nt2<%d>", p.MT); break;
    case GEMM_BX3_SPLIT: snprintf(form, sizeof form, "bx3_split<%d>", p.MT); break;
    case GEMM_BX3U_1: case GEMM_BX3U_2: snprintf(form, sizeof form, "bx3u<%d>", p.MT); break;
    case GEMM_WK: snprintf(form, sizeof form, "wk"); break;
    case GEMM_NO_FIT: return snprintf(buf, cap, "error: chunk partials do not fit in LDS");
  }
  static const char* const red[] = {"none", "consumer", "rows1", "rows2", "rows4", "tiles"};
  const bool fused = p.reduce == GEMM_RED_ROWS1 || p.reduce == GEMM_RED_ROWS2 || p.reduce == GEMM_RED_ROWS4;
  return snprintf(buf, cap, "%s grid=%ux%ux%u wg=%u lds=%zu chunks=%d loop=%d reduce=%s norm=%s mt=%d wg_cols=%d nt_stride=%d ws_ntiles=%d vec=%d ws=%zu",
                  form, p.gx, p.gy, p.gz, p.block, p.lds, p.chunks, p.chunk_loop, red[p.reduce],
                  p.row_norm ? "separate" : (has_norm && fused ? "fused" : "none"), p.MT, p.wg_cols, p.nt_stride, p.ws_ntiles, p.vec, p.ws_bytes);
}
#endif
