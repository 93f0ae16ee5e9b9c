// dsm_kernels.h — hand-written HIP kernels for gfx950 (MI355X / CDNA4).  Included by dsm_engine.hip.
//
// Every kernel follows the canonical reduction orders of dsm_numerics.h so that its f32
// results are bit-identical to the CPU oracle (oracle/dsm_oracle.c).  Wavefront = 64 lanes.
//
//   gemm_mfma_kernel   Y = X . W^T on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain:
//                      experiments/numerics_probe.hip).  One workgroup = S waves, wave w owns the
//                      K-chunk [512w, 512w+512); chunk partials are summed left to right through
//                      LDS.  Fused epilogues: bias / GELU / layer-scale / residual / ELU copy,
//                      QKV split + RoPE + ring-cache scatter, SiLU gate, RVQ distance + argmin.
//   row_norm_kernel    RMSNorm / LayerNorm, one wave per row, xor-butterfly reductions.
//   attn_kernel        softmax(q.K^T/sqrt(hd) + ring mask).V, one 4-wave workgroup per (slot, head),
//                      K/V streamed once from HBM with 16-byte loads, scores staged in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dsm_numerics.h"
#include "dsm_sampling.h"
#include "dsm_token_scores.h"
#include "dsm_text_bias.h"
#include "dsm_pcm_format.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short dsm_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------------------------
// GEMM
// ------------------------------------------------------------------------------------------
enum { EPI_STORE = 0, EPI_QKV = 1, EPI_GATE = 2, EPI_RVQ = 3 };

struct RowMap {  // row m -> element offset: (m / rpb) * bstride + ((m % rpb) + toff) * ld
  long bstride;
  int rpb;
  int ld;
  int toff;
  __host__ __device__ long off(int m) const { return (long)(m / rpb) * bstride + (long)((m % rpb) + toff) * ld; }
};

struct GemmArgs {
  const float* X;
  RowMap xmap;
  const void* W;  // packed [Npad][Kpad], K zero-padded to a multiple of 32, rows to a multiple of 16
  int Kpad, K, N, M;
  int nt_stride;  // row distance between the NT n-tiles of one wave (16, or `hidden` for the gate)
  int wpacked;    // bf16 W is fragment-major [N / 16][Kpad / 32][64][8] (pack_linear, r04) instead of row-major [N][Kpad]
  int w_ntiles;   // 16-row tiles of W in all (chunk-major experiment, dsm_gemm_wk.h)
  int wg_cols;    // weight rows per workgroup (0 = 64).  128 with nt_stride 64: gemm_bx3_kernel's two-n-tile form for plain
                  // epilogues — wave w owns columns 16w.. and 64 + 16w.. of the workgroup's 128
  // EPI_STORE
  const float* bias;   // [N] or null
  const float* scale;  // [N] or null (LayerScale)
  const float* res;    // residual source or null
  RowMap rmap;
  float* Y;
  RowMap ymap;
  float* Y2;  // optional ELU(y) copy
  RowMap y2map;
  int act;  // 0 none, 1 gelu_erf (applied right after bias)
  int vec;  // 1: every row offset of Y / Y2 / res is a multiple of 4 floats and N % 4 == 0 -> 16-byte accesses
  // EPI_QKV
  int d, hd, H, T, ctx;
  void* kcache;
  void* vcache;               // [B][H][ctx][hd]
  const uint32_t* widx;       // [B*T] ring slot written by row (b,t)
  const float* rope_cs;       // [B*T][hd/2][2] (cos, sin) or null
  const uint8_t* active;      // [B]
  // EPI_RVQ
  float* pval;     // [n_tiles][M]
  uint32_t* pidx;  // [n_tiles][M]
  // split-K workspace of the tiled kernel: [chunks][M padded to 16][ws_ntiles*16] f32, row-major
  float* ws;
  int ws_ntiles;
  int defer_reduce;  // EPI_QKV, T = 1: leave the slabs to the attention kernel's prologue (AttnFused)
  int chunk_loop;    // > 1: one workgroup walks all K-chunks itself (grid.y = 1) and adds the chunk sums left to right in
                     // registers — no slabs, no reduce launch; chosen when the (n, m) tiles alone fill the chip
  // optional row norm fused behind an EPI_STORE GEMM whose N is d_model (gemm_reduce_rows_kernel)
  const float* norm_w;
  const float* norm_b;
  float* norm_out;
  float norm_eps;
  int norm_rms;
  // optional device-clock bracket of the launch (timeline diagnostics, dsm_prof_timeline): {first workgroup in, last out}
  unsigned long long* ts;
};

// Where lane (r, q) finds its 8 consecutive k of weight row n0 + r in the first 32-wide block, and how far apart blocks are
// (elements): row-major, or — bf16 weights since r04 — fragment-major (pack_linear).  n0 is a multiple of 16.
template <typename WT>
__device__ __forceinline__ const WT* dsm_wbase(const GemmArgs& a, const WT* W, int n0, int r, int q) {
  if (sizeof(WT) == 2 && a.wpacked) return W + ((long)(n0 >> 4) * (a.Kpad >> 5)) * 512 + (q * 16 + r) * 8;
  return W + (long)(n0 + r) * a.Kpad + 8 * q;
}
template <typename WT>
__device__ __forceinline__ int dsm_wstep(const GemmArgs& a) { return (sizeof(WT) == 2 && a.wpacked) ? 16 : 1; }  // x k (multiples of 32)

// first / last workgroups of a launch stamp the wall clock (dispatch is in index order; a few hundred atomics at most)
__device__ __forceinline__ void launch_stamp_begin(unsigned long long* ts) {
  if (!ts || threadIdx.x != 0) return;
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (lin < 128) atomicMin(&ts[0], wall_clock64());
}
__device__ __forceinline__ void launch_stamp_end(unsigned long long* ts) {
  if (!ts || threadIdx.x != 0) return;
  const unsigned total = gridDim.x * gridDim.y * gridDim.z;
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (lin + 512 >= total) atomicMax(&ts[1], wall_clock64());
}

template <typename WT>
__device__ __forceinline__ void load_w8(const WT* p, float (&o)[8]);
template <>
__device__ __forceinline__ void load_w8<uint16_t>(const uint16_t* p, float (&o)[8]) {
  uint4 v = *reinterpret_cast<const uint4*>(p);
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xFFFF0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xFFFF0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xFFFF0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xFFFF0000u);
}
template <>
__device__ __forceinline__ void load_w8<float>(const float* p, float (&o)[8]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// 8 consecutive cache elements kept as raw words until they are used (prefetch registers of the attention kernel)
template <typename KVT>
struct Raw8;
typedef unsigned int dsm_u32x4 __attribute__((ext_vector_type(4)));
typedef float dsm_f32x4v __attribute__((ext_vector_type(4)));
template <>
struct Raw8<uint16_t> {
  uint4 v;
  __device__ __forceinline__ void load(const uint16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  // non-temporal: a ring cache is read once per step and is far larger than the Infinity Cache — do not let it evict the
  // weights the other stream group is about to read again
  __device__ __forceinline__ void load_nt(const uint16_t* p) {
    const dsm_u32x4 t = __builtin_nontemporal_load(reinterpret_cast<const dsm_u32x4*>(p));
    v = make_uint4(t[0], t[1], t[2], t[3]);
  }
  __device__ __forceinline__ void unpack(float (&o)[8]) const {
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xFFFF0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xFFFF0000u);
    o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xFFFF0000u);
    o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xFFFF0000u);
  }
};
template <>
struct Raw8<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void load_nt(const float* p) {
    const dsm_f32x4v t0 = __builtin_nontemporal_load(reinterpret_cast<const dsm_f32x4v*>(p));
    const dsm_f32x4v t1 = __builtin_nontemporal_load(reinterpret_cast<const dsm_f32x4v*>(p + 4));
    a = make_float4(t0[0], t0[1], t0[2], t0[3]);
    b = make_float4(t1[0], t1[1], t1[2], t1[3]);
  }
  __device__ __forceinline__ void unpack(float (&o)[8]) const {
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
};

__device__ __forceinline__ void store_kv(uint16_t* p, float v) { *p = dsm_f32_to_bf16(v); }
__device__ __forceinline__ void store_kv(float* p, float v) { *p = v; }

__device__ __forceinline__ void store_kv4(uint16_t* p, const float (&o)[4]) {
  uint2 v;
  v.x = (uint32_t)dsm_f32_to_bf16(o[0]) | ((uint32_t)dsm_f32_to_bf16(o[1]) << 16);
  v.y = (uint32_t)dsm_f32_to_bf16(o[2]) | ((uint32_t)dsm_f32_to_bf16(o[3]) << 16);
  *reinterpret_cast<uint2*>(p) = v;
}
__device__ __forceinline__ void store_kv4(float* p, const float (&o)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- epilogues (shared by the three GEMM kernels).  A lane holds rows n..n+3 of column m of a 16x16 tile. ----
template <typename KVT, int EPI>
__device__ __forceinline__ void epi_store_qkv(const GemmArgs& a, f32x4 v, int m, int n) {
  if (m >= a.M || n >= a.N) return;
  const bool full = a.vec && (n + 3 < a.N);
  if (EPI == EPI_STORE) {
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t = v[i];
      if (n + i < a.N) {
        if (a.bias) t = t + a.bias[n + i];
        if (a.act == 1) t = dsm_gelu_erf(t);
        if (a.scale) t = t * a.scale[n + i];
      }
      o[i] = t;
    }
    if (a.res) {
      const float* rp = a.res + a.rmap.off(m) + n;
      if (full) {
        float4 rv = *reinterpret_cast<const float4*>(rp);
        o[0] = rv.x + o[0]; o[1] = rv.y + o[1]; o[2] = rv.z + o[2]; o[3] = rv.w + o[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < a.N) o[i] = rp[i] + o[i];
      }
    }
    if (a.Y) {
      float* y = a.Y + a.ymap.off(m) + n;
      if (full) {
        *reinterpret_cast<float4*>(y) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < a.N) y[i] = o[i];
      }
    }
    if (a.Y2) {
      float* y2 = a.Y2 + a.y2map.off(m) + n;
      if (full) {
        *reinterpret_cast<float4*>(y2) = make_float4(dsm_elu(o[0]), dsm_elu(o[1]), dsm_elu(o[2]), dsm_elu(o[3]));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < a.N) y2[i] = dsm_elu(o[i]);
      }
    }
  } else {  // EPI_QKV
    // n in [0, 3d): part 0 = q, 1 = k, 2 = v; (b,t,3,H,hd) layout — core/batched_transformer.rs:77-82
    const int part = n / a.d, c = n - part * a.d, h = c / a.hd, i0 = c - h * a.hd;
    const int b = m / a.T;
    float o[4] = {v[0], v[1], v[2], v[3]};
    if (part < 2 && a.rope_cs) {  // rope_i on interleaved pairs — core/transformer.rs:373-377
      const float4 cs = *reinterpret_cast<const float4*>(a.rope_cs + ((long)m * (a.hd / 2) + (i0 >> 1)) * 2);
      const float co[2] = {cs.x, cs.z}, si[2] = {cs.y, cs.w};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float x0 = v[2 * p], x1 = v[2 * p + 1];
        float t0 = x0 * co[p], t1 = x1 * si[p], t2 = x0 * si[p], t3 = x1 * co[p];
        o[2 * p] = t0 - t1;
        o[2 * p + 1] = t2 + t3;
      }
    }
    if (part == 0) {
      *reinterpret_cast<float4*>(a.Y + (long)m * a.d + c) = make_float4(o[0], o[1], o[2], o[3]);
    } else if (a.active[b]) {  // inactive slots: the reference scatters garbage that is never read
      KVT* cache = reinterpret_cast<KVT*>(part == 1 ? a.kcache : a.vcache);
      store_kv4(cache + (((long)b * a.H + h) * a.ctx + a.widx[m]) * a.hd + i0, o);
    }
  }
}

// Mlp::Gating — core/batched_transformer.rs:170-176: silu(first half) * second half
__device__ __forceinline__ void epi_gate(const GemmArgs& a, f32x4 g, f32x4 u, int m, int n) {
  if (m >= a.M || n >= a.N) return;
  float o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = dsm_silu(g[i]) * u[i];
  float* y = a.Y + a.ymap.off(m) + n;
  if (a.vec && n + 3 < a.N) {
    *reinterpret_cast<float4*>(y) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (n + i < a.N) y[i] = o[i];
  }
}

// EuclideanCodebook::encode_slow — core/quantization.rs:122-131: dist = c2 - dot, argmin over the 16 codebook
// rows of this tile (first occurrence on ties); all 64 lanes of the wave must call it.
__device__ __forceinline__ void epi_rvq(const GemmArgs& a, f32x4 v, int m, int n, int tile16, int q) {
  float bv = DSM_INF_F;
  uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float dist = a.bias[n + i] - v[i];
    if (n + i < a.N && (dist < bv || (dist == bv && (uint32_t)(n + i) < bi))) { bv = dist; bi = (uint32_t)(n + i); }
  }
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    float ov = __shfl_xor(bv, off, 64);
    uint32_t oi = __shfl_xor(bi, off, 64);
    if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (q == 0 && m < a.M) {
    a.pval[(long)tile16 * a.M + m] = bv;
    a.pidx[(long)tile16 * a.M + m] = bi;
  }
}

// ---- generic GEMM (any K, any X alignment): one workgroup = S waves, wave w accumulates K-chunks w, w+S, ...
// and parks each chunk's partial tile in LDS; the partials are summed left to right.  Used for the few layers
// the tiled kernel below cannot take (K % 32 != 0 or unaligned rows: the 1-channel input conv, tiny test models).
template <typename WT, typename KVT, int MT, int NT, int EPI, bool XALIGNED, bool BX3 = false>
__global__ void gemm_mfma_kernel(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_part[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m_base = blockIdx.y * (16 * MT);
  const int n_base = blockIdx.x * ((EPI == EPI_GATE) ? 16 : 16 * NT);
  const WT* W = reinterpret_cast<const WT*>(a.W);
  constexpr int TILES = NT * MT;

  const WT* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = dsm_wbase<WT>(a, W, n_base + nt * a.nt_stride, r, q);
  const int wst = dsm_wstep<WT>(a);
  const float* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int m = m_base + 16 * mt + r;
    m = m < a.M ? m : a.M - 1;  // padded rows re-read the last real row; their results are discarded
    xrow[mt] = a.X + a.xmap.off(m) + 8 * q;
  }
  f32x4 acc[NT][MT];
  const int chunks = (a.Kpad + DSM_KC - 1) / DSM_KC;

  for (int c = wave; c < chunks; c += S) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int k0 = c * DSM_KC;
    const int k1 = min(k0 + DSM_KC, a.Kpad);
    for (int kb = k0; kb < k1; kb += 32) {
      float wa[NT][8], xb[MT][8];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) load_w8<WT>(wrow[nt] + (long)kb * wst, wa[nt]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (XALIGNED) {
          load_w8<float>(xrow[mt] + kb, xb[mt]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xb[mt][j] = (kb + 8 * q + j < a.K) ? xrow[mt][kb + j] : 0.0f;
        }
      }
      if (BX3) {  // dot_mode 1: three bf16 pieces of the activations against the bf16 weights (gemm_bx3_kernel's order)
        dsm_bf16x8 wv[NT], xp[3][MT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 8; ++j) wv[nt][j] = (short)(__float_as_uint(wa[nt][j]) >> 16);  // the weights are bf16 values
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            uint16_t h, m, l;
            dsm_split3(xb[mt][j], &h, &m, &l);
            xp[0][mt][j] = (short)l; xp[1][mt][j] = (short)m; xp[2][mt][j] = (short)h;
          }
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[nt], xp[p][mt], acc[nt][mt], 0, 0, 0);
        continue;
      }
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[nt][s], xb[mt][s], acc[nt][mt], 0, 0, 0);
    }
    if (chunks > 1) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          *reinterpret_cast<f32x4*>(&lds_part[(((c * TILES) + nt * MT + mt) * 64 + lane) * 4]) = acc[nt][mt];
    }
  }
  // split-K combine ((c0 + c1) + c2) + ...  GATE needs both tiles of an m-tile in one wave: wave w' owns
  // m-tiles w', w'+S, ...; otherwise tile (nt, mt) is owned by wave (nt*MT + mt) % S.
  const bool multi = chunks > 1;
  if (multi) {
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int owner = (EPI == EPI_GATE) ? (mt % S) : ((nt * MT + mt) % S);
        if (owner != wave) continue;
        f32x4 tot = *reinterpret_cast<f32x4*>(&lds_part[((nt * MT + mt) * 64 + lane) * 4]);
        for (int c = 1; c < chunks; ++c) {
          f32x4 p = *reinterpret_cast<f32x4*>(&lds_part[(((c * TILES) + nt * MT + mt) * 64 + lane) * 4]);
          tot = tot + p;
        }
        acc[nt][mt] = tot;
      }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + 16 * mt + r;
    if (EPI == EPI_GATE) {
      if (multi && (mt % S) != wave) continue;
      epi_gate(a, acc[0][mt], acc[NT - 1][mt], m, n_base + 4 * q);
      continue;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      if (multi && ((nt * MT + mt) % S) != wave) continue;  // wave-uniform
      const int n = n_base + nt * a.nt_stride + 4 * q;
      if (EPI == EPI_RVQ)
        epi_rvq(a, acc[nt][mt], m, n, (n_base + nt * a.nt_stride) >> 4, q);
      else
        epi_store_qkv<KVT, EPI>(a, acc[nt][mt], m, n);
    }
  }
}

// ---- tiled GEMM (fast path: K % 32 == 0, 16-byte aligned X rows).
// Workgroup = 4 waves; tile = 64 weight rows (wave w owns 16-row n-tile w; for the gate also the matching
// "up" tile at +nt_stride) x 16*MT activation rows x ONE K-chunk (blockIdx.y).  The 32-wide activation block
// [16*MT][32] f32 is fetched once per workgroup with coalesced full-line loads, staged in LDS and shared by the four
// waves; weights stream straight to registers.  LDS image (r02): unpadded 32-float rows whose eight 16-byte units are
// XOR-swizzled by bits 1 and 3 of the row (dsm_xs_sw) — the lane groups that one ds_read_b128 services together are
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS), i.e. fragment rows {0-3, 12-15} of one
// k-quarter with rows {4-11} of the next, and NO row padding separates those (r01's 36-float rows: two 2-way conflicts
// per group, SQ_LDS_BANK_CONFLICT = 34 % of the kernel's cycles at M = 512); with the swizzle each group's sixteen
// 16-byte reads fall on sixteen different bank quads, and the eight lanes of a ds_write_b128 group fill one row.  Loads of block i+1 are in flight behind the MFMAs of block i (double-buffered LDS, one barrier
// per block).  chunks == 1: fused epilogue.  chunks > 1: the chunk's partial tiles go to a workspace slab in
// MFMA register layout and gemm_reduce_kernel sums the slabs left to right (canonical order) and runs the epilogue.
#define DSM_XS_LD 32
__device__ __forceinline__ int dsm_xs_sw(int row) { return ((row >> 1) & 1) | (((row >> 3) & 1) << 2); }
template <typename WT, typename KVT, int MT, int NT, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_tile_kernel(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) float Xs[2][16 * MT][DSM_XS_LD];
  launch_stamp_begin(a.ts);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int xu0 = 4 * ((2 * q) ^ dsm_xs_sw(r)), xu1 = xu0 ^ 4;  // this lane's two 16-byte units of a fragment row (swizzled)
  const int chunks = gridDim.y;  // split-K across workgroups; 1 when a.chunk_loop walks the chunks below
  const int m_base = blockIdx.z * (16 * MT);
  const int n_base = blockIdx.x * 64 + 16 * wave;  // this wave's n-tile
  const WT* W = reinterpret_cast<const WT*>(a.W);

  const WT* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = dsm_wbase<WT>(a, W, n_base + nt * a.nt_stride, r, q);
  const int wst = dsm_wstep<WT>(a);
  // cooperative X fetch: 16*MT rows x 8 float4 pieces; thread t takes piece t (and t+256 when MT == 4).
  // Scalars, not arrays: small per-thread arrays ended up in scratch memory here.
  constexpr int PIECES = 16 * MT * 8;
  constexpr bool TWO = PIECES > 256;
  const bool has0 = tid < PIECES;
  const int row0 = has0 ? (tid >> 3) : 0, part = tid & 7;  // !has0: loads row 0 (valid), stores nothing
  int m0 = m_base + row0;
  m0 = m0 < a.M ? m0 : a.M - 1;
  const float* xsrc0 = a.X + a.xmap.off(m0) + 4 * part;
  const int xdst0 = row0 * DSM_XS_LD + 4 * (part ^ dsm_xs_sw(row0));
  int m1 = m_base + row0 + 32;
  m1 = m1 < a.M ? m1 : a.M - 1;
  const float* xsrc1 = a.X + a.xmap.off(m1) + 4 * part;
  const int xdst1 = (row0 + 32) * DSM_XS_LD + 4 * (part ^ dsm_xs_sw(row0));  // +32 leaves bits 1 and 3 of the row alone

  const int nloop = a.chunk_loop > 1 ? a.chunk_loop : 1;
  f32x4 acc[NT][MT], tot[NT][MT];
  float xbA[MT][8], xbB[MT][8];  // activation fragments: even blocks in A, odd blocks in B
  for (int cl = 0; cl < nloop; ++cl) {
  const int chunk = a.chunk_loop > 1 ? cl : (int)blockIdx.y;
  const int k0 = chunk * DSM_KC;
  const int k1 = min(k0 + DSM_KC, a.Kpad);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Every load of the chunk — 8 activation pieces and 8 weight fragments per thread — is issued up front, in the
  // order the blocks consume them and without a branch around any of them (block indices are clamped to the chunk's
  // last block; threads without an activation piece load a row they never store).  A load under a branch makes the
  // compiler wait for it on the spot, and s_waitcnt counts loads in issue order, so fetching "two blocks ahead"
  // inside the loop had been serialising every block behind the HBM latency: half the MFMA rate.  Now the latency
  // is paid once per workgroup, while the co-resident workgroups (3-4 per CU) keep the MFMA pipe busy.
  const int nkb = (k1 - k0) >> 5;  // 1..8 blocks of 32
  // named scalars, not arrays: the 8-entry prefetch arrays were left in scratch memory by the compiler
#define DSM_FOR8(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define DSM_LOADBLK(I)                                                                 \
  float4 xp##I, xq##I;                                                                 \
  Raw8<WT> rw##I[NT];                                                                  \
  {                                                                                    \
    const int kb_ = k0 + 32 * ((I) < nkb ? (I) : nkb - 1);                             \
    xp##I = *reinterpret_cast<const float4*>(xsrc0 + kb_);                             \
    xq##I = TWO ? *reinterpret_cast<const float4*>(xsrc1 + kb_) : xp##I;               \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) rw##I[nt].load(wrow[nt] + (long)kb_ * wst);  \
  }
  DSM_FOR8(DSM_LOADBLK)
  __builtin_amdgcn_sched_barrier(0);  // all requests issued before the first block waits for its own
  // Fragments of block i+1 are read from LDS while the MFMAs of block i run (r02): a block opens with its first MFMA
  // group right behind the barrier instead of "store, barrier, wait for the LDS read".  One barrier per block: block
  // i+1's activations are stored before it and read after it; the buffer they overwrite was last read (as block i-1)
  // before the previous barrier.
#define DSM_XSTORE(I)                                                                  \
  {                                                                                    \
    float* xs_ = &Xs[(I) & 1][0][0];                                                   \
    if (has0) *reinterpret_cast<float4*>(xs_ + xdst0) = xp##I;                         \
    if (TWO) *reinterpret_cast<float4*>(xs_ + xdst1) = xq##I;                          \
  }
#define DSM_XFRAG(XB, I)                                                               \
  _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                                  \
    const float* fp = &Xs[(I) & 1][0][0] + (16 * mt + r) * DSM_XS_LD;                  \
    const float4 f0 = *reinterpret_cast<const float4*>(fp + xu0), f1 = *reinterpret_cast<const float4*>(fp + xu1); \
    XB[mt][0] = f0.x; XB[mt][1] = f0.y; XB[mt][2] = f0.z; XB[mt][3] = f0.w;            \
    XB[mt][4] = f1.x; XB[mt][5] = f1.y; XB[mt][6] = f1.z; XB[mt][7] = f1.w;            \
  }
#define DSM_XMFMA(CUR, S0, S1)                                                         \
  _Pragma("unroll") for (int s = (S0); s < (S1); ++s) {                                \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                  \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                  \
      acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[nt][s], CUR[mt][s], acc[nt][mt], 0, 0, 0); \
    if (NT * MT > 1) __builtin_amdgcn_sched_barrier(0); /* round-robin over the accumulators */ \
  }
  // PIPE: the two-fragment-set form.  The gate's two n-tiles per wave do not have the registers for it (178 VGPRs: one
  // workgroup per CU less; 16x4 m-tiles: spills), so NT = 2 keeps the plain order: store, barrier, read, multiply.
  constexpr bool PIPE = NT == 1;
  if (PIPE) {
    if (cl > 0) __syncthreads();  // chunk loop: the previous chunk's last fragment reads are done before Xs[0] is rewritten
    DSM_XSTORE(0)
    __syncthreads();
    DSM_XFRAG(xbA, 0)
  }
#define DSM_BLOCK(I, IN, CUR, NXT)                                                     \
  if ((I) < nkb) { /* workgroup-uniform */                                             \
    float wa[NT][8];                                                                   \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) rw##I[nt].unpack(wa[nt]);        \
    if (PIPE) {                                                                        \
      if ((I) + 1 < nkb) DSM_XSTORE(IN)                                                \
      __syncthreads();                                                                 \
      DSM_XMFMA(CUR, 0, 1)                                                             \
      if ((I) + 1 < nkb) { DSM_XFRAG(NXT, IN) }                                        \
      __builtin_amdgcn_sched_barrier(0);                                               \
      DSM_XMFMA(CUR, 1, 8)                                                             \
    } else {                                                                           \
      DSM_XSTORE(I)                                                                    \
      __syncthreads();                                                                 \
      DSM_XFRAG(xbA, I)                                                                \
      DSM_XMFMA(xbA, 0, 8)                                                             \
    }                                                                                  \
  }
  DSM_BLOCK(0, 1, xbA, xbB) DSM_BLOCK(1, 2, xbB, xbA) DSM_BLOCK(2, 3, xbA, xbB) DSM_BLOCK(3, 4, xbB, xbA)
  DSM_BLOCK(4, 5, xbA, xbB) DSM_BLOCK(5, 6, xbB, xbA) DSM_BLOCK(6, 7, xbA, xbB) DSM_BLOCK(7, 7, xbB, xbA)
#undef DSM_FOR8
#undef DSM_LOADBLK
#undef DSM_BLOCK
#undef DSM_XSTORE
#undef DSM_XFRAG
#undef DSM_XMFMA
  // canonical split-K order: chunk sums added left to right (here in registers, otherwise by the reduce kernels)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) tot[nt][mt] = cl == 0 ? acc[nt][mt] : tot[nt][mt] + acc[nt][mt];
  }  // chunk loop
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = tot[nt][mt];

  if (chunks > 1) {
    // slab[chunk][m][n] f32, row-major with ld = ws_ntiles*16: a lane stores its 4 consecutive n of row m
    const long ld = (long)a.ws_ntiles * 16;
    const long mpad = (long)((a.M + 15) >> 4) * 16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + 16 * mt + r;
      if (m >= mpad) continue;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * a.nt_stride + 4 * q;
        *reinterpret_cast<f32x4*>(a.ws + ((long)blockIdx.y * mpad + m) * ld + n) = acc[nt][mt];
      }
    }
    launch_stamp_end(a.ts);
    return;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + 16 * mt + r;
    if (EPI == EPI_GATE) {
      epi_gate(a, acc[0][mt], acc[NT - 1][mt], m, n_base + 4 * q);
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * a.nt_stride + 4 * q;
        if (EPI == EPI_RVQ)
          epi_rvq(a, acc[nt][mt], m, n, (n_base + nt * a.nt_stride) >> 4, q);
        else
          epi_store_qkv<KVT, EPI>(a, acc[nt][mt], m, n);
      }
    }
  }
  launch_stamp_end(a.ts);
}

// ---- tiled GEMM, whole K inside the workgroup (large batches: the (n, m) tiles alone fill the chip, so there is no
// split-K across workgroups, no slabs, no reduce launch).  Same tile, same LDS staging, same canonical order as
// gemm_tile_kernel — chunk sums of 256 k are formed in `acc` and added left to right into `tot` — but the loads run as a
// ROLLING window over the 32-wide blocks of the whole K range: four register slots hold blocks g .. g+3, and as soon
// as block g has been consumed its slot requests block g+4, across chunk boundaries.  (The r01 chunk loop inside
// gemm_tile_kernel requested a whole chunk only after finishing the previous one: every 8 blocks the MFMA pipe of the
// wave drained behind an L2 / HBM round trip — 64 % of the f32-MFMA rate at B >= 512.)
// Named scalars and a hand-unrolled body, not arrays: see gemm_tile_kernel.  Window depth D: 4 blocks, or 2 where a
// block is twice the MFMA work (the gate's two n-tiles per wave) or twice the registers (f32 weights) — the same ~4096
// MFMA cycles of cover, and the four-slot form of those two spilled.
template <typename WT, int NT>
struct LoopDepth {
  static constexpr int MAX = (NT == 2 || sizeof(WT) == 4) ? 2 : 4;
};
template <typename WT, typename KVT, int MT, int NT, int EPI, int D, int OCC = 2>
__global__ __launch_bounds__(256, OCC) void gemm_loop_kernel(GemmArgs a) {
  static_assert(D == 2 || D == 4, "window depth");
  launch_stamp_begin(a.ts);
  __shared__ __attribute__((aligned(16))) float Xs[2][16 * MT][DSM_XS_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int xu0 = 4 * ((2 * q) ^ dsm_xs_sw(r)), xu1 = xu0 ^ 4;  // this lane's two 16-byte units of a fragment row (swizzled)
  const int m_base = blockIdx.z * (16 * MT);
  const int n_base = blockIdx.x * 64 + 16 * wave;
  const WT* W = reinterpret_cast<const WT*>(a.W);
  const WT* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = dsm_wbase<WT>(a, W, n_base + nt * a.nt_stride, r, q);
  const int wst = dsm_wstep<WT>(a);
  constexpr int PIECES = 16 * MT * 8;
  constexpr bool TWO = PIECES > 256;
  const bool has0 = tid < PIECES;
  const int row0 = has0 ? (tid >> 3) : 0, part = tid & 7;
  int m0 = m_base + row0;
  m0 = m0 < a.M ? m0 : a.M - 1;
  const float* xsrc0 = a.X + a.xmap.off(m0) + 4 * part;
  const int xdst0 = row0 * DSM_XS_LD + 4 * (part ^ dsm_xs_sw(row0));
  int m1 = m_base + row0 + 32;
  m1 = m1 < a.M ? m1 : a.M - 1;
  const float* xsrc1 = a.X + a.xmap.off(m1) + 4 * part;
  const int xdst1 = (row0 + 32) * DSM_XS_LD + 4 * (part ^ dsm_xs_sw(row0));  // +32 leaves bits 1 and 3 of the row alone
  const int nb = a.Kpad >> 5;  // 32-wide blocks of the whole reduction

  f32x4 acc[NT][MT], tot[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      tot[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  float4 xp0, xp1, xp2, xp3, xq0, xq1, xq2, xq3;
  Raw8<WT> rw0[NT], rw1[NT], rw2[NT], rw3[NT];
  // block indices are clamped to the last block (loaded again, never used): no branch around any load
#define DSM_LLOAD(S, G)                                                              \
  {                                                                                  \
    const int kb_ = 32 * min((G), nb - 1);                                           \
    xp##S = *reinterpret_cast<const float4*>(xsrc0 + kb_);                           \
    xq##S = TWO ? *reinterpret_cast<const float4*>(xsrc1 + kb_) : xp##S;             \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) rw##S[nt].load(wrow[nt] + (long)kb_ * wst); \
  }
  DSM_LLOAD(0, 0) DSM_LLOAD(1, 1)
  if (D == 4) { DSM_LLOAD(2, 2) DSM_LLOAD(3, 3) }
  __builtin_amdgcn_sched_barrier(0);
  // The activation fragments of block g+1 are fetched from LDS while the MFMAs of block g run (two register sets, A for even
  // blocks, B for odd ones): a block no longer opens with "store to LDS, barrier, wait for the LDS read" in front of its
  // first MFMA — with two waves per SIMD running the same program those gaps line up and idle the matrix pipe (PMC: 64 %
  // MFMA-busy at M = 512 before, profiles/r02).  One barrier per block remains; what it orders: block g+1's activations
  // are stored before it and read after it, and the buffer they overwrite was last read (as block g-1) before the
  // previous barrier.
  float xbA[MT][8], xbB[MT][8];
#define DSM_LSTORE(S, BUF)                                                           \
  {                                                                                  \
    float* xs_ = &Xs[BUF][0][0];                                                     \
    if (has0) *reinterpret_cast<float4*>(xs_ + xdst0) = xp##S;                       \
    if (TWO) *reinterpret_cast<float4*>(xs_ + xdst1) = xq##S;                        \
  }
#define DSM_LFRAG(XB, BUF)                                                           \
  _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                                \
    const float* fp = &Xs[BUF][0][0] + (16 * mt + r) * DSM_XS_LD;                    \
    const float4 f0 = *reinterpret_cast<const float4*>(fp + xu0), f1 = *reinterpret_cast<const float4*>(fp + xu1); \
    XB[mt][0] = f0.x; XB[mt][1] = f0.y; XB[mt][2] = f0.z; XB[mt][3] = f0.w;          \
    XB[mt][4] = f1.x; XB[mt][5] = f1.y; XB[mt][6] = f1.z; XB[mt][7] = f1.w;          \
  }
  DSM_LSTORE(0, 0)
  __syncthreads();
  DSM_LFRAG(xbA, 0)
  // S: this block's slot, SN: the next block's slot, CUR / NXT: fragment sets (g % D == 0 and D is even: block parity == S parity)
#define DSM_LMFMA(CUR, S0, S1)                                                       \
  _Pragma("unroll") for (int s = (S0); s < (S1); ++s) {                              \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)                                \
      acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[nt][s], CUR[mt][s], acc[nt][mt], 0, 0, 0); \
    if (NT * MT > 1) __builtin_amdgcn_sched_barrier(0); /* round-robin over the accumulators */ \
  }
#define DSM_LSTEP(S, SN, CUR, NXT)                                                   \
  {                                                                                  \
    const int gb = g + (S);                                                          \
    float wa[NT][8];                                                                 \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) rw##S[nt].unpack(wa[nt]);      \
    if (gb < nb) { /* workgroup-uniform */                                           \
      if (gb + 1 < nb) DSM_LSTORE(SN, ((S) + 1) & 1)                                 \
      __syncthreads();                                                               \
      /* the first MFMA group goes out right behind the barrier; the LDS reads of the NEXT block's fragments follow it   \
         (issued in front, the compiler makes every MFMA of this block wait for them) */ \
      DSM_LMFMA(CUR, 0, 1)                                                           \
      if (gb + 1 < nb) { DSM_LFRAG(NXT, ((S) + 1) & 1) }                             \
      __builtin_amdgcn_sched_barrier(0);                                             \
    }                                                                                \
    DSM_LLOAD(S, gb + D) /* the slot is free again: D blocks ahead, whatever chunk that is */ \
    __builtin_amdgcn_sched_barrier(0);                                               \
    if (gb < nb) {                                                                   \
      DSM_LMFMA(CUR, 1, 8)                                                           \
      if ((gb & 7) == 7 || gb == nb - 1) { /* a 256-wide chunk is complete: canonical left-to-right chunk sum */ \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                            \
        _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                          \
          tot[nt][mt] = tot[nt][mt] + acc[nt][mt]; /* first chunk: +0 + acc == acc bit for bit (acc starts at +0, so it is never -0) */ \
          acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};                                 \
        }                                                                            \
      }                                                                              \
    }                                                                                \
  }
#pragma clang loop unroll(disable)
  for (int g = 0; g < nb; g += D) {
    if (D == 4) {
      DSM_LSTEP(0, 1, xbA, xbB) DSM_LSTEP(1, 2, xbB, xbA) DSM_LSTEP(2, 3, xbA, xbB) DSM_LSTEP(3, 0, xbB, xbA)
    } else {
      DSM_LSTEP(0, 1, xbA, xbB) DSM_LSTEP(1, 0, xbB, xbA)
    }
  }
#undef DSM_LSTORE
#undef DSM_LFRAG
#undef DSM_LMFMA
#undef DSM_LLOAD
#undef DSM_LSTEP
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + 16 * mt + r;
    if (EPI == EPI_GATE) {
      epi_gate(a, tot[0][mt], tot[NT - 1][mt], m, n_base + 4 * q);
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * a.nt_stride + 4 * q;
        if (EPI == EPI_RVQ)
          epi_rvq(a, tot[nt][mt], m, n, (n_base + nt * a.nt_stride) >> 4, q);
        else
          epi_store_qkv<KVT, EPI>(a, tot[nt][mt], m, n);
      }
    }
  }
  launch_stamp_end(a.ts);
}

// ---- dot_mode 1 ("bx3"): the bf16-weight GEMMs on v_mfma_f32_16x16x32_bf16 (r03) -------------------------------------------
// Same tile, same grid, same slabs / epilogues as gemm_tile_kernel and gemm_loop_kernel — only the dot product of a K-chunk
// differs: per 32-wide block  acc = mfma(w, x_lo, acc); acc = mfma(w, x_mid, acc); acc = mfma(w, x_hi, acc)  with x = hi + mid +
// lo the exact three-bf16 split of dsm_split3 (every product exact; the instruction's adder: dsm_bf16_mfma_model.h, restated
// by the oracle's orc_linear_bx3).  3 x 16 matrix-pipe cycles per 32 k and tile instead of 8 x 32, and the matrix pipe no
// longer holds the vector ALU (experiments/fused_roles_probe.hip).  The activation block is split while it is staged: LDS holds
// three bf16 planes [16 MT rows][32 k] (64-byte rows, 16-byte units XOR-swizzled by bits 1-2 of the row), double-buffered, one
// barrier per block; weights go from HBM to the A operand as they are (eight bf16 = one 16-byte load per lane and block).
// LOOP: one workgroup walks every K-chunk (grid.y = 1) and adds the chunk sums left to right in registers; otherwise
// blockIdx.y is the chunk and, with more than one, the partial tile goes to the split-K slab.
template <typename KVT, int MT, int NT, int EPI, bool LOOP>
__global__ __launch_bounds__(256, 2) void gemm_bx3_kernel(GemmArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t Xp[2][3][16 * MT][32];
  launch_stamp_begin(a.ts);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int chunks = LOOP ? 1 : (int)gridDim.y;
  const int m_base = blockIdx.z * (16 * MT);
  const int n_base = blockIdx.x * (a.wg_cols ? a.wg_cols : 64) + 16 * wave;
  const uint16_t* W = reinterpret_cast<const uint16_t*>(a.W);
  const uint16_t* wrow[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = dsm_wbase<uint16_t>(a, W, n_base + nt * a.nt_stride, r, q);
  const int wst = dsm_wstep<uint16_t>(a);
  constexpr int PIECES = 16 * MT * 8;
  constexpr bool TWO = PIECES > 256;
  const bool has0 = tid < PIECES;
  const int row0 = has0 ? (tid >> 3) : 0, part = tid & 7;
  int m0 = m_base + row0;
  m0 = m0 < a.M ? m0 : a.M - 1;
  const float* xsrc0 = a.X + a.xmap.off(m0) + 4 * part;
  int m1 = m_base + row0 + 32;
  m1 = m1 < a.M ? m1 : a.M - 1;
  const float* xsrc1 = a.X + a.xmap.off(m1) + 4 * part;
  // four consecutive k of one row -> 8 bytes in each plane
  auto stage = [&](int buf, const float4& v, int row) {
    uint16_t h[4], m[4], l[4];
    dsm_split3(v.x, &h[0], &m[0], &l[0]); dsm_split3(v.y, &h[1], &m[1], &l[1]);
    dsm_split3(v.z, &h[2], &m[2], &l[2]); dsm_split3(v.w, &h[3], &m[3], &l[3]);
    const int off = row * 32 + (((part >> 1) ^ ((row >> 1) & 3)) * 8) + (part & 1) * 4;
    *reinterpret_cast<uint2*>(&Xp[buf][0][0][0] + off) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
    *reinterpret_cast<uint2*>(&Xp[buf][1][0][0] + off) = make_uint2((uint32_t)m[0] | ((uint32_t)m[1] << 16), (uint32_t)m[2] | ((uint32_t)m[3] << 16));
    *reinterpret_cast<uint2*>(&Xp[buf][2][0][0] + off) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
  };
  const int kb0 = LOOP ? 0 : (int)blockIdx.y * (DSM_KC >> 5);
  const int kb1 = LOOP ? (a.Kpad >> 5) : min(kb0 + (DSM_KC >> 5), a.Kpad >> 5);
  f32x4 acc[NT][MT], tot[NT][MT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      tot[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  float4 xa = *reinterpret_cast<const float4*>(xsrc0 + 32 * kb0);
  float4 xb = TWO ? *reinterpret_cast<const float4*>(xsrc1 + 32 * kb0) : xa;
  uint4 wv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wv[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + (long)32 * kb0 * wst);
  for (int g = kb0; g < kb1; ++g) {
    const int buf = (g - kb0) & 1;
    if (has0) stage(buf, xa, row0);
    if (TWO) stage(buf, xb, row0 + 32);
    dsm_bf16x8 wa[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const uint4 w = wv[nt];
      wa[nt][0] = (short)(w.x & 0xFFFF); wa[nt][1] = (short)(w.x >> 16); wa[nt][2] = (short)(w.y & 0xFFFF); wa[nt][3] = (short)(w.y >> 16);
      wa[nt][4] = (short)(w.z & 0xFFFF); wa[nt][5] = (short)(w.z >> 16); wa[nt][6] = (short)(w.w & 0xFFFF); wa[nt][7] = (short)(w.w >> 16);
    }
    {  // the next block's loads fly behind this block's MFMAs (clamped to the last block: loaded again, never used)
      const int gn = g + 1 < kb1 ? g + 1 : g;
      xa = *reinterpret_cast<const float4*>(xsrc0 + 32 * gn);
      if (TWO) xb = *reinterpret_cast<const float4*>(xsrc1 + 32 * gn);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) wv[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + (long)32 * gn * wst);
    }
    __syncthreads();  // block g's planes are complete; buffer buf ^ 1 was last read before the previous barrier
#pragma unroll
    for (int p = 0; p < 3; ++p)  // canonical order of the pieces: lo, mid, hi
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int row = 16 * mt + r;
        const dsm_bf16x8 xf = *reinterpret_cast<const dsm_bf16x8*>(&Xp[buf][p][0][0] + row * 32 + ((q ^ ((row >> 1) & 3)) * 8));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[nt], xf, acc[nt][mt], 0, 0, 0);
      }
    if (LOOP && ((g & 7) == 7 || g == kb1 - 1)) {  // a 256-wide chunk is complete: canonical left-to-right chunk sum
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          tot[nt][mt] = tot[nt][mt] + acc[nt][mt];  // first chunk: +0 + acc (the oracle does the same)
          acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
  }
  if (!LOOP) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) tot[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f} + acc[nt][mt];  // +0 + chunk sum, as above
  }
  if (chunks > 1) {
    const long ld = (long)a.ws_ntiles * 16;
    const long mpad = (long)((a.M + 15) >> 4) * 16;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + 16 * mt + r;
      if (m >= mpad) continue;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * a.nt_stride + 4 * q;
        *reinterpret_cast<f32x4*>(a.ws + ((long)blockIdx.y * mpad + m) * ld + n) = tot[nt][mt];
      }
    }
    launch_stamp_end(a.ts);
    return;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m_base + 16 * mt + r;
    if (EPI == EPI_GATE) {
      epi_gate(a, tot[0][mt], tot[NT - 1][mt], m, n_base + 4 * q);
    } else {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) epi_store_qkv<KVT, EPI>(a, tot[nt][mt], m, n_base + nt * a.nt_stride + 4 * q);
    }
  }
  launch_stamp_end(a.ts);
}

// Ordered sum of `chunks` slab values at p, p + cstride, ...: loads are issued eight at a time, the adds stay
// strictly left to right (canonical split-K order).
__device__ __forceinline__ f32x4 slab_sum(const float* p, long cstride, int chunks) {
  f32x4 t = *reinterpret_cast<const f32x4*>(p);
  for (int c0 = 1; c0 < chunks; c0 += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + u < chunks ? c0 + u : chunks - 1;  // clamped duplicate load, discarded below
      v[u] = *reinterpret_cast<const f32x4*>(p + c * cstride);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c0 + u < chunks) t = t + v[u];
  }
  return t;
}

// Ordered split-K reduce + epilogue: one wave per 16x16 output tile (a gate/up tile pair for EPI_GATE).
template <typename KVT, int EPI>
__global__ __launch_bounds__(256) void gemm_reduce_kernel(GemmArgs a, int chunks) {
  launch_stamp_begin(a.ts ? a.ts + 2 : nullptr);  // the reduce launch owns the record after its GEMM's
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int mtiles = (a.M + 15) >> 4;
  const int out_ntiles = (a.N + 15) >> 4;  // gate: a.N is the hidden width
  const int t = blockIdx.x * 4 + wave;
  if (t >= mtiles * out_ntiles) return;
  const int mtile = t / out_ntiles, ntile = t % out_ntiles;
  constexpr int NT = (EPI == EPI_GATE) ? 2 : 1;
  const long ld = (long)a.ws_ntiles * 16, cstride = (long)mtiles * 16 * ld;
  const int m = mtile * 16 + r, n = ntile * 16 + 4 * q;
  f32x4 tot[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    tot[nt] = slab_sum(a.ws + (long)m * ld + n + nt * a.nt_stride, cstride, chunks);
  }
  if (EPI == EPI_GATE)
    epi_gate(a, tot[0], tot[NT - 1], m, n);
  else if (EPI == EPI_RVQ)
    epi_rvq(a, tot[0], m, n, ntile, q);
  else
    epi_store_qkv<KVT, EPI>(a, tot[0], m, n);
  launch_stamp_end(a.ts ? a.ts + 2 : nullptr);
}

#include "dsm_gemm_wk.h"  // whole-K-in-the-workgroup GEMM for M <= 64 (r04): no slabs, no reduce launch

// Canonical row reduction (dsm_numerics.h): 256 threads per row, thread t owns elements 1024*it + 4*t + j;
// wave butterflies, then the 4 wave totals left to right.  `red` = 8 floats of LDS.
__device__ __forceinline__ void block_row_sums(float& s, float& s2, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  s = wave_sum64(s);
  s2 = wave_sum64(s2);
  if (lane == 0) { red[wave] = s; red[4 + wave] = s2; }
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
  s2 = ((red[4] + red[5]) + red[6]) + red[7];
}

#define DSM_ROW_ITS 4  // d_model <= 4096

__device__ __forceinline__ void row_norm_apply(const float4 (&v)[DSM_ROW_ITS], float s, float s2, int d, float eps, int rms,
                                               const float* __restrict__ w, const float* __restrict__ b,
                                               float* __restrict__ out) {
  float mm = 1.f, mean = 0.f, inv = 0.f;
  if (rms) {
    mm = sqrtf(s2 / (float)d + eps);
  } else {
    mean = s / (float)d;
    float var = s2 / (float)d - mean * mean;
    inv = 1.0f / sqrtf(var + eps);
  }
#pragma unroll
  for (int it = 0; it < DSM_ROW_ITS; ++it) {
    const int i = it * 1024 + 4 * (int)threadIdx.x;
    if (i < d) {
      const float4 wv = *reinterpret_cast<const float4*>(w + i);
      float4 o;
      if (rms) {
        o.x = (v[it].x / mm) * wv.x; o.y = (v[it].y / mm) * wv.y; o.z = (v[it].z / mm) * wv.z; o.w = (v[it].w / mm) * wv.w;
      } else {
        const float4 bv = *reinterpret_cast<const float4*>(b + i);
        o.x = ((v[it].x - mean) * inv) * wv.x + bv.x; o.y = ((v[it].y - mean) * inv) * wv.y + bv.y;
        o.z = ((v[it].z - mean) * inv) * wv.z + bv.z; o.w = ((v[it].w - mean) * inv) * wv.w + bv.w;
      }
      *reinterpret_cast<float4*>(out + i) = o;
    }
  }
}

// Ordered split-K reduce + STORE epilogue (bias / act / scale / residual) + the row norm that follows it, one
// workgroup per output row (N = d_model).  Same per-element arithmetic as epi_store_qkv<EPI_STORE> followed by
// row_norm_kernel, and the same canonical row reduction (dsm_numerics.h: thread t of 256 chains its elements
// 1024*it + 4*t + j over it = 0, 1, ...) — but the work of "thread t" is spread over ITS threads, one per 1024-element group
// (workgroup of 256 * ITS threads), so that every slab load of the row is in flight at once: a launch has only M
// workgroups (32 per stream group at B = 64) and its time is the number of dependent load rounds.  The chain over `it`
// is handed from group to group through LDS (ITS - 1 barriers of ALU work).  r01 form: 256 threads, eight chunks of every
// group per round = three rounds for the 22-chunk ff_out reduce, 6.8 us per launch.
template <int ITS>  // 1024-element groups per row: ceil(d / 1024) rounded up to 1, 2 or 4
__global__ __launch_bounds__(256 * ITS) void gemm_reduce_rows_kernel(GemmArgs a, int chunks) {
  constexpr int RS = ITS == 4 ? 16 : 24;  // chunk loads per round (VGPR budget: 1024 threads leave 128 each)
  __shared__ float red[8];
  __shared__ float carry[2][256];
  launch_stamp_begin(a.ts ? a.ts + 2 : nullptr);
  const int m = blockIdx.x;
  const int d = a.N;
  const int it = threadIdx.x >> 8, t = threadIdx.x & 255;
  const long ld = (long)a.ws_ntiles * 16, cstride = (long)((a.M + 15) >> 4) * 16 * ld;
  const int i = it * 1024 + 4 * t;
  const bool live = i < d;
  // A thread beyond d re-reads the row's first four elements and is dropped.  (Not 4 * t: with d < 1024 that is past the row for
  // t >= d / 4, and past the workspace, the residual and the norm weights for the last row — Mimi's d = 512.)
  const int ic = live ? i : 0;
  const float* p = a.ws + (long)m * ld + ic;
  // The epilogue's operands — bias, LayerScale, residual, norm weights — do not depend on the sums: requested FIRST, unconditionally
  // (an absent operand re-reads the slab word, a valid address, and is never used), so that they travel with the slab loads instead
  // of costing two more dependent memory round trips behind them (r04: 5.6 -> 4.x us per launch, 64 launches per step on the chain).
  const f32x4 bias4 = *reinterpret_cast<const f32x4*>(a.bias ? a.bias + ic : p);
  const f32x4 scale4 = *reinterpret_cast<const f32x4*>(a.scale ? a.scale + ic : p);
  const f32x4 res4 = *reinterpret_cast<const f32x4*>(a.res ? a.res + a.rmap.off(m) + ic : p);
  const f32x4 nw4 = *reinterpret_cast<const f32x4*>(a.norm_w + ic);
  const f32x4 nb4 = *reinterpret_cast<const f32x4*>(a.norm_rms ? p : a.norm_b + ic);
  f32x4 tot = *reinterpret_cast<const f32x4*>(p);
  for (int c0 = 1; c0 < chunks; c0 += RS) {
    f32x4 w[RS];
#pragma unroll
    for (int u = 0; u < RS; ++u) {
      const int c = c0 + u < chunks ? c0 + u : chunks - 1;  // clamped duplicate load, discarded below
      w[u] = *reinterpret_cast<const f32x4*>(p + c * cstride);
    }
    __builtin_amdgcn_sched_barrier(0);  // every load of the round is issued before the first add waits
#pragma unroll
    for (int u = 0; u < RS; ++u)
      if (c0 + u < chunks) tot = tot + w[u];
  }
  float o[4] = {tot[0], tot[1], tot[2], tot[3]};
  if (live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (a.bias) o[j] = o[j] + bias4[j];
      if (a.act == 1) o[j] = dsm_gelu_erf(o[j]);
      if (a.scale) o[j] = o[j] * scale4[j];
    }
    if (a.res) {
      o[0] = res4[0] + o[0]; o[1] = res4[1] + o[1]; o[2] = res4[2] + o[2]; o[3] = res4[3] + o[3];
    }
    *reinterpret_cast<float4*>(a.Y + a.ymap.off(m) + i) = make_float4(o[0], o[1], o[2], o[3]);
  }
  // thread t's chain, continued group by group
  float s = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < ITS; ++k) {
    if (it == k) {
      if (k > 0) { s = carry[0][t]; s2 = carry[1][t]; }
      if (live) {
        s = s + o[0]; s2 = DSM_FMAF(o[0], o[0], s2);
        s = s + o[1]; s2 = DSM_FMAF(o[1], o[1], s2);
        s = s + o[2]; s2 = DSM_FMAF(o[2], o[2], s2);
        s = s + o[3]; s2 = DSM_FMAF(o[3], o[3], s2);
      }
      if (k + 1 < ITS) { carry[0][t] = s; carry[1][t] = s2; }
    }
    if (k + 1 < ITS) __syncthreads();
  }
  if (it == ITS - 1) {  // these 4 waves hold the 256 thread totals: wave butterflies, then the wave totals left to right
    const int lane = t & 63, wave = t >> 6;
    s = wave_sum64(s);
    s2 = wave_sum64(s2);
    if (lane == 0) { red[wave] = s; red[4 + wave] = s2; }
  }
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
  s2 = ((red[4] + red[5]) + red[6]) + red[7];
  if (live) {
    float mm = 1.f, mean = 0.f, inv = 0.f;
    if (a.norm_rms) {
      mm = sqrtf(s2 / (float)d + a.norm_eps);
    } else {
      mean = s / (float)d;
      float var = s2 / (float)d - mean * mean;
      inv = 1.0f / sqrtf(var + a.norm_eps);
    }
    float4 r;
    if (a.norm_rms) {
      r.x = (o[0] / mm) * nw4[0]; r.y = (o[1] / mm) * nw4[1]; r.z = (o[2] / mm) * nw4[2]; r.w = (o[3] / mm) * nw4[3];
    } else {
      r.x = ((o[0] - mean) * inv) * nw4[0] + nb4[0]; r.y = ((o[1] - mean) * inv) * nw4[1] + nb4[1];
      r.z = ((o[2] - mean) * inv) * nw4[2] + nb4[2]; r.w = ((o[3] - mean) * inv) * nw4[3] + nb4[3];
    }
    *reinterpret_cast<float4*>(a.norm_out + (long)m * d + i) = r;
  }
  launch_stamp_end(a.ts ? a.ts + 2 : nullptr);
}

// ------------------------------------------------------------------------------------------
// Row norms — one workgroup per row.  rms 1: RmsNorm (core/batched_transformer.rs:194-198),
// rms 0: LayerNorm (core/batched_transformer.rs:200-222).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_norm_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ b, int rows,
                                                       int d, float eps, int rms) {
  __shared__ float red[8];
  const int row = blockIdx.x;
  const float* xr = x + (long)row * d;
  float4 v[DSM_ROW_ITS];
  float s = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int it = 0; it < DSM_ROW_ITS; ++it) {
    const int i = it * 1024 + 4 * (int)threadIdx.x;
    v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < d) {  // d % 4 == 0: a thread's four elements are in range together
      v[it] = *reinterpret_cast<const float4*>(xr + i);
      s = s + v[it].x; s2 = DSM_FMAF(v[it].x, v[it].x, s2);
      s = s + v[it].y; s2 = DSM_FMAF(v[it].y, v[it].y, s2);
      s = s + v[it].z; s2 = DSM_FMAF(v[it].z, v[it].z, s2);
      s = s + v[it].w; s2 = DSM_FMAF(v[it].w, v[it].w, s2);
    }
  }
  block_row_sums(s, s2, red);
  row_norm_apply(v, s, s2, d, eps, rms, w, b, y + (long)row * d);
}

// The same norm for a row wider than the 1024 * DSM_ROW_ITS elements row_norm_kernel keeps in registers (it would leave the rest
// of such a row out of the sums and unwritten): the row is read twice, sums first.  Same canonical order — thread t chains its
// elements 1024 * it + 4 * t + j over every it — and row_norm_apply's arithmetic.  No shipped model is this wide; the GEMM
// launcher takes this kernel for a row norm behind a product with N > 4096 (d % 4 == 0 as above).
__global__ __launch_bounds__(256) void row_norm_wide_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                            const float* __restrict__ w, const float* __restrict__ b, int rows,
                                                            int d, float eps, int rms) {
  __shared__ float red[8];
  const float* xr = x + (long)blockIdx.x * d;
  float* yr = y + (long)blockIdx.x * d;
  float s = 0.0f, s2 = 0.0f;
  for (int i = 4 * (int)threadIdx.x; i < d; i += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    s = s + v.x; s2 = DSM_FMAF(v.x, v.x, s2);
    s = s + v.y; s2 = DSM_FMAF(v.y, v.y, s2);
    s = s + v.z; s2 = DSM_FMAF(v.z, v.z, s2);
    s = s + v.w; s2 = DSM_FMAF(v.w, v.w, s2);
  }
  block_row_sums(s, s2, red);
  float mm = 1.f, mean = 0.f, inv = 0.f;
  if (rms) {
    mm = sqrtf(s2 / (float)d + eps);
  } else {
    mean = s / (float)d;
    float var = s2 / (float)d - mean * mean;
    inv = 1.0f / sqrtf(var + eps);
  }
  for (int i = 4 * (int)threadIdx.x; i < d; i += 1024) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    const float4 wv = *reinterpret_cast<const float4*>(w + i);
    float4 o;
    if (rms) {
      o.x = (v.x / mm) * wv.x; o.y = (v.y / mm) * wv.y; o.z = (v.z / mm) * wv.z; o.w = (v.w / mm) * wv.w;
    } else {
      const float4 bv = *reinterpret_cast<const float4*>(b + i);
      o.x = ((v.x - mean) * inv) * wv.x + bv.x; o.y = ((v.y - mean) * inv) * wv.y + bv.y;
      o.z = ((v.z - mean) * inv) * wv.z + bv.z; o.w = ((v.w - mean) * inv) * wv.w + bv.w;
    }
    *reinterpret_cast<float4*>(yr + i) = o;
  }
}

// ------------------------------------------------------------------------------------------
// Attention over the ring cache — core/batched_transformer.rs:107-113 + mask semantics of
// core/kv_cache.rs:119-237 in closed form: slot j is visible to query t iff
//   j <= e1  and  (e1 - j) mod ctx >= T-1-t,   e1 = start_pos + T - 1.
// One workgroup (4 waves) per (slot b, head h).  LPK = HD/8 lanes per key, G = 64/LPK keys per
// wave-instruction, key j -> wave (j/G)%4, lane group j%G (canonical order, dsm_numerics.h).
// ------------------------------------------------------------------------------------------
// Where one batch row of a launch keeps its K / V when the rows do not sit in one [rows][H][ctx][hd] block: the [H][ctx][hd]
// blocks of the row (TTS cross-attention: the row's private blocks, or a voice that several rows share — dsm_tts_voice.inc).
// One 16-byte entry per row, read once per workgroup; it lives in device memory because a captured launch keeps its arguments.
struct alignas(16) AttnRowSrc {
  const void *k, *v;
};
// A table entry's pointer as what it is, a global address: built from plain bits the K / V accesses behind it would become flat_*
// instructions (counted twice, checked against the LDS aperture) instead of global_* ones — for every launch of the kernel.
template <typename KVT>
__device__ __forceinline__ const KVT* attn_row_base(uint64_t bits) {
  return (const KVT*)(const __attribute__((address_space(1))) KVT*)bits;
}

// T = 1 only: the QKV GEMM left its split-K slabs in place and this kernel finishes the job for its own (slot, head) —
// ordered slab sums of the 3 x HD values, RoPE on q and k, K/V rows rounded into the ring cache at widx — before it
// attends.  Same arithmetic, same order as gemm_reduce_kernel<KVT, EPI_QKV>; one launch and the q round trip less.
struct AttnFused {
  const float* ws;  // null: q comes from qbuf, K/V are already in the cache
  long ld, cstride;
  int chunks;
  const float* rope_cs;
  const uint32_t* widx;
  int nt;  // K / V rows with non-temporal loads (the bf16 rings)
  int q_only;  // the slabs hold a [M][d] query projection only (cross-attention, r04): no K / V rows, no RoPE, nothing scattered
  // Row b's K / V sit at kcache / vcache + b * H * ctx * hd, or — for a launch that passes NO kcache (null) — where src[b] says.
  // The kernels test kcache, not src: it shares a kernarg cache line with what they read first anyway, src sits in a line that
  // the other launches (the STT hot path) then never wait for.
  const AttnRowSrc* src;
};

// UNRB: keys per lane group and batch on a bf16 ring (8: 126 VGPRs, 4: 78).  The key -> (wave, lane group) assignment and the order
// inside a group do not depend on it (same bits).  4 is faster outright at head_dim 64 (stt-2.6b: 39.2 against 42.8 us per 64-slot
// launch, 9.18 against 9.63 ms per step); at head_dim 128 the kernel itself is 3-4 % faster with 8 (launch_attn_t picks; r04, late;
// profiles/r04/experiments/timing_notes.txt).
template <typename KVT, int HD, int T, int UNRB = 8>
__global__ __launch_bounds__(256, 4) void attn_kernel(float* __restrict__ out, const float* __restrict__ qbuf,
                                                   const KVT* __restrict__ kcache, const KVT* __restrict__ vcache,
                                                   const uint32_t* __restrict__ start_pos,
                                                   const uint8_t* __restrict__ active, int H, int ctx, int d,
                                                   unsigned long long* __restrict__ ts, AttnFused fq) {
  constexpr int NW = 4, LPK = HD / 8, G = 64 / LPK;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  // Row b's table entry, in flight across the `active` test: a VECTOR load on purpose (the uniform row index is handed over in a
  // VGPR), so that it is counted with the load of active[b] and one wait covers both.  As a scalar load it was waited for on its
  // own ahead of that load — one more memory round trip per launch (+14.5 us on the 16 launches of a B = 32 step: DESIGN.md
  // section 5.4.1, "The kernels", has the numbers and the tool that repeats them).  Both forms compute the same values: once a
  // compiler overlaps the scalar load's wait with the `active` load, plain `fq.src[b]` may come back.
  uint4 rs_kv = {0u, 0u, 0u, 0u};
  if (!kcache) {
    int bv = b;
    asm volatile("" : "+v"(bv));
    rs_kv = *reinterpret_cast<const uint4*>(fq.src + bv);
  }
  // optional device-clock bracket of the whole launch (dsm_prof_read_device): first workgroup in, last one out.
  // HIP events around a launch also count the time it queues behind other streams' kernels; this does not.
  // Only the first 256 workgroups race for the start stamp and the last 1024 for the end stamp (dispatch is in index
  // order): thousands of atomics on one address would themselves stretch a large launch.
  const bool ts_first = ts && threadIdx.x == 0 && blockIdx.x < 256;
  const bool ts_last = ts && threadIdx.x == 0 && blockIdx.x + 1024 >= gridDim.x;
  if (ts_first) atomicMin(&ts[0], wall_clock64());
  if (!active[b]) {  // inactive slots: output unused by the reference (core/asr.rs:221-223)
    if (ts_last) atomicMax(&ts[1], wall_clock64());
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane / LPK, li = lane % LPK;
  float* sc = lds;                       // [T][ctx]
  float* red = lds + T * ctx;            // [NW][T][HD] then small scratch
  float* scratch = red + NW * T * HD;    // [16]

  const uint32_t sp = start_pos[b];
  const long e1 = (long)sp + T - 1;
  const int nvalid = (int)((e1 + 1 < (long)ctx) ? e1 + 1 : ctx);  // slots > e1 were never written
  const float scale = (float)(1.0 / sqrt((double)HD));

  const KVT* Kb = kcache + ((long)b * H + h) * ctx * HD;
  const KVT* Vb = vcache + ((long)b * H + h) * ctx * HD;
  if (!kcache) {  // the row's own K / V block (every lane loaded the same entry: back to scalar registers)
    const uint64_t kp = ((uint64_t)__builtin_amdgcn_readfirstlane(rs_kv.y) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(rs_kv.x);
    const uint64_t vp = ((uint64_t)__builtin_amdgcn_readfirstlane(rs_kv.w) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(rs_kv.z);
    Kb = attn_row_base<KVT>(kp) + (long)h * ctx * HD;
    Vb = attn_row_base<KVT>(vp) + (long)h * ctx * HD;
  }
  if (T == 1 && fq.ws) {
    // row m = b of the [M][3d] QKV product: q at n = h*HD + i, k at d + ..., v at 2d + ... (core/batched_transformer.rs:77-82)
    if (tid < (fq.q_only ? HD / 4 : 3 * HD / 4)) {
      const int part = tid / (HD / 4), i0 = 4 * (tid % (HD / 4));
      const f32x4 v = slab_sum(fq.ws + (long)b * fq.ld + part * d + h * HD + i0, fq.cstride, fq.chunks);
      float o[4] = {v[0], v[1], v[2], v[3]};
      if (part < 2 && fq.rope_cs) {  // rope_i on interleaved pairs — core/transformer.rs:373-377
        const float4 cs = *reinterpret_cast<const float4*>(fq.rope_cs + ((long)b * (HD / 2) + (i0 >> 1)) * 2);
        const float co[2] = {cs.x, cs.z}, si[2] = {cs.y, cs.w};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          float x0 = v[2 * p], x1 = v[2 * p + 1];
          float t0 = x0 * co[p], t1 = x1 * si[p], t2 = x0 * si[p], t3 = x1 * co[p];
          o[2 * p] = t0 - t1;
          o[2 * p + 1] = t2 + t3;
        }
      }
      if (part == 0) {
        red[i0] = o[0]; red[i0 + 1] = o[1]; red[i0 + 2] = o[2]; red[i0 + 3] = o[3];  // q staged in the (still unused) red area; ctx*4 B is not a multiple of 16: scalar accesses
      } else {
        KVT* row = const_cast<KVT*>(part == 1 ? Kb : Vb) + (long)fq.widx[b] * HD + i0;
        store_kv4(row, o);
      }
    }
    __syncthreads();  // q visible in LDS; this workgroup's K/V row visible to its own loads below
  }
  float qv[T][8];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (T == 1 && fq.ws) {
#pragma unroll
      for (int dd = 0; dd < 8; ++dd) qv[t][dd] = red[8 * li + dd];
    } else {
      const float* qp = qbuf + ((long)(b * T + t)) * d + h * HD + 8 * li;
      float4 q0 = *reinterpret_cast<const float4*>(qp), q1 = *reinterpret_cast<const float4*>(qp + 4);
      qv[t][0] = q0.x; qv[t][1] = q0.y; qv[t][2] = q0.z; qv[t][3] = q0.w;
      qv[t][4] = q1.x; qv[t][5] = q1.y; qv[t][6] = q1.z; qv[t][7] = q1.w;
    }
  }
  if (T == 1 && fq.ws) __syncthreads();  // every lane holds its q before `red` is reused for the partial outputs

  // ---- phase 1: scores.  Software-pipelined: while one batch of UNR keys per lane is reduced, the next batch's
  // 16-byte loads are already in flight (raw cache words, converted at use), so a wave keeps UNR..2*UNR loads
  // outstanding instead of draining to zero every iteration.  Out-of-range keys are clamped to the last valid row
  // (loaded, never used) so that the loads need no branches. ----
  constexpr int UNR = sizeof(KVT) == 2 ? UNRB : 4;
  constexpr int STEP = UNR * NW * G;
  const int jlast = nvalid - 1;
  const int last_slot = (int)(e1 % ctx);  // ring slot holding the newest key
  Raw8<KVT> ra[UNR], rb[UNR];
#define DSM_ISSUE(R, BASE, J0)                                                        \
  _Pragma("unroll") for (int u = 0; u < UNR; ++u) {                                    \
    const int jj = min((J0) + u * NW * G + g, jlast);                                  \
    if (fq.nt) R[u].load_nt(BASE + (long)jj * HD + 8 * li);                            \
    else R[u].load(BASE + (long)jj * HD + 8 * li);                                     \
  }
#define DSM_SCORES(R, J0)                                                              \
  _Pragma("unroll") for (int u = 0; u < UNR; ++u) {                                    \
    const int j = (J0) + u * NW * G + g;                                               \
    int delta = last_slot - min(j, jlast); /* == (e1 - j) mod ctx, no 64-bit division */ \
    delta += (delta < 0) ? ctx : 0;                                                    \
    float kv[8];                                                                       \
    R[u].unpack(kv);                                                                   \
    _Pragma("unroll") for (int t = 0; t < T; ++t) {                                    \
      float p = 0.0f;                                                                  \
      _Pragma("unroll") for (int dd = 0; dd < 8; ++dd) p = DSM_FMAF(qv[t][dd], kv[dd], p); \
      _Pragma("unroll") for (int off = LPK / 2; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64); \
      if (li == 0 && j < nvalid) sc[t * ctx + j] = (delta >= T - 1 - t) ? p * scale : -DSM_INF_F; \
    }                                                                                  \
  }
  {
    int j0 = wave * G;
    DSM_ISSUE(ra, Kb, j0)
    while (j0 < nvalid) {
      DSM_ISSUE(rb, Kb, j0 + STEP)
      DSM_SCORES(ra, j0)
      j0 += STEP;
      if (j0 >= nvalid) break;
      DSM_ISSUE(ra, Kb, j0 + STEP)
      DSM_SCORES(rb, j0)
      j0 += STEP;
    }
  }
  // the first batch of V rows does not depend on the softmax: put it in flight across the statistics phase
  DSM_ISSUE(ra, Vb, wave * G)
  __syncthreads();

  // ---- phase 1.5: softmax statistics (softmax_last_dim) ----
  float lsum[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float m = -DSM_INF_F;
    for (int j = tid; j < nvalid; j += 256) m = fmaxf(m, sc[t * ctx + j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) scratch[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
    __syncthreads();
    float tp = 0.0f;
    for (int j = tid; j < nvalid; j += 256) {
      float p = dsm_expf(sc[t * ctx + j] - m);
      sc[t * ctx + j] = p;
      tp = tp + p;
    }
    tp = wave_sum64(tp);
    if (lane == 0) scratch[4 + wave] = tp;
    __syncthreads();
    lsum[t] = ((scratch[4] + scratch[5]) + scratch[6]) + scratch[7];
    __syncthreads();
  }

  // ---- phase 2: P.V ----
  float acc[T][8];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) acc[t][dd] = 0.0f;
#define DSM_PV(R, J0)                                                                  \
  _Pragma("unroll") for (int u = 0; u < UNR; ++u) { /* ascending j per (wave, group): canonical order */ \
    const int j = (J0) + u * NW * G + g;                                               \
    float vv[8];                                                                       \
    R[u].unpack(vv);                                                                   \
    _Pragma("unroll") for (int t = 0; t < T; ++t) {                                    \
      /* out-of-range keys get weight 0: fmaf(0, v, acc) == acc for the finite v of the clamped row */ \
      const float wgt = (j < nvalid) ? sc[t * ctx + j] / lsum[t] : 0.0f;               \
      _Pragma("unroll") for (int dd = 0; dd < 8; ++dd) acc[t][dd] = DSM_FMAF(wgt, vv[dd], acc[t][dd]); \
    }                                                                                  \
  }
  {
    int j0 = wave * G;  // ra already holds this batch
    while (j0 < nvalid) {
      DSM_ISSUE(rb, Vb, j0 + STEP)
      DSM_PV(ra, j0)
      j0 += STEP;
      if (j0 >= nvalid) break;
      DSM_ISSUE(ra, Vb, j0 + STEP)
      DSM_PV(rb, j0)
      j0 += STEP;
    }
  }
#undef DSM_ISSUE
#undef DSM_SCORES
#undef DSM_PV
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) {
      float v = acc[t][dd];
#pragma unroll
      for (int off = 32; off >= LPK; off >>= 1) v = v + __shfl_xor(v, off, 64);
      acc[t][dd] = v;
    }
  if (g == 0) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int dd = 0; dd < 8; ++dd) red[(wave * T + t) * HD + 8 * li + dd] = acc[t][dd];
  }
  __syncthreads();
  for (int i = tid; i < T * HD; i += 256) {
    int t = i / HD, dd = i % HD;
    float tot = ((red[(0 * T + t) * HD + dd] + red[(1 * T + t) * HD + dd]) + red[(2 * T + t) * HD + dd]) +
                red[(3 * T + t) * HD + dd];
    out[((long)(b * T + t)) * d + h * HD + dd] = tot;
  }
  if (ts_last) atomicMax(&ts[1], wall_clock64());
}

// ---- attention over a SHORT ring (r04): T = 1, at most 32 positions, head_dim 64 — the DepFormer's rings (one position per
// codebook slice) and their cousins in small test models.  attn_kernel spends a 256-thread workgroup, five barriers and a
// 128-key software pipeline on what is at most 32 keys; here one WAVE owns a (slot, head) and a workgroup four of them.
// Same arithmetic, same canonical order: key j belongs to canonical wave j / 8 and lane group j % 8, so the physical wave walks
// the four canonical waves' keys (one key per lane group each), keeps the four partial outputs apart, folds each over its lane
// groups with the same butterfly (offsets 32, 16, 8) and adds them left to right; the softmax sum sits one probability per lane
// (thread j of canonical wave 0 in attn_kernel) under the same 64-lane butterfly, the other canonical waves contribute +0.
// Keys beyond the valid range contribute fma(0, v, +0) = +0 there and nothing here.
template <typename KVT, int HD>
__global__ __launch_bounds__(256) void attn_small_kernel(float* __restrict__ out, const float* __restrict__ qbuf,
                                                         const KVT* __restrict__ kcache, const KVT* __restrict__ vcache,
                                                         const uint32_t* __restrict__ start_pos, const uint8_t* __restrict__ active,
                                                         int BH, int H, int ctx, int d, AttnFused fq) {
  static_assert(HD == 64, "one lane group of 8 lanes per key");
  constexpr int LPK = HD / 8;
  __shared__ __attribute__((aligned(16))) float lds_all[4][32 + HD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int unit = blockIdx.x * 4 + wave;
  const int uc = unit < BH ? unit : BH - 1;
  const int b = uc / H, h = uc % H;
  const bool on = unit < BH && active[b];
  float* sc = lds_all[wave];  // [32] scores, then probabilities
  float* qs = sc + 32;        // [HD] the query (fused prologue)
  const int g = lane / LPK, li = lane % LPK;
  const uint32_t sp = start_pos[b];
  const long e1 = (long)sp;
  const int nvalid = (int)((e1 + 1 < (long)ctx) ? e1 + 1 : ctx);
  const float scale = (float)(1.0 / sqrt((double)HD));
  const KVT* Kb = kcache + ((long)b * H + h) * ctx * HD;
  const KVT* Vb = vcache + ((long)b * H + h) * ctx * HD;
  if (!kcache) {  // the row's own K / V block, as in attn_kernel
    Kb = attn_row_base<KVT>((uint64_t)fq.src[b].k) + (long)h * ctx * HD;
    Vb = attn_row_base<KVT>((uint64_t)fq.src[b].v) + (long)h * ctx * HD;
  }
  if (fq.ws) {  // attn_kernel's prologue, lane for thread
    if (on && lane < (fq.q_only ? HD / 4 : 3 * HD / 4)) {
      const int part = lane / (HD / 4), i0 = 4 * (lane % (HD / 4));
      const f32x4 v = slab_sum(fq.ws + (long)b * fq.ld + part * d + h * HD + i0, fq.cstride, fq.chunks);
      float o[4] = {v[0], v[1], v[2], v[3]};
      if (part < 2 && fq.rope_cs) {
        const float4 cs = *reinterpret_cast<const float4*>(fq.rope_cs + ((long)b * (HD / 2) + (i0 >> 1)) * 2);
        const float co[2] = {cs.x, cs.z}, si[2] = {cs.y, cs.w};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          float x0 = v[2 * p], x1 = v[2 * p + 1];
          float t0 = x0 * co[p], t1 = x1 * si[p], t2 = x0 * si[p], t3 = x1 * co[p];
          o[2 * p] = t0 - t1;
          o[2 * p + 1] = t2 + t3;
        }
      }
      if (part == 0) {
        qs[i0] = o[0]; qs[i0 + 1] = o[1]; qs[i0 + 2] = o[2]; qs[i0 + 3] = o[3];
      } else {
        KVT* row = const_cast<KVT*>(part == 1 ? Kb : Vb) + (long)fq.widx[b] * HD + i0;
        store_kv4(row, o);
      }
    }
    __syncthreads();  // the new K / V row is visible to this workgroup's loads (every wave arrives: no wave has left yet)
  }
  if (!on) return;
  float qv[8];
  if (fq.ws) {
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) qv[dd] = qs[8 * li + dd];
  } else {
    const float* qp = qbuf + (long)b * d + h * HD + 8 * li;
    const float4 q0 = *reinterpret_cast<const float4*>(qp), q1 = *reinterpret_cast<const float4*>(qp + 4);
    qv[0] = q0.x; qv[1] = q0.y; qv[2] = q0.z; qv[3] = q0.w; qv[4] = q1.x; qv[5] = q1.y; qv[6] = q1.z; qv[7] = q1.w;
  }
  const int jlast = nvalid - 1;
  Raw8<KVT> rk[4], rv[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int jj = min(8 * w + g, jlast);  // clamped: loaded, never used
    rk[w].load(Kb + (long)jj * HD + 8 * li);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int jj = min(8 * w + g, jlast);
    rv[w].load(Vb + (long)jj * HD + 8 * li);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int j = 8 * w + g;
    float kv[8];
    rk[w].unpack(kv);
    float p = 0.0f;
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) p = DSM_FMAF(qv[dd], kv[dd], p);
#pragma unroll
    for (int off = LPK / 2; off >= 1; off >>= 1) p = p + __shfl_xor(p, off, 64);
    if (li == 0 && j < nvalid) sc[j] = p * scale;  // T = 1: every written slot is visible
  }
  // softmax_last_dim: thread j of canonical wave 0 owns probability j
  float m = -DSM_INF_F;
  if (lane < nvalid) m = fmaxf(m, sc[lane]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  float tp = 0.0f;
  if (lane < nvalid) {
    const float p = dsm_expf(sc[lane] - m);
    sc[lane] = p;
    tp = tp + p;
  }
  tp = wave_sum64(tp);
  const float lsum = ((tp + 0.0f) + 0.0f) + 0.0f;  // canonical waves 1..3 hold no probability
  float tot[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int j = 8 * w + g;
    float vv[8];
    rv[w].unpack(vv);
    const float wgt = (j < nvalid) ? sc[j] / lsum : 0.0f;
#pragma unroll
    for (int dd = 0; dd < 8; ++dd) {
      float v = (j < nvalid) ? DSM_FMAF(wgt, vv[dd], 0.0f) : 0.0f;
#pragma unroll
      for (int off = 32; off >= LPK; off >>= 1) v = v + __shfl_xor(v, off, 64);
      tot[dd] = w == 0 ? v : tot[dd] + v;  // ((r0 + r1) + r2) + r3
    }
  }
  if (g == 0) {
    float* o = out + (long)b * d + h * HD + 8 * li;
    *reinterpret_cast<float4*>(o) = make_float4(tot[0], tot[1], tot[2], tot[3]);
    *reinterpret_cast<float4*>(o + 4) = make_float4(tot[4], tot[5], tot[6], tot[7]);
  }
}

// ------------------------------------------------------------------------------------------
// ScatteredCacheBuilder step on the device (core/kv_cache.rs:119-237): write slots, start
// positions, advance for active slots, and the RoPE table for the positions AFTER the advance
// (core/batched_transformer.rs:438-447).
// ------------------------------------------------------------------------------------------
__global__ void kv_builder_kernel(uint32_t* __restrict__ pos, uint32_t* __restrict__ idx,
                                  const uint8_t* __restrict__ active, uint32_t* __restrict__ start_pos,
                                  uint32_t* __restrict__ widx, float* __restrict__ rope_cs,
                                  const float* __restrict__ inv_freq, int B, int T, int ctx, int hd,
                                  int rope_before) {
  // rope_before: the non-batched transformer rotates by current_seq_len BEFORE the append (core/transformer.rs:925-926);
  // the batched one reads the builder's positions after indices_and_mask advanced them
  const int b = blockIdx.x;
  if (b >= B) return;
  __shared__ uint32_t s_pos_after;
  if (threadIdx.x == 0) {
    uint32_t p = pos[b], i = idx[b];
    const uint32_t p0 = p;
    start_pos[b] = p;
    for (int t = 0; t < T; ++t) widx[b * T + t] = active[b] ? (uint32_t)((i + t) % ctx) : i;
    if (active[b]) {
      pos[b] = p + T;
      idx[b] = (uint32_t)((i + T) % ctx);
      p += T;
    }
    s_pos_after = rope_before ? p0 : p;
  }
  __syncthreads();
  if (rope_cs) {
    const int half = hd / 2;
    for (int e = threadIdx.x; e < T * half; e += blockDim.x) {
      int t = e / half, i = e % half;
      float ang = (float)(s_pos_after + (uint32_t)t) * inv_freq[i];
      float s, c;
      dsm_sincosf(ang, &s, &c);
      rope_cs[((long)(b * T + t) * half + i) * 2] = c;
      rope_cs[((long)(b * T + t) * half + i) * 2 + 1] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------
// ASR glue — core/asr.rs:165-189 (token shift, pad select) + core/lm.rs:983-995 (embedding sum)
// one workgroup per slot.
// ------------------------------------------------------------------------------------------
__global__ void lm_input_kernel(float* __restrict__ x, const uint16_t* __restrict__ text_emb,
                                const uint16_t* __restrict__ audio_emb /* [nc][audio_vocab][d] */,
                                const uint32_t* __restrict__ codes /* [B][nc] */, uint32_t* __restrict__ next_cb,
                                const uint32_t* __restrict__ text_token, const uint8_t* __restrict__ first_step,
                                const uint8_t* __restrict__ active, int nc, int d, int audio_vocab,
                                uint32_t pad_tok, uint32_t start_tok) {
  // grid (B, d / 512): each thread sums 2 adjacent columns over the 1 + nc tables (independent 4-byte loads)
  const int b = blockIdx.x;
  __shared__ uint32_t toks[64];
  const bool first = first_step[b] != 0;
  if (threadIdx.x < nc) toks[threadIdx.x] = first ? pad_tok : next_cb[b * nc + threadIdx.x];
  __syncthreads();
  const uint32_t tt = first ? start_tok : text_token[b];
  const int j = (blockIdx.y * blockDim.x + threadIdx.x) * 2;
  if (j < d) {
    uint32_t t2 = *reinterpret_cast<const uint32_t*>(text_emb + (long)tt * d + j);
    float e0 = __uint_as_float(t2 << 16), e1 = __uint_as_float(t2 & 0xFFFF0000u);
    for (int i = 0; i < nc; ++i) {  // emb = emb + e, in codebook order — core/lm.rs:988-993
      uint32_t a2 = *reinterpret_cast<const uint32_t*>(audio_emb + ((long)i * audio_vocab + toks[i]) * d + j);
      e0 = e0 + __uint_as_float(a2 << 16);
      e1 = e1 + __uint_as_float(a2 & 0xFFFF0000u);
    }
    *reinterpret_cast<float2*>(x + (long)b * d + j) = make_float2(e0, e1);
  }
}

// next_codebooks = mask ? new codes : old (core/asr.rs:177-183); runs after lm_input_kernel consumed the old values
__global__ void lm_next_codebooks_kernel(const uint32_t* __restrict__ codes, uint32_t* __restrict__ next_cb,
                                         const uint8_t* __restrict__ active, int B, int nc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * nc && active[i / nc]) next_cb[i] = codes[i];
}

// first-occurrence argmax of one row by a 256-thread block; valid in every thread after the call
__device__ inline int block_argmax_first(const float* __restrict__ lg, int V) {
  float bv = -DSM_INF_F;
  int bi = 0x7FFFFFFF;
  for (int j = threadIdx.x; j < V; j += blockDim.x) {
    float v = lg[j];
    if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
  }
  __shared__ float sv[256];
  __shared__ int si[256];
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int off = blockDim.x / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      float ov = sv[threadIdx.x + off];
      int oi = si[threadIdx.x + off];
      if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
        sv[threadIdx.x] = ov;
        si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  const int r = si[0] == 0x7FFFFFFF ? 0 : si[0];  // all-NaN row: index 0, like a `>` scan from element 0
  __syncthreads();
  return r;
}

// argmax over the text logits (first occurrence on ties, core/asr.rs:208-210) + item-state update
__global__ void lm_argmax_kernel(const float* __restrict__ logits, int V, uint32_t* __restrict__ text_out,
                                 uint32_t* __restrict__ text_token, uint8_t* __restrict__ first_step,
                                 const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  const uint32_t tok = (uint32_t)block_argmax_first(logits + (long)b * V, V);
  if (threadIdx.x == 0) {
    text_out[b] = tok;
    if (active[b]) {
      text_token[b] = tok;
      first_step[b] = 0;
    }
  }
}

// temperature > 0 (r04): candle_nn::sampling::gumbel_softmax of the text logits — core/asr.rs:211-215, dsm_sampling.h
// dsm_gumbel_value — with one seeded ChaCha12 stream per slot: entry j of the step takes word pos + j (pos a multiple of 16: a
// thread produces whole blocks), argmax with first occurrence on ties; an active slot's stream advances by V rounded up to 16.
__global__ void lm_gumbel_kernel(const float* __restrict__ logits, int V, float temperature, const uint32_t* __restrict__ rng_key,
                                 unsigned long long* __restrict__ rng_pos, uint32_t* __restrict__ text_out,
                                 uint32_t* __restrict__ text_token, uint8_t* __restrict__ first_step,
                                 const uint8_t* __restrict__ active) {
  const int b = blockIdx.x;
  const float* lg = logits + (long)b * V;
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = rng_key[b * 8 + i];
  const unsigned long long pos = rng_pos[b];
  float bv = -DSM_INF_F;
  int bi = 0x7FFFFFFF;
  const int nblk = (V + 15) >> 4;
  for (int blk = threadIdx.x; blk < nblk; blk += blockDim.x) {
    uint32_t w[16];
    dsm_chacha_block(key, (pos >> 4) + (unsigned long long)blk, 12, w);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = 16 * blk + i;
      if (j < V) {
        const float v = dsm_gumbel_value(lg[j], w[i], temperature);
        if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
      }
    }
  }
  __shared__ float sv[256];
  __shared__ int si[256];
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int off = blockDim.x / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const float ov = sv[threadIdx.x + off];
      const int oi = si[threadIdx.x + off];
      if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const uint32_t tok = si[0] == 0x7FFFFFFF ? 0u : (uint32_t)si[0];
    text_out[b] = tok;
    if (active[b]) {
      text_token[b] = tok;
      first_step[b] = 0;
      rng_pos[b] = pos + 16ull * (unsigned long long)nblk;
    }
  }
}

__device__ __forceinline__ float dsm_unpaired(float v);  // below, with the SEANet front end that first needed it

// Token scores (dsm_token_scores.h; this project's own, off by default): log-probability of the step's text token and the top_n
// best entries of its logits row.  One 256-thread workgroup per batch row, launched behind lm_argmax_kernel / lm_gumbel_kernel on
// the same stream, whose text_out it reads.  1 + max(top_n, 1) passes over the row, any V >= 1.  STAGED (rows up to
// DSM_SCORES_STAGE_MAX floats: 32 KB at V = 8000): the first pass copies the row into dynamic LDS and the others read it there —
// thread t only ever touches entries j = t (mod 256), its own copies, so the row needs no barrier; a longer row is re-read from
// L2 in every pass.  Every pick is a block reduction over (value, id) pairs in the order "value descending, id ascending"
// restricted to the entries behind the previous pick — exact, no float sort; the exp-sum follows the lane / tree order of the
// header, so the host function gives the same bits.
// lp [rows], top_id / top_lp [rows][DSM_SCORES_MAX_TOP]: entries top_n .. 7 are written as padding.
#define DSM_SCORES_STAGE_MAX 15360  // 60 KB of dynamic LDS beside 1 KB static: inside the default 64 KB per workgroup
struct ScorePick {
  float v;
  uint32_t i;
};
// first of the order among the block's candidates; the same in every thread after the call.  sv / si: 4 entries of LDS.
__device__ inline ScorePick block_score_first(float bv, uint32_t bi, float* sv, uint32_t* si) {
  for (int off = 32; off >= 1; off >>= 1) {  // (a lane beyond the wave's end gets its own pair back: harmless for a maximum)
    const float ov = __shfl_down(bv, off);
    const uint32_t oi = (uint32_t)__shfl_down((int)bi, off);
    if (dsm_score_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = bv;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = sv[0];
  bi = si[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (dsm_score_before(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
  __syncthreads();
  return ScorePick{bv, bi};
}

template <bool STAGED>
__global__ void __launch_bounds__(256) lm_token_scores_kernel(const float* __restrict__ logits, int V, const uint32_t* __restrict__ text_out,
                                                              int top_n, float* __restrict__ lp, uint32_t* __restrict__ top_id,
                                                              float* __restrict__ top_lp) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (long)b * V;
  extern __shared__ __align__(16) float srow[];  // STAGED: V floats
  __shared__ float sv[4];
  __shared__ uint32_t si[4];
  __shared__ float sp[DSM_SCORES_LANES];
  // A thread walks its entries UN at a time: UN independent loads in flight, then the compares in ascending j.  An entry
  // beyond the row is a NaN, which no comparison picks.
  constexpr int UN = 8, STEP = UN * DSM_SCORES_LANES;
  const float beyond = dsm_u32_as_f32(0x7FC00000u);
  // round 0: the first entry of the order, whose value is m; the pass that stages the row
  float bv = -DSM_INF_F;
  uint32_t bi = DSM_SCORES_NONE;
  for (int j0 = tid; j0 < V; j0 += STEP) {
    float v[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) v[k] = j0 + k * DSM_SCORES_LANES < V ? lg[j0 + k * DSM_SCORES_LANES] : beyond;
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int j = j0 + k * DSM_SCORES_LANES;
      if (STAGED && j < V) srow[j] = v[k];
      if (dsm_score_before(v[k], (uint32_t)j, bv, bi)) { bv = v[k]; bi = (uint32_t)j; }
    }
  }
  ScorePick prev = block_score_first(bv, bi, sv, si);
  if (prev.i == DSM_SCORES_NONE) prev.v = -DSM_INF_F;  // a row of NaN alone
  const float m = prev.v;
  // the picks: round r's stays in thread r's registers (top_n <= 8 < 256)
  float my_v = prev.v;
  uint32_t my_i = prev.i;
  for (int r = 1; r < top_n; ++r) {
    bv = -DSM_INF_F;
    bi = DSM_SCORES_NONE;
    if (prev.i != DSM_SCORES_NONE) {
      for (int j0 = tid; j0 < V; j0 += STEP) {
        float v[UN];
#pragma unroll
        for (int k = 0; k < UN; ++k) {
          const int j = j0 + k * DSM_SCORES_LANES;
          v[k] = j < V ? (STAGED ? srow[j] : lg[j]) : beyond;
        }
#pragma unroll
        for (int k = 0; k < UN; ++k) {
          const uint32_t j = (uint32_t)(j0 + k * DSM_SCORES_LANES);
          if (dsm_score_behind(v[k], j, prev.v, prev.i) && dsm_score_before(v[k], j, bv, bi)) { bv = v[k]; bi = j; }
        }
      }
    }
    prev = block_score_first(bv, bi, sv, si);
    if (prev.i == DSM_SCORES_NONE) prev.v = -DSM_INF_F;
    if (tid == r) { my_v = prev.v; my_i = prev.i; }
  }
  float p = 0.0f;
  for (int j0 = tid; j0 < V; j0 += STEP) {  // the lane's terms in ascending j, one f32 add each
    float v[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int j = j0 + k * DSM_SCORES_LANES;
      v[k] = j < V ? (STAGED ? srow[j] : lg[j]) : beyond;
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) v[k] = dsm_expf(dsm_unpaired(v[k] - m));
#pragma unroll
    for (int k = 0; k < UN; ++k)
      if (j0 + k * DSM_SCORES_LANES < V) p = dsm_unpaired(p + v[k]);
  }
  sp[tid] = p;
  __syncthreads();
  if (tid < 128) sp[tid] = sp[tid] + sp[tid + 128];
  __syncthreads();
  if (tid < 64) {  // wave 0: lane t of level `off` adds lane t + off, which is the tree of dsm_score_tree_sum for t < off
    float q = sp[tid] + sp[tid + 64];
    for (int off = 32; off >= 1; off >>= 1) q = q + __shfl_down(q, off);
    if (tid == 0) sp[0] = q;
  }
  __syncthreads();
  const float log_s = dsm_logf(sp[0]);
  if (tid == 0) {
    const uint32_t tok = text_out[b];
    lp[b] = tok < (uint32_t)V ? dsm_score_logprob(lg[tok], m, log_s) : dsm_u32_as_f32(0x7FC00000u);
  }
  if (tid < DSM_SCORES_MAX_TOP) {
    const bool have = tid < top_n && my_i != DSM_SCORES_NONE;
    top_id[(long)b * DSM_SCORES_MAX_TOP + tid] = have ? my_i : DSM_SCORES_NONE;
    top_lp[(long)b * DSM_SCORES_MAX_TOP + tid] = have ? dsm_score_logprob(my_v, m, log_s) : -DSM_INF_F;
  }
}

// Text bias (dsm_text_bias.h; this project's own, off by default): the pick of the step's text token over x = raw logits + the
// slot's token biases + the boosts of its trie node's edges, and the node's advance.  Stands in for lm_argmax_kernel /
// lm_gumbel_kernel when dsm_asr_set_text_bias is on: one 256-thread workgroup per batch row of the stream group, one launch, none
// added.  The row is staged in dynamic LDS (V <= DSM_SCORES_STAGE_MAX, which the switch checks), the two lists are scatter-added
// there — their entries are distinct, so no atomics; a barrier between them fixes the order of the two adds on a token that is in
// both — and the pick reads LDS: the raw logits in global memory stay as the GEMM wrote them.  The lists are reached through
// engine-owned memory only — `sets` (DSM_BIAS_MAX_SETS descriptors; entry 0 is "no set"), the slot's set index and node — so
// every launch argument is an engine buffer and the step replays as one hipGraph.  The maximum is exact and first-occurrence,
// so the reduction tree's shape cannot show in the result; it is block_argmax_first's.
struct BiasSetDesc {
  const uint32_t* table;  // the set's flat table (dsm_text_bias.h), device memory; null in entry 0 and in free entries
  uint32_t n_tokens, n_nodes, n_edges, reserved;
};

template <bool GUMBEL>
__global__ void __launch_bounds__(256) lm_pick_biased_kernel(const float* __restrict__ logits, int V, float temperature,
                                                             const uint32_t* __restrict__ rng_key, unsigned long long* __restrict__ rng_pos,
                                                             const BiasSetDesc* __restrict__ sets, const uint32_t* __restrict__ slot_set,
                                                             uint32_t* __restrict__ slot_node, uint32_t* __restrict__ text_out,
                                                             uint32_t* __restrict__ text_token, uint8_t* __restrict__ first_step,
                                                             const uint8_t* __restrict__ active) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (long)b * V;
  extern __shared__ __align__(16) float xrow[];  // V floats
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ uint32_t s_child;
  const uint32_t set = slot_set[b];
  const bool has_set = set != 0 && set < DSM_BIAS_MAX_SETS;
  BiasSetDesc d{nullptr, 0u, 0u, 0u, 0u};
  if (has_set) d = sets[set];
  const uint32_t node = has_set && d.table ? slot_node[b] : DSM_BIAS_DEAD;
  const bool live = node < d.n_nodes;  // DEAD (0xFFFFFFFF) is never below a node count
  // 1: stage the row; thread t owns entries j = t (mod 256), UN independent loads in flight
  constexpr int UN = 8, STEP = UN * 256;
  for (int j0 = tid; j0 < V; j0 += STEP) {
    float v[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) v[k] = j0 + k * 256 < V ? lg[j0 + k * 256] : 0.0f;
#pragma unroll
    for (int k = 0; k < UN; ++k)
      if (j0 + k * 256 < V) xrow[j0 + k * 256] = v[k];
  }
  if (tid == 0) s_child = DSM_BIAS_DEAD;
  __syncthreads();
  // 2: token biases (a list longer than the block is walked in strides)
  if (d.table) {
    const uint32_t* tb = dsm_bias_tokens_of(d.table);
    for (uint32_t i = tid; i < d.n_tokens; i += 256) {
      const uint32_t t = tb[2u * i];
      if (t < (uint32_t)V) xrow[t] = dsm_unpaired(xrow[t] + dsm_u32_as_f32(tb[2u * i + 1u]));
    }
  }
  __syncthreads();
  // 3: the node's edges, behind the barrier: (l + bias) + boost
  const uint32_t* edges = nullptr;
  uint32_t eb = 0, ee = 0;
  if (live) {
    const uint32_t* first = dsm_bias_first_of(d.table, d.n_tokens);
    edges = dsm_bias_edges_of(d.table, d.n_tokens, d.n_nodes);
    eb = first[node];
    ee = first[node + 1];
    if (ee > d.n_edges) ee = d.n_edges;
    for (uint32_t e = eb + tid; e < ee; e += 256) {
      const uint32_t t = edges[3u * e];
      if (t < (uint32_t)V) xrow[t] = dsm_unpaired(xrow[t] + dsm_u32_as_f32(edges[3u * e + 1u]));
    }
  }
  __syncthreads();
  // 4: the pick over the LDS row
  float bv = -DSM_INF_F;
  int bi = 0x7FFFFFFF;
  unsigned long long pos = 0;
  const int nblk = (V + 15) >> 4;
  if (GUMBEL) {
    uint32_t key[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) key[i] = rng_key[b * 8 + i];
    pos = rng_pos[b];
    for (int blk = tid; blk < nblk; blk += 256) {
      uint32_t w[16];
      dsm_chacha_block(key, (pos >> 4) + (unsigned long long)blk, 12, w);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = 16 * blk + i;
        if (j < V) {
          const float v = dsm_gumbel_value(xrow[j], w[i], temperature);
          if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
        }
      }
    }
  } else {
    for (int j = tid; j < V; j += 256) {
      const float v = xrow[j];
      if (v > bv || (v == bv && j < bi)) { bv = v; bi = j; }
    }
  }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
      const float ov = sv[tid + off];
      const int oi = si[tid + off];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
    }
    __syncthreads();
  }
  const uint32_t tok = si[0] == 0x7FFFFFFF ? 0u : (uint32_t)si[0];
  // 5: the picked token among the node's edges — tokens are distinct inside a node, so at most one thread finds it
  for (uint32_t e = eb + tid; e < ee; e += 256)
    if (edges[3u * e] == tok) s_child = edges[3u * e + 2u];
  __syncthreads();
  if (tid == 0) {
    text_out[b] = tok;
    if (active[b]) {
      text_token[b] = tok;
      first_step[b] = 0;
      if (GUMBEL) rng_pos[b] = pos + 16ull * (unsigned long long)nblk;
      if (has_set && d.table) slot_node[b] = dsm_bias_advance(node, tok, live ? s_child : DSM_BIAS_DEAD);
    }
  }
}

// ------------------------------------------------------------------------------------------
// TTS glue — core/tts_streaming.rs:117-242, core/lm.rs:640-684, :983-995
// ------------------------------------------------------------------------------------------

// tokens [B][1+nc] int32: text token, then one entry per codebook; -1 = None ("literal zeros": the embedding is skipped)
// x, xin ("lm.input": x is overwritten by the layers) and tokens start at the group's first row r0.  cond [slots][d] / cond_on
// [slots] are the whole batch's: a slot whose flag is set adds its Condition::AddToInput row last, to every row it owns
// (emb.broadcast_add(v), core/lm.rs:996-1000,1062-1066).  Behind the flag, never a zero row: x + 0.0f would turn -0.0f into +0.0f.
__global__ void tts_input_kernel(float* __restrict__ x, float* __restrict__ xin, const uint16_t* __restrict__ text_emb,
                                 const uint16_t* __restrict__ audio_emb /* [nc][audio_vocab][d] */,
                                 const int32_t* __restrict__ tokens, int nc, int d, int audio_vocab,
                                 const float* __restrict__ cond, const uint8_t* __restrict__ cond_on, int r0, int rps) {
  const int b = blockIdx.x;
  __shared__ int32_t toks[72];
  if ((int)threadIdx.x < 1 + nc) toks[threadIdx.x] = tokens[b * (1 + nc) + threadIdx.x];
  __syncthreads();
  const int j = (blockIdx.y * blockDim.x + threadIdx.x) * 2;
  if (j < d) {
    uint32_t t2 = *reinterpret_cast<const uint32_t*>(text_emb + (long)toks[0] * d + j);
    float e0 = __uint_as_float(t2 << 16), e1 = __uint_as_float(t2 & 0xFFFF0000u);
    for (int i = 0; i < nc; ++i) {
      const int32_t t = toks[1 + i];
      if (t < 0) continue;
      uint32_t a2 = *reinterpret_cast<const uint32_t*>(audio_emb + ((long)i * audio_vocab + t) * d + j);
      e0 = e0 + __uint_as_float(a2 << 16);
      e1 = e1 + __uint_as_float(a2 & 0xFFFF0000u);
    }
    const int slot = (r0 + b) / rps;
    if (cond_on[slot]) {
      const float2 c = *reinterpret_cast<const float2*>(cond + (long)slot * d + j);
      e0 = dsm_unpaired(e0 + c.x);  // two scalar adds, not a v_pk_add_f32
      e1 = dsm_unpaired(e1 + c.y);
    }
    *reinterpret_cast<float2*>(x + (long)b * d + j) = make_float2(e0, e1);
    *reinterpret_cast<float2*>(xin + (long)b * d + j) = make_float2(e0, e1);
  }
}

// One slot's Condition::AddToInput row (core/conditioner.rs:50-58 condition_lut, :102-110 condition_cont, :168-175 learnt_padding):
// row[j] = sum_k in[k] * W[j][k], ONE f32 fma chain per output element over k = 0 .. dim - 1 ascending, starting from 0.
// in [dim]: the LUT's embedding row, or the sin embedding already rounded to bf16; W [d][dim] = output_proj.weight.
// W == nullptr: row = in [d] (learnt_padding).  Sets the slot's flag behind the row; one launch per dsm_tts_set_condition_* call.
__global__ void tts_cond_row_kernel(float* __restrict__ row, uint8_t* __restrict__ on, const float* __restrict__ in,
                                    const float* __restrict__ W, int d, int dim) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < d) {
    float acc = 0.0f;
    if (W) {
      const float* w = W + (long)j * dim;
      for (int k = 0; k < dim; ++k) acc = __builtin_fmaf(in[k], w[k], acc);
    } else {
      acc = in[j];
    }
    row[j] = acc;
  }
  if (j == 0) *on = 1;
}

// Seeded top-k sampling of one row by a 256-thread block (dsm_sampling.h: LogitsProcessor with Sampling::TopK).
// keys: LDS, vpad (power of two >= V) u64 entries; scratch: LDS, 9 floats.  Returns the token in every thread and
// advances the slot's generator by one word.  Reductions follow the canonical block order (thread t owns j = t mod 256
// ascending, wave butterflies, four wave totals left to right); the bitonic sort orders unique keys, so its network
// shape does not matter.
struct SampleArgs {
  const int32_t* top_k;   // [B]: 0 = ArgMax
  const float* inv_t;     // [B]: (float)(1 / temperature)
  const uint32_t* key;    // [B][8] ChaCha key
  uint32_t* pos;          // [B] words drawn so far from this processor's stream
  int vpad;
};
__device__ inline uint32_t block_sample_topk(const float* __restrict__ lg, int V, int k, float invT,
                                             const uint32_t* __restrict__ key, uint32_t* __restrict__ pos, int vpad,
                                             uint64_t* keys, float* scratch) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float m = -DSM_INF_F;
  for (int j = tid; j < V; j += 256) m = fmaxf(m, lg[j] * invT);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (lane == 0) scratch[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(scratch[0], scratch[1]), fmaxf(scratch[2], scratch[3]));
  float tp = 0.0f;
  for (int j = tid; j < V; j += 256) {
    const float e = dsm_expf(lg[j] * invT - m);
    keys[j] = (uint64_t)__float_as_uint(e);
    tp = tp + e;
  }
  tp = wave_sum64(tp);
  if (lane == 0) scratch[4 + wave] = tp;
  __syncthreads();
  const float sum = ((scratch[4] + scratch[5]) + scratch[6]) + scratch[7];
  for (int j = tid; j < vpad; j += 256)
    keys[j] = j < V ? dsm_sample_key(__uint_as_float((uint32_t)keys[j]) / sum, (uint32_t)j) : 0ull;
  __syncthreads();
  if (k < V) {  // bitonic sort, descending
    for (int size = 2; size <= vpad; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < (vpad >> 1); i += 256) {
          const int lo = 2 * i - (i & (stride - 1));
          const int hi = lo + stride;
          const bool desc = (lo & size) == 0;
          const uint64_t a = keys[lo], b = keys[hi];
          if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
        }
        __syncthreads();
      }
  }
  if (tid == 0) {
    const uint32_t u = dsm_chacha_word(key, (uint64_t)*pos, 12);
    *pos = *pos + 1u;
    scratch[8] = __uint_as_float(dsm_weighted_draw(keys, k < V ? k : V, u));
  }
  __syncthreads();
  const uint32_t tok = __float_as_uint(scratch[8]);
  __syncthreads();
  return tok;
}

// text-token rule of State::step (:178-197).  allowed >= 0: Text(v); -1: Pad; -2: PadOrEpad (text_lp.sample of the text
// logits — argmax, or seeded top-k for slots configured with dsm_tts_set_sampling — decides pad vs end-of-pad unless
// force_eop, i.e. consecutive_pads > max_consecutive_pads)
__global__ void tts_text_token_kernel(const float* __restrict__ logits, int V, const int32_t* __restrict__ allowed,
                                      const uint8_t* __restrict__ force_eop, uint32_t pad, uint32_t eop,
                                      uint32_t* __restrict__ text_token, uint32_t* __restrict__ last_tok, SampleArgs sa,
                                      const uint8_t* __restrict__ active) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  if (!active[b]) return;  // a paused slot takes no step: in particular its text_lp draws nothing (r03: it used to advance the slot's generator)
  const int32_t al = allowed[b];
  uint32_t tok;
  if (al >= 0) tok = (uint32_t)al;
  else if (al == -1) tok = pad;
  else if (force_eop[b]) tok = eop;
  else {  // block-uniform branch
    uint32_t sampled;
    if (sa.top_k && sa.top_k[b] > 0)
      sampled = block_sample_topk(logits + (long)b * V, V, sa.top_k[b], sa.inv_t[b], sa.key + 8 * b, sa.pos + b, sa.vpad,
                                  reinterpret_cast<uint64_t*>(smem), reinterpret_cast<float*>(smem + 8 * (size_t)sa.vpad));
    else
      sampled = (uint32_t)block_argmax_first(logits + (long)b * V, V);
    tok = (sampled == pad) ? pad : eop;
  }
  if (threadIdx.x == 0) {
    text_token[b] = tok;
    last_tok[b] = tok;
  }
}

// e[row] = table[last_tok[row / rps]] (LowRankEmbeddings::forward with the low-rank product folded into the table at load);
// rps batch rows per slot: both rows of a guided slot take the slot's token (core/lm.rs:702-709)
__global__ void dep_gather_kernel(float* __restrict__ e, const float* __restrict__ table,
                                  const uint32_t* __restrict__ last_tok, int vocab, int D, int rps) {
  const int b = blockIdx.x;
  uint32_t t = last_tok[b / rps];
  if (t >= (uint32_t)vocab) t = 0;
  const float4* src = reinterpret_cast<const float4*>(table + (long)t * D);
  float4* dst = reinterpret_cast<float4*>(e + (long)b * D);
  for (int j = threadIdx.x; j < D / 4; j += blockDim.x) dst[j] = src[j];
}

// DepFormer slice head (r03): what dep_gather_kernel + the depformer_in GEMM's reduce/residual epilogue + kv_builder_kernel
// (T = 1, no RoPE) + row_norm_kernel did in five launches, for one batch row per workgroup (256 threads):
//   x  = emb_k[last token] + proj[row][g*D ...]   (core/lm.rs:655-661: depformer_in(xs) + emb; proj = ALL weight groups' input
//        projections of the main LM's output, one GEMM per step — they do not depend on the slice)
//   ring bookkeeping of ScatteredCacheBuilder for one new position (kv_builder_kernel's thread 0)
//   xn = norm1 of layer 0 over x, canonical row reduction (row_norm_kernel's arithmetic)
// `rv + o` of the GEMM epilogue is a single f32 add either way: same bits as the five launches.
struct DepHeadArgs {
  float* x;             // [rows][D] the slice's input (null: no head — dep_argmax_kernel's last slice)
  float* xn;            // [rows][D] norm1 of layer 0 over x
  const float* table;   // emb_k, [vocab][D]
  int vocab, D, rps;
  const float* proj;    // this slice's weight group inside the stacked projections, row stride proj_ld
  long proj_ld;
  uint32_t* pos;
  uint32_t* idx;
  const uint8_t* active;  // per batch row
  uint32_t* start_pos;
  uint32_t* widx;
  int ctx;
  const float* nw;
  const float* nb;
  float eps;
  int rms;
};
// one batch row b with the slot's token t; all 256 threads; `red` = 8 floats of LDS (a barrier separates two calls)
__device__ __forceinline__ void dep_head_row(const DepHeadArgs& h, int b, uint32_t t, float* red) {
  if (threadIdx.x == 0) {  // kv_builder_kernel, T = 1
    const uint32_t p = h.pos[b], i = h.idx[b];
    h.start_pos[b] = p;
    h.widx[b] = i;  // active: (i + 0) % ctx = i (i < ctx); inactive: i
    if (h.active[b]) {
      h.pos[b] = p + 1;
      h.idx[b] = (uint32_t)((i + 1) % h.ctx);
    }
  }
  if (t >= (uint32_t)h.vocab) t = 0;
  const int D = h.D;
  const float* er = h.table + (long)t * D;
  const float* pr = h.proj + (long)b * h.proj_ld;
  float4 v[DSM_ROW_ITS];
  float s = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int it = 0; it < DSM_ROW_ITS; ++it) {
    const int i = it * 1024 + 4 * (int)threadIdx.x;
    v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < D) {
      const float4 ev = *reinterpret_cast<const float4*>(er + i);
      const float4 pv = *reinterpret_cast<const float4*>(pr + i);
      v[it] = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
      *reinterpret_cast<float4*>(h.x + (long)b * D + i) = v[it];
      s = s + v[it].x; s2 = DSM_FMAF(v[it].x, v[it].x, s2);
      s = s + v[it].y; s2 = DSM_FMAF(v[it].y, v[it].y, s2);
      s = s + v[it].z; s2 = DSM_FMAF(v[it].z, v[it].z, s2);
      s = s + v[it].w; s2 = DSM_FMAF(v[it].w, v[it].w, s2);
    }
  }
  block_row_sums(s, s2, red);
  row_norm_apply(v, s, s2, D, h.eps, h.rms, h.nw, h.nb, h.xn + (long)b * D);
}
__global__ __launch_bounds__(256) void dep_head_kernel(DepHeadArgs h, const uint32_t* __restrict__ last_tok) {
  __shared__ float red[8];
  const int b = blockIdx.x;
  dep_head_row(h, b, last_tok[b / h.rps], red);
}

// Classifier-free guidance mix of a slot's two batch rows — core/tts_streaming.rs:166-172, core/lm.rs:718-721:
//   ((l0 * a)? - (l1 * (a - 1.))?)?   with Tensor * f64 = affine(mul, 0.): v * (mul as f32) + 0f32 on the CPU backend.
// out [B][V]; rows [B * 2][V]; slots without guidance copy row 0.  grid (ceil(V / 256), B).
__global__ void cfg_mix_kernel(float* __restrict__ out, const float* __restrict__ rows, int V, const uint8_t* __restrict__ on,
                               const float* __restrict__ fa, const float* __restrict__ fb) {
  const int b = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= V) return;
  const float l0 = rows[(long)(2 * b) * V + j];
  float o = l0;
  if (on[b]) {
    const float l1 = rows[(long)(2 * b + 1) * V + j];
    const float x = l0 * fa[b] + 0.0f, y = l1 * fb[b] + 0.0f;
    o = x - y;
  }
  out[(long)b * V + j] = o;
}

// compute_kv(CaSrc::Tokens) of one batch row — core/transformer.rs:299-318: kv [n][2][H][hd] (the in_proj_kv product) ->
// K, V [H][smax][hd] in the cache dtype (rounded like the ring cache's rows).  kc / vc point at the row's block.
template <typename KVT>
__global__ void ca_kv_scatter_kernel(const float* __restrict__ kv, KVT* __restrict__ kc, KVT* __restrict__ vc, int n, int d,
                                     int hd, int smax) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)n * d) return;
  const int j = (int)(i / d), c = (int)(i % d), h = c / hd, ii = c % hd;
  store_kv(kc + ((long)h * smax + j) * hd + ii, kv[(long)j * 2 * d + c]);
  store_kv(vc + ((long)h * smax + j) * hd + ii, kv[(long)j * 2 * d + d + c]);
}

// DepFormer::sample slice epilogue: lp.sample (ArgMax, or seeded top-k per slot), forced pre-delay pad for the NEXT
// slice's input (:671-680)
// Where a slot's logits come from (r03): the output GEMM's split-K slabs, summed here in canonical order (gemm_reduce_kernel's
// arithmetic for a plain EPI_STORE: no bias, scale, residual), or the finished rows; with two batch rows per slot the
// guidance mix of cfg_mix_kernel is applied on the way.  One launch instead of reduce + mix + sampler per depformer slice.
struct LogitSrc {
  const float* ws;    // non-null: slabs, row m of chunk c at ws + c * cstride + m * ld
  long ld, cstride;
  int chunks;
  const float* rows;  // ws null: [batch rows][V]
  float* store;       // ws non-null, optional: the summed rows are also left here [batch rows][V] (debug tap)
  int rps;            // batch rows per slot
  const uint8_t* cfg_on;
  const float* fa;
  const float* fb;
};
__device__ __forceinline__ f32x4 logit4(const LogitSrc& s, int row, int V, int j) {
  if (s.ws) return slab_sum(s.ws + (long)row * s.ld + j, s.cstride, s.chunks);
  return *reinterpret_cast<const f32x4*>(s.rows + (long)row * V + j);
}

// r04: the sampler's workgroup also runs the NEXT slice's head for its slot's batch rows (dep_head_row: embedding of the token it
// just chose + that slice's projection, ring bookkeeping, norm1) — one launch less per slice; slots that are not running keep
// their last token, as the separate head launch found it.
__global__ __launch_bounds__(256) void dep_argmax_kernel(LogitSrc src, int V, int k, int S, uint32_t* __restrict__ lat,
                                                          uint32_t* __restrict__ last_tok, const uint8_t* __restrict__ run,
                                                          const uint8_t* __restrict__ forced, uint32_t pad, SampleArgs sa, int lds_row_off,
                                                          DepHeadArgs next) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t s_next;
  __shared__ float hred[8];
  const int b = blockIdx.x;
  if (!run[b]) {
    if (!next.x) return;
    if (threadIdx.x == 0) s_next = last_tok[b];
  } else {
  float* logits = reinterpret_cast<float*>(smem + lds_row_off);  // the slot's row, staged once (V % 4 == 0)
  const bool mix = src.rps == 2 && src.cfg_on[b];
  if (src.ws || (V & 3) == 0) {
    for (int j = 4 * (int)threadIdx.x; j < V; j += 4 * (int)blockDim.x) {
      f32x4 o = logit4(src, b * src.rps, V, j);
      if (src.ws && src.store) *reinterpret_cast<f32x4*>(src.store + (long)(b * src.rps) * V + j) = o;
      if (mix) {  // cfg_mix_kernel: (l0 * a + 0) - (l1 * (a - 1) + 0)
        const f32x4 l1 = logit4(src, b * src.rps + 1, V, j);
        if (src.ws && src.store) *reinterpret_cast<f32x4*>(src.store + (long)(b * src.rps + 1) * V + j) = l1;
        const float fa = src.fa[b], fb = src.fb[b];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = o[i] * fa + 0.0f, y = l1[i] * fb + 0.0f;
          o[i] = x - y;
        }
      }
      *reinterpret_cast<f32x4*>(logits + j) = o;
    }
  } else {  // finished rows of a width that is no multiple of four
    for (int j = threadIdx.x; j < V; j += blockDim.x) {
      float o = src.rows[(long)(b * src.rps) * V + j];
      if (mix) {
        const float x = o * src.fa[b] + 0.0f, y = src.rows[(long)(b * src.rps + 1) * V + j] * src.fb[b] + 0.0f;
        o = x - y;
      }
      logits[j] = o;
    }
  }
  __syncthreads();
  uint32_t tok;
  if (sa.top_k && sa.top_k[b] > 0)
    tok = block_sample_topk(logits, V, sa.top_k[b], sa.inv_t[b], sa.key + 8 * b, sa.pos + b, sa.vpad,
                            reinterpret_cast<uint64_t*>(smem), reinterpret_cast<float*>(smem + 8 * (size_t)sa.vpad));
  else
    tok = (uint32_t)block_argmax_first(logits, V);
  if (threadIdx.x == 0) {
    lat[(long)b * S + k] = tok;
    const uint32_t nt = (forced[b] && k > 0) ? pad : tok;
    last_tok[b] = nt;
    s_next = nt;
  }
  if (!next.x) return;
  }
  __syncthreads();
  const uint32_t t = s_next;
  for (int j = 0; j < next.rps; ++j) {
    if (j > 0) __syncthreads();  // hred is reused
    dep_head_row(next, b * next.rps + j, t, hred);
  }
}

// extra heads: f32 softmax over `dim` classes, class-0 probability -> prs[head][slot] (core/asr.rs:195-203)
__global__ void extra_heads_kernel(const float* __restrict__ eh /* [B][nh*dim] */, float* __restrict__ prs, int B,
                                   int nh, int dim, int prs_stride /* slots of the whole batch */) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * nh) return;
  int b = i / nh, h = i % nh;
  const float* lg = eh + ((long)b * nh + h) * dim;
  float m = lg[0];
  for (int k = 1; k < dim; ++k) m = lg[k] > m ? lg[k] : m;
  float sum = 0.0f, e0 = 0.0f;
  for (int k = 0; k < dim; ++k) {
    float e = dsm_expf(lg[k] - m);
    if (k == 0) e0 = e;
    sum = sum + e;
  }
  prs[(long)h * prs_stride + b] = e0 / sum;
}

// ------------------------------------------------------------------------------------------
// SEANet front end, fused (r02): the encoder's first three convs for one slot and 64 output frames in one workgroup —
//   init conv (1 -> 64, k 7)  ->  [ELU -> conv k 3 (64 -> 32) -> ELU -> conv k 1 (32 -> 64)] + skip  ->  ELU
// (core/seanet.rs:292-302 with SeaNetResnetBlock::step :140-150; core/conv.rs:335-367 for the carried frames).  As three
// GEMM launches these layers move ~7 GB at the capacity batch for 65 GFLOP of work (K = 7 / 192 / 32, N = 64 / 32 / 64
// over B x 1920 rows: 3.3 ms of a 69 ms step at B = 2048); here the 64-channel intermediates never leave LDS: the
// workgroup reads 72 PCM samples and writes one [64][64] tile of the next conv's input.
// Arithmetic is the GEMM path's, operation for operation (dsm_numerics.h):
//   * init conv: K = 7 sits in lane group q = 0 of one 32-block, so the canonical chain is fmaf over taps 0..6 from +0
//     (the zero-padded taps add +0 to an accumulator that is never -0), then + bias: VALU, no MFMA, and one scalar chain per
//     channel (dsm_unpaired: never packed pairs);
//   * conv k 3: K = 192 = six 32-blocks of one chunk, v_mfma_f32_16x16x4_f32 in the canonical order
//     (k = 32 blk + 8 q + s, s outer), + bias, ELU; its im2col rows are windows of the ELU'd tile in LDS;
//   * conv k 1: one 32-block, + bias, skip + value (the raw init-conv output, kept in LDS), ELU.
// Carried frames: the k-3 conv's two past frames are read from its concat buffer's prefix (written by
// conv_state_shift_kernel after the previous step) by the first tile of a slot; the last tile leaves the slot's two newest
// ELU'd frames in that buffer's tail for the shift to carry.  The buffers in between (raw init output, the k-1 conv's
// input) are not written at all.
// ------------------------------------------------------------------------------------------
struct SeanetFrontArgs {
  const float* cat_init;  // [B][S0 + T] PCM with S0 = 6 carried samples in front
  const float *w0, *b0;   // [64][ld0] (7 taps used), bias or null
  const float *w1, *b1;   // [32][ld1], k = tap * 64 + channel
  const float *w2, *b2;   // [64][ld2]
  float* cat_ra;          // [B][2 + T][64]: ELU'd init output as the k-3 conv sees it (prefix read, tail written)
  float* cat_down;        // [B][Sd + T][64]: the strided conv's concat buffer, rows Sd.. written
  int ld0, ld1, ld2;
  int T, S0, Sd;
};

// A value the compiler may not pair with a neighbour's into one packed operation (v_pk_fma_f32 / v_pk_add_f32); no instruction
// is emitted.  seanet_front_kernel's init conv needs it: two channels' tap chains, paired, became a chain of DEPENDENT
// v_pk_fma_f32 whose taps wait for their LDS operand in between, and the compiler counts that s_waitcnt as the wait state a
// packed-f32 result needs before a dependent vector instruction reads it.  A wait that is already satisfied takes no issue
// cycle; the next tap then read the low half of the accumulator pair before the tap in front had written it, and one row of
// sixteen lanes lost that tap in channel 4 cq.  Scalar v_fma_f32 / v_fmac_f32 are fully interlocked.
__device__ __forceinline__ float dsm_unpaired(float v) {
  asm("" : "+v"(v));
  return v;
}

template <int TM>
constexpr size_t seanet_front_lds() { return sizeof(float) * ((TM + 2) * 64 + TM * 64 + TM * 32 + (TM + 2 + 7 - 1)); }
template <int TM>  // frames per workgroup: 64 or 32 (smaller tiles: more workgroups per CU to hide the three phases behind each other)
__global__ __launch_bounds__(256) void seanet_front_kernel(SeanetFrontArgs a) {
  constexpr int C0 = 64, C1 = 32, TAPS0 = 7, MTILES = TM / 16;
  static_assert(TM == 64 || TM == 32, "tile");
  // Dynamic LDS (seanet_front_lds<TM>() bytes), not static arrays: a static 41 KB tells the compiler that three workgroups fit on a
  // CU and it pads the register allocation up to that occupancy (136 VGPRs for 88 used) — registers the LM streams' workgroups
  // can use beside this kernel (r04, see gemm_bx3u_kernel).
  extern __shared__ __attribute__((aligned(16))) float front_lds[];
  float* e0 = front_lds;                    // [(TM + 2) * C0] ELU(init conv), frames t0-2 .. t0+TM-1; 16-byte unit u of row R at u ^ (R & 15)
  float* y0 = e0 + (TM + 2) * C0;           // [TM * C0] raw init conv (the skip), same swizzle
  float* hs = y0 + TM * C0;                 // [TM * C1] ELU(conv k 3 + bias): the k-1 conv's activation block (dsm_xs_sw swizzle)
  float* xs = hs + TM * C1;                 // [TM + 2 + TAPS0 - 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * TM;
  const bool first = t0 == 0, last = t0 + TM == a.T;
  const float* cat = a.cat_init + (long)b * (a.S0 + a.T);
  // e0 row R (frame t0 - 2 + R) needs cat[t0 - 2 + R + s], s = 0..6
  for (int i = tid; i < TM + 2 + TAPS0 - 1; i += 256) {
    const int c = t0 - 2 + i;
    xs[i] = c >= 0 ? cat[c] : 0.0f;  // c < 0 only feeds rows 0 and 1 of the first tile, which come from the carried frames
  }
  // ---- init conv + ELU (VALU): a thread keeps its four channels' taps and biases in registers and walks rows tid / 16 + 16 i ----
  const int cq = tid & 15;
  float w0r[4][TAPS0], b0r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int sidx = 0; sidx < TAPS0; ++sidx) w0r[j][sidx] = a.w0[(long)(4 * cq + j) * a.ld0 + sidx];
    b0r[j] = a.b0 ? a.b0[4 * cq + j] : 0.0f;
  }
  __syncthreads();
  for (int R = tid >> 4; R < TM + 2; R += 16) {
    float4 ev;
    if (first && R < 2) {
      ev = *reinterpret_cast<const float4*>(a.cat_ra + ((long)b * (2 + a.T) + R) * C0 + 4 * cq);
    } else {
      float xr[TAPS0];
#pragma unroll
      for (int sidx = 0; sidx < TAPS0; ++sidx) xr[sidx] = xs[R + sidx];
      float yv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int sidx = 0; sidx < TAPS0; ++sidx) acc = dsm_unpaired(DSM_FMAF(w0r[j][sidx], xr[sidx], acc));
        yv[j] = a.b0 ? dsm_unpaired(acc + b0r[j]) : acc;
      }
      ev = make_float4(dsm_elu(yv[0]), dsm_elu(yv[1]), dsm_elu(yv[2]), dsm_elu(yv[3]));
      if (R >= 2) *reinterpret_cast<float4*>(&y0[(R - 2) * C0 + 4 * (cq ^ ((R - 2) & 15))]) = make_float4(yv[0], yv[1], yv[2], yv[3]);
      if (last && R >= TM)  // frames T-2, T-1: what conv_state_shift_kernel carries into the next step
        *reinterpret_cast<float4*>(a.cat_ra + ((long)b * (2 + a.T) + 2 + (t0 - 2 + R)) * C0 + 4 * cq) = ev;
    }
    *reinterpret_cast<float4*>(&e0[R * C0 + 4 * (cq ^ (R & 15))]) = ev;
  }
  __syncthreads();
  // ---- conv k 3: [TM frames][K = 192] x [32][192]^T.  TM = 64: wave -> (n-tile wave & 1, m-tiles 2 (wave >> 1) + {0, 1});
  //      TM = 32: wave -> (n-tile wave & 1, m-tile wave >> 1) ----
  {
    constexpr int MPW = MTILES / 2;  // m-tiles per wave
    const int nt = wave & 1, mh = wave >> 1;
    f32x4 acc[MPW];
#pragma unroll
    for (int m2 = 0; m2 < MPW; ++m2) acc[m2] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* wrow = a.w1 + (long)(16 * nt + r) * a.ld1 + 8 * q;
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
      float wa[8], xb[MPW][8];
      load_w8<float>(wrow + 32 * blk, wa);
      const int tap = blk >> 1, u0 = (blk & 1) * 8 + 2 * q;  // k = 32 blk + 8 q: tap k / 64, channel k % 64
#pragma unroll
      for (int m2 = 0; m2 < MPW; ++m2) {
        const int R = 16 * (MPW * mh + m2) + r + tap;
        const float4 f0 = *reinterpret_cast<const float4*>(&e0[R * C0 + 4 * (u0 ^ (R & 15))]);
        const float4 f1 = *reinterpret_cast<const float4*>(&e0[R * C0 + 4 * ((u0 + 1) ^ (R & 15))]);
        xb[m2][0] = f0.x; xb[m2][1] = f0.y; xb[m2][2] = f0.z; xb[m2][3] = f0.w;
        xb[m2][4] = f1.x; xb[m2][5] = f1.y; xb[m2][6] = f1.z; xb[m2][7] = f1.w;
      }
#pragma unroll
      for (int sidx = 0; sidx < 8; ++sidx)
#pragma unroll
        for (int m2 = 0; m2 < MPW; ++m2) acc[m2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[sidx], xb[m2][sidx], acc[m2], 0, 0, 0);
    }
#pragma unroll
    for (int m2 = 0; m2 < MPW; ++m2) {
      const int m = 16 * (MPW * mh + m2) + r, n = 16 * nt + 4 * q;  // the lane holds channels n..n+3 of frame m
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = dsm_elu(a.b1 ? acc[m2][i] + a.b1[n + i] : acc[m2][i]);
      *reinterpret_cast<float4*>(&hs[m * C1 + 4 * ((n >> 2) ^ dsm_xs_sw(m))]) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();
  // ---- conv k 1 + skip + ELU: [TM frames][32] x [64][32]^T; wave -> n-tile `wave`, every m-tile ----
  {
    f32x4 acc[MTILES];
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float wa[8], xb[MTILES][8];
    load_w8<float>(a.w2 + (long)(16 * wave + r) * a.ld2 + 8 * q, wa);
    const int xu0 = 4 * ((2 * q) ^ dsm_xs_sw(r)), xu1 = xu0 ^ 4;
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt) {
      const float* fp = &hs[(16 * mt + r) * C1];
      const float4 f0 = *reinterpret_cast<const float4*>(fp + xu0), f1 = *reinterpret_cast<const float4*>(fp + xu1);
      xb[mt][0] = f0.x; xb[mt][1] = f0.y; xb[mt][2] = f0.z; xb[mt][3] = f0.w;
      xb[mt][4] = f1.x; xb[mt][5] = f1.y; xb[mt][6] = f1.z; xb[mt][7] = f1.w;
    }
#pragma unroll
    for (int sidx = 0; sidx < 8; ++sidx)
#pragma unroll
      for (int mt = 0; mt < MTILES; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[sidx], xb[mt][sidx], acc[mt], 0, 0, 0);
    float* out = a.cat_down + ((long)b * (a.Sd + a.T) + a.Sd + t0) * C0;
#pragma unroll
    for (int mt = 0; mt < MTILES; ++mt) {
      const int m = 16 * mt + r, n = 16 * wave + 4 * q;
      const float4 rv = *reinterpret_cast<const float4*>(&y0[m * C0 + 4 * ((n >> 2) ^ (m & 15))]);
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = a.b2 ? acc[mt][i] + a.b2[n + i] : acc[mt][i];
      o[0] = rv.x + o[0]; o[1] = rv.y + o[1]; o[2] = rv.z + o[2]; o[3] = rv.w + o[3];
      *reinterpret_cast<float4*>(out + (long)m * C0 + n) = make_float4(dsm_elu(o[0]), dsm_elu(o[1]), dsm_elu(o[2]), dsm_elu(o[3]));
    }
  }
}

// ------------------------------------------------------------------------------------------
// Streaming-conv state: in-place shift of the consumer's concat buffer after it ran
// (core/conv.rs:335-367).  desc[i] = {ptr, state_len S, step frames T, channels C, batch stride}.
// active slots: cat[b][0..S) = cat[b][T..T+S); inactive: unchanged (zeroed on the first call).
// ------------------------------------------------------------------------------------------
struct ConvStateDesc {
  float* cat;
  long bstride;
  int S, T, C, replicate;
};

// started (optional, [B]): per-slot freshness instead of the module-level first call (the TTS decode path): the states of
// a slot that has not started are zero already (allocation, slot reset), and this launch — the last one of a decode step, behind
// every reader of the flag — records that an active slot has started.
// keep (optional, [B], read on the module's first call only): a slot whose state was imported before that call
// (dsm_asr_import_slots) — it is not a fresh slot, so an inactive one keeps its state instead of being zeroed.
__global__ void conv_state_shift_kernel(const ConvStateDesc* __restrict__ descs, const uint8_t* __restrict__ active,
                                        int first_call, uint8_t* __restrict__ started, const uint8_t* __restrict__ keep) {
  const ConvStateDesc dsc = descs[blockIdx.y];
  const int b = blockIdx.x;
  float* base = dsc.cat + (long)b * dsc.bstride;
  const int n = dsc.S * dsc.C;
  if (active[b]) {
    const float* src = base + (long)dsc.T * dsc.C;
    // S <= T for every conv of the model, so source and destination do not overlap
    for (int i = threadIdx.x; i < n; i += blockDim.x) base[i] = src[i];
    if (started && blockIdx.y == 0 && threadIdx.x == 0) started[b] = 1;
  } else if (first_call && !started && !(keep && keep[b])) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) base[i] = 0.0f;
  }
}

// first call of a replicate-padded conv (ConvDownsample1d, core/conv.rs:318-327,530): the left pad
// repeats the first input frame of every slot
// keep (optional, [B]): slots whose left pad was imported (dsm_asr_import_slots) are left alone
__global__ void conv_replicate_init_kernel(ConvStateDesc dsc, const uint8_t* __restrict__ keep) {
  const int b = blockIdx.x;
  if (keep && keep[b]) return;
  float* base = dsc.cat + (long)b * dsc.bstride;
  const float* first = base + (long)dsc.S * dsc.C;
  for (int i = threadIdx.x; i < dsc.S * dsc.C; i += blockDim.x) base[i] = first[i % dsc.C];
}

__global__ void conv_state_reset_kernel(const ConvStateDesc* __restrict__ descs, int slot) {
  const ConvStateDesc dsc = descs[blockIdx.x];
  float* base = dsc.cat + (long)slot * dsc.bstride;
  for (int i = threadIdx.x; i < dsc.S * dsc.C; i += blockDim.x) base[i] = 0.0f;
}

// ------------------------------------------------------------------------------------------
// Slot snapshots (dsm_asr_export_slots / import / move): gather the state of n slots into one contiguous staging buffer,
// or scatter it back, in ONE launch.  The engine describes a slot's state as a table of sections — per-slot byte ranges
// `bytes` long, `stride` apart between slots, section i of slot s at base + s * stride — and gives each a 16-byte-aligned
// offset `off` inside the slot's `slot_bytes` of staging.  Work is cut into kSlotChunk-byte pieces of one section; chunk0 is
// the number of pieces in front of the section, so a workgroup finds the section of piece w by bisection.  Grid (pieces, n):
// x is capped by the launcher and strides the rest.
// The ring sections (megabytes, 16-byte aligned at both ends) move as uint4, four loads in flight per thread; a conv
// state is a few floats at a 4-byte-aligned engine address (config_tiny: 6 floats) and moves as words; first_step is a byte.
// A section's length is its own: nothing is stored past it, on either side — the staging gaps stay as the caller left them.
// ------------------------------------------------------------------------------------------
struct SlotSection {
  char* base;
  long stride, bytes, off;
  unsigned chunk0, pad_;
};
constexpr long kSlotChunk = 16384;  // 256 threads x 4 x 16 bytes

template <bool PACK>
__device__ __forceinline__ void slot_state_copy(const SlotSection* __restrict__ secs, int nsec, unsigned total_chunks,
                                                const int* __restrict__ slots, char* __restrict__ stage, long slot_bytes) {
  const int j = blockIdx.y;
  const long slot = slots[j];
  for (unsigned w = blockIdx.x; w < total_chunks; w += gridDim.x) {
    int lo = 0, hi = nsec - 1;  // the last section with chunk0 <= w
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (secs[mid].chunk0 <= w) lo = mid; else hi = mid - 1;
    }
    const SlotSection s = secs[lo];
    const long at = (long)(w - s.chunk0) * kSlotChunk;
    const long len = s.bytes - at < kSlotChunk ? s.bytes - at : kSlotChunk;
    char* eng = s.base + slot * s.stride + at;
    char* stg = stage + (long)j * slot_bytes + s.off + at;
    const char* src = PACK ? eng : stg;
    char* dst = PACK ? stg : eng;
    const unsigned long al = (unsigned long)(uintptr_t)s.base | (unsigned long)s.stride | (unsigned long)s.bytes;
    if ((al & 15) == 0) {  // `at`, `off`, slot_bytes and the staging base are multiples of 16 by construction
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long o = ((long)u * 256 + threadIdx.x) * 16;
        if (o < len) v[u] = *reinterpret_cast<const uint4*>(src + o);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long o = ((long)u * 256 + threadIdx.x) * 16;
        if (o < len) *reinterpret_cast<uint4*>(dst + o) = v[u];
      }
    } else if ((al & 3) == 0) {
      for (long o = (long)threadIdx.x * 4; o < len; o += (long)blockDim.x * 4)
        *reinterpret_cast<uint32_t*>(dst + o) = *reinterpret_cast<const uint32_t*>(src + o);
    } else {
      for (long o = threadIdx.x; o < len; o += blockDim.x) dst[o] = src[o];
    }
  }
}
__global__ void __launch_bounds__(256) slot_state_pack_kernel(const SlotSection* __restrict__ secs, int nsec, unsigned total_chunks,
                                                              const int* __restrict__ slots, char* __restrict__ stage, long slot_bytes) {
  slot_state_copy<true>(secs, nsec, total_chunks, slots, stage, slot_bytes);
}
__global__ void __launch_bounds__(256) slot_state_unpack_kernel(const SlotSection* __restrict__ secs, int nsec, unsigned total_chunks,
                                                                const int* __restrict__ slots, char* __restrict__ stage, long slot_bytes) {
  slot_state_copy<false>(secs, nsec, total_chunks, slots, stage, slot_bytes);
}

// ------------------------------------------------------------------------------------------
// RVQ select: reduce the per-tile (dist, idx) partials, emit the code, update the residual
// (core/quantization.rs:219-229).  One workgroup per row.
// ------------------------------------------------------------------------------------------
__global__ void rvq_select_kernel(const float* __restrict__ pval, const uint32_t* __restrict__ pidx, int n_tiles,
                                  int M, uint32_t* __restrict__ codes, int code_stride, int code_off,
                                  float* __restrict__ residual, const float* __restrict__ E, int dim, int ldE) {
  const int m = blockIdx.x;
  __shared__ uint32_t s_code;
  if (threadIdx.x < 64) {
    float bv = DSM_INF_F;
    uint32_t bi = 0xFFFFFFFFu;
    for (int t = threadIdx.x; t < n_tiles; t += 64) {
      float v = pval[(long)t * M + m];
      uint32_t i = pidx[(long)t * M + m];
      if (v < bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      float ov = __shfl_xor(bv, off, 64);
      uint32_t oi = __shfl_xor(bi, off, 64);
      if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (threadIdx.x == 0) {
      s_code = bi;
      codes[(long)m * code_stride + code_off] = bi;
    }
  }
  __syncthreads();
  const uint32_t c = s_code;
  for (int i = threadIdx.x; i < dim; i += blockDim.x)
    residual[(long)m * dim + i] = residual[(long)m * dim + i] - E[(long)c * ldE + i];
}

// ------------------------------------------------------------------------------------------
// Decode side (Mimi::decode_step, core/mimi.rs:217-225)
// ------------------------------------------------------------------------------------------
// ResidualVectorQuantization::decode — core/quantization.rs:231-248: gather E_i[code_i] and sum the layers in order.
// One workgroup per slot; q_first = layer 0 of rvq_first, q_rest = sum over rvq_rest layers.
struct RvqGatherArgs {
  const float* const* emb;  // n_q device pointers: [bins][ldE] f32 (index 0 = rvq_first, 1.. = rvq_rest)
  int n_q, bins, dim, ldE;
};
__global__ void rvq_gather_sum_kernel(RvqGatherArgs a, const uint32_t* __restrict__ codes, float* __restrict__ q_first,
                                      float* __restrict__ q_rest) {
  const int b = blockIdx.x;
  for (int dd = threadIdx.x; dd < a.dim; dd += blockDim.x) {
    uint32_t c0 = codes[b * a.n_q];
    c0 = c0 < (uint32_t)a.bins ? c0 : 0u;
    q_first[(long)b * a.dim + dd] = a.emb[0][(long)c0 * a.ldE + dd];
    float acc = 0.0f;
    for (int i = 1; i < a.n_q; ++i) {
      uint32_t c = codes[b * a.n_q + i];
      c = c < (uint32_t)a.bins ? c : 0u;
      float ev = a.emb[i][(long)c * a.ldE + dd];
      acc = (i == 1) ? ev : acc + ev;
    }
    if (a.n_q > 1) q_rest[(long)b * a.dim + dd] = acc;
  }
}

// ConvTrUpsample1d::step — depthwise ConvTranspose1d k = 2*stride, one input frame per step, no bias
// (core/conv.rs:558-606, :448-501).  x [B][C]; w [k][C]; carry [B][k - s][C]; y [B][s][C].
// started (optional, [B]): the carry term is applied iff the SLOT has decoded a frame before (has_state is ignored).
__global__ void upsample_dw_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ carry,
                                   float* __restrict__ y, const uint8_t* __restrict__ active, int C, int s, int k,
                                   int has_state, const uint8_t* __restrict__ started) {
  const int b = blockIdx.x;
  if (started) has_state = started[b];  // a slot that has not started keeps the zero carry of its allocation / reset
  for (int i = threadIdx.x; i < s * C; i += blockDim.x) {
    const int o = i / C, c = i % C;
    const float xv = x[(long)b * C + c];
    float v = xv * w[(long)o * C + c];
    if (has_state) v = v + carry[((long)b * (k - s) + o) * C + c];
    y[((long)b * s + o) * C + c] = v;
    if (o < k - s) {  // k - s == s: the thread that consumed carry[o] also refreshes it (no cross-thread hazard)
      const float nv = xv * w[(long)(s + o) * C + c];
      float* cp = &carry[((long)b * (k - s) + o) * C + c];
      if (active[b]) *cp = nv;
      else if (!has_state) *cp = 0.0f;
    }
  }
}

// StreamableConvTranspose1d::step epilogue — core/conv.rs:448-501 with k == 2*stride.  The GEMM produced
// z[(b,t)][kk*OC + co] = sum_ci x[b][t][ci] * w[ci][co][kk]; output frame o = t*s + kk (kk < s) is
//   t == 0 : (z[t][kk] + bias) + (carry[kk] - bias)          (first call of the module: no carry term)
//   t  > 0 : (z[t-1][kk+s] + z[t][kk]) + bias
// new carry[j] = z[T-1][j+s] + bias (kept for inactive slots).  Writes y (raw) and/or y2 (ELU copy).
struct OverlapAddArgs {
  const float* z;
  const float* bias;
  float* carry;  // [B][s][OC]
  const uint8_t* active;
  int T, s, OC, has_state;
  float* Y;
  RowMap ymap;  // rows are (b, o), rpb = T*s
  float* Y2;
  RowMap y2map;
  const uint8_t* started;  // optional [B]: the carry term is applied iff the SLOT has decoded a frame before (has_state is ignored)
};
__global__ void convtr_overlap_add_kernel(OverlapAddArgs a) {
  const int b = blockIdx.y;
  if (a.started) a.has_state = a.started[b];
  const int per_b = a.T * a.s * (a.OC >> 2);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per_b; i += gridDim.x * blockDim.x) {
    const int c4 = i % (a.OC >> 2), o = i / (a.OC >> 2);
    const int co = c4 * 4, t = o / a.s, kk = o % a.s;
    const long ldz = (long)2 * a.s * a.OC;
    const float4 zb = *reinterpret_cast<const float4*>(a.z + ((long)b * a.T + t) * ldz + (long)kk * a.OC + co);
    const float4 bs = *reinterpret_cast<const float4*>(a.bias + co);
    float4 v;
    if (t > 0) {
      const float4 za = *reinterpret_cast<const float4*>(a.z + ((long)b * a.T + t - 1) * ldz + (long)(kk + a.s) * a.OC + co);
      v.x = (za.x + zb.x) + bs.x; v.y = (za.y + zb.y) + bs.y; v.z = (za.z + zb.z) + bs.z; v.w = (za.w + zb.w) + bs.w;
    } else {
      v.x = zb.x + bs.x; v.y = zb.y + bs.y; v.z = zb.z + bs.z; v.w = zb.w + bs.w;
      float* cp = a.carry + ((long)b * a.s + kk) * a.OC + co;
      if (a.has_state) {
        const float4 cv = *reinterpret_cast<const float4*>(cp);
        v.x = v.x + (cv.x - bs.x); v.y = v.y + (cv.y - bs.y); v.z = v.z + (cv.z - bs.z); v.w = v.w + (cv.w - bs.w);
      }
      const float4 zl = *reinterpret_cast<const float4*>(a.z + ((long)b * a.T + a.T - 1) * ldz + (long)(kk + a.s) * a.OC + co);
      if (a.active[b])
        *reinterpret_cast<float4*>(cp) = make_float4(zl.x + bs.x, zl.y + bs.y, zl.z + bs.z, zl.w + bs.w);
      else if (!a.has_state)
        *reinterpret_cast<float4*>(cp) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int m = b * a.T * a.s + o;
    if (a.Y) *reinterpret_cast<float4*>(a.Y + a.ymap.off(m) + co) = v;
    if (a.Y2) *reinterpret_cast<float4*>(a.Y2 + a.y2map.off(m) + co) = make_float4(dsm_elu(v.x), dsm_elu(v.y), dsm_elu(v.z), dsm_elu(v.w));
  }
}

// The frame a TTS step completes, assembled where the samples are: State::last_audio_tokens (core/tts_streaming.rs:275-287)
// with the test of srv/tts.rs:537.  s = the slot's step index before the step.  Row s - acoustic_delay of the slot's token table is
// complete after this step: codebook 0 was sampled acoustic_delay steps ago (kept in a ring of acoustic_delay + 1 entries per
// slot), codebooks >= 1 are this step's samples — except row 0, whose codebooks >= 1 the table took at step 0 (the write-back
// clamps `step - delay` to 0 and keeps the first write), kept in row0.  A slot emits iff it is active, s >= text_audio_delay +
// acoustic_delay and no token of the row is a pad (>= pad).  Writes the decoder's codes [B][S] and mask [B] of buffer *sel
// (the host rotates the buffers: a decode of an earlier step may still be reading another one).  One thread per slot.
struct TtsFrameArgs {
  const uint32_t* lat;   // [nslots][S] this step's samples (defined for running slots)
  const uint8_t* mask;   // [nslots] the slot steps
  const uint8_t* run;    // [nslots] ... and its depformer ran
  const int32_t* step;   // [nslots]
  const uint8_t* sel;    // one byte: the buffer this step fills
  uint32_t* ring;        // [nslots][ad + 1]
  uint32_t* row0;        // [nslots][S]
  uint32_t* codes;       // buffer 0 of this group's slots; buffer i at + i * codes_stride
  uint8_t* valid;        // likewise, + i * valid_stride
  long codes_stride, valid_stride;
  int nslots, S, ad, tad;
  uint32_t pad;
};
__global__ void tts_frame_kernel(TtsFrameArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.nslots) return;
  const int sel = *a.sel, S = a.S, ad = a.ad;
  uint32_t* codes = a.codes + (long)sel * a.codes_stride + (long)b * S;
  const uint32_t* lat = a.lat + (long)b * S;
  const bool run = a.run[b] != 0;
  bool ok = false;
  if (a.mask[b]) {
    const int s = a.step[b];
    uint32_t* ring = a.ring + (long)b * (ad + 1);
    const uint32_t c0 = run ? lat[0] : a.pad;
    ring[s % (ad + 1)] = c0;
    if (s == 0)
      for (int k = 1; k < S; ++k) a.row0[(long)b * S + k] = run ? lat[k] : a.pad;
    if (s >= a.tad + ad) {
      ok = true;
      const bool first_row = ad > 0 && s == ad;
      for (int k = 0; k < S; ++k) {
        uint32_t tok;
        if (k == 0) tok = ad > 0 ? ring[(s - ad) % (ad + 1)] : c0;
        else if (first_row) tok = a.row0[(long)b * S + k];
        else tok = run ? lat[k] : a.pad;
        ok = ok && tok < a.pad;
        codes[k] = tok < a.pad ? tok : 0u;
      }
    }
  }
  if (!ok)
    for (int k = 0; k < S; ++k) codes[k] = 0u;
  a.valid[(long)sel * a.valid_stride + b] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// The TTS request loop on the device (dsm_tts_request.inc): the inference loop of srv/tts.rs:574-621 and the integer
// bookkeeping of State::step (core/tts_streaming.rs:126-158,195-237) per slot, so that the host can enqueue K steps without
// reading a result.  Two launches per step on the model stream, outside the groups' graphs (the step of the block is a
// launch argument): tts_sched_kernel in front of the groups, tts_commit_kernel behind their join.  One thread per slot,
// plain stores.
// ------------------------------------------------------------------------------------------
enum { TTS_REQ_IDLE = 0, TTS_REQ_RUNNING = 1, TTS_REQ_WAITING = 2, TTS_REQ_DONE = 3, TTS_REQ_DONE_LIMIT = 4 };  // == DSM_TTS_REQ_*
struct TtsReqState {  // one per slot, in HBM
  int32_t status;
  int32_t step;       // State::step_idx == the loop's step_idx
  int32_t cur_word;   // push-order index of the current word; -1: the initial empty word (srv/tts.rs:577)
  int32_t has_word;   // 0: word_tokens == None (the queue was closed and drained)
  int32_t token_idx, step_past_last, last_epad;
  uint32_t last_text;  // the loop's last_text_token: the next step's prev_text_token
  int32_t cpads;       // State::consecutive_pads
  int32_t max_seq_len, extra_steps;
  int32_t n_words, closed;  // the queue: words pushed so far; in_tx.send(None) was seen
};
// A step's record of one slot in the block buffer: TTS_REC_HDR int32 then the S audio tokens.
enum { TTS_REC_STEPPED = 0, TTS_REC_RUN = 1, TTS_REC_TEXT = 2, TTS_REC_OVW = 3, TTS_REC_EV = 4, TTS_REC_EV_WORD = 5,
       TTS_REC_EV_START = 6, TTS_REC_EV_STOP = 7, TTS_REC_HDR = 8 };
struct TtsSchedArgs {
  TtsReqState* req;        // [B]
  const uint32_t* q_tok;   // [B][qcap] the words' tokens back to back
  const int32_t* q_end;    // [B][qcap] end offset of word w in q_tok (its start is the end of word w - 1)
  int qcap;
  int32_t* rec;            // this step's records [B][rec_ld]
  int rec_ld;
  // what dsm_tts_step uploads: tokens [R][1 + nc], allowed [B], the flag block
  int32_t* tokens;
  int32_t* allowed;
  uint8_t *mask, *force, *run, *forced, *rmask, *rrun, *ca_act, *fsel;
  int32_t* step;
  const uint32_t* lat;     // [B][S] the slot's last depformer samples: row step - 1 of its token table, codebook 0, and row
                           // step - 1 - acoustic_delay, codebooks >= 1 (the rows input assembly reads, :138,148)
  const uint32_t* row0;    // [B][S] row 0's codebooks >= 1 (tts_frame_kernel keeps them: the write-back clamps to row 0)
  const uint8_t* cfg_on;   // [B]
  const uint8_t* ca_has;   // [R] the batch row has a cross-attention source
  int B, rps, nc, S, ad, tad, max_cpads, text_in_vocab, n_steps /* rows of the token table: the engine's own limit */;
  uint32_t pad;            // audio pad token
  int sel;                 // frame buffer this step fills
};
__global__ void tts_sched_kernel(TtsSchedArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  if (b == 0) *a.fsel = (uint8_t)a.sel;
  TtsReqState r = a.req[b];
  int32_t* rec = a.rec + (long)b * a.rec_ld;
  int ovw = 0;
  if (r.status == TTS_REQ_WAITING) {  // in_rx.recv() of srv/tts.rs:606, resolved once the word (or the close) has arrived
    if (r.cur_word + 1 < r.n_words) { r.cur_word += 1; r.status = TTS_REQ_RUNNING; }
    else if (r.closed) { r.has_word = 0; r.status = TTS_REQ_RUNNING; ovw = 1; }  // :607-610, on the previous step's text token
  }
  bool steps = false;
  int32_t al = -1;
  if (r.status == TTS_REQ_RUNNING) {
    if (r.step >= r.max_seq_len || r.step + 1 >= a.n_steps) {  // `for step_idx in 0..max_seq_len`; the step that would bail with "max step-idx reached"
      r.status = TTS_REQ_DONE_LIMIT;
    } else if (!r.has_word) {  // :582-588
      r.step_past_last += 1;
      if (r.step_past_last > r.extra_steps + a.tad) r.status = TTS_REQ_DONE;
      else steps = true;  // Pad
    } else {  // :589-592
      const int32_t* qe = a.q_end + (long)b * a.qcap;
      const int w0 = r.cur_word > 0 ? qe[r.cur_word - 1] : 0;
      const int w1 = r.cur_word >= 0 ? qe[r.cur_word] : 0;
      al = r.token_idx < w1 - w0 ? (int32_t)a.q_tok[(long)b * a.qcap + w0 + r.token_idx] : -2;  // Text(id) : PadOrEpad
      steps = true;
    }
  }
  a.req[b] = r;
  rec[TTS_REC_STEPPED] = steps ? 1 : 0;
  rec[TTS_REC_RUN] = 0;
  rec[TTS_REC_TEXT] = 0;
  rec[TTS_REC_OVW] = ovw;
  rec[TTS_REC_EV] = 0;
  // input assembly — core/tts_streaming.rs:126-158; a slot that does not step gets what the host writes for a masked-off one
  const int s = r.step, nc = a.nc;
  const bool run = steps && s >= a.tad;
  int32_t* tk = a.tokens + (long)b * a.rps * (1 + nc);
  tk[0] = steps && r.last_text < (uint32_t)a.text_in_vocab ? (int32_t)r.last_text : 0;
  for (int cb = 0; cb < nc; ++cb) {
    int32_t tok = -1;  // None
    if (steps && cb < a.S) {
      if (cb == 0) {
        if (s == 0) tok = (int32_t)a.pad;
        else if (s > a.tad) tok = (int32_t)a.lat[(long)b * a.S];
      } else if (s <= a.ad) tok = (int32_t)a.pad;
      else if (s > a.tad + a.ad) tok = (int32_t)(s == a.ad + 1 ? a.row0[(long)b * a.S + cb] : a.lat[(long)b * a.S + cb]);
    }
    tk[1 + cb] = tok;
  }
  for (int j = 1; j < a.rps; ++j)
    for (int i = 0; i < 1 + nc; ++i) tk[(long)j * (1 + nc) + i] = tk[i];
  a.allowed[b] = al;
  a.mask[b] = steps ? 1 : 0;
  a.force[b] = r.cpads > a.max_cpads ? 1 : 0;
  a.run[b] = run ? 1 : 0;
  a.forced[b] = s < a.ad ? 1 : 0;
  a.step[b] = s;
  for (int j = 0; j < a.rps; ++j) {
    const int row = b * a.rps + j;
    const bool on = j == 0 || a.cfg_on[b];
    a.rmask[row] = steps && on ? 1 : 0;
    a.rrun[row] = run && on ? 1 : 0;
    a.ca_act[row] = steps && on && a.ca_has[row] ? 1 : 0;
  }
}

struct TtsCommitArgs {
  TtsReqState* req;
  int32_t* rec;
  int rec_ld;
  const uint8_t *mask, *run;
  const uint32_t* text_token;  // [B] what the text-token rule returned
  const uint32_t* lat;         // [B][S]
  int B, S;
  uint32_t text_pad, text_eop;
};
// What follows State::step's sampling (core/tts_streaming.rs:195-237) and the loop body behind it (srv/tts.rs:596-614).  The
// token table itself stays on the host (the record carries what its write-back needs); the rows the next input assembly reads
// are the slot's samples in `lat`, which only a step of this slot rewrites.
__global__ void tts_commit_kernel(TtsCommitArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  int32_t* rec = a.rec + (long)b * a.rec_ld;
  const bool run = a.mask[b] && a.run[b];
  for (int k = 0; k < a.S; ++k) rec[TTS_REC_HDR + k] = (int32_t)(run ? a.lat[(long)b * a.S + k] : 0xFFFFFFFFu);
  if (!a.mask[b]) return;
  TtsReqState r = a.req[b];
  const uint32_t tok = a.text_token[b];
  r.cpads = tok == a.text_pad ? r.cpads + 1 : 0;
  rec[TTS_REC_RUN] = run ? 1 : 0;
  rec[TTS_REC_TEXT] = (int32_t)tok;
  if (tok == a.text_eop) {  // the value decides, whatever rule produced it: a pushed Text(eop) ends the word too
    if (r.has_word) {
      rec[TTS_REC_EV] = 1;
      rec[TTS_REC_EV_WORD] = r.cur_word;
      rec[TTS_REC_EV_START] = r.last_epad;
      rec[TTS_REC_EV_STOP] = r.step;
      if (r.cur_word + 1 < r.n_words) r.cur_word += 1;
      else if (r.closed) { r.has_word = 0; rec[TTS_REC_OVW] = rec[TTS_REC_OVW] | 2; }  // overwrite_last_text_token(pad) on THIS step's token
      else r.status = TTS_REQ_WAITING;
    }
    r.last_epad = r.step;
    r.token_idx = 0;
  } else if (tok != a.text_pad) {
    r.token_idx += 1;
  }
  r.last_text = tok;  // the loop variable keeps the end-of-pad (:609 rewrites the table only)
  r.step += 1;
  a.req[b] = r;
}
// request_begin / reset, and the queue's counters: the value travels in the launch, so a later push cannot be seen early
__global__ void tts_req_init_kernel(TtsReqState* dst, TtsReqState v) { *dst = v; }
__global__ void tts_req_store_kernel(int32_t* dst, int32_t v) { *dst = v; }

// ------------------------------------------------------------------------------------------
// Speaker encoder (dsm_speaker.inc): the whole-clip, non-streaming Mimi encode of SpeakerEncoder::encode —
// core/tts_streaming.rs:382-409.  Tolerance-pinned, not bit-pinned: the oracle has only the streaming Mimi.
// ------------------------------------------------------------------------------------------

// A block-wide f64 sum in a fixed order: every thread's chain (elements tid, tid + 1024, ...), an xor butterfly inside each
// wave, the 16 wave totals left to right.  `red` holds 16 doubles; every thread returns the total.
__device__ __forceinline__ double spk_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  __syncthreads();  // the previous total has been read by everyone
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = t + red[w];
  return t;
}

// pcm * 0.08 / sqrt(mean((pcm - mean(pcm))^2)) per clip (:388-389; the output is not mean-subtracted).  One workgroup of 1024
// threads per clip: mean, then the mean squared deviation, both summed in f64 in the order above (the same bits every run), then
// the f32 product and quotient of the reference.  The scaled clip goes straight into the first convolution's concat buffer
// behind its zero left pad (out + clip * out_stride); the f32 standard deviation goes to stdev[clip] for the host's check, and a
// clip whose deviation is zero or not finite is left unscaled (the call fails before anything reads it).
__global__ __launch_bounds__(1024) void spk_normalize_kernel(const float* __restrict__ pcm, int n, float* __restrict__ out,
                                                             long out_stride, float* __restrict__ stdev) {
  __shared__ double red[16];
  const int clip = blockIdx.x;
  const float* x = pcm + (long)clip * n;
  float* y = out + (long)clip * out_stride;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s = s + (double)x[i];
  const double mean = spk_block_sum(s, red) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double dv = (double)x[i] - mean;
    q = DSM_FMA(dv, dv, q);
  }
  const float sd = (float)sqrt(spk_block_sum(q, red) / (double)n);
  if (threadIdx.x == 0) stdev[clip] = sd;
  const bool ok = sd > 0.0f && sd < DSM_INF_F;
  for (int i = threadIdx.x; i < n; i += blockDim.x) y[i] = ok ? (x[i] * 0.08f) / sd : x[i];
}

// (cos, sin) of (pos0 + t) * inv_freq[i] for t < T: the table the streaming encoder's kv_builder_kernel writes per step, for the
// whole clip at once.  pos0 = frames per step where the batched transformer reads its positions after the builder advanced them
// (0 with rope_pos_before).
__global__ void spk_rope_table_kernel(float* __restrict__ cs, const float* __restrict__ inv_freq, int T, int half, int pos0) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= T * half) return;
  const int t = e / half, i = e % half;
  float s, c;
  dsm_sincosf((float)(uint32_t)(pos0 + t) * inv_freq[i], &s, &c);
  cs[2 * (long)e] = c;
  cs[2 * (long)e + 1] = s;
}

// Causal self-attention over a whole sequence: softmax(rope(q) . rope(k)^T / sqrt(HD) + causal mask) . v for the T positions of
// one clip.  qkv [clips * T][3 d] is the plain in_proj product (q | k | v, heads inside each — core/batched_transformer.rs:77-82);
// out [clips * T][d] is what out_proj reads.  One workgroup = SPK_QB = 16 queries of one (clip, head):
//   1. the 16 queries, rotated (rope_i on interleaved pairs, cs [T][HD / 2][2]), into LDS;
//   2. keys 0 .. last query of the block in tiles of 64 rows: rotated on load into LDS (row stride HD + 1: the 16 keys a half-wave
//      reads sit on 16 different banks), thread (query tid / 16, key lane tid % 16) chains its four keys' dot products over
//      the head dim and stores score * scale, or -inf behind the diagonal, in sc [16][Tp];
//   3. softmax per query by its 16 lanes: lane chains of max, exp and sum over keys lane, lane + 16, ..., a 16-lane xor
//      butterfly, the weights divided by the sum once;
//   4. value tiles of 64 rows into LDS, thread (query, dims lane + 16 i) chains weight * v over the keys in ascending order.
// Every sum has one order that depends on T alone, and every chain is scalar (dsm_unpaired on the rotation's products, the QK
// dot and the PV accumulators: paired, they were dependent v_pk_fma_f32 / v_pk_add_f32 with at most an s_waitcnt in between,
// the sequence that lost taps in seanet_front_kernel; tools/packed_f32_hazards.py keeps the library free of it).  cs null: no positional embedding inside the transformer, q and k are used as
// they are.  K and V of one head at T = 250, HD = 64 are 128 KB: they pass through a 16.6 KB tile instead, so the launch stays
// inside the default 64 KB of dynamic LDS up to T = 700 at HD = 64 (860 at HD = 32; spk_attn_lds); attach refuses a longer context.
#define SPK_QB 16
#define SPK_KT 64
template <int HD>
__host__ __device__ constexpr size_t spk_attn_lds(int T) {
  return sizeof(float) * ((size_t)SPK_QB * HD + (size_t)SPK_KT * (HD + 1) + (size_t)SPK_QB * ((T + 3) & ~3));
}
template <int HD>
__global__ __launch_bounds__(256) void spk_attn_kernel(float* __restrict__ out, const float* __restrict__ qkv,
                                                       const float* __restrict__ cs, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int d = H * HD, Tp = (T + 3) & ~3;
  float* qs = lds;                      // [16][HD]
  float* kv = qs + SPK_QB * HD;         // [64][HD + 1]: a key tile, later a value tile
  float* sc = kv + SPK_KT * (HD + 1);   // [16][Tp]
  const int tid = threadIdx.x, h = blockIdx.y, clip = blockIdx.z;
  const int q0 = blockIdx.x * SPK_QB;
  const int nq = min(SPK_QB, T - q0), nkeys = q0 + nq;  // keys 0 .. nkeys - 1 are visible to some query of the block
  const float* base = qkv + (long)clip * T * 3 * d + h * HD;
  const float scale = (float)(1.0 / sqrt((double)HD));
  // a rotated row tile: rows [r0, r0 + nr) of part (0 q, 1 k) into dst with row stride ld
  auto load_rot = [&](float* dst, int ld, int part, int r0, int nr) {
    for (int e = tid; e < nr * (HD / 2); e += 256) {
      const int r = e / (HD / 2), p = e % (HD / 2);
      const float2 x = *reinterpret_cast<const float2*>(base + (long)(r0 + r) * 3 * d + part * d + 2 * p);
      const float2 c = cs ? *reinterpret_cast<const float2*>(cs + ((long)(r0 + r) * (HD / 2) + p) * 2) : make_float2(1.0f, 0.0f);
      const float t0 = dsm_unpaired(x.x * c.x), t1 = dsm_unpaired(x.y * c.y), t2 = dsm_unpaired(x.x * c.y), t3 = dsm_unpaired(x.y * c.x);
      dst[r * ld + 2 * p] = t0 - t1;
      dst[r * ld + 2 * p + 1] = t2 + t3;
    }
  };
  load_rot(qs, HD, 0, q0, nq);
  const int qi = tid >> 4, kl = tid & 15;
  const int qpos = q0 + qi;  // (rows qi >= nq compute on stale LDS and are never stored)
  for (int k0 = 0; k0 < nkeys; k0 += SPK_KT) {
    const int nk = min(SPK_KT, nkeys - k0);
    __syncthreads();  // the previous tile has been consumed (first pass: nothing to wait for but qs' writers)
    load_rot(kv, HD + 1, 1, k0, nk);
    __syncthreads();
    if (qi < nq) {
#pragma unroll
      for (int u = 0; u < SPK_KT / 16; ++u) {
        const int jl = kl + 16 * u, j = k0 + jl;
        if (jl < nk) {
          float p = 0.0f;
#pragma unroll 8
          for (int dd = 0; dd < HD; ++dd) p = dsm_unpaired(DSM_FMAF(qs[qi * HD + dd], kv[jl * (HD + 1) + dd], p));
          sc[qi * Tp + j] = j <= qpos ? p * scale : -DSM_INF_F;
        }
      }
    }
  }
  __syncthreads();
  if (qi < nq) {  // softmax_last_dim over keys 0 .. nkeys - 1 (exp(-inf - m) = 0: the masked keys weigh nothing)
    float* row = sc + qi * Tp;
    float m = -DSM_INF_F;
    for (int j = kl; j < nkeys; j += 16) m = fmaxf(m, row[j]);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float s = 0.0f;
    for (int j = kl; j < nkeys; j += 16) {
      const float p = dsm_expf(row[j] - m);
      row[j] = p;
      s = s + p;
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) s = s + __shfl_xor(s, off, 64);
    for (int j = kl; j < nkeys; j += 16) row[j] = row[j] / s;
  }
  float acc[HD / 16];
#pragma unroll
  for (int i = 0; i < HD / 16; ++i) acc[i] = 0.0f;
  for (int k0 = 0; k0 < nkeys; k0 += SPK_KT) {
    const int nk = min(SPK_KT, nkeys - k0);
    __syncthreads();  // the weights are final / the previous value tile has been consumed
    for (int e = tid; e < nk * (HD / 4); e += 256) {
      const int r = e / (HD / 4), c4 = 4 * (e % (HD / 4));
      const float4 v = *reinterpret_cast<const float4*>(base + (long)(k0 + r) * 3 * d + 2 * d + c4);
      float* dst = kv + r * (HD + 1) + c4;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    __syncthreads();
    if (qi < nq) {
      const float* w = sc + qi * Tp + k0;
      for (int j = 0; j < nk; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int i = 0; i < HD / 16; ++i) acc[i] = dsm_unpaired(DSM_FMAF(wj, kv[j * (HD + 1) + kl + 16 * i], acc[i]));
      }
    }
  }
  if (qi < nq) {
    float* o = out + ((long)clip * T + qpos) * d + h * HD;
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) o[kl + 16 * i] = acc[i];
  }
}

// Rows [row0, row0 + nrows) of a source [rows][dim] = learnt_padding + pos_emb[row]: the speakers a request does not name
// (core/tts_streaming.rs:397-403) and SpeakerEncoder::empty (:411-416).  zeros_like + learnt_padding is the padding itself
// (+0 + x = x), then add_sin_embeddings' one f32 add.
__global__ void spk_pad_rows_kernel(float* __restrict__ rows, const float* __restrict__ pad, const float* __restrict__ pos, long row0,
                                    long nrows, int dim) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nrows * dim) return;
  const long at = row0 * dim + e;
  rows[at] = (0.0f + pad[e % dim]) + pos[at];
}

__global__ void fill_u32_kernel(uint32_t* p, uint32_t v, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ------------------------------------------------------------------------------------------
// Ingest and egress (dsm_pcm_format.h, which holds the definition once, with a direction; this project's own, off by default):
// two kernels of one shape.  One 256-thread workgroup per slot; the slot's history and the step's input samples are staged in
// dynamic LDS as f32; each thread walks outputs n = tid, tid + 256, ... with the serial fp64 chain of dsm_pcm_output (a product
// of two floats is exact in double: v_fma_f64 gives the host's multiply-add bits); then the input's last `taps` samples become
// the history.  A slot that is masked off, or does not emit, returns at once: nothing read, nothing written.  Every index is
// bounded by the descriptor, which the engine admits through dsm_pcm::check only.
// ------------------------------------------------------------------------------------------

// buf[0 .. taps): the slot's history, zeros while the slot has not started
__device__ __forceinline__ void pcm_stage_history(float* buf, const float* hist, uint32_t taps, uint32_t started, uint32_t tid) {
  for (uint32_t i = tid; i < taps; i += 256) buf[i] = started ? hist[i] : 0.0f;
}
// the last `taps` of the n_in input samples behind the history become the history (LDS is read-only since the barrier)
__device__ __forceinline__ void pcm_keep_history(float* hist, const float* buf, uint32_t n_in, uint32_t taps, uint32_t tid) {
  for (uint32_t i = tid; i < taps; i += 256) hist[i] = buf[n_in + i];
}

// Ingest (DSM_PCM_IN): a slot's raw frame — its own sample rate and sample format — to the 1920 samples at 24 kHz of the step,
// written where upload_pcm's 2-D copy writes them: MimiState::pcm at the init conv's pitch.  LDS: taps + frame <= 136 + 3840 =
// 3976 floats; coefficient reads inside the table.
struct IngestArgs {
  const uint8_t* raw;           // [B][pitch] bytes
  size_t pitch;
  const uint8_t* mask;          // [B]
  const uint32_t* slot_desc;    // [B] index into descs
  const dsm_pcm_desc* descs;
  const float* coef;            // the coefficient arena
  const float* g711;            // [2][256]
  float* hist;                  // [B][DSM_PCM_MAX_TAPS_IN]
  uint32_t* started;            // [B]
  float* pcm;                   // slot 0's frame; slots are pcm_pitch floats apart
  long pcm_pitch;
};

constexpr size_t ingest_lds() { return sizeof(float) * (DSM_PCM_MAX_TAPS_IN + DSM_PCM_MAX_FRAME); }
__global__ __launch_bounds__(256) void ingest_resample_kernel(IngestArgs a) {
  extern __shared__ float ingest_buf[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!a.mask[b]) return;
  const dsm_pcm_desc d = a.descs[a.slot_desc[b]];
  const uint8_t* row = a.raw + (size_t)b * a.pitch;
  float* out = a.pcm + (long)b * a.pcm_pitch;
  float* hist = a.hist + (size_t)b * DSM_PCM_MAX_TAPS_IN;
  const uint32_t started = a.started[b];
  pcm_stage_history(ingest_buf, hist, d.taps, started, tid);
  for (uint32_t i = tid; i < d.frame; i += 256) ingest_buf[d.taps + i] = dsm_unpaired(dsm_pcm_decode(d.fmt, row, i, a.g711));
  __syncthreads();
  const float* coef = a.coef + d.table_off;
  for (int n = tid; n < DSM_FRAME_SIZE; n += 256) out[n] = dsm_pcm_output(DSM_PCM_IN, &d, coef, ingest_buf, started, n);
  pcm_keep_history(hist, ingest_buf, d.frame, d.taps, tid);
  if (tid == 0) a.started[b] = 1u;
}

// Egress (DSM_PCM_OUT): the 1920 samples at 24 kHz a slot's decode produced — MimiDecState::pcm — to a frame of the slot's own
// output sample rate and sample format, in the slot's row of the staging buffer the download reads.  Outputs n < frame, each
// encoded and stored (a dword, a short or a byte: at most 3840 stores a row).  LDS: taps + 1920 <= 204 + 1920 = 2124 floats;
// coefficient reads inside the table, stores inside frame_bytes <= 15360 <= pitch.
struct EgressArgs {
  const float* pcm;             // [B][DSM_FRAME_SIZE] the decoder's frames
  const uint8_t* valid;         // [B] the decoder's mask: the slot emits
  const uint32_t* slot_desc;    // [B] index into descs
  const dsm_pcm_desc* descs;
  const float* coef;            // the coefficient arena
  float* hist;                  // [B][DSM_PCM_MAX_TAPS_OUT]
  uint32_t* started;            // [B]
  uint8_t* raw;                 // [B][pitch] bytes, rows 16-byte aligned
  size_t pitch;
};

constexpr size_t egress_lds() { return sizeof(float) * (DSM_PCM_MAX_TAPS_OUT + DSM_FRAME_SIZE); }
__global__ __launch_bounds__(256) void egress_resample_kernel(EgressArgs a) {
  extern __shared__ float egress_buf[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!a.valid[b]) return;
  const dsm_pcm_desc d = a.descs[a.slot_desc[b]];
  const float* frame = a.pcm + (size_t)b * DSM_FRAME_SIZE;
  uint8_t* row = (uint8_t*)__builtin_assume_aligned(a.raw + (size_t)b * a.pitch, 16);
  if (d.taps == 0u && d.fmt == DSM_PCM_F32) {  // pass-through: the bits as they are, no state but "started"
    const uint32_t* src = (const uint32_t*)frame;
    uint32_t* dst = (uint32_t*)row;
    for (int n = tid; n < DSM_FRAME_SIZE; n += 256) dst[n] = src[n];
    if (tid == 0) a.started[b] = 1u;
    return;
  }
  float* hist = a.hist + (size_t)b * DSM_PCM_MAX_TAPS_OUT;
  const uint32_t started = a.started[b];
  pcm_stage_history(egress_buf, hist, d.taps, started, tid);
  for (uint32_t i = tid; i < DSM_FRAME_SIZE; i += 256) egress_buf[d.taps + i] = frame[i];
  __syncthreads();
  const float* coef = a.coef + d.table_off;
  for (uint32_t n = tid; n < d.frame; n += 256)
    dsm_pcm_store(d.fmt, row, n, dsm_unpaired(dsm_pcm_output(DSM_PCM_OUT, &d, coef, egress_buf, started, (int)n)));
  pcm_keep_history(hist, egress_buf, DSM_FRAME_SIZE, d.taps, tid);
  if (tid == 0) a.started[b] = 1u;
}

// ------------------------------------------------------------------------------------------
// Clips (dsm_asr_clip.h, which holds the definition; dsm_asr_run, dsm_asr_clip.inc): a slot's audio lies on the device in the
// slot's own ingest format and is cut into frames here, one launch per step in front of ingest_resample_kernel.  Neither kernel
// is part of a captured graph: the step's index k is a launch argument, every pointer an engine buffer.
// ------------------------------------------------------------------------------------------
struct AsrClipSlot {  // one per slot, uploaded with a block's table
  uint32_t bytes;        // the clip's length as of the block (<= cap)
  uint32_t frame_bytes;  // the slot's format's frame (<= pitch)
  uint32_t silence;      // the byte behind the clip's end (dsm_asr_clip::silence_byte)
  uint32_t reserved;
};
struct AsrClipArgs {
  const uint8_t* clips;        // [B][cap] bytes, cap % 16 == 0, 16-byte aligned
  size_t cap;
  const AsrClipSlot* slots;    // [B]
  const uint32_t* frame;       // [K][B] the block's table: frame index
  const uint8_t* step_mask;    // [K][B] and mask
  uint8_t* raw;                // [B][pitch] the raw staging ingest_resample_kernel reads, rows 16-byte aligned
  size_t pitch;                // % 16 == 0
  uint8_t* mask;               // [B] the step's mask (MimiState::mask)
  int B;
};

// Step k of a block: slot b's frame — bytes [i fb, (i + 1) fb) of its clip, the silence byte from the clip's end on — into its
// staging row, and the step's mask.  One 256-thread workgroup per slot; a slot that sits the step out writes its mask byte only.
// A frame starts wherever i fb falls (882-byte frames at 11025 Hz mu-law, 3528-byte ones at 11025 Hz f32): 16-byte loads when
// the source is 16-byte aligned, dwords when it is 4-byte aligned, bytes otherwise; the row is always stored 16 bytes at a time
// where whole 16-byte groups of clip bytes or of silence lie.  Reads stay inside [0, bytes) of the slot's clip, writes inside
// the first min(fb, pitch) bytes of its row.
__global__ __launch_bounds__(256) void asr_clip_frame_kernel(AsrClipArgs a, int k) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t on = a.step_mask[(size_t)k * a.B + b];
  if (tid == 0) a.mask[b] = on;
  if (!on) return;
  const AsrClipSlot s = a.slots[b];
  const uint32_t fb = s.frame_bytes < a.pitch ? s.frame_bytes : (uint32_t)a.pitch;
  const uint64_t off = (uint64_t)a.frame[(size_t)k * a.B + b] * s.frame_bytes;
  const uint32_t len = s.bytes < a.cap ? s.bytes : (uint32_t)a.cap;
  const uint32_t have = off >= len ? 0u : (len - off < fb ? (uint32_t)(len - off) : fb);
  const uint8_t* src = a.clips + (size_t)b * a.cap + (have ? (size_t)off : 0);
  uint8_t* dst = (uint8_t*)__builtin_assume_aligned(a.raw + (size_t)b * a.pitch, 16);
  const uint32_t whole = have & ~15u;  // clip bytes in whole 16-byte groups of the row
  if (((uintptr_t)src & 15u) == 0) {
    const uint4* s16 = (const uint4*)src;
    for (uint32_t i = tid; i < whole / 16; i += 256) ((uint4*)dst)[i] = s16[i];
  } else if (((uintptr_t)src & 3u) == 0) {
    const uint32_t* s4 = (const uint32_t*)src;
    for (uint32_t i = tid; i < whole / 16; i += 256) ((uint4*)dst)[i] = make_uint4(s4[4 * i], s4[4 * i + 1], s4[4 * i + 2], s4[4 * i + 3]);
  } else {
    for (uint32_t i = tid; i < whole / 16; i += 256) {
      uint32_t w[4];
      for (int j = 0; j < 4; ++j)
        w[j] = (uint32_t)src[16 * i + 4 * j] | (uint32_t)src[16 * i + 4 * j + 1] << 8 | (uint32_t)src[16 * i + 4 * j + 2] << 16 |
               (uint32_t)src[16 * i + 4 * j + 3] << 24;
      ((uint4*)dst)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  // the group the clip ends in, byte by byte: clip bytes, then silence up to the next 16-byte boundary or the frame's end
  const uint32_t edge = (have + 15u) & ~15u, mid_end = edge < fb ? edge : fb;
  for (uint32_t i = whole + tid; i < mid_end; i += 256) dst[i] = i < have ? src[i] : (uint8_t)s.silence;
  // silence in whole groups, then the frame's last bytes
  const uint32_t sil = s.silence * 0x01010101u, fill_end = fb & ~15u;
  for (uint32_t i = mid_end / 16 + tid; i < fill_end / 16; i += 256) ((uint4*)dst)[i] = make_uint4(sil, sil, sil, sil);
  for (uint32_t i = (fill_end > mid_end ? fill_end : mid_end) + tid; i < fb; i += 256) dst[i] = (uint8_t)s.silence;
}

// Behind a stream group's LM step, on that group's stream: what the step left for the group's slots [b0, b0 + nb) — text
// token, log-probability (lp NULL: token scores are off, the quiet NaN) and VAD values prs [heads][B] — into row k of the
// block's records (dsm_asr_clip::record_words words a row: text [B], logprob [B], prs [heads][B]).
__global__ void asr_clip_record_kernel(uint32_t* __restrict__ rec, int k, const uint32_t* __restrict__ text, const float* __restrict__ lp,
                                       const float* __restrict__ prs, int b0, int nb, int B, int heads) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb * (2 + heads)) return;
  const int part = i / nb, b = b0 + i % nb;
  uint32_t* row = rec + (size_t)k * B * (2 + heads);
  uint32_t v;
  if (part == 0) v = text[b];
  else if (part == 1) v = lp ? dsm_f32_as_u32(lp[b]) : 0x7FC00000u;
  else v = dsm_f32_as_u32(prs[(size_t)(part - 2) * B + b]);
  row[(size_t)part * B + b] = v;
}
