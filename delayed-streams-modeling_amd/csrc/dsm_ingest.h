/*
 * dsm_ingest.h — per-stream input sample rate and sample format: the definition, once for the HIP kernel
 * (ingest_resample_kernel, dsm_kernels.h) and the host (dsm_ingest_host), the checked descriptor of a format, and the
 * phase-table builder the whole-clip resampler (dsm_mp3::resample, dsm_resample) shares.  This project's own: the reference
 * resamples request bodies only (srv/batched_asr.rs:835-838) and its sockets must send 24 kHz f32.
 *
 * SAMPLE FORMATS (include/dsm.h): DSM_PCM_F32 as it is; DSM_PCM_S16 little endian, (float)v * (1.0f / 32768);
 * DSM_PCM_MULAW / DSM_PCM_ALAW the ITU-T G.711 expansions to 16-bit linear, then the s16 scaling — one 256-entry f32 table
 * each, built by the formulas below (dsm_g711_*_to_s16), so a G.711 sample is one table read.
 *
 * RATES: 8000 <= rate <= 48000 with 2 rate % 25 == 0, so a frame of 80 ms is F_in = 2 rate / 25 whole input samples, and
 * L = 24000 / gcd(rate, 24000) <= 4096.  rate 24000 does not resample: the frame is its 1920 decoded samples (24000 / F32 is
 * the pass-through format: 1920 floats copied untouched).
 *
 * THE SIGNAL.  x = the slot's decoded input since its format was last set (or the slot last reset); y = the whole-clip
 * resampler on x, L / M = 24000 / rate in lowest terms: output j sits at input position j M / L, i0 = floor(j M / L),
 * phase p = j M mod L, and
 *     y[j] = (float) sum over k = 0 .. taps-1, ascending, in double, from +0.0, of (double)c[p][k] * (double)x[i0 + k - half + 1]
 * with x = 0 outside the clip.  A product of two floats is exact in double, so fma and multiply-add give the same bits; a
 * zero sample adds +-0.0 to an accumulator that began at +0.0 and is never -0.0, which is the clip function's skipped tap.
 * Step t delivers z_t[n] = y[1920 t + n - D], 0 where the index is negative.  D = floor(half L / M) is the format's latency
 * in output samples: the smallest for which no tap of frame t reaches past the F_in (t + 1) samples received so far
 * (tests/test_ingest_cpu.py finds it by brute force).  Relative to the frame, with q = n - D:
 *     i0 = F_in t + floor(q M / L),  p = q M mod L  (floor and mod towards minus infinity; 1920 t M / L = F_in t exactly)
 * so a step needs the `taps` samples in front of its frame — the HISTORY, zeros at the start — and nothing of t itself.
 * Taps reach back at most ceil(D M / L) + half - 1 < taps samples.
 *
 * THE DESCRIPTOR, twelve u32 words (dsm_ingest_desc): rate, fmt, L, M, half, taps, F_in, frame_bytes, D, table_off,
 * table_words, reserved 0.  table_off: where the rate's L x taps coefficients start in the coefficient arena it is used with
 * (floats).  Every other word is a function of (rate, fmt); dsm_ingest::check recomputes them and refuses what differs, and
 * checks the table against the arena's length.
 *
 * PER-SLOT STATE, per Mimi side: `taps` history floats and a "started" word (0: no frame since the format was set or the
 * slot reset; the outputs with a negative index are then 0 whatever the frame holds).
 */
#ifndef DSM_INGEST_H
#define DSM_INGEST_H

#include <stdint.h>
#include "../../include/dsm.h"
#include "dsm_numerics.h"

#define DSM_INGEST_OUT_RATE 24000
#define DSM_INGEST_MAX_TAPS 136u   /* 48 kHz: half = ceil(32 / 0.475) = 68 */
#define DSM_INGEST_MAX_FRAME 3840u /* 48 kHz x 80 ms */
#define DSM_INGEST_MAX_FRAME_BYTES (4u * DSM_INGEST_MAX_FRAME)
#define DSM_INGEST_DESC_WORDS 12u

typedef struct dsm_ingest_desc {
  uint32_t rate, fmt, L, M, half, taps, F_in, frame_bytes, D, table_off, table_words, reserved;
} dsm_ingest_desc;

DSM_HD uint32_t dsm_ingest_sample_bytes(uint32_t fmt) { return fmt == DSM_PCM_F32 ? 4u : fmt == DSM_PCM_S16 ? 2u : 1u; }

/* ITU-T G.711 mu-law: the byte is stored inverted; sign 0x80, exponent 0x70, mantissa 0x0F;
 * magnitude = ((mantissa << 3) + 0x84) << exponent, minus the bias 0x84 */
DSM_HD int dsm_g711_ulaw_to_s16(uint32_t byte) {
  const uint32_t u = ~byte & 0xFFu;
  const int t = (int)((((u & 0x0Fu) << 3) + 0x84u) << ((u & 0x70u) >> 4));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}

/* ITU-T G.711 A-law: even bits inverted (xor 0x55); sign 0x80 set = positive; exponent 0: (mantissa << 4) + 8, else
 * ((mantissa << 4) + 0x108) << (exponent - 1) */
DSM_HD int dsm_g711_alaw_to_s16(uint32_t byte) {
  const uint32_t a = (byte ^ 0x55u) & 0xFFu;
  const uint32_t e = (a & 0x70u) >> 4;
  int t = (int)((a & 0x0Fu) << 4);
  t = e == 0u ? t + 8 : (t + 0x108) << (e - 1u);
  return (a & 0x80u) ? t : -t;
}

DSM_HD float dsm_ingest_s16_to_f32(int v) { return (float)v * (1.0f / 32768.0f); }

/* sample i of a raw frame.  g711: [2][256] floats, mu-law then A-law (dsm_ingest::g711_tables) */
DSM_HD float dsm_ingest_decode(uint32_t fmt, const void* raw, uint32_t i, const float* g711) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint8_t* r = (const uint8_t*)__builtin_assume_aligned(raw, 16);  /* the engine's rows: pitch % 16 == 0 */
#else
  const uint8_t* r = (const uint8_t*)raw;  /* any alignment; both sides are little endian */
#endif
  if (fmt == DSM_PCM_F32) {
    uint32_t w;
    __builtin_memcpy(&w, r + 4u * i, 4);
    return dsm_u32_as_f32(w);
  }
  if (fmt == DSM_PCM_S16) {
    int16_t v;
    __builtin_memcpy(&v, r + 2u * i, 2);
    return dsm_ingest_s16_to_f32((int)v);
  }
  return g711[(fmt == DSM_PCM_ALAW ? 256u : 0u) + r[i]];
}

/* output n (0 .. 1919) of a step.  buf: the `taps` history samples followed by the F_in decoded samples of the frame;
 * coef: the rate's phase table [L][taps].  started 0: the outputs in front of the stream (n < D) are 0. */
DSM_HD float dsm_ingest_output(const dsm_ingest_desc* d, const float* coef, const float* buf, uint32_t started, int n) {
  if (d->taps == 0u) return buf[n];  /* 24 kHz in: no filter */
  const int q = n - (int)d->D;
  if (q < 0 && !started) return 0.0f;
  const int L = (int)d->L, num = q * (int)d->M;  /* |q| < 1920, M <= 1920: fits */
  int i0 = num / L, p = num - i0 * L;
  if (p < 0) { p += L; i0 -= 1; }
  const float* c = coef + (size_t)p * d->taps;
  const float* x = buf + ((int)d->taps + i0 - (int)d->half + 1);
  double a = 0.0;
  for (uint32_t k = 0; k < d->taps; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
    a = DSM_FMA((double)c[k], (double)x[k], a);
#else
    a = a + (double)c[k] * (double)x[k];
#endif
  }
  return (float)a;
}

/* ---- host only from here: the phase table, the descriptor and its checked reader, the streaming host state ---- */
#if defined(__cplusplus)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace dsm_ingest {

inline int fail(std::string* err, const char* fmt, long a = 0, long b = 0) {
  if (err) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    *err = buf;
  }
  return DSM_ERR_INVALID;
}

inline long gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }

inline double bessel_i0(double x) {
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 64; ++k) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
  return s;
}

/* The windowed-sinc phase table of rin -> rout (rin != rout), the one dsm_mp3::resample has always used: Kaiser window beta
 * 8.6, 32 zero crossings each side, cut-off 0.95 x the lower Nyquist, every phase normalised to unit DC gain, stored as
 * float.  -1 when the ratio needs more than 4096 phases. */
inline int phase_table(int rin, int rout, long* L_out, long* M_out, int* half_out, std::vector<float>* ph_out) {
  if (rin <= 0 || rout <= 0 || rin == rout) return -1;
  const long g = gcd(rin, rout), L = rout / g, M = rin / g;
  if (L > 4096) return -1;  // the phase table would be unreasonable: not a ratio between audio rates
  const int Z = 32;
  const double fc = 0.95 * (rout < rin ? (double)rout / rin : 1.0);  // relative to the input's Nyquist
  const int half = (int)ceil(Z / fc);
  const int taps = 2 * half;
  if (L_out) *L_out = L;
  if (M_out) *M_out = M;
  if (half_out) *half_out = half;
  if (!ph_out) return 0;
  const double beta = 8.6, i0b = bessel_i0(beta);
  std::vector<float>& ph = *ph_out;
  ph.assign((size_t)L * taps, 0.0f);
  for (long p = 0; p < L; ++p) {  // phase p: fractional position p / L past the integer input index
    double sum = 0.0;
    for (int k = 0; k < taps; ++k) {
      const double t = (k - half + 1) - (double)p / L;  // distance (input samples) from the output instant to tap k
      const double x = M_PI * fc * t;
      const double w = fabs(t) < half ? bessel_i0(beta * sqrt(1.0 - (t / half) * (t / half))) / i0b : 0.0;
      const double v = fc * (fabs(x) < 1e-12 ? 1.0 : sin(x) / x) * w;
      ph[(size_t)p * taps + k] = (float)v;
      sum += v;
    }
    for (int k = 0; k < taps; ++k) ph[(size_t)p * taps + k] = (float)(ph[(size_t)p * taps + k] / sum);  // unit DC gain per phase
  }
  return 0;
}

/* [2][256]: mu-law, A-law, each entry the expansion scaled like an s16 sample */
inline const float* g711_tables() {
  static const std::vector<float> t = [] {
    std::vector<float> v(512);
    for (uint32_t b = 0; b < 256u; ++b) {
      v[b] = dsm_ingest_s16_to_f32(dsm_g711_ulaw_to_s16(b));
      v[256u + b] = dsm_ingest_s16_to_f32(dsm_g711_alaw_to_s16(b));
    }
    return v;
  }();
  return t.data();
}

/* (rate, fmt) -> every word of the descriptor but table_off (left 0).  DSM_ERR_INVALID with a message for anything else. */
inline int describe(long rate, long fmt, dsm_ingest_desc* d, std::string* err) {
  if (fmt != DSM_PCM_F32 && fmt != DSM_PCM_S16 && fmt != DSM_PCM_MULAW && fmt != DSM_PCM_ALAW)
    return fail(err, "input format: sample format %ld (0 f32, 1 s16, 2 mu-law, 3 A-law)", fmt);
  if (rate < 8000 || rate > 48000) return fail(err, "input format: sample rate %ld Hz is outside 8000 .. 48000", rate);
  if ((2 * rate) % 25 != 0) return fail(err, "input format: %ld Hz does not give a whole number of samples per 80 ms frame", rate);
  memset(d, 0, sizeof *d);
  d->rate = (uint32_t)rate;
  d->fmt = (uint32_t)fmt;
  d->F_in = (uint32_t)(2 * rate / 25);
  d->frame_bytes = d->F_in * dsm_ingest_sample_bytes(d->fmt);
  if (rate == DSM_INGEST_OUT_RATE) {
    d->L = d->M = 1u;
    return 0;
  }
  long L = 0, M = 0;
  int half = 0;
  if (phase_table((int)rate, DSM_INGEST_OUT_RATE, &L, &M, &half, nullptr))
    return fail(err, "input format: %ld Hz needs more than 4096 filter phases", rate);
  d->L = (uint32_t)L;
  d->M = (uint32_t)M;
  d->half = (uint32_t)half;
  d->taps = 2u * d->half;
  d->D = (uint32_t)(((long)half * L) / M);
  d->table_words = d->L * d->taps;
  if (d->taps > DSM_INGEST_MAX_TAPS || d->F_in > DSM_INGEST_MAX_FRAME) return fail(err, "input format: %ld Hz is outside the filter's bounds", rate);
  return 0;
}

/* Everything the step relies on, so that no descriptor — however it was made — reads outside the frame, the history or the
 * coefficient arena of `arena_words` floats: each word against what (rate, fmt) gives, the table inside the arena. */
inline int check(const dsm_ingest_desc* d, size_t arena_words, std::string* err) {
  if (!d) return fail(err, "input format descriptor: NULL");
  dsm_ingest_desc want;
  if (int rc = describe((long)d->rate, (long)d->fmt, &want, err)) return rc;
  want.table_off = d->table_off;
  if (memcmp(&want, d, sizeof want) != 0) return fail(err, "input format descriptor: its words are not those of %ld Hz, format %ld", (long)d->rate, (long)d->fmt);
  if ((uint64_t)d->table_off + d->table_words > (uint64_t)arena_words)
    return fail(err, "input format descriptor: its table ends at word %ld of an arena of %ld", (long)((uint64_t)d->table_off + d->table_words), (long)arena_words);
  return 0;
}

/* One slot's streaming state on the host: descriptor, its own coefficient arena, history + frame, the started word */
struct Host {
  dsm_ingest_desc d{};
  std::vector<float> coef, buf;
  uint32_t started = 0;
};

inline int host_new(long rate, long fmt, Host* h, std::string* err) {
  if (int rc = describe(rate, fmt, &h->d, err)) return rc;
  h->coef.clear();
  if (h->d.taps) {
    if (phase_table((int)rate, DSM_INGEST_OUT_RATE, nullptr, nullptr, nullptr, &h->coef)) return fail(err, "input format: no phase table for %ld Hz", rate);
  }
  h->buf.assign((size_t)h->d.taps + h->d.F_in, 0.0f);
  h->started = 0;
  return check(&h->d, h->coef.size(), err);
}

/* one frame of `bytes` raw bytes -> 1920 samples at 24 kHz.  A frame of another length than the format's is refused. */
inline int host_step(Host* h, const void* raw, size_t bytes, float* out, std::string* err) {
  if (!h || !raw || !out) return fail(err, "ingest: a NULL pointer");
  const dsm_ingest_desc& d = h->d;
  if (int rc = check(&d, h->coef.size(), err)) return rc;
  if (bytes != d.frame_bytes) return fail(err, "ingest: a frame of %ld bytes, the format's frame has %ld", (long)bytes, (long)d.frame_bytes);
  if (h->buf.size() != (size_t)d.taps + d.F_in) return fail(err, "ingest: the state does not belong to its descriptor");
  if (d.taps == 0u && d.fmt == DSM_PCM_F32) {  // pass-through: the bytes as they are
    memcpy(out, raw, sizeof(float) * DSM_FRAME_SIZE);
    h->started = 1;
    return 0;
  }
  float* buf = h->buf.data();
  if (h->started) memmove(buf, buf + d.F_in, sizeof(float) * d.taps);  // F_in >= 640 > taps: the last taps samples of the frame before
  const float* g = g711_tables();
  for (uint32_t i = 0; i < d.F_in; ++i) buf[d.taps + i] = dsm_ingest_decode(d.fmt, raw, i, g);
  for (int n = 0; n < DSM_FRAME_SIZE; ++n) out[n] = dsm_ingest_output(&d, h->coef.data(), buf, h->started, n);
  h->started = 1;
  return 0;
}

}  // namespace dsm_ingest
#endif /* host */

#endif /* DSM_INGEST_H */
