/*
 * dsm_pcm_format.h — a sample rate and a sample format per slot, on the way in (STT ingest: a stream's raw frames -> the 24 kHz
 * f32 frames Mimi takes) and on the way out (TTS egress: the 24 kHz f32 frames Mimi's decoder gives -> a slot's raw rows).  ONE
 * definition with a direction — DSM_PCM_IN is rate -> 24000, DSM_PCM_OUT is 24000 -> rate — stated once for the two HIP kernels
 * (ingest_resample_kernel, egress_resample_kernel: dsm_kernels.h) and for the host (dsm_ingest_host, dsm_egress_host), with the
 * checked descriptor of a format, the sample codecs, and the phase-table builder the whole-clip resampler (dsm_mp3::resample,
 * dsm_resample) shares.  This project's own: the reference resamples request bodies only (srv/batched_asr.rs:835-838), its STT
 * sockets must send 24 kHz f32 and its TTS sockets send 24 kHz f32 (srv/tts.rs:528-544).
 *
 * FORMATS: a rate, 8000 <= rate <= 48000 with 2 rate % 25 == 0, so a frame of 80 ms is `frame` = 2 rate / 25 whole samples at
 * `rate`, and the filter has L <= 4096 phases (in: L = 24000 / gcd(rate, 24000); out: L = rate / gcd(rate, 24000)); and a sample
 * format of include/dsm.h.  rate 24000 does not resample: the frame is the step's 1920 samples, decoded or encoded.  24000 / F32
 * is the pass-through format and every slot's default: 1920 floats copied bit for bit, latency 0.
 *
 * SAMPLE FORMATS, decoded (in): DSM_PCM_F32 as it is; DSM_PCM_S16 little endian, (float)v * (1.0f / 32768); DSM_PCM_MULAW /
 * DSM_PCM_ALAW the ITU-T G.711 expansions to 16-bit linear, then the s16 scaling — one 256-entry f32 table each, built by the
 * formulas below (dsm_g711_*_to_s16), so a G.711 sample is one table read.
 * SAMPLE FORMATS, encoded (out; integer or float code, no table): F32 the float as it is.  S16: r = rintf(v * 32768.0f) (round
 * half to even; the product is exact), NaN gives 0, clamped to [-32768, 32767], stored little endian.  mu-law from that s16
 * value s: sign = s < 0, mag = min(|s|, 32635) + 0x84, e = floor(log2 mag) - 7 (0 .. 7), m = (mag >> (e + 3)) & 0xF,
 * byte = ~(sign << 7 | e << 4 | m) & 0xFF.  A-law from s: sign = s < 0, mag = sign ? -s - 1 : s, e = mag < 256 ? 0 :
 * floor(log2 mag) - 7, m = e == 0 ? (mag >> 4) & 0xF : (mag >> (e + 3)) & 0xF, byte = ((sign ? 0 : 0x80) | e << 4 | m) ^ 0x55.
 * Both invert the expanders (encode(decode(b)) == b for every byte but mu-law's negative zero 0x7F, which decodes to 0 and
 * encodes as 0xFF) and are monotone.
 *
 * THE SIGNAL.  x = the slot's input since its format was last set (or the slot last reset); y = the whole-clip resampler on x,
 * dsm_resample(x, from, to), L / M = to / from in lowest terms (in: 24000 / rate; out: rate / 24000): output j sits at input
 * position j M / L, i0 = floor(j M / L), phase p = j M mod L, and
 *     y[j] = (float) sum over k = 0 .. taps-1, ascending, in double, from +0.0, of (double)c[p][k] * (double)x[i0 + k - half + 1]
 * with x = 0 outside the clip.  A product of two floats is exact in double, so fma and multiply-add give the same bits; a
 * zero sample adds +-0.0 to an accumulator that began at +0.0 and is never -0.0, which is the clip function's skipped tap.
 * A step takes N_in input samples and delivers N_out = N_in L / M output samples (exactly), z_t[n] = y[N_out t + n - D], 0 where
 * the index is negative.  D = floor(half L / M) is the format's latency in output samples: the smallest delay for which no tap
 * of frame t reaches past the N_in (t + 1) samples received so far (tests/test_ingest_cpu.py and tests/test_egress_cpu.py find
 * it by brute force).  Relative to the frame, with q = n - D:
 *     i0 = N_in t + floor(q M / L),  p = q M mod L  (floor and mod towards minus infinity; N_out t M / L = N_in t exactly)
 * so a step needs the `taps` samples in front of its frame — the HISTORY, zeros at the start — and the frame itself, and nothing
 * that depends on t.  Taps reach back at most ceil(D M / L) + half - 1 < taps samples in front of the frame and forward to the
 * frame's last sample at most.
 *
 * DSM_PCM_IN: x = the slot's decoded raw frames; N_in = `frame` samples at `rate`, N_out = 1920 is the fixed side.  D counts
 * 24 kHz samples.  What a NaN or an infinity in the input gives is whatever the chain gives: no bits are promised for it.
 *
 * DSM_PCM_OUT: x = the slot's emitted 24 kHz PCM; only the frames of steps in which the slot emits count — a step in which it
 * does not contributes nothing and leaves the state alone.  N_in = 1920 is the fixed side, N_out = `frame` samples at `rate`,
 * each through the sample encoder.  D counts samples at `rate`.  A sum that is a NaN is delivered as the quiet NaN 0x7FC00000:
 * which sign and payload an instruction set gives a NaN it generates or passes on is not the same on the two sides, and one
 * definition has to hold on both.  THE LAST D OUTPUT SAMPLES OF A GENERATION (at most 4.25 ms) ARE NEVER DELIVERED: they would
 * need input behind the last frame.  There is no flush call.
 *
 * THE DESCRIPTOR, twelve u32 words (dsm_pcm_desc): rate, fmt, L, M, half, taps, frame, frame_bytes, D, table_off, table_words,
 * reserved 0.  table_off: where the rate's L x taps coefficients start in the coefficient arena it is used with (floats).
 * Every other word is a function of (direction, rate, fmt); dsm_pcm::check recomputes them and refuses what differs, and
 * checks the table against the arena's length.  The direction is not a word of the descriptor: whoever holds one knows which
 * way it runs, and a resampling descriptor made for one direction does not pass check in the other.
 *
 * PER-SLOT STATE (in: per Mimi side): `taps` history floats and a "started" word (0: no frame since the format was set or the
 * slot reset; the history then reads as zeros and the outputs with a negative index are 0 whatever the frame holds).
 */
#ifndef DSM_PCM_FORMAT_H
#define DSM_PCM_FORMAT_H

#include <stdint.h>
#include "../../include/dsm.h"
#include "dsm_numerics.h"

#define DSM_PCM_IN 0   /* rate -> 24000 */
#define DSM_PCM_OUT 1  /* 24000 -> rate */
#define DSM_PCM_RATE 24000          /* the fixed side */
#define DSM_PCM_MAX_TAPS_IN 136u    /* 48 kHz in: half = ceil(32 / 0.475) = 68 */
#define DSM_PCM_MAX_TAPS_OUT 204u   /* 8 kHz out: half = ceil(32 / (0.95 / 3)) = 102 */
#define DSM_PCM_MAX_FRAME 3840u     /* 48 kHz x 80 ms */
#define DSM_PCM_MAX_FRAME_BYTES (4u * DSM_PCM_MAX_FRAME)
#define DSM_PCM_DESC_WORDS 12u

typedef struct dsm_pcm_desc {
  uint32_t rate, fmt, L, M, half, taps, frame, frame_bytes, D, table_off, table_words, reserved;
} dsm_pcm_desc;

DSM_HD uint32_t dsm_pcm_sample_bytes(uint32_t fmt) { return fmt == DSM_PCM_F32 ? 4u : fmt == DSM_PCM_S16 ? 2u : 1u; }

/* ---- sample codecs ---- */

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

/* ITU-T G.711 mu-law compression of a 16-bit value (the inverse of dsm_g711_ulaw_to_s16) */
DSM_HD uint32_t dsm_g711_s16_to_ulaw(int s) {
  const uint32_t sign = s < 0 ? 1u : 0u;
  uint32_t mag = (uint32_t)(s < 0 ? -s : s);
  if (mag > 32635u) mag = 32635u;
  mag += 0x84u;                                          /* 0x84 .. 0x7FFF: bit 7 .. bit 14 leads */
  const uint32_t e = (31u - (uint32_t)__builtin_clz(mag)) - 7u;
  const uint32_t m = (mag >> (e + 3u)) & 0xFu;
  return ~(sign << 7 | e << 4 | m) & 0xFFu;
}

/* ITU-T G.711 A-law compression of a 16-bit value (the inverse of dsm_g711_alaw_to_s16) */
DSM_HD uint32_t dsm_g711_s16_to_alaw(int s) {
  const uint32_t sign = s < 0 ? 1u : 0u;
  const uint32_t mag = (uint32_t)(s < 0 ? -s - 1 : s);  /* 0 .. 32767 */
  const uint32_t e = mag < 256u ? 0u : (31u - (uint32_t)__builtin_clz(mag)) - 7u;
  const uint32_t m = e == 0u ? (mag >> 4) & 0xFu : (mag >> (e + 3u)) & 0xFu;
  return ((sign ? 0u : 0x80u) | e << 4 | m) ^ 0x55u;
}

DSM_HD float dsm_pcm_s16_to_f32(int v) { return (float)v * (1.0f / 32768.0f); }

/* f32 -> the s16 value: round half to even, NaN 0, clamped */
DSM_HD int dsm_pcm_f32_to_s16(float v) {
  if (v != v) return 0;
  const float r = __builtin_rintf(v * 32768.0f);
  if (r >= 32767.0f) return 32767;
  if (r <= -32768.0f) return -32768;
  return (int)r;
}

/* sample i of a raw frame.  g711: [2][256] floats, mu-law then A-law (dsm_pcm::g711_tables) */
DSM_HD float dsm_pcm_decode(uint32_t fmt, const void* raw, uint32_t i, const float* g711) {
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
    return dsm_pcm_s16_to_f32((int)v);
  }
  return g711[(fmt == DSM_PCM_ALAW ? 256u : 0u) + r[i]];
}

/* sample i of a row.  Rows of the engine are 16-byte aligned; a host row may sit anywhere (both sides are little endian) */
DSM_HD void dsm_pcm_store(uint32_t fmt, void* row, uint32_t i, float v) {
  uint8_t* r = (uint8_t*)row;
  if (fmt == DSM_PCM_F32) {
    const uint32_t w = dsm_f32_as_u32(v);
    __builtin_memcpy(r + 4u * i, &w, 4);
    return;
  }
  const int s = dsm_pcm_f32_to_s16(v);
  if (fmt == DSM_PCM_S16) {
    const int16_t h = (int16_t)s;
    __builtin_memcpy(r + 2u * i, &h, 2);
    return;
  }
  r[i] = (uint8_t)(fmt == DSM_PCM_ALAW ? dsm_g711_s16_to_alaw(s) : dsm_g711_s16_to_ulaw(s));
}

/* ---- the chain ---- */

/* output n (in: 0 .. 1919; out: 0 .. frame - 1, before the sample encoder) of a step.  buf: the `taps` history samples followed
 * by the step's input samples (in: the `frame` decoded samples; out: the 1920 samples of the emitted frame); coef: the rate's
 * phase table [L][taps].  started 0: the outputs in front of the stream (n < D) are 0. */
DSM_HD float dsm_pcm_output(int dir, const dsm_pcm_desc* d, const float* coef, const float* buf, uint32_t started, int n) {
  if (d->taps == 0u) return buf[n];  /* 24 kHz: no filter */
  const int q = n - (int)d->D;
  if (q < 0 && !started) return 0.0f;
  const int L = (int)d->L, num = q * (int)d->M;  /* |q| < 3840, M <= 1920 (in: |q| < 1920; out: M <= 960): fits */
  int i0 = num / L, p = num - i0 * L;
  if (p < 0) { p += L; i0 -= 1; }
  const float* c = coef + (size_t)p * d->taps;
  const float* x = buf + ((int)d->taps + i0 - (int)d->half + 1);  /* 1 <= index, index + taps - 1 <= taps + N_in - 1 */
  double a = 0.0;
  for (uint32_t k = 0; k < d->taps; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
    a = DSM_FMA((double)c[k], (double)x[k], a);
#else
    a = a + (double)c[k] * (double)x[k];
#endif
  }
  if (dir == DSM_PCM_OUT && a != a) return dsm_u32_as_f32(0x7FC00000u);
  return (float)a;
}

/* ---- host only from here: the phase table, the descriptor and its checked reader, the streaming host state ---- */
#if defined(__cplusplus)
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace dsm_pcm {

__attribute__((format(printf, 2, 3))) inline int fail(std::string* err, const char* fmt, ...) {
  if (err) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
  }
  return DSM_ERR_INVALID;
}

/* the word the messages about a format begin with */
inline const char* side(int dir) { return dir == DSM_PCM_IN ? "input" : "output"; }

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

/* the phase table of a format's rate: rate -> 24000 in, 24000 -> rate out */
inline int rate_table(int dir, long rate, long* L_out, long* M_out, int* half_out, std::vector<float>* ph_out) {
  return dir == DSM_PCM_IN ? phase_table((int)rate, DSM_PCM_RATE, L_out, M_out, half_out, ph_out)
                           : phase_table(DSM_PCM_RATE, (int)rate, L_out, M_out, half_out, ph_out);
}

/* [2][256]: mu-law, A-law, each entry the expansion scaled like an s16 sample */
inline const float* g711_tables() {
  static const std::vector<float> t = [] {
    std::vector<float> v(512);
    for (uint32_t b = 0; b < 256u; ++b) {
      v[b] = dsm_pcm_s16_to_f32(dsm_g711_ulaw_to_s16(b));
      v[256u + b] = dsm_pcm_s16_to_f32(dsm_g711_alaw_to_s16(b));
    }
    return v;
  }();
  return t.data();
}

/* (dir, rate, fmt) -> every word of the descriptor but table_off (left 0).  DSM_ERR_INVALID with a message for anything else. */
inline int describe(int dir, long rate, long fmt, dsm_pcm_desc* d, std::string* err) {
  const char* s = side(dir);
  if (fmt != DSM_PCM_F32 && fmt != DSM_PCM_S16 && fmt != DSM_PCM_MULAW && fmt != DSM_PCM_ALAW)
    return fail(err, "%s format: sample format %ld (0 f32, 1 s16, 2 mu-law, 3 A-law)", s, fmt);
  if (rate < 8000 || rate > 48000) return fail(err, "%s format: sample rate %ld Hz is outside 8000 .. 48000", s, rate);
  if ((2 * rate) % 25 != 0) return fail(err, "%s format: %ld Hz does not give a whole number of samples per 80 ms frame", s, rate);
  memset(d, 0, sizeof *d);
  d->rate = (uint32_t)rate;
  d->fmt = (uint32_t)fmt;
  d->frame = (uint32_t)(2 * rate / 25);
  d->frame_bytes = d->frame * dsm_pcm_sample_bytes(d->fmt);
  if (rate == DSM_PCM_RATE) {
    d->L = d->M = 1u;
    return 0;
  }
  long L = 0, M = 0;
  int half = 0;
  if (rate_table(dir, rate, &L, &M, &half, nullptr)) return fail(err, "%s format: %ld Hz needs more than 4096 filter phases", s, rate);
  d->L = (uint32_t)L;
  d->M = (uint32_t)M;
  d->half = (uint32_t)half;
  d->taps = 2u * d->half;
  d->D = (uint32_t)(((long)half * L) / M);
  d->table_words = d->L * d->taps;
  if (d->taps > (dir == DSM_PCM_IN ? DSM_PCM_MAX_TAPS_IN : DSM_PCM_MAX_TAPS_OUT) || d->frame > DSM_PCM_MAX_FRAME)
    return fail(err, "%s format: %ld Hz is outside the filter's bounds", s, rate);
  return 0;
}

/* Everything the step relies on, so that no descriptor — however it was made — reads outside the frame, the history or the
 * coefficient arena of `arena_words` floats, or writes outside its row: each word against what (dir, rate, fmt) gives, the
 * table inside the arena. */
inline int check(int dir, const dsm_pcm_desc* d, size_t arena_words, std::string* err) {
  const char* s = side(dir);
  if (!d) return fail(err, "%s format descriptor: NULL", s);
  dsm_pcm_desc want;
  if (int rc = describe(dir, (long)d->rate, (long)d->fmt, &want, err)) return rc;
  want.table_off = d->table_off;
  if (memcmp(&want, d, sizeof want) != 0)
    return fail(err, "%s format descriptor: its words are not those of %ld Hz, format %ld", s, (long)d->rate, (long)d->fmt);
  if ((uint64_t)d->table_off + d->table_words > (uint64_t)arena_words)
    return fail(err, "%s format descriptor: its table ends at word %ld of an arena of %ld", s, (long)((uint64_t)d->table_off + d->table_words),
                (long)arena_words);
  return 0;
}

/* One slot's streaming state on the host: direction, descriptor, its own coefficient arena, history + the step's input samples,
 * the started word */
struct Host {
  int dir = DSM_PCM_IN;
  dsm_pcm_desc d{};
  std::vector<float> coef, buf;
  uint32_t started = 0;
  uint32_t n_in() const { return dir == DSM_PCM_IN ? d.frame : (uint32_t)DSM_FRAME_SIZE; }   // samples a step takes
  uint32_t n_out() const { return dir == DSM_PCM_IN ? (uint32_t)DSM_FRAME_SIZE : d.frame; }  // samples a step delivers
};

inline int host_new(int dir, long rate, long fmt, Host* h, std::string* err) {
  h->dir = dir;
  if (int rc = describe(dir, rate, fmt, &h->d, err)) return rc;
  h->coef.clear();
  if (h->d.taps && rate_table(dir, rate, nullptr, nullptr, nullptr, &h->coef)) return fail(err, "%s format: no phase table for %ld Hz", side(dir), rate);
  h->buf.assign((size_t)h->d.taps + h->n_in(), 0.0f);
  h->started = 0;
  return check(dir, &h->d, h->coef.size(), err);
}

/* What the two step functions share.  host_admit: the checks in front of a step — nothing is read or written before they pass
 * (raw_bytes: the length of a raw frame, in only: another length than the format's is refused).  host_pass: the pass-through
 * format, the bytes as they are.  host_shift: the last `taps` samples of the step before become the history (n_in >= 640 >
 * taps); returns where the step's input samples go.  host_emit: every output of the step, in order, handed to `put`. */
inline int host_admit(const Host* h, int dir, const void* in, const void* out, const size_t* raw_bytes, std::string* err) {
  const char* who = dir == DSM_PCM_IN ? "ingest" : "egress";
  if (!h || !in || !out) return fail(err, "%s: a NULL pointer", who);
  if (int rc = check(h->dir, &h->d, h->coef.size(), err)) return rc;
  if (raw_bytes && *raw_bytes != h->d.frame_bytes)
    return fail(err, "%s: a frame of %ld bytes, the format's frame has %ld", who, (long)*raw_bytes, (long)h->d.frame_bytes);
  if (h->dir != dir || h->buf.size() != (size_t)h->d.taps + h->n_in()) return fail(err, "%s: the state does not belong to its descriptor", who);
  return 0;
}

inline bool host_pass(Host* h, const void* in, void* out) {
  if (h->d.taps != 0u || h->d.fmt != DSM_PCM_F32) return false;
  memcpy(out, in, sizeof(float) * DSM_FRAME_SIZE);
  h->started = 1;
  return true;
}

inline float* host_shift(Host* h) {
  float* buf = h->buf.data();
  if (h->started) memmove(buf, buf + h->n_in(), sizeof(float) * h->d.taps);
  return buf + h->d.taps;
}

template <typename Put>
inline void host_emit(Host* h, Put put) {
  const uint32_t n_out = h->n_out();
  for (uint32_t n = 0; n < n_out; ++n) put(n, dsm_pcm_output(h->dir, &h->d, h->coef.data(), h->buf.data(), h->started, (int)n));
  h->started = 1;
}

/* in: one frame of `bytes` raw bytes -> 1920 samples at 24 kHz */
inline int host_step_in(Host* h, const void* raw, size_t bytes, float* out, std::string* err) {
  if (int rc = host_admit(h, DSM_PCM_IN, raw, out, &bytes, err)) return rc;
  if (host_pass(h, raw, out)) return 0;
  float* x = host_shift(h);
  const float* g = g711_tables();
  for (uint32_t i = 0; i < h->d.frame; ++i) x[i] = dsm_pcm_decode(h->d.fmt, raw, i, g);
  host_emit(h, [&](uint32_t n, float v) { out[n] = v; });
  return 0;
}

/* out: one emitted frame of 1920 samples at 24 kHz -> the format's frame_bytes bytes in out_row */
inline int host_step_out(Host* h, const float* frame1920, void* out_row, std::string* err) {
  if (int rc = host_admit(h, DSM_PCM_OUT, frame1920, out_row, nullptr, err)) return rc;
  if (host_pass(h, frame1920, out_row)) return 0;
  memcpy(host_shift(h), frame1920, sizeof(float) * DSM_FRAME_SIZE);
  host_emit(h, [&](uint32_t n, float v) { dsm_pcm_store(h->d.fmt, out_row, n, v); });
  return 0;
}

}  // namespace dsm_pcm
#endif /* host */

#endif /* DSM_PCM_FORMAT_H */
