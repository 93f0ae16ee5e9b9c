/*
 * dsm_egress.h — per-slot TTS output sample rate and sample format: the definition, once for the HIP kernel
 * (egress_resample_kernel, dsm_kernels.h) and the host (dsm_egress_host), and the checked descriptor of a format.  The ingest
 * section (dsm_ingest.h) run the other way: the same rate set, the same sample formats, the same filter family — the phase
 * table is dsm_ingest::phase_table(24000, rate) and nothing here designs a filter.  This project's own: the reference's TTS
 * sockets send 24 kHz f32 (srv/tts.rs:528-544).
 *
 * FORMATS: a rate, 8000 <= rate <= 48000 with 2 rate % 25 == 0, so a step's 80 ms are F_out = 2 rate / 25 whole samples; and a
 * sample format, DSM_PCM_F32 / DSM_PCM_S16 / DSM_PCM_MULAW / DSM_PCM_ALAW (include/dsm.h).  24000 / F32 is the pass-through
 * format and every slot's default: its row is the step's 1920 floats copied bit for bit, latency 0.
 *
 * THE SIGNAL.  x = the slot's emitted 24 kHz PCM since its format was last set (or the slot last reset); only the frames of
 * steps in which the slot emits count — a step in which it does not contributes nothing and leaves the state alone.
 * y = the whole-clip resampler on x, dsm_resample(x, 24000, rate): L / M = rate / 24000 in lowest terms, output j sits at input
 * position j M / L, i0 = floor(j M / L), phase p = j M mod L, and
 *     y[j] = (float) sum over k = 0 .. taps-1, ascending, in double, from +0.0, of (double)c[p][k] * (double)x[i0 + k - half + 1]
 * with x = 0 outside the clip — dsm_ingest_output's chain (a product of two floats is exact in double, so fma and multiply-add
 * give the same bits; a zero adds +-0.0 to an accumulator that began at +0.0 and is never -0.0: the clip function's skipped
 * tap).  A sum that is a NaN is delivered as the quiet NaN 0x7FC00000: which sign and payload an instruction set gives a NaN
 * it generates or passes on is not the same on the two sides, and one definition has to hold on both.
 * The slot's e-th emitted frame delivers z_e[n] = y[F_out e + n - D], n = 0 .. F_out - 1, 0 where the index is negative.
 * D = floor(half L / M) is the format's latency in output samples: the smallest delay for which no tap of frame e reaches past
 * the 1920 (e + 1) input samples produced so far (tests/test_egress_cpu.py finds it by brute force).  Relative to the frame,
 * with q = n - D:
 *     i0 = 1920 e + floor(q M / L),  p = q M mod L  (floor and mod towards minus infinity; F_out M / L = 1920 exactly)
 * so a step needs the `taps` samples in front of its frame — the HISTORY, zeros at the start — and the frame itself.  Taps reach
 * back at most taps - 1 samples in front of the frame and forward to the frame's last sample at most.
 * THE LAST D OUTPUT SAMPLES OF A GENERATION (at most 4.25 ms) ARE NEVER DELIVERED: they would need input behind the last frame.
 * There is no flush call.
 *
 * SAMPLE ENCODERS (integer or float code, no table): F32 the float as it is.  S16: r = rintf(v * 32768.0f) (round half to even;
 * the product is exact), NaN gives 0, clamped to [-32768, 32767], stored little endian.  mu-law from that s16 value s:
 * sign = s < 0, mag = min(|s|, 32635) + 0x84, e = floor(log2 mag) - 7 (0 .. 7), m = (mag >> (e + 3)) & 0xF,
 * byte = ~(sign << 7 | e << 4 | m) & 0xFF.  A-law from s: sign = s < 0, mag = sign ? -s - 1 : s, e = mag < 256 ? 0 :
 * floor(log2 mag) - 7, m = e == 0 ? (mag >> 4) & 0xF : (mag >> (e + 3)) & 0xF, byte = ((sign ? 0 : 0x80) | e << 4 | m) ^ 0x55.
 * Both invert the expanders of dsm_ingest.h (encode(decode(b)) == b for every byte but mu-law's negative zero 0x7F, which
 * decodes to 0 and encodes as 0xFF) and are monotone.
 *
 * THE DESCRIPTOR, twelve u32 words (dsm_egress_desc): rate, fmt, L, M, half, taps, F_out, frame_bytes, D, table_off,
 * table_words, reserved 0.  table_off: where the rate's L x taps coefficients start in the coefficient arena it is used with
 * (floats).  Every other word is a function of (rate, fmt); dsm_egress::check recomputes them and refuses what differs, and
 * checks the table against the arena's length.
 *
 * PER-SLOT STATE: `taps` history floats and a "started" word (0: no frame since the format was set or the slot reset; the
 * history then reads as zeros and the outputs with a negative index are 0).
 */
#ifndef DSM_EGRESS_H
#define DSM_EGRESS_H

#include "dsm_ingest.h"

#define DSM_EGRESS_IN_RATE 24000
#define DSM_EGRESS_MAX_TAPS 204u   /* 8 kHz: half = ceil(32 / (0.95 / 3)) = 102 */
#define DSM_EGRESS_MAX_FRAME 3840u /* 48 kHz x 80 ms */
#define DSM_EGRESS_MAX_FRAME_BYTES (4u * DSM_EGRESS_MAX_FRAME)
#define DSM_EGRESS_DESC_WORDS 12u

typedef struct dsm_egress_desc {
  uint32_t rate, fmt, L, M, half, taps, F_out, frame_bytes, D, table_off, table_words, reserved;
} dsm_egress_desc;

/* f32 -> the s16 value: round half to even, NaN 0, clamped */
DSM_HD int dsm_egress_f32_to_s16(float v) {
  if (v != v) return 0;
  const float r = __builtin_rintf(v * 32768.0f);
  if (r >= 32767.0f) return 32767;
  if (r <= -32768.0f) return -32768;
  return (int)r;
}

/* ITU-T G.711 mu-law compression of a 16-bit value (the inverse of dsm_g711_ulaw_to_s16) */
DSM_HD uint32_t dsm_egress_s16_to_ulaw(int s) {
  const uint32_t sign = s < 0 ? 1u : 0u;
  uint32_t mag = (uint32_t)(s < 0 ? -s : s);
  if (mag > 32635u) mag = 32635u;
  mag += 0x84u;                                          /* 0x84 .. 0x7FFF: bit 7 .. bit 14 leads */
  const uint32_t e = (31u - (uint32_t)__builtin_clz(mag)) - 7u;
  const uint32_t m = (mag >> (e + 3u)) & 0xFu;
  return ~(sign << 7 | e << 4 | m) & 0xFFu;
}

/* ITU-T G.711 A-law compression of a 16-bit value (the inverse of dsm_g711_alaw_to_s16) */
DSM_HD uint32_t dsm_egress_s16_to_alaw(int s) {
  const uint32_t sign = s < 0 ? 1u : 0u;
  const uint32_t mag = (uint32_t)(s < 0 ? -s - 1 : s);  /* 0 .. 32767 */
  const uint32_t e = mag < 256u ? 0u : (31u - (uint32_t)__builtin_clz(mag)) - 7u;
  const uint32_t m = e == 0u ? (mag >> 4) & 0xFu : (mag >> (e + 3u)) & 0xFu;
  return ((sign ? 0u : 0x80u) | e << 4 | m) ^ 0x55u;
}

/* sample i of a row.  Rows of the engine are 16-byte aligned; a host row may sit anywhere (both sides are little endian) */
DSM_HD void dsm_egress_store(uint32_t fmt, void* row, uint32_t i, float v) {
  uint8_t* r = (uint8_t*)row;
  if (fmt == DSM_PCM_F32) {
    const uint32_t w = dsm_f32_as_u32(v);
    __builtin_memcpy(r + 4u * i, &w, 4);
    return;
  }
  const int s = dsm_egress_f32_to_s16(v);
  if (fmt == DSM_PCM_S16) {
    const int16_t h = (int16_t)s;
    __builtin_memcpy(r + 2u * i, &h, 2);
    return;
  }
  r[i] = (uint8_t)(fmt == DSM_PCM_ALAW ? dsm_egress_s16_to_alaw(s) : dsm_egress_s16_to_ulaw(s));
}

/* output n (0 .. F_out - 1) of an emitted frame, before the sample encoder.  buf: the `taps` history samples followed by the
 * 1920 samples of the frame; coef: the rate's phase table [L][taps].  started 0: the outputs in front of the stream (n < D)
 * are 0 (the history is staged as zeros). */
DSM_HD float dsm_egress_output(const dsm_egress_desc* d, const float* coef, const float* buf, uint32_t started, int n) {
  if (d->taps == 0u) return buf[n];  /* 24 kHz out: no filter */
  const int q = n - (int)d->D;
  if (q < 0 && !started) return 0.0f;
  const int L = (int)d->L, num = q * (int)d->M;  /* |q| < 3840, M <= 960: fits */
  int i0 = num / L, p = num - i0 * L;
  if (p < 0) { p += L; i0 -= 1; }
  const float* c = coef + (size_t)p * d->taps;
  const float* x = buf + ((int)d->taps + i0 - (int)d->half + 1);  /* 1 <= index, index + taps - 1 <= taps + 1919 */
  double a = 0.0;
  for (uint32_t k = 0; k < d->taps; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
    a = DSM_FMA((double)c[k], (double)x[k], a);
#else
    a = a + (double)c[k] * (double)x[k];
#endif
  }
  if (a != a) return dsm_u32_as_f32(0x7FC00000u);
  return (float)a;
}

/* ---- host only from here: the descriptor and its checked reader, the streaming host state ---- */
#if defined(__cplusplus)

namespace dsm_egress {

/* (rate, fmt) -> every word of the descriptor but table_off (left 0).  DSM_ERR_INVALID with a message for anything else. */
inline int describe(long rate, long fmt, dsm_egress_desc* d, std::string* err) {
  using dsm_ingest::fail;
  if (fmt != DSM_PCM_F32 && fmt != DSM_PCM_S16 && fmt != DSM_PCM_MULAW && fmt != DSM_PCM_ALAW)
    return fail(err, "output format: sample format %ld (0 f32, 1 s16, 2 mu-law, 3 A-law)", fmt);
  if (rate < 8000 || rate > 48000) return fail(err, "output format: sample rate %ld Hz is outside 8000 .. 48000", rate);
  if ((2 * rate) % 25 != 0) return fail(err, "output format: %ld Hz does not give a whole number of samples per 80 ms frame", rate);
  memset(d, 0, sizeof *d);
  d->rate = (uint32_t)rate;
  d->fmt = (uint32_t)fmt;
  d->F_out = (uint32_t)(2 * rate / 25);
  d->frame_bytes = d->F_out * dsm_ingest_sample_bytes(d->fmt);
  if (rate == DSM_EGRESS_IN_RATE) {
    d->L = d->M = 1u;
    return 0;
  }
  long L = 0, M = 0;
  int half = 0;
  if (dsm_ingest::phase_table(DSM_EGRESS_IN_RATE, (int)rate, &L, &M, &half, nullptr))
    return fail(err, "output format: %ld Hz needs more than 4096 filter phases", rate);
  d->L = (uint32_t)L;
  d->M = (uint32_t)M;
  d->half = (uint32_t)half;
  d->taps = 2u * d->half;
  d->D = (uint32_t)(((long)half * L) / M);
  d->table_words = d->L * d->taps;
  if (d->taps > DSM_EGRESS_MAX_TAPS || d->F_out > DSM_EGRESS_MAX_FRAME) return fail(err, "output format: %ld Hz is outside the filter's bounds", rate);
  return 0;
}

/* Everything the step relies on, so that no descriptor — however it was made — reads outside the frame, the history or the
 * coefficient arena of `arena_words` floats, or writes outside its row: each word against what (rate, fmt) gives, the table
 * inside the arena. */
inline int check(const dsm_egress_desc* d, size_t arena_words, std::string* err) {
  using dsm_ingest::fail;
  if (!d) return fail(err, "output format descriptor: NULL");
  dsm_egress_desc want;
  if (int rc = describe((long)d->rate, (long)d->fmt, &want, err)) return rc;
  want.table_off = d->table_off;
  if (memcmp(&want, d, sizeof want) != 0) return fail(err, "output format descriptor: its words are not those of %ld Hz, format %ld", (long)d->rate, (long)d->fmt);
  if ((uint64_t)d->table_off + d->table_words > (uint64_t)arena_words)
    return fail(err, "output format descriptor: its table ends at word %ld of an arena of %ld", (long)((uint64_t)d->table_off + d->table_words), (long)arena_words);
  return 0;
}

/* One slot's streaming state on the host: descriptor, its own coefficient arena, history + frame, the started word */
struct Host {
  dsm_egress_desc d{};
  std::vector<float> coef, buf;
  uint32_t started = 0;
};

inline int host_new(long rate, long fmt, Host* h, std::string* err) {
  if (int rc = describe(rate, fmt, &h->d, err)) return rc;
  h->coef.clear();
  if (h->d.taps) {
    if (dsm_ingest::phase_table(DSM_EGRESS_IN_RATE, (int)rate, nullptr, nullptr, nullptr, &h->coef))
      return dsm_ingest::fail(err, "output format: no phase table for %ld Hz", rate);
  }
  h->buf.assign((size_t)h->d.taps + DSM_FRAME_SIZE, 0.0f);
  h->started = 0;
  return check(&h->d, h->coef.size(), err);
}

/* one emitted frame of 1920 samples at 24 kHz -> the format's frame_bytes bytes in out_row */
inline int host_step(Host* h, const float* frame1920, void* out_row, std::string* err) {
  if (!h || !frame1920 || !out_row) return dsm_ingest::fail(err, "egress: a NULL pointer");
  const dsm_egress_desc& d = h->d;
  if (int rc = check(&d, h->coef.size(), err)) return rc;
  if (h->buf.size() != (size_t)d.taps + DSM_FRAME_SIZE) return dsm_ingest::fail(err, "egress: the state does not belong to its descriptor");
  if (d.taps == 0u && d.fmt == DSM_PCM_F32) {  // pass-through: the bytes as they are
    memcpy(out_row, frame1920, sizeof(float) * DSM_FRAME_SIZE);
    h->started = 1;
    return 0;
  }
  float* buf = h->buf.data();
  if (h->started) memmove(buf, buf + DSM_FRAME_SIZE, sizeof(float) * d.taps);  // 1920 > taps: the last taps samples of the frame before
  memcpy(buf + d.taps, frame1920, sizeof(float) * DSM_FRAME_SIZE);
  for (uint32_t n = 0; n < d.F_out; ++n) dsm_egress_store(d.fmt, out_row, n, dsm_egress_output(&d, h->coef.data(), buf, h->started, (int)n));
  h->started = 1;
  return 0;
}

}  // namespace dsm_egress
#endif /* host */

#endif /* DSM_EGRESS_H */
