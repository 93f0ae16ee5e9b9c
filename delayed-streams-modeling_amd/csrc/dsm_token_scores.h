/*
 * dsm_token_scores.h — log-probability of the chosen text token and the N best alternatives of one logits row, defined once
 * for the HIP kernel (lm_token_scores_kernel, dsm_kernels.h) and the host (dsm_token_scores_host): same source, both
 * compilers, the same bits.  This project's own output: the reference returns the argmax and drops the row (core/asr.rs:208-215).
 *
 * For a row l[0..V), V >= 1, a chosen token tok < V and 0 <= N <= 8:
 *   order    value descending, then id ascending (dsm_score_before).  NaN loses every comparison, so a NaN entry is never
 *            listed and never the maximum; the scores of a row that holds one are unspecified.
 *   m        the value of the FIRST entry of that order (the maximum; among +0.0 and -0.0 the one with the lower id, so that
 *            m has one bit pattern whatever the scan order).
 *   p_t      lane t of 256: sum of dsm_expf(l[j] - m) over j = t, t + 256, ... ascending, from 0.0f, plain f32 adds;
 *            a lane without an element holds 0.0f.
 *   S        the tree sum of the lanes: for off = 128, 64, ..., 1: p_t = p_t + p_{t+off} for t < off  (dsm_score_tree_sum).
 *   logprob  (l[j] - m) - dsm_logf(S): two f32 operations in that order (dsm_score_logprob).
 *   top-N    the N first entries of the order, each an id and its logprob; entries i >= V (or beyond the last non-NaN
 *            entry) are id DSM_SCORES_NONE and logprob -inf.
 * Always softmax temperature 1 over the raw logits, also when the token itself was drawn with Gumbel noise.
 */
#ifndef DSM_TOKEN_SCORES_H
#define DSM_TOKEN_SCORES_H

#include <stdint.h>
#include "dsm_numerics.h"

#define DSM_SCORES_LANES 256
#ifndef DSM_SCORES_MAX_TOP
#define DSM_SCORES_MAX_TOP 8 /* include/dsm.h: the most alternatives a step can list, and the row stride of the top buffers */
#endif
#define DSM_SCORES_NONE 0xFFFFFFFFu

/* (av, ai) comes before (bv, bi) in the order */
DSM_HD int dsm_score_before(float av, uint32_t ai, float bv, uint32_t bi) { return av > bv || (av == bv && ai < bi); }

/* entry j is a candidate of the round after the pick (pv, pi): strictly behind it in the order */
DSM_HD int dsm_score_behind(float v, uint32_t j, float pv, uint32_t pi) { return v < pv || (v == pv && j > pi); }

DSM_HD float dsm_score_logprob(float l, float m, float log_s) {
  const float d = l - m;
  return d - log_s;
}

/* p[DSM_SCORES_LANES] -> S, in place */
DSM_HD float dsm_score_tree_sum(float* p) {
  for (int off = DSM_SCORES_LANES / 2; off >= 1; off >>= 1)
    for (int t = 0; t < off; ++t) p[t] = p[t] + p[t + off];
  return p[0];
}

/* The first entry of the order (has_prev = 0) or the first one behind (pv, pi); DSM_SCORES_NONE when there is none. */
DSM_HD uint32_t dsm_score_next(const float* l, int V, int has_prev, float pv, uint32_t pi) {
  float bv = -DSM_INF_F;
  uint32_t bi = DSM_SCORES_NONE;
  for (int j = 0; j < V; ++j) {
    const float v = l[j];
    if (has_prev && !dsm_score_behind(v, (uint32_t)j, pv, pi)) continue;
    if (dsm_score_before(v, (uint32_t)j, bv, bi)) { bv = v; bi = (uint32_t)j; }
  }
  return bi;
}

/* The whole definition, serially.  top_ids / top_lps: top_n entries each (may be null when top_n == 0). */
DSM_HD void dsm_token_scores_row(const float* l, int V, uint32_t tok, int top_n, float* logprob, uint32_t* top_ids, float* top_lps) {
  uint32_t ids[DSM_SCORES_MAX_TOP];
  const int rounds = top_n > 0 ? top_n : 1;  /* round 0 finds m */
  for (int r = 0; r < rounds; ++r) {
    const uint32_t prev = r > 0 ? ids[r - 1] : DSM_SCORES_NONE;
    ids[r] = (r > 0 && prev == DSM_SCORES_NONE) ? DSM_SCORES_NONE : dsm_score_next(l, V, r > 0, r > 0 ? l[prev] : 0.0f, prev);
  }
  const float m = ids[0] == DSM_SCORES_NONE ? -DSM_INF_F : l[ids[0]];
  float p[DSM_SCORES_LANES];
  for (int t = 0; t < DSM_SCORES_LANES; ++t) p[t] = 0.0f;
  for (int j = 0; j < V; ++j) p[j % DSM_SCORES_LANES] = p[j % DSM_SCORES_LANES] + dsm_expf(l[j] - m);
  const float log_s = dsm_logf(dsm_score_tree_sum(p));
  *logprob = dsm_score_logprob(l[tok], m, log_s);
  for (int i = 0; i < top_n; ++i) {
    top_ids[i] = ids[i];
    top_lps[i] = ids[i] == DSM_SCORES_NONE ? -DSM_INF_F : dsm_score_logprob(l[ids[i]], m, log_s);
  }
}

#endif /* DSM_TOKEN_SCORES_H */
