"""Shared by test_token_scores_cpu.py and test_token_scores_gpu.py: the crafted logits rows, the float64 reference of the
scores, the tolerance of the issue's error count, and a Python restatement of the engine's word assembly."""
import math

import numpy as np

VOCABS = (1, 5, 64, 255, 256, 257, 1000, 8000)  # lanes of the 256-lane sum empty, exactly full, uneven; the served vocabulary
NONE = 0xFFFFFFFF
EXP_ULP, LOG_ULP = 1.0, 1.0  # what csrc/dsm_numerics.h states; test_exp_and_log_stay_within_the_stated_ulps measures them


def crafted_rows(V):
    """Five f32 rows of V logits and a token each: a dominant entry over a +-20 spread, -inf entries, heavy ties, a constant row
    (every pick decided by the id), and a gaussian row with +0.0 / -0.0 at the maximum."""
    rng = np.random.default_rng(1000 + V)
    rows = np.zeros((5, V), dtype=np.float32)
    rows[0] = rng.uniform(-20, 20, V)
    rows[0, rng.integers(V)] = 24.0
    rows[1] = 3 * rng.standard_normal(V)
    rows[1, rng.random(V) < 0.4] = -np.inf
    rows[1, rng.integers(V)] = 1.5  # never a row of -inf alone
    rows[2] = rng.integers(-2, 3, V)
    rows[3] = -7.25
    rows[4] = -np.abs(5 * rng.standard_normal(V))
    rows[4, 0] = -0.0
    rows[4, V - 1] = 0.0
    toks = np.array([int(np.argmax(rows[0])), int(rng.integers(V)), int(rng.integers(V)), V - 1, V // 2], dtype=np.uint32)
    return rows, toks


def reference(row, tok, top_n):
    """float64 log-softmax of the f32 row: (logprob of tok, ids [top_n], logprobs [top_n], ln S, m) with the order
    value descending, id ascending; entries beyond V are (NONE, -inf)."""
    l = row.astype(np.float64)
    m = l.max()
    with np.errstate(divide="ignore"):
        S = np.exp(l - m).sum()
        lp = (l - m) - math.log(S)
    order = np.lexsort((np.arange(l.size), -l))[:top_n]  # -0.0 == 0.0: the id decides, as in the definition
    ids = np.full(top_n, NONE, dtype=np.uint32)
    ids[:order.size] = order
    lps = np.full(top_n, -np.inf)
    lps[:order.size] = lp[order]
    return lp[tok], ids, lps, math.log(S), m


def tolerance(V, ln_s, l_minus_m):
    """2 * 2^-24 * [(ceil(V/256) + 8 + exp ulps) + (1 + log ulps) |ln S| + |l - m|]: ceil(V/256) sequential adds and 8 tree levels
    at one rounding each, dsm_expf per term, dsm_logf and the final subtraction on |ln S|, the rounding of l - m; the factor 2 in
    front is the margin.  With both functions at the stated 1 ulp this is 2 * 2^-24 * [(ceil(V/256) + 9) + 2 |ln S| + |l - m|]."""
    return 2 * 2.0 ** -24 * ((math.ceil(V / 256) + 8 + EXP_ULP) + (1 + LOG_ULP) * abs(ln_s) + abs(l_minus_m))


def assert_close(got, want, tol, what):
    if math.isinf(want):
        assert got == want, (what, got, want)
    else:
        assert abs(float(got) - want) <= tol, (what, float(got), want, abs(float(got) - want), tol)


class WordAssembly:
    """assemble_words of the engine (core/asr.rs:218-252) for one slot, with a score beside every token."""

    def __init__(self, delay):
        self.delay, self.step_idx, self.tokens, self.scores = delay, 0, [], []

    def reset(self):
        self.step_idx, self.tokens, self.scores = 0, [], []

    def step(self, token, score):
        """-> the (tokens, scores) of the Word this step closes, or None"""
        self.step_idx += 1
        if self.step_idx < self.delay:
            return None
        if token in (0, 3):
            if self.tokens:
                out = (self.tokens, self.scores)
                self.tokens, self.scores = [], []
                return out
            return None
        self.tokens.append(int(token))
        self.scores.append(np.float32(score))
        return None
