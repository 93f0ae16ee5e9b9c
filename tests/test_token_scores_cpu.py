"""Token scores, host side (csrc/dsm_token_scores.h behind dsm_token_scores_host): the new calls exist, the serial definition agrees
with a float64 log-softmax within the error its operation count allows, picks and ties follow the stated order, and bad
arguments are refused.  No device needed."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from token_scores_cases import NONE, VOCABS, assert_close, crafted_rows, reference, tolerance
import token_scores_cases as cases

NEW_SYMBOLS = ("dsm_asr_set_token_scores", "dsm_asr_token_scores", "dsm_asr_token_scores_dev", "dsm_asr_poll_word_scores",
               "dsm_token_scores_host", "dsm_debug_token_scores", "dsm_worker_set_word_scores")
DSM_ERR_INVALID, DSM_ERR_STATE = -1, -4


def test_the_new_symbols_exist(dsm, lib):
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"libdsm_mi355x.so does not export {s}"
        assert s in dsm.ABI_SYMBOLS
    for m in ("set_token_scores", "token_scores", "token_scores_dev", "poll_word_scores", "debug_token_scores"):
        assert callable(getattr(dsm.AsrEngine, m))
    assert callable(dsm.token_scores_host) and callable(dsm.Worker.set_word_scores)
    assert dsm.SCORES_MAX_TOP == 8


def test_exp_and_log_stay_within_the_stated_ulps(orc):
    """The tolerance of the comparison below counts dsm_expf and dsm_logf at 1 ulp each (csrc/dsm_numerics.h: "~1 ulp", "< 1 ulp").
    Measured here against float64 on dense samples of the ranges the scores use — exp on [-87, 0], log on [1, 8000] —: 0.93 and
    0.74 ulp, so the formula stands with the stated figures (cases.EXP_ULP, cases.LOG_ULP)."""
    L = orc.lib()
    for name in ("orc_expf", "orc_logf"):
        getattr(L, name).restype, getattr(L, name).argtypes = C.c_float, [C.c_float]

    def worst_ulp(fn, ref_fn, xs):
        xs = xs.astype(np.float32)
        got = np.array([fn(float(x)) for x in xs], dtype=np.float32).astype(np.float64)
        ref = ref_fn(xs.astype(np.float64))
        ok = ref != 0.0
        ulp = np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64)
        assert np.array_equal(got[~ok], ref[~ok])  # log(1) is exactly 0
        return float(np.max(np.abs(got[ok] - ref[ok]) / ulp))

    e = worst_ulp(L.orc_expf, np.exp, np.linspace(-87, 0, 30001))
    g = worst_ulp(L.orc_logf, np.log, np.concatenate([np.linspace(1, 8000, 30001), np.linspace(1, 3, 10001)]))
    print(f"dsm_expf on [-87, 0]: {e:.3f} ulp; dsm_logf on [1, 8000]: {g:.3f} ulp")
    assert e <= cases.EXP_ULP and g <= cases.LOG_ULP


@pytest.mark.parametrize("V", VOCABS)
def test_host_scores_against_float64_log_softmax(dsm, lib, V):
    """Ids exactly (value descending, ties to the ascending id, padding beyond V); logprobs within
    2 * 2^-24 * [(ceil(V/256) + 9) + 2 |ln S| + |l - m|] of the float64 log-softmax of the same f32 row."""
    rows, toks = crafted_rows(V)
    worst = 0.0
    for r in range(rows.shape[0]):
        for N in (0, 1, 8):
            lp, ids, lps = dsm.token_scores_host(rows[r], toks[r], N)
            want_lp, want_ids, want_lps, ln_s, m = reference(rows[r], int(toks[r]), N)
            assert ids.dtype == np.uint32 and ids.shape == (N,) and lps.shape == (N,)
            assert np.array_equal(ids, want_ids), (V, r, N, ids, want_ids)
            assert_close(lp, want_lp, tolerance(V, ln_s, rows[r, toks[r]] - m), (V, r, N, "token"))
            for i in range(N):
                if ids[i] == NONE:
                    assert i >= V and lps[i] == -np.inf
                    continue
                assert_close(lps[i], want_lps[i], tolerance(V, ln_s, float(rows[r, ids[i]]) - m), (V, r, N, i))
                if not math.isinf(want_lps[i]):
                    worst = max(worst, abs(float(lps[i]) - want_lps[i]) / tolerance(V, ln_s, float(rows[r, ids[i]]) - m))
            if N:  # the order itself, from the returned values: descending, equal values by ascending id
                v = rows[r, ids[ids != NONE]]
                k = ids[ids != NONE].astype(np.int64)
                assert all(v[i] > v[i + 1] or (v[i] == v[i + 1] and k[i] < k[i + 1]) for i in range(len(v) - 1))
    print(f"V = {V}: worst error / tolerance = {worst:.3f}")


def test_ties_go_to_the_lower_id_and_padding_follows_the_vocabulary(dsm, lib):
    lp, ids, lps = dsm.token_scores_host(np.array([1.0, 2.0, 2.0, -np.inf, 2.0], dtype=np.float32), 4, 8)
    assert ids.tolist() == [1, 2, 4, 0, 3, NONE, NONE, NONE]
    assert lps[0] == lps[1] == lps[2] == lp and lps[4] == -np.inf and np.all(lps[5:] == -np.inf)
    assert abs(float(lp) + math.log(3 + math.exp(-1.0))) < 1e-6
    lp, ids, lps = dsm.token_scores_host(np.array([3.5], dtype=np.float32), 0, 8)  # V = 1 < N
    assert lp == 0.0 and ids.tolist() == [0] + [NONE] * 7 and lps[0] == 0.0
    lp, ids, lps = dsm.token_scores_host(np.array([-0.0, 0.0, -0.0], dtype=np.float32), 2, 1)  # +0 == -0: the id decides
    assert ids.tolist() == [0]


@pytest.mark.parametrize("V", VOCABS)
def test_token_logprob_is_the_top_entry_bit_for_bit(dsm, lib, V):
    rows, _ = crafted_rows(V)
    for r in range(rows.shape[0]):
        _, ids, lps = dsm.token_scores_host(rows[r], 0, 8)
        for i, tok in enumerate(ids):
            if tok == NONE:
                continue
            for N in (0, 8):
                lp, ids2, lps2 = dsm.token_scores_host(rows[r], tok, N)
                assert np.float32(lp).view(np.uint32) == lps[i].view(np.uint32), (V, r, i, N)
                assert N == 0 or (np.array_equal(ids2, ids) and np.array_equal(lps2.view(np.uint32), lps.view(np.uint32)))


def test_invalid_arguments_are_refused(dsm, lib):
    row = np.zeros(4, dtype=np.float32)
    lp, ids, lps = np.zeros(1, np.float32), np.zeros(8, np.uint32), np.zeros(8, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = lib.dsm_token_scores_host
    assert f(p(row), 4, 3, 8, p(lp), p(ids), p(lps)) == 0
    assert f(p(row), 4, 0, 0, p(lp), None, None) == 0  # no top list wanted: the two pointers may be NULL
    assert f(p(row), 0, 0, 0, p(lp), None, None) == DSM_ERR_INVALID    # V < 1
    assert f(p(row), -3, 0, 0, p(lp), None, None) == DSM_ERR_INVALID
    assert f(p(row), 4, 4, 0, p(lp), None, None) == DSM_ERR_INVALID    # token >= V
    assert f(p(row), 4, 0xFFFFFFFF, 0, p(lp), None, None) == DSM_ERR_INVALID
    assert f(p(row), 4, 0, -1, p(lp), p(ids), p(lps)) == DSM_ERR_INVALID  # top_n outside 0..8
    assert f(p(row), 4, 0, 9, p(lp), p(ids), p(lps)) == DSM_ERR_INVALID
    assert f(None, 4, 0, 0, p(lp), None, None) == DSM_ERR_INVALID       # NULL where a pointer is required
    assert f(p(row), 4, 0, 0, None, None, None) == DSM_ERR_INVALID
    assert f(p(row), 4, 0, 2, p(lp), None, p(lps)) == DSM_ERR_INVALID
    assert f(p(row), 4, 0, 2, p(lp), p(ids), None) == DSM_ERR_INVALID
    with pytest.raises(dsm.DsmError):
        dsm.token_scores_host(row, 7, 0)
    for call in (lib.dsm_asr_set_token_scores, ):
        assert call(None, 0) == DSM_ERR_INVALID


def test_word_scores_need_the_engine_as_backend(dsm, lib):
    """dsm_worker_set_word_scores on a worker with a caller-supplied backend: DSM_ERR_STATE, and its messages stay as they were."""
    be = dsm.WorkerBackend()
    cbs = (dsm.BE_ENCODE(lambda s, pcm, mask: 0), dsm.BE_RESET(lambda s, slot: 0), dsm.BE_STEP(lambda s, mask, text, prs: 0),
           dsm.BE_POLL(lambda s, msgs, cap, toks, tcap: 0))
    be.batch_size, be.asr_delay_in_tokens, be.extra_heads_num = 2, 2, 0
    be.encode_step, be.reset_slot, be.step_tokens, be.poll_msgs = cbs
    w = dsm.Worker(backend=be)
    assert lib.dsm_worker_set_word_scores(w.h, 1) == DSM_ERR_STATE
    assert lib.dsm_worker_set_word_scores(w.h, 0) == DSM_ERR_STATE
    assert lib.dsm_worker_set_word_scores(None, 1) == DSM_ERR_INVALID
    with pytest.raises(dsm.DsmError) as ei:
        w.set_word_scores(True)
    assert ei.value.code == DSM_ERR_STATE and "backend" in str(ei.value)
    w.close()


def test_the_default_word_bytes_are_unchanged(dsm, lib):
    """Off is the default: a Word is the three-entry map of the reference, byte for byte."""
    import msgpack
    raw = dsm.encode_out_msg("Word", text="hi", time=1.25)
    assert msgpack.unpackb(raw) == {"type": "Word", "text": "hi", "start_time": 1.25}
    assert raw == b"\x83\xa4type\xa4Word\xa4text\xa2hi\xaastart_time\xcb" + struct.pack(">d", 1.25)
