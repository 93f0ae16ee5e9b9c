"""Every GEMM plan class run alone: one product through dsm_debug_gemm (launch_gemm itself, on a live engine) against the oracle's
bits and a float64 bound, with guards around every output.

The cases are tests/golden/gemm_cases.json (tools/find_gemm_cases.py; tests/test_gemm_case_coverage_cpu.py proves on the CPU that
they reach every served class the aid offers, and that the oracle itself stays inside the bounds).  Each case runs five data
families on fixed seeds (tests/gemm_ref.py: plain, index-revealing integers, wide range, cancellation, edges of the contract) and
asserts, per family: the plan line that ran is the committed one; the bits of Y / Y2 / the norm equal the oracle's on every
element with m < M, n < N; they lie inside the float64 bound (integers: equal the float64 product exactly); every element
outside m < M, n < N of the whole buffers — ld > N where the map allows, the rows up to the next multiple of 64 and 64 more —
still holds its guard; X, W and res are unchanged; a second run gives the same bits (split-K order)."""
import time

import numpy as np
import pytest

import gemm_cases as G
import gemm_ref as R

pytestmark = pytest.mark.gpu
CASES = G.load_cases()


@pytest.fixture(scope="module")
def eng(gpu, lib, dsm, tiny_weights):
    e = dsm.AsrEngine(dsm.config_tiny(), 2, *tiny_weights)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(eng, c, inp, bufs):
    return eng.debug_gemm(c["M"], c["N"], c["K"], inp["X"], c["xmap"], inp["W"], c["weight_bf16"], epi=c["epi"], bias=inp["bias"],
                          scale=inp["scale"], act=c["act"], res=inp["res"], rmap=c["rmap"], Y=bufs["Y"], ymap=c["ymap"], Y2=bufs["Y2"],
                          y2map=c["y2map"], norm_w=inp["norm_w"], norm_b=inp["norm_b"], norm_out=bufs["norm_out"], may_defer=c["may_defer"],
                          knobs=c["knobs"])


def case_buffers(c):
    M, N = c["M"], c["N"]
    return dict(Y=R.out_buffer(c["ymap"], M, N) if c["ymap"] else None, Y2=R.out_buffer(c["y2map"], M, N) if c["y2map"] else None,
                norm_out=R.guard_fill(((M + 63) // 64 * 64 + 64) * N) if c["norm"] else None)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["id"] for c in CASES])
def test_case(eng, orc, ci):
    c = CASES[ci]
    M, N = c["M"], c["N"]
    orc.set_num_threads(orc.default_num_threads())  # a tiny-model oracle of an earlier test leaves the team at four threads
    t_start = time.time()
    failures = []  # every family runs, so that a failure says which data found it

    def check(ok, *what):
        if not ok:
            failures.append(what)

    for fi, fam in enumerate(R.FAMILIES):
        inp = R.make_inputs(c, fam, 1000 * ci + fi)
        ref = R.reference_bits(orc, c, inp)
        val = R.reference_value(c, inp, ref)
        bufs = case_buffers(c)
        out = run(eng, c, inp, bufs)
        assert out["plan"] == c["line"], (fam, out["plan"])
        again = run(eng, c, inp, bufs)
        # nothing the call only reads has changed
        check(np.array_equal(bits(out["x_back"]), bits(inp["X"])), fam, "X changed")
        check(inp["res"] is None or np.array_equal(bits(out["res_back"]), bits(inp["res"])), fam, "res changed")
        check(not out["w_changed"], fam, "W changed")
        for key, rkey, rmap in (("Y", "Y", c["ymap"]), ("Y2", "Y2", c["y2map"]), ("norm_out", "norm", (0, M, N, 0) if c["norm"] else None)):
            if rmap is None:
                continue
            got_buf, want = out[key], ref[rkey]
            inside = R.inside_mask(got_buf.size, rmap, M, N)
            touched = np.flatnonzero(~inside & (bits(got_buf) != bits(bufs[key])))
            check(touched.size == 0, fam, key, "guard overwritten at", touched[:8].tolist(), "ld", rmap[2])
            got = R.gather(got_buf, rmap, M, N)
            wrong = np.argwhere(bits(got) != bits(want))
            v, b = val[rkey]
            err = np.abs(got.astype(np.float64) - v)
            ok = np.isfinite(b)  # false where the bound says nothing (an ill-conditioned LayerNorm row): counted, printed, limited
            void = 1.0 - float(ok.mean())
            check(void <= 0.1, fam, key, "the float64 bound is void on this fraction of the output", void)
            ratio = float((err[ok] / np.maximum(b[ok], 1e-300)).max()) if ok.any() else float("inf")
            print(f"{c['id']} {fam} {key}: {wrong.shape[0]} of {got.size} elements differ from the oracle, error / bound {ratio:.3f}, "
                  f"bound void on {void:.4f} of the elements")
            check(wrong.shape[0] == 0, fam, key, "bits: first (m, n) that differ from the oracle", wrong[:4].tolist())
            check(ratio <= 1.0, fam, key, "error / float64 bound", ratio)
            if fam == "index" and key == "Y" and R.exact_expected(c):
                check(np.array_equal(got.astype(np.float64), v), fam, key, "integers: not the exact float64 product")
            check(np.array_equal(bits(again[key]), bits(got_buf)), fam, key, "a second run gave other bits")
    print(f"{c['id']}: {time.time() - t_start:.2f} s")
    assert not failures, failures


def test_epilogues_left_to_the_model_tests_are_refused(eng, dsm):
    x, w, y = np.ones(16 * 64, np.float32), np.ones(64 * 64, np.float32), np.zeros(16 * 64, np.float32)
    for kw in (dict(epi=dsm.EPI_RVQ), dict(epi=dsm.EPI_QKV), dict(epi=dsm.EPI_QKV, may_defer=True)):  # K = 64: one chunk, nothing to defer
        with pytest.raises(dsm.DsmError, match="not offered"):
            eng.debug_gemm(16, 64, 64, x, (0, 16, 64, 0), w, True, Y=y, ymap=(0, 16, 64, 0), **kw)
    with pytest.raises(dsm.DsmError, match="outside"):
        eng.debug_gemm(17, 64, 64, x, (0, 17, 64, 0), w, True, Y=np.zeros(17 * 64, np.float32), ymap=(0, 17, 64, 0))


def test_engine_steps_as_before_after_aid_calls(eng, dsm, orc, tiny_weights):
    """Fifty aid calls in both modes and with lowered knobs (the split-K workspace grows, the knobs are set and restored): the
    engine's next step_pcm still equals the oracle's."""
    from dsm_amd import synth
    cfg = dsm.config_tiny()
    ora = orc.OracleAsr(cfg, 2, *tiny_weights)
    pcm, mask = synth.synth_pcm(2, 4), np.array([1, 1], dtype=np.uint8)

    def step(s):
        ec, et, ep = eng.step_pcm(pcm[s], mask)
        oc, ot, op = ora.step_pcm(pcm[s], mask)
        assert np.array_equal(ec, oc) and np.array_equal(et, ot) and np.array_equal(bits(ep), bits(op)), s

    step(0)
    step(1)
    small = [c for c in CASES if G.case_mnk(c) < 4_000_000][:10]
    for i in range(50):
        c = small[i % len(small)]
        out = run(eng, c, R.make_inputs(c, "plain", i), case_buffers(c))
        assert out["plan"] == c["line"]
    step(2)
    step(3)
    ora.close()
