"""The stand-alone GEMM kernel tests cover what serving launches, and their bounds are the reference's own — checked here,
without a GPU.

tests/gemm_cases.py says what is served (SERVED) and tests/golden/gemm_cases.json holds the cases tests/test_gemm_kernels_gpu.py
runs through dsm_debug_gemm (written by tools/find_gemm_cases.py).  This file proves: every class (gemm_classes.gemm_class) of a
served product whose epilogue the aid offers is the class of some case; what is left to the model tests is exactly the EPI_RVQ
products and the EPI_QKV products whose plan is not reduce=consumer (printed by name); no case that is not an edge case is
redundant; every case still gets the plan line it was committed with; and the ORACLE stays inside the float64 bounds of
tests/gemm_ref.py for every case and data family, so that the GPU assertion can only fail on the kernel's side."""
import time

import numpy as np
import pytest

import gemm_cases as G
import gemm_classes as GC
import gemm_ref as R

CASES = G.load_cases()


def served_classes(dsm, lib):
    """({class: [names]} of the served products the aid offers, [rows left to the model tests])."""
    offered, left = {}, []
    for r in G.served_rows(dsm):
        line = GC.plans.plan_line(lib, r)
        assert not line.startswith("error"), (r, line)
        if G.offered(r, line):
            offered.setdefault(GC.gemm_class(r, line), []).append(r["name"])
        else:
            left.append((r, line))
    return offered, left


def case_class(c):
    return GC.gemm_class(G.case_query_row(c), c["line"])


def test_cases_get_their_committed_plan(lib):
    assert len({c["id"] for c in CASES}) == len(CASES)
    wrong = [(c["id"], G.case_plan_line(lib, c), c["line"]) for c in CASES if G.case_plan_line(lib, c) != c["line"]]
    assert not wrong, wrong
    assert all(G.case_mnk(c) <= 2 * G.CASE_MNK_CAP and c["M"] * c["N"] * c["K"] <= G.CASE_MNK_CAP for c in CASES)
    assert all(len(c["knobs"]) == 5 and min(c["knobs"]) >= 0 for c in CASES), "a case names all five knobs"


def test_every_served_class_is_run_by_a_case(dsm, lib):
    served, _ = served_classes(dsm, lib)
    covered = {case_class(c) for c in CASES}
    missing = set(served) - covered
    assert not missing, "served classes that no case runs:\n" + "\n".join(f"  {' '.join(c)}    e.g. {served[c][0]}" for c in sorted(missing))


def test_what_is_left_to_the_model_tests(dsm, lib):
    """Exactly the RVQ products and the QKV products with a direct epilogue (RoPE + ring scatter)."""
    _, left = served_classes(dsm, lib)
    names = sorted({r["name"].split(" B=")[0].split(" dot_mode=")[0] + ("  [" + GC.EPI_NAMES[r["epi"]] + ", " + line.split()[0] + "]") for r, line in left})
    print("left to the model tests:\n  " + "\n  ".join(names))
    for r, line in left:
        assert r["epi"] == GC.plans.RVQ or (r["epi"] == GC.plans.QKV and GC.plan_fields(line)["reduce"] != "consumer"), (r, line)
    assert {r["epi"] for r, _ in left} == {GC.plans.RVQ, GC.plans.QKV}


def test_no_case_is_redundant(dsm, lib):
    """Removing any one case that is not an edge case uncovers a served class."""
    served, _ = served_classes(dsm, lib)
    owners = {}
    for c in CASES:
        owners.setdefault(case_class(c), []).append(c)
    for c in CASES:
        if c["edge"]:
            continue
        cls = case_class(c)
        assert cls in served, f"{c['id']} runs a class nothing served has: tag it edge or drop it"
        others = [o["id"] for o in owners[cls] if o is not c and not o["edge"]]
        assert not others, f"{c['id']} is redundant: {others} run the same class"


def test_edge_cases_are_there():
    """The edges beyond serving that the table promises (tools/find_gemm_cases.py: edge_cases)."""
    edge = [c for c in CASES if c["edge"]]
    f = {c["id"]: GC.plan_fields(c["line"]) for c in edge}
    assert any(c["N"] < 16 for c in edge) and any(16 < c["N"] < 64 for c in edge)
    for mode in (0, 1):
        gen = [c for c in edge if f[c["id"]]["form"].startswith("mfma") and c["knobs"][0] == mode and c["weight_bf16"]]
        assert any(c["K"] < 32 for c in gen) and any(c["K"] % 32 and c["K"] > 32 for c in gen) and any(c["K"] > 16 * 256 for c in gen), mode
    assert any(c["xmap"][2] % 4 for c in edge) and any(f[c["id"]]["vec"] == "0" for c in edge)
    assert any(c["y2map"] and c["y2map"][3] for c in edge) and any(c["M"] == 1 for c in edge) and any(c["M"] % 16 == 1 and c["M"] > 16 for c in edge)
    norms = {(f[c["id"]]["reduce"] if f[c["id"]]["norm"] == "fused" else f[c["id"]]["norm"], c["norm"]) for c in edge if c["norm"]}
    assert norms >= {(k, n) for k in ("rows1", "rows2", "rows4", "separate") for n in (1, 2)}, norms
    assert any(c["N"] == 4100 and f[c["id"]]["norm"] == "separate" for c in edge)
    # the separate norm of the shipped models (row_norm_kernel, N <= 4096) behind the generic kernel, a loop form and a tile reduce
    sep = [(f[c["id"]], c) for c in edge if f[c["id"]]["norm"] == "separate" and c["N"] <= 4096]
    for n in (1, 2):
        assert any(p["form"].startswith("mfma") for p, c in sep if c["norm"] == n), n
        assert any(int(p["loop"]) > 1 and c["N"] == 2048 for p, c in sep if c["norm"] == n), n
        assert any(p["reduce"] == "tiles" for p, c in sep if c["norm"] == n), n


def test_the_served_separate_norm_runs_the_served_kernel(dsm, lib):
    """Which kernel a separate norm is follows N alone (launch_gemm), so it is part of the class: every served class with a
    separate norm is row_norm_kernel's, and the case that stands for it has N <= 4096."""
    served, _ = served_classes(dsm, lib)
    sep = [cls for cls in served if "norm=separate" in cls]
    assert sep and all(cls[-1] == "row_norm" for cls in sep), sep
    for c in CASES:
        if not c["edge"] and "norm=separate" in case_class(c):
            assert c["N"] <= 4096 and case_class(c)[-1] == "row_norm", c["id"]


def test_oracle_stays_inside_the_bounds(orc):
    """Every case, every family: the bit reference against the float64 reference, under the derived bound.  Also times the bit
    reference (the GPU file computes the same) and checks that family "edges" keeps every result zero or normal."""
    orc.set_num_threads(orc.default_num_threads())
    t_ref, worst = 0.0, (0.0, None)
    for ci, c in enumerate(CASES):
        for fi, fam in enumerate(R.FAMILIES):
            inp = R.make_inputs(c, fam, 1000 * ci + fi)
            t0 = time.time()
            ref = R.reference_bits(orc, c, inp)
            t_ref += time.time() - t0
            val = R.reference_value(c, inp, ref)
            for k in ("Y", "Y2", "norm"):
                if ref[k] is None:
                    continue
                assert np.isfinite(ref[k]).all(), (c["id"], fam, k)
                v, b = val[k]
                err = np.abs(ref[k].astype(np.float64) - v)
                ok = np.isfinite(b)
                assert ok.mean() > 0.9, (c["id"], fam, k, "the bound is void on most of the output")
                ratio = float((err[ok] / np.maximum(b[ok], 1e-300)).max())
                if ratio > worst[0]:
                    worst = (ratio, (c["id"], fam, k))
                assert ratio <= 1.0, (c["id"], fam, k, ratio)
                if fam == "index" and k == "Y" and R.exact_expected(c):
                    assert np.array_equal(ref[k].astype(np.float64), v), (c["id"], "integers: the product is exact")
                if fam == "edges":
                    a = np.abs(ref[k])
                    assert not ((a > 0) & (a < 2.0 ** -126)).any(), (c["id"], k, "a subnormal result: outside what the model header covers")
    print(f"bit reference of {len(CASES)} cases x {len(R.FAMILIES)} families: {t_ref:.1f} s on {orc.default_num_threads()} threads; "
          f"largest error / bound {worst[0]:.3f} at {worst[1]}")
