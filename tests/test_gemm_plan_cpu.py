"""Which kernel a matrix product gets, without a GPU: dsm_debug_gemm_plan (plan_gemm, csrc/dsm_gemm_plan.h) against
tests/golden/gemm_plans.json — one query per branch of the decision at the smallest shape that reaches it, and the products of the
shipped presets (tools/make_gemm_plans.py writes the file and says where each shape comes from).

The golden was written from plan_gemm itself.  It is a pin for later kernel work — a gate change shows up here as the shapes
that moved — and not the proof that plan_gemm decides what the four launcher functions before it decided: that proof is the
launch-for-launch comparison of kernel traces on the GPU (profiles/r08/gemm_plan_check.txt)."""
import ctypes as C
import json
import os
import re


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")))
EPI_RVQ, MAY_DEFER = 3, 1 << 10


def plan_line(lib, r):
    buf = C.create_string_buffer(512)
    n = lib.dsm_debug_gemm_plan(r["stt"], r["dot_mode"], r["weight_bf16"], r["epi"], r["nt"], r["M"], r["N"], r["K"], r["flags"], buf, len(buf))
    assert n > 0, r
    return buf.value.decode()


def fields(line):
    f = dict(kv.split("=") for kv in line.split()[1:])
    f["form"] = line.split()[0]
    f["grid"] = [int(x) for x in f["grid"].split("x")]
    return f


def test_plans_match_the_golden(lib):
    assert len(ROWS) >= 90 and len({r["name"] for r in ROWS}) == len(ROWS)
    wrong = [(r["name"], plan_line(lib, r), r["line"]) for r in ROWS if plan_line(lib, r) != r["line"]]
    assert not wrong, wrong


def test_every_branch_has_its_row():
    """The golden reaches every kernel form, every reduce outcome, both norm outcomes and the error case."""
    lines = [r["line"] for r in ROWS]
    forms = {re.sub(r"<.*", "", l.split()[0]) for l in lines if not l.startswith("error")}
    assert forms == {"mfma", "tile", "loop2", "loop4", "bx3_loop", "bx3_loop_nt2", "bx3_split", "bx3u", "wk"}
    assert {"bx3u<1>", "bx3u<2>"} <= {l.split()[0] for l in lines}
    assert {fields(l)["reduce"] for l in lines if not l.startswith("error")} == {"none", "consumer", "rows1", "rows2", "rows4", "tiles"}
    assert {fields(l)["norm"] for l in lines if not l.startswith("error")} == {"none", "fused", "separate"}
    assert any(l.startswith("error: chunk partials do not fit in LDS") for l in lines)


def test_plan_invariants(lib):
    for r in ROWS:
        line = plan_line(lib, r)
        if line.startswith("error"):
            continue
        f = fields(line)
        chunks, loop, mt, mtiles = int(f["chunks"]), int(f["loop"]), int(f["mt"]), (r["M"] + 15) // 16
        # slabs are left only by a product that is split-K across workgroups, and only to a caller that asked for them
        if f["reduce"] == "consumer":
            assert chunks > 1 and loop == 0 and r["flags"] & MAY_DEFER, (r, line)
        assert (f["reduce"] == "none") == (chunks == 1), (r, line)
        # the workspace holds chunks x M padded to 16 x ws_ntiles * 16 floats; one chunk per workgroup column leaves no slabs
        assert int(f["ws"]) == (chunks * mtiles * int(f["ws_ntiles"]) * 1024 if chunks > 1 else 0), (r, line)
        # the m-tile axis covers every row: grid.z of the tiled kernels, grid.y of the generic one
        m_axis = f["grid"][1] if f["form"].startswith("mfma") else f["grid"][2]
        assert m_axis * 16 * mt >= r["M"], (r, line)
        if r["epi"] == EPI_RVQ:
            assert "bx3" not in f["form"] and f["form"] != "wk", (r, line)


def test_bad_queries_are_refused(lib):
    buf = C.create_string_buffer(64)
    assert lib.dsm_debug_gemm_plan(1, 1, 1, 4, 1, 16, 64, 64, 0, buf, len(buf)) < 0   # no such epilogue
    assert lib.dsm_debug_gemm_plan(1, 1, 1, 0, 3, 16, 64, 64, 0, buf, len(buf)) < 0   # n-tiles per wave: 1 or 2
    assert lib.dsm_debug_gemm_plan(1, 1, 1, 0, 1, 0, 64, 64, 0, buf, len(buf)) < 0    # no rows
    assert lib.dsm_debug_gemm_plan(1, 1, 1, 0, 1, 16, 64, 64, 0, None, 0) < 0
