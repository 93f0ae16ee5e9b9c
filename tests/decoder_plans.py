"""The matrix products of one Mimi::decode_step and the kernel each gets, without a GPU (a helper, not a test).

The geometry is not restated here: tools/make_gemm_plans.py works the products out of a Mimi configuration the way the engine's
call sites do (mimi_products), and dsm_debug_gemm_plan answers with the plan plan_gemm (csrc/dsm_gemm_plan.h) makes for each.

Which kernel a decoder product gets depends on M = B x rows per slot, so what a test at one batch covers is a set of CLASSES of
(product, plan): everything that selects a kernel instantiation, a launch shape family or an epilogue path — and not the product's
name.  tests/test_decoder_plan_coverage_cpu.py compares the classes the served batches reach with those the GPU tests run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gemm_plans as plans  # noqa: E402

Y, Y2, RES, BIAS, Y_PLAIN = plans.Y, plans.Y2, plans.RES, plans.BIAS, plans.Y_PLAIN
FLAG_NAMES = ((Y, "Y"), (Y2, "Y2"), (RES, "RES"), (BIAS, "BIAS"), (Y_PLAIN, "Y_PLAIN"))


def decoder_products(mimi, B, stt, dot_mode):
    """Rows (name, M, N, K, flags and the other arguments of dsm_debug_gemm_plan) of the decoder's products at batch B for a Mimi
    that belongs to an STT (stt = 1) or a TTS (stt = 0) engine in the given dot_mode."""
    return [r for r in plans.mimi_products(mimi, B, stt=stt, dot_mode=dot_mode) if r["name"].startswith(plans.DEC)]


def plan_fields(line):
    f = dict(kv.split("=") for kv in line.split()[1:])
    f["form"] = line.split()[0]
    return f


def n_bucket(N):
    """N relative to the 64 columns of a workgroup: one ragged 16-column tile, idle waves, whole tiles, a ragged last tile."""
    return "N<16" if N < 16 else "N<64" if N < 64 else "N%64==0" if N % 64 == 0 else "N ragged"


def plan_class(row, line):
    """What a (product, plan) pair exercises, as a hashable, printable tuple."""
    f = plan_fields(line)
    flags = "|".join(name for bit, name in FLAG_NAMES if row["flags"] & bit)
    # a last m-tile that is partly empty: its loads clamp to row M - 1 and its epilogue drops rows >= M
    ragged = "ragged M" if row["M"] % (16 * int(f["mt"])) else "whole M"
    return (f["form"], "loop" if int(f["loop"]) > 1 else "-", "split" if int(f["chunks"]) > 1 else "-", "reduce=" + f["reduce"],
            "norm=" + f["norm"], "vec=" + f["vec"], flags, n_bucket(row["N"]), ragged)


def decoder_classes(lib, mimi, B, stt, dot_mode):
    """{class: [product names]} of one decode step."""
    out = {}
    for r in decoder_products(mimi, B, stt, dot_mode):
        line = plans.plan_line(lib, r)
        assert not line.startswith("error"), (r, line)
        out.setdefault(plan_class(r, line), []).append(r["name"])
    return out
