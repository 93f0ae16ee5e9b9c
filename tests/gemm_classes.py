"""What a (matrix product, plan) pair exercises, as a hashable, printable tuple (a helper, not a test).

Which kernel a product gets depends on its shape, its row maps and five knobs (plan_gemm, csrc/dsm_gemm_plan.h), so what a test
at one shape covers is a CLASS of (product, plan): everything that selects a kernel instantiation, a launch shape family or an
epilogue path, and not the product's name.  plan_class is the tuple the decoder coverage test has always used
(tests/decoder_plans.py); gemm_class extends it with what the stand-alone kernel tests tell apart besides
(tests/gemm_cases.py, tests/test_gemm_case_coverage_cpu.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_gemm_plans as plans  # noqa: E402

Y, Y2, RES, BIAS, Y_PLAIN = plans.Y, plans.Y2, plans.RES, plans.BIAS, plans.Y_PLAIN
FLAG_NAMES = ((Y, "Y"), (Y2, "Y2"), (RES, "RES"), (BIAS, "BIAS"), (Y_PLAIN, "Y_PLAIN"))
EPI_NAMES = ("EPI_STORE", "EPI_QKV", "EPI_GATE", "EPI_RVQ")


def plan_fields(line):
    f = dict(kv.split("=") for kv in line.split()[1:])
    f["form"] = line.split()[0]
    return f


def n_bucket(N):
    """N relative to the 64 columns of a workgroup: one ragged 16-column tile, idle waves, whole tiles, a ragged last tile."""
    return "N<16" if N < 16 else "N<64" if N < 64 else "N%64==0" if N % 64 == 0 else "N ragged"


def m_bucket(M):
    """M against the 16-row tiles a workgroup can hold: one, two, four, more than one workgroup of four."""
    return "M<=16" if M <= 16 else "M<=32" if M <= 32 else "M<=64" if M <= 64 else "M>64"


def plan_class(row, line):
    f = plan_fields(line)
    flags = "|".join(name for bit, name in FLAG_NAMES if row["flags"] & bit)
    # a last m-tile that is partly empty: its loads clamp to row M - 1 and its epilogue drops rows >= M
    ragged = "ragged M" if row["M"] % (16 * int(f["mt"])) else "whole M"
    return (f["form"], "loop" if int(f["loop"]) > 1 else "-", "split" if int(f["chunks"]) > 1 else "-", "reduce=" + f["reduce"],
            "norm=" + f["norm"], "vec=" + f["vec"], flags, n_bucket(row["N"]), ragged)


def gemm_class(row, line):
    """plan_class and: the epilogue, the weight type, dot_mode, aligned activation rows or not, a K tail (K % 32) or not, the
    M bucket, and which kernel a separate row norm is.  That last choice is launch_gemm's, by N alone, and not in the plan line:
    row_norm_kernel (a row of at most 4096 values in registers: every shipped model) or row_norm_wide_kernel beyond."""
    norm_kernel = "-" if plan_fields(line)["norm"] != "separate" else "row_norm_wide" if row["N"] > 4096 else "row_norm"
    return plan_class(row, line) + (EPI_NAMES[row["epi"]], "bf16" if row["weight_bf16"] else "f32", "dot_mode=%d" % row["dot_mode"],
                                    "aligned" if row["flags"] & plans.ALIGNED else "unaligned",
                                    "K tail" if row["K"] % 32 else "K%32==0", m_bucket(row["M"]), norm_kernel)
