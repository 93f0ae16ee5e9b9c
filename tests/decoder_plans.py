"""The matrix products of one Mimi::decode_step and the kernel each gets, without a GPU (a helper, not a test).

The geometry is not restated here: tools/make_gemm_plans.py works the products out of a Mimi configuration the way the engine's
call sites do (mimi_products), and dsm_debug_gemm_plan answers with the plan plan_gemm (csrc/dsm_gemm_plan.h) makes for each.

Which kernel a decoder product gets depends on M = B x rows per slot, so what a test at one batch covers is a set of CLASSES of
(product, plan): everything that selects a kernel instantiation, a launch shape family or an epilogue path — and not the product's
name (plan_class, tests/gemm_classes.py).  tests/test_decoder_plan_coverage_cpu.py compares the classes the served batches reach
with those the GPU tests run."""
from gemm_classes import FLAG_NAMES, Y, Y2, RES, BIAS, Y_PLAIN, n_bucket, plan_class, plan_fields, plans  # noqa: F401


def decoder_products(mimi, B, stt, dot_mode):
    """Rows (name, M, N, K, flags and the other arguments of dsm_debug_gemm_plan) of the decoder's products at batch B for a Mimi
    that belongs to an STT (stt = 1) or a TTS (stt = 0) engine in the given dot_mode."""
    return [r for r in plans.mimi_products(mimi, B, stt=stt, dot_mode=dot_mode) if r["name"].startswith(plans.DEC)]


def decoder_classes(lib, mimi, B, stt, dot_mode):
    """{class: [product names]} of one decode step."""
    out = {}
    for r in decoder_products(mimi, B, stt, dot_mode):
        line = plans.plan_line(lib, r)
        assert not line.startswith("error"), (r, line)
        out.setdefault(plan_class(r, line), []).append(r["name"])
    return out
