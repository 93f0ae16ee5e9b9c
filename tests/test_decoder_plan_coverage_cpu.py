"""The GPU decode tests cover what serving runs — checked here, without a GPU.

Which kernel a decoder product gets is decided by M = B x rows per slot (plan_gemm, csrc/dsm_gemm_plan.h), not by a knob, so a
small batch cannot stand in for a served one.  This file computes, for the real Mimi, the classes of (product, plan) that the
served batches B = 32, 48 and 64 reach in either engine kind (tests/decoder_plans.py: kernel form with MT, chunk loop, split-K,
reduce kind, norm kind, 16-byte stores, the Y / Y2 / RES / BIAS / Y_PLAIN bits, N against the 64-column tile, a ragged last
m-tile), and the same for every case of tests/test_decode_serving_gpu.py::CASES.  Serving must be a subset of what the cases
reach, and no case may be redundant: the GPU file runs the smallest table that does the job, and
a later change of a gate in plan_gemm that moves a served shape to a class no case reaches fails here, on the CPU."""
import decoder_plans as D
from test_decode_serving_gpu import CASES

SERVED_BATCHES = (32, 48, 64)
ENGINE_KINDS = ((1, 1), (0, 1), (0, 0))  # (stt, dot_mode): the STT engine as benchmarked, a TTS engine in either mode (the same knobs)


def served_classes(lib, mimi):
    out = {}
    for B in SERVED_BATCHES:
        for stt, dot_mode in ENGINE_KINDS:
            for c, names in D.decoder_classes(lib, mimi, B, stt, dot_mode).items():
                out.setdefault(c, []).extend(f"{n} (B={B} stt={stt} dot_mode={dot_mode})" for n in names)
    return out


def case_classes(lib, mimi, case):
    kind, dot_mode, B = case
    return set(D.decoder_classes(lib, mimi, B, {"stt": 1, "tts": 0}[kind], dot_mode))


def describe(classes, where):
    return "\n".join(f"  {' '.join(c)}    e.g. {where[c][0]}" for c in sorted(classes))


def test_every_served_class_is_run_by_a_case(dsm, lib):
    mimi = dsm.config_stt_1b_en_fr().mimi
    served = served_classes(lib, mimi)
    assert len(D.decoder_products(mimi, 64, 1, 1)) == 21, "one decode step of the real Mimi is 21 matrix products"
    covered = set().union(*(case_classes(lib, mimi, c) for c in CASES))
    missing = set(served) - covered
    assert not missing, "served classes that no case of CASES runs:\n" + describe(missing, served)


def test_no_case_is_redundant(dsm, lib):
    """Removing any one case uncovers at least one served class (shown with the class and a served product that has it)."""
    mimi = dsm.config_stt_1b_en_fr().mimi
    served = served_classes(lib, mimi)
    assert len(set(CASES)) == len(CASES)
    for case in CASES:
        rest = set().union(*(case_classes(lib, mimi, c) for c in CASES if c != case))
        only = set(served) - rest
        print(f"only {case} runs:\n" + describe(only, served))
        assert only, f"{case} is redundant: the other cases reach every served class it does"
