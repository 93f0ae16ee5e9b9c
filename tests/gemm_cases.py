"""The stand-alone GEMM kernel tests' table (a helper, not a test): what serving launches, and one small product per class of it.

SERVED says which engines at which batches count as served; served_rows() works their matrix products out of the presets the way
the engines' call sites do (tools/make_gemm_plans.py).  The cases (tests/golden/gemm_cases.json, written by
tools/find_gemm_cases.py, read by load_cases) hold, for every class (gemm_classes.gemm_class) of a served product that
dsm_debug_gemm can run, the product of least M N K that reaches the class under explicit knobs, with the plan line it must get;
and the edge cases beyond serving, tagged "edge".
tests/test_gemm_case_coverage_cpu.py proves the table against SERVED without a GPU; tests/test_gemm_kernels_gpu.py runs it."""
import gemm_classes as GC

plans = GC.plans

# What counts as served: (preset, engine batches).  Every entry runs in both dot modes.  Rows per launch follow the engines' own
# group rules (plans.stt_group_rows: two stream groups of whole 16-row blocks from B = 32 on; plans.tts_group_rows: one group below
# 96 slots), the TTS engine with two batch rows per slot (cfg_rows: the guided configuration, the larger M of the two).  The Mimi
# encoder runs at the batches of tests/test_decoder_plan_coverage_cpu.py, in an engine of either kind.
SERVED = (
    ("stt-1b-en_fr", (1, 32, 48, 64, 128, 1024)),
    ("stt-2.6b-en", (1, 32, 48, 64, 128, 1024)),
    ("tts_v202501", (1, 32, 48, 64, 384)),
    ("mimi encoder", (32, 48, 64)),
)
TTS_ROWS_PER_SLOT = 2
MIMI_ENGINE_KINDS = ((1, 1), (1, 0), (0, 1), (0, 0))  # (stt, dot_mode)
CASE_MNK_CAP = 608 * 1000 * 1000  # M N K of a case: the two-n-tile loop form needs 256 workgroups of 128 columns x 64 rows over two K-chunks (K = 288).
# Measured: the bit reference of all 258 cases x five families takes 24.8 s on 16 CPU threads (the host of an MI355X; the bx3
# integer path does about 0.5 G products a second on 8 threads of a slower host: 117 s there); the whole GPU file, references
# included, takes 59 s, the slowest case 2.0 s.


def explicit_knobs(knobs, stt=True):
    """(dot_mode, chunk_loop_min_tiles, smallk_min_tiles, smallk_mt, loop_depth) with every -1 replaced by what an engine of the
    kind starts from (gemm_default_knobs, csrc/dsm_gemm_plan.h): a case names all five, so an engine's environment cannot move it."""
    dflt = (0, 192 if stt and knobs[0] == 1 else 384, 1024, 4, 4)
    return [d if k < 0 else k for k, d in zip(knobs, dflt)]


def _ok4(m):
    return m is None or (m[0] % 4 == 0 and m[2] % 4 == 0)  # an absent map is all zero (base_args)


def case_flags(c):
    """The DSM_GEMMQ_* bits launch_gemm derives from a case's arguments (gemm_query, csrc/dsm_engine.hip)."""
    f = plans.ALIGNED if (c["xmap"][0] % 4 == 0 and c["xmap"][2] % 4 == 0) else 0
    f |= (plans.Y if c["ymap"] else 0) | (plans.Y2 if c["y2map"] else 0) | (plans.RES if c["rmap"] else 0)
    f |= (plans.BIAS if c["bias"] else 0) | (plans.NORM if c["norm"] else 0) | (plans.MAY_DEFER if c["may_defer"] else 0)
    f |= (plans.Y_OK4 if _ok4(c["ymap"]) else 0) | (plans.Y2_OK4 if _ok4(c["y2map"]) else 0) | (plans.RES_OK4 if _ok4(c["rmap"]) else 0)
    return f | (plans.Y_PLAIN if (c["ymap"] is None or c["ymap"][0] == 0) else 0)


def case_query_row(c):
    """A case as a row of plans.add: what gemm_classes.gemm_class and dsm_debug_gemm_plan_knobs take."""
    return dict(name=c["id"], stt=1, dot_mode=c["knobs"][0], weight_bf16=c["weight_bf16"], epi=c["epi"], nt=2 if c["epi"] == plans.GATE else 1,
                M=c["M"], N=c["N"], K=c["K"], flags=case_flags(c))


def case_plan_line(lib, c):
    return plans.plan_line_knobs(lib, case_query_row(c), c["knobs"])


def case_mnk(c):
    return c["M"] * c["N"] * c["K"] * (2 if c["epi"] == plans.GATE else 1)


def load_cases():
    import json
    import os
    with open(os.path.join(GC.ROOT, "tests", "golden", "gemm_cases.json")) as f:
        return json.load(f)


def offered(row, line):
    """dsm_debug_gemm runs the store and gate epilogues, and the QKV one only where the plan leaves the slabs to the consumer."""
    if row["epi"] == plans.RVQ:
        return False
    return row["epi"] != plans.QKV or GC.plan_fields(line)["reduce"] == "consumer"


def served_rows(dsm):
    """Every product of SERVED as a row of plans.add (name, stt, dot_mode, weight_bf16, epi, nt, M, N, K, flags)."""
    rows = []
    for preset, batches in SERVED:
        for B in batches:
            for dot_mode in (0, 1):
                if preset.startswith("stt"):
                    cfg = dsm.config_stt_1b_en_fr() if preset == "stt-1b-en_fr" else dsm.config_stt_2_6b_en()
                    for M in sorted(set(plans.stt_group_rows(B))):
                        plans.stt_lm_products(rows, f"{preset} B={B} dot_mode={dot_mode} group of {M}", cfg, M, dot_mode)
                elif preset.startswith("tts"):
                    for M in sorted(set(plans.tts_group_rows(B, TTS_ROWS_PER_SLOT))):
                        plans.tts_lm_products(rows, f"{preset} B={B} dot_mode={dot_mode} group of {M} rows", dsm.config_tts_v202501(), M, dot_mode)
            if preset == "mimi encoder":
                for stt, dot_mode in MIMI_ENGINE_KINDS:
                    for r in plans.mimi_products(dsm.config_stt_1b_en_fr().mimi, B, stt=stt, dot_mode=dot_mode):
                        if not r["name"].startswith(plans.DEC):
                            rows.append(dict(r, name=f"{r['name']} B={B} stt={stt} dot_mode={dot_mode}"))
    return rows
