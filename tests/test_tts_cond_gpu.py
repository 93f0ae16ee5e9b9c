"""GPU tests of the TTS conditioners (core/conditioner.rs; dsm_tts_attach_conditioners / dsm_tts_set_condition_*): the slot's row
against tests/tts_cond_ref.py, the input sum tts_input_kernel writes with and without it, the oracle — which knows no
conditions — on the unconditioned slots of a mixed batch, graph replay, the request path and the refused calls."""
import ctypes as C
import os

import numpy as np
import pytest

import tts_cond_ref as CR
import tts_request_ref as Q
from tts_schedule import schedule

pytestmark = pytest.mark.gpu
WDIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
DSM_ERR_INVALID, DSM_ERR_IO, DSM_ERR_STATE = -1, -2, -4
B = 4
DESC, TAIL, SPEED = CR.CONDS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _setup(dsm, **kw):
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny(**kw)
    tag = "tts_tiny_ca" if kw.get("cross_attention") else "tts_tiny"
    path = synth.make_synth_tts_weights(cfg, WDIR, tag=tag, conditioners=CR.CONDS)
    return dict(cfg=cfg, path=path, t=CR.cond_tensors(path), tables=CR.emb_tables(path, cfg))


@pytest.fixture(scope="module")
def fx(dsm, lib):
    """Weights, conditioner tensors and embedding tables, read once and left unchanged."""
    return _setup(dsm)


@pytest.fixture(scope="module")
def fx_cfg(dsm, lib):
    return _setup(dsm, cross_attention=True, cfg_rows=True)


def _engine(dsm, f, nb=B, attach=True):
    eng = dsm.TtsEngine(f["cfg"], nb, f["path"])
    if attach:
        eng.attach_conditioners(CR.CONDS, f["path"])
    return eng


def cond_rows(eng):
    d = eng.cfg.lm.d_model
    return eng.debug_read("cond.row", eng.B * d).reshape(eng.B, d)


def step_checked(eng, f, prev, allowed, mask, conditioned, guided=()):
    """One step, then the input identity on every active slot: lm.input of a row == f32(plain sum + the slot's condition row)
    for a conditioned slot, the plain sum otherwise; both rows of a guided slot.  The plain sum is restated in numpy from the
    checkpoint's tables and the slot's OWN token history (a conditioned slot soon generates other tokens than its plain twin).
    Returns (text, audio, lm.input [B][rps][d])."""
    cfg = f["cfg"]
    rps, d = (2 if cfg.cfg_rows else 1), cfg.lm.d_model
    before = [eng.step_idx(b) for b in range(eng.B)]
    text, audio = eng.step(prev, allowed, mask)
    inp = eng.debug_read("lm.input", eng.B * rps * d).reshape(eng.B, rps, d)
    rows = cond_rows(eng)
    for b in range(eng.B):
        if not mask[b]:
            continue
        want = CR.plain_input_row(cfg, f["tables"], prev[b], before[b], lambda i: eng.audio_tokens(b, i))
        if b in conditioned:
            assert np.any(rows[b] != 0)
            want = (want + rows[b]).astype(np.float32)
        else:
            assert not np.any(bits(rows[b])), f"slot {b} has no condition: its row must read zeros"
        for j in range(rps if b in guided else 1):
            assert np.array_equal(bits(inp[b, j]), bits(want)), f"lm.input of slot {b} row {j} at step index {before[b]}"
    return text, audio, inp


def test_lut_rows_and_learnt_padding_are_the_reference_bits(gpu, dsm, fx):
    """dim 16 / n_bins 31 and dim 5 / n_bins 4, first and last possible value: "cond.row" equals the numpy chain bit for bit;
    learnt_padding is the tensor; a later set replaces the row, clearing zeroes it."""
    eng, t = _engine(dsm, fx), fx["t"]
    for slot, (c, value) in enumerate([(DESC, "very_bad"), (DESC, "very_good"), (TAIL, "a"), (TAIL, "e")]):
        eng.set_condition(slot, c["name"], value)
        got, want = cond_rows(eng)[slot], CR.lut_row(t, c, value)
        assert np.any(want != 0) and np.array_equal(bits(got), bits(want)), (c["name"], value, np.abs(got - want).max())
    for slot, c in enumerate(CR.CONDS):
        eng.set_condition_padding(slot, c["name"])
        assert np.array_equal(bits(cond_rows(eng)[slot]), bits(CR.padding_row(t, c))), c["name"]
    assert np.array_equal(bits(cond_rows(eng)[3]), bits(CR.lut_row(t, TAIL, "e")))  # the other slots' rows are left alone
    eng.clear_condition(3)
    eng.reset_batch_idx(0)
    rows = cond_rows(eng)
    assert not np.any(bits(rows[3])) and not np.any(bits(rows[0])) and np.any(rows[1] != 0)
    eng.close()


def test_continuous_rows_are_within_the_bound_of_their_inputs(gpu, dsm, fx):
    """dim 8: against a float64 evaluation, per element sum |W| |e| 2^-8 (a bf16 ulp on every input) + dim 2^-24 sum |W e|
    (the f32 chain), computed from the weights."""
    eng, t = _engine(dsm, fx), fx["t"]
    values = [0.0, 0.25, -1.5, 3.0]
    for slot, value in enumerate(values):
        eng.set_condition(slot, "speed", value)
    rows = cond_rows(eng)
    for slot, value in enumerate(values):
        want, bound = CR.cont_row_f64(t, SPEED, value)
        err = np.abs(rows[slot].astype(np.float64) - want)
        print(f"speed = {value}: max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}, "
              f"differs from the host recipe in {int(np.sum(bits(rows[slot]) != bits(CR.cont_row_chain(t, SPEED, value))))} elements")
        assert np.all(np.isfinite(rows[slot])) and np.all(err <= bound), (value, err.max(), bound.min())
    eng.close()


@pytest.mark.parametrize("cfg_rows", [False, True])
def test_the_input_sum_gains_the_row_and_nothing_else_changes(gpu, dsm, fx, fx_cfg, cfg_rows):
    """Two engines over one schedule, conditions on slots 1 and 3 of one of them.  With cfg_rows slot 1 is guided (both its rows
    get the row) and slot 0 is guided without a condition."""
    from dsm_amd import synth
    f = fx_cfg if cfg_rows else fx
    cfg = f["cfg"]
    plain, eng = _engine(dsm, f, attach=False), _engine(dsm, f)
    guided = ()
    if cfg_rows:
        guided = (0, 1)
        for x in (plain, eng):
            x.set_ca_src(0, synth.synth_ca_src(cfg, 9, 3), synth.synth_ca_src(cfg, 9, 99), 1.5)
            x.set_ca_src(1, synth.synth_ca_src(cfg, 20, 1), synth.synth_ca_src(cfg, 9, 99), 2.5)
            x.set_ca_src(3, synth.synth_ca_src(cfg, 8, 2))
    eng.set_condition(1, "description", "good")
    eng.set_condition(3, "speed", -0.5)
    rows = cond_rows(eng)
    tad = cfg.text_audio_delay_in_tokens
    for s, (prev, allowed, mask) in enumerate(schedule(cfg, B, 12)):
        before = [eng.step_idx(b) for b in range(B)]
        tp, ap, ip = step_checked(plain, f, prev, allowed, mask, conditioned=(), guided=guided)
        te, ae, ie = step_checked(eng, f, prev, allowed, mask, conditioned=(1, 3), guided=guided)
        for b in range(B):
            if not mask[b]:
                continue
            for j in range(2 if b in guided else 1):
                if b in (0, 2):  # the slots are independent: an unconditioned slot does not see its neighbours' conditions
                    assert np.array_equal(bits(ie[b, j]), bits(ip[b, j])), f"unconditioned slot {b} row {j} differs at step {s}"
                elif before[b] <= tad:  # no generated token has reached the input yet: the twin's row is the plain sum
                    assert np.array_equal(bits(ie[b, j]), bits((ip[b, j] + rows[b]).astype(np.float32))), f"slot {b} row {j} at step {s}"
            if b in (0, 2):
                assert te[b] == tp[b] and np.array_equal(ae[b], ap[b])
    assert eng.metrics().capture_failures == 0
    plain.close(); eng.close()


def test_unconditioned_slots_of_a_mixed_batch_still_match_the_oracle(gpu, dsm, orc, fx):
    """Slots 1 and 3 conditioned, the oracle knows no conditions: slots 0 and 2 match it bit for bit (tokens, depformer tokens,
    lm.hidden, the audio_tokens table); slots 1 and 3 leave it at their first step."""
    cfg, d = fx["cfg"], fx["cfg"].lm.d_model
    eng, ora = _engine(dsm, fx), orc.OracleTts(cfg, B, fx["path"])
    eng.set_condition(1, "description", "bad")
    eng.set_condition_padding(3, "tail")
    first = {}
    for s, (prev, allowed, mask) in enumerate(schedule(cfg, B, cfg.text_audio_delay_in_tokens + 17)):
        te, ae = eng.step(prev, allowed, mask)
        to, ao = ora.step(prev, allowed, mask)
        he, ho = eng.debug_read("lm.hidden", B * d).reshape(B, d), ora.debug_read("lm.hidden", B * d).reshape(B, d)
        for b in range(B):
            if not mask[b]:
                continue
            same = np.array_equal(bits(he[b]), bits(ho[b]))
            if b in (0, 2):
                assert same, f"LM hidden bits of slot {b} differ at step {s}"
                assert te[b] == to[b] and np.array_equal(ae[b], ao[b]), f"tokens of slot {b} differ at step {s}"
            else:
                first.setdefault(b, same)
    assert first == {1: False, 3: False}, "a conditioned slot's first step equals the unconditioned oracle's"
    for b in (0, 2):
        assert eng.step_idx(b) == ora.step_idx(b) > cfg.text_audio_delay_in_tokens
        for i in range(eng.step_idx(b)):
            assert np.array_equal(eng.audio_tokens(b, i), ora.audio_tokens(b, i))
    eng.close(); ora.close()


def test_a_condition_set_after_capture_is_seen_on_replay(gpu, dsm, orc, fx):
    """Step until graphs replay, reset slot 1 and give it another condition: the identity holds on the replayed steps, nothing is
    recaptured or fails; after a reset without a new condition the slot is the oracle's again."""
    cfg, d = fx["cfg"], fx["cfg"].lm.d_model
    eng, ora = _engine(dsm, fx), orc.OracleTts(cfg, B, fx["path"])
    eng.set_condition(1, "description", "neutral")
    eng.set_condition(3, "speed", 1.25)
    sched = schedule(cfg, B, 40)
    s = 0
    while eng.metrics().graph_launches == 0:
        assert s < 16, "no graph replay after 16 steps"
        step_checked(eng, fx, *sched[s], conditioned=(1, 3))
        ora.step(*sched[s])
        s += 1
    eng.reset_batch_idx(1); ora.reset_batch_idx(1)
    assert not np.any(bits(cond_rows(eng)[1]))
    eng.set_condition(1, "tail", "d")
    assert np.array_equal(bits(cond_rows(eng)[1]), bits(CR.lut_row(fx["t"], TAIL, "d")))
    eager, graphs = eng.metrics().eager_bodies, eng.metrics().graph_launches
    for _ in range(6):
        step_checked(eng, fx, *sched[s], conditioned=(1, 3))
        ora.step(*sched[s])
        s += 1
    m = eng.metrics()
    assert m.capture_failures == 0, m.capture_error
    assert m.graph_launches >= graphs + 6 and m.eager_bodies == eager, (m.graph_launches, graphs, m.eager_bodies, eager)
    eng.reset_batch_idx(1); ora.reset_batch_idx(1)
    for _ in range(6):
        prev, allowed, mask = sched[s]
        te, ae, _ = step_checked(eng, fx, prev, allowed, mask, conditioned=(3,))
        to, ao = ora.step(prev, allowed, mask)
        he, ho = eng.debug_read("lm.hidden", B * d).reshape(B, d), ora.debug_read("lm.hidden", B * d).reshape(B, d)
        for b in (0, 1, 2):
            if mask[b]:
                assert np.array_equal(bits(he[b]), bits(ho[b])) and te[b] == to[b] and np.array_equal(ae[b], ao[b]), (b, s)
        s += 1
    assert eng.metrics().capture_failures == 0
    eng.close(); ora.close()


def test_the_request_path_applies_the_condition(gpu, dsm, lib):
    """One request per slot: dsm_tts_run (K = 4 per visit) and dsm_tts_step driven by the reference loop give the same text and
    audio tokens under the same conditions, and other tokens than the unconditioned run."""
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny()
    path = synth.make_synth_tts_weights(cfg, WDIR, seed=Q.WEIGHT_SEED, tag="tts_tiny_s%d" % Q.WEIGHT_SEED, conditioners=CR.CONDS)
    f = dict(cfg=cfg, path=path)
    conds = {0: lambda e, b: e.set_condition(b, "description", "good"), 1: lambda e, b: e.set_condition(b, "speed", 0.75),
             2: lambda e, b: e.set_condition_padding(b, "tail"), 3: lambda e, b: e.set_condition(b, "tail", "c")}

    def gens(conditioned):
        g = Q.whole_prompts(cfg)
        for x in g:
            if conditioned:
                x["setup"] = conds[x["slot"]]
        return g

    twin = _engine(dsm, f)
    want, _ = Q.run(twin, cfg, B, gens(True), 64)
    twin.close()
    bare = _engine(dsm, f)
    plain, _ = Q.run(bare, cfg, B, gens(False), 64)
    bare.close()
    eng = _engine(dsm, f)
    got = [dict(text=[], audio=[]) for _ in range(B)]
    for g in gens(True):
        b = g["slot"]
        g["setup"](eng, b)
        eng.request_begin(b, g["max_seq_len"], g["extra_steps"])
        if g["words"]:
            eng.push_words(b, g["words"])
        eng.request_close(b)
    for _ in range(16):
        eng.run(4)
        blk = eng.collect()
        for s in range(blk.n_steps):
            for b in range(B):
                if blk.stepped[s, b]:
                    got[b]["text"].append(int(blk.text_token[s, b]))
                    got[b]["audio"].append(blk.audio[s, b].copy())
    assert eng.metrics().capture_failures == 0
    eng.close()

    def differs(a, b):
        return a["text"] != b["text"] or len(a["audio"]) != len(b["audio"]) or any(not np.array_equal(x, y) for x, y in zip(a["audio"], b["audio"]))

    for b in range(B):
        assert got[b]["text"] == want[b]["text"], f"slot {b}: text tokens of the two paths differ"
        assert not differs(got[b], want[b]), f"slot {b}: audio tokens of the two paths differ"
    changed = [differs(want[b], plain[b]) for b in range(B)]
    print("slots whose tokens the condition changed:", changed, "steps:", [len(w["text"]) for w in want])
    assert changed[0] and changed[1], changed  # the two slots that run 64 steps


def _msg(lib, eng):
    m = lib.dsm_tts_last_error(eng.h)
    return m.decode() if m else ""


def test_refused_calls(gpu, dsm, lib, fx):
    """DSM_ERR_INVALID with a message: no conditioners attached, unknown name, unlisted LUT value, a string for a continuous
    conditioner, a number for a LUT.  DSM_ERR_STATE on a slot that has stepped, the next step unchanged.  Attaching from a file
    without the tensors (or with another shape) fails and the engine goes on."""
    from dsm_amd import synth
    cfg, d = fx["cfg"], fx["cfg"].lm.d_model
    eng, twin = _engine(dsm, fx, attach=False), _engine(dsm, fx, attach=False)
    sched = schedule(cfg, B, 6)

    def invalid(call, word):
        assert call() == DSM_ERR_INVALID
        assert word in _msg(lib, eng), _msg(lib, eng)
        assert not np.any(bits(cond_rows(eng)))

    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, 0, b"description", b"good"), "attach")
    invalid(lambda: lib.dsm_tts_set_condition_padding(eng.h, 0, b"description"), "attach")
    # a checkpoint without the tensors; a descriptor whose dim is not the file's
    with pytest.raises(dsm.DsmError, match="cannot find tensor condition_provider.conditioners.description.embed.weight"):
        eng.attach_conditioners(CR.CONDS, synth.make_synth_tts_weights(cfg, WDIR, tag="tts_tiny"))
    with pytest.raises(dsm.DsmError, match="shape mismatch"):
        eng.attach_conditioners([dict(DESC, dim=8)], fx["path"])
    with pytest.raises(dsm.DsmError, match="even dim"):
        eng.attach_conditioners([dict(SPEED, dim=2)], fx["path"])
    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, 0, b"description", b"good"), "attach")
    for x in (eng, twin):
        t0 = x.step(*sched[0])
    eng.attach_conditioners(CR.CONDS, fx["path"])  # after steps, and after the failed attempts
    with pytest.raises(dsm.DsmError, match="already"):
        eng.attach_conditioners(CR.CONDS, fx["path"])
    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, 2, b"mood", b"good"), "mood")
    invalid(lambda: lib.dsm_tts_set_condition_padding(eng.h, 2, b"mood"), "mood")
    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, 2, b"description", b"also_good"), "also_good")
    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, 2, b"speed", b"good"), "speed")
    invalid(lambda: lib.dsm_tts_set_condition_cont(eng.h, 2, b"description", 1.0), "description")
    invalid(lambda: lib.dsm_tts_set_condition_lut(eng.h, B, b"description", b"good"), "slot")
    invalid(lambda: lib.dsm_tts_clear_condition(eng.h, -1), "slot")
    # slots 0 and 1 stepped (the schedule always runs them): no condition any more
    for call in (lambda: lib.dsm_tts_set_condition_lut(eng.h, 0, b"description", b"good"),
                 lambda: lib.dsm_tts_set_condition_cont(eng.h, 1, b"speed", 1.0),
                 lambda: lib.dsm_tts_set_condition_padding(eng.h, 1, b"tail")):
        assert call() == DSM_ERR_STATE and "fresh slot" in _msg(lib, eng)
    assert not np.any(bits(cond_rows(eng)))
    assert lib.dsm_tts_clear_condition(eng.h, 0) == 0  # clearing is always allowed
    for s in range(1, 6):
        (te, ae), (tt, ta) = eng.step(*sched[s]), twin.step(*sched[s])
        act = sched[s][2].astype(bool)
        assert np.array_equal(te[act], tt[act]) and np.array_equal(ae[act], ta[act]), f"step {s} after the refused calls"
        he, ht = eng.debug_read("lm.hidden", B * d).reshape(B, d), twin.debug_read("lm.hidden", B * d).reshape(B, d)
        assert np.array_equal(bits(he[act]), bits(ht[act]))
    eng.reset_batch_idx(0)
    eng.set_condition(0, "description", "good")  # a reset slot takes one
    eng.close(); twin.close()


def test_served_shapes(gpu, dsm, lib):
    """config_tts_v202501 with cross_attention and cfg_rows, B = 2, the shipped LUT (dim 16): the row's bits and the input identity
    at d_model 2048 (several column blocks of the input kernel), slot 0 conditioned and guided, three steps.  One engine, run
    twice — without and with the condition — stands in for the two engines: in these three steps no generated token has
    reached the input, so the first run's rows are the plain sums."""
    from dsm_amd import synth
    cfg = dsm.config_tts_v202501()
    cfg.text_audio_delay_in_tokens, cfg.max_steps = 2, 64
    cfg.cross_attention, cfg.ca_norm, cfg.ca_dim, cfg.ca_max_len, cfg.cfg_rows = 1, 0, 0, 128, 1
    path = synth.make_synth_tts_weights(cfg, WDIR, tag="tts-v202501-ca", conditioners=[DESC])
    try:
        f = dict(cfg=cfg, path=path, t=CR.cond_tensors(path), tables=CR.emb_tables(path, cfg))
        nb, d = 2, cfg.lm.d_model
        assert d == 2048
        eng = dsm.TtsEngine(cfg, nb, path)
        eng.attach_conditioners([DESC], path)
        sched = schedule(cfg, nb, 3)
        runs = []
        for conditioned in ((), (0,)):
            for b in range(nb):
                eng.reset_batch_idx(b)
            eng.set_ca_src(0, synth.synth_ca_src(cfg, 125, 1), synth.synth_ca_src(cfg, 125, 9), 2.0)
            if conditioned:
                eng.set_condition(0, "description", "very_good")
                rows = cond_rows(eng)
                assert np.array_equal(bits(rows[0]), bits(CR.lut_row(f["t"], DESC, "very_good"))) and not np.any(bits(rows[1]))
            runs.append([step_checked(eng, f, *sched[s], conditioned=conditioned, guided=(0,))[2] for s in range(3)])
        for s in range(3):
            for j in range(2):
                assert np.array_equal(bits(runs[1][s][0, j]), bits((runs[0][s][0, j] + rows[0]).astype(np.float32))), (s, j)
            assert np.array_equal(bits(runs[1][s][1]), bits(runs[0][s][1])), s
        assert eng.metrics().capture_failures == 0
        eng.close()
    finally:
        os.remove(path)  # 1.1 GB
