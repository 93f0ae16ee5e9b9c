"""GPU parity of the device-side request loop (dsm_tts_request_* / dsm_tts_run / dsm_tts_collect) against a twin engine on
the same weights that tests/tts_request_ref.py — the reference's inference loop, srv/tts.rs:574-621 — steps one step_pcm at a
time.  step_pcm itself is pinned to the oracle bit for bit by test_tts_pcm_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import tts_pcm_ref as R
import tts_request_ref as Q
from tts_schedule import schedule

pytestmark = pytest.mark.gpu
DSM_ERR_INVALID, DSM_ERR_STATE = -1, -4
B = R.B


def _engine(dsm, cfg_t, tts_path, mimi, nb=B):
    eng = dsm.TtsEngine(cfg_t, nb, tts_path)
    eng.attach_mimi(mimi[0].mimi, mimi[2])
    return eng


@pytest.fixture(scope="module")
def fx(dsm, lib):
    """Inputs and the whole-prompt reference (a twin stepped by the reference loop), computed once and left unchanged."""
    cfg_t, tts_path = Q.tts_setup(dsm)
    mimi = R.mimi_setup(dsm)
    twin = _engine(dsm, cfg_t, tts_path, mimi)
    ref, stepped = Q.run(twin, cfg_t, B, Q.whole_prompts(cfg_t), 64, decode=True)
    twin.close()
    Q.check_branches(cfg_t, ref)
    assert sum(sum(r["valid"]) for r in ref) >= 20  # frames are decoded
    return dict(cfg_t=cfg_t, tts_path=tts_path, mimi=mimi, ref=ref, stepped=stepped)


def drive(eng, cfg_t, gens, K, n_iter, decode=True, between=None):
    """The request API over `gens` (see tts_request_ref): begins, pushes and closes happen between blocks of K steps, at the
    first block boundary at or after the iteration the generation's `at` / script names (they must fall on one).  Returns
    (results, stepped) shaped like tts_request_ref.run's."""
    nb = eng.B
    res = [dict(text=[], audio=[], valid=[], pcm=[], events=[], slot=g["slot"]) for g in gens]
    live, pushed = {}, {}
    stepped = []

    def finish(i):
        b = gens[i]["slot"]
        res[i]["status"], res[i]["step_idx"] = eng.request_status(b), eng.step_idx(b)
        res[i]["table"] = [eng.audio_tokens(b, k).copy() for k in range(eng.step_idx(b))]

    for it0 in range(0, n_iter, K):
        for i, g in enumerate(gens):
            at = g.get("at", 0)
            if it0 <= at < it0 + K:
                assert at == it0, "a generation begins at a block boundary"
                b = g["slot"]
                if b in live:
                    finish(live[b])
                if g.get("reset"):
                    eng.reset_batch_idx(b)
                    assert eng.request_status(b) == Q.IDLE
                if g.get("setup"):
                    g["setup"](eng, b)
                eng.request_begin(b, g["max_seq_len"], g["extra_steps"])
                assert eng.request_status(b) == Q.RUNNING
                live[b], pushed[i] = i, [0, False]
        for b, i in live.items():
            g = gens[i]
            n, closed = 0, False
            for at, nw, cl in g.get("script") or [(g.get("at", 0), len(g["words"]), True)]:
                if at <= it0:
                    n, closed = nw, cl
            if n > pushed[i][0]:
                eng.push_words(b, g["words"][pushed[i][0]:n])
                pushed[i][0] = n
            if closed and not pushed[i][1]:
                eng.request_close(b)
                pushed[i][1] = True
        if between:
            between(it0)
        eng.run(K, decode=decode)
        blk = eng.collect()
        assert blk.n_steps == K
        stepped.append(blk.stepped.copy())
        for s in range(K):
            for b, i in live.items():
                if blk.stepped[s, b]:
                    v = int(blk.pcm_valid[s, b]) if decode else 0
                    res[i]["text"].append(int(blk.text_token[s, b]))
                    res[i]["audio"].append(blk.audio[s, b].copy())
                    res[i]["valid"].append(v)
                    res[i]["pcm"].append(blk.pcm[s, b].copy() if v else None)
        for b, w, a, z in blk.events:
            res[live[b]]["events"].append((w, a, z))
        assert [int(x) for x in blk.status] == [eng.request_status(b) for b in range(nb)]
    for i in set(live.values()):
        finish(i)
    return res, np.concatenate(stepped)[:n_iter]


def same(got, want, what=""):
    """Every step a slot took: text token, audio tokens, pcm_valid, PCM bits; then word events, step index, table, status."""
    assert got["text"] == want["text"], f"{what}: text tokens differ"
    assert len(got["audio"]) == len(want["audio"])
    for s, (a, b) in enumerate(zip(got["audio"], want["audio"])):
        assert np.array_equal(a, b), f"{what}: audio tokens differ at step {s}"
    assert got["valid"] == want["valid"], f"{what}: pcm_valid differs"
    for s, (a, b) in enumerate(zip(got["pcm"], want["pcm"])):
        if want["valid"][s]:
            assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: PCM bits differ at step {s}"
    assert got["events"] == want["events"], f"{what}: word events differ"
    assert got["step_idx"] == want["step_idx"] and got["status"] == want["status"], (what, got["step_idx"], got["status"])
    assert len(got["table"]) == len(want["table"]) and all(np.array_equal(a, b) for a, b in zip(got["table"], want["table"])), f"{what}: tables differ"


@pytest.mark.parametrize("K", [1, 3, 16])
def test_whole_prompts(gpu, dsm, fx, K):
    """Four prompts, every branch of the loop; the results do not depend on K (K = 16 reuses frame and PCM buffers)."""
    eng = _engine(dsm, fx["cfg_t"], fx["tts_path"], fx["mimi"])
    got, stepped = drive(eng, fx["cfg_t"], Q.whole_prompts(fx["cfg_t"]), K, 64)
    for b in range(B):
        same(got[b], fx["ref"][b], f"K={K} slot {b}")
    assert np.array_equal(stepped, fx["stepped"])
    assert eng.metrics().capture_failures == 0
    eng.close()


def test_words_arriving_late(gpu, dsm, fx):
    """Words pushed between blocks: the same per-slot sequences, later; the stepped flags show the steps sat out."""
    cfg_t = fx["cfg_t"]
    eng = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    seen = {}
    got, stepped = drive(eng, cfg_t, Q.late_prompts(cfg_t), 16, Q.LATE_ITERS, between=lambda it0: seen.setdefault(it0, eng.request_status(1)))
    for b in range(B):
        same(got[b], fx["ref"][b], f"late slot {b}")
    twin = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    _, want = Q.run(twin, cfg_t, B, Q.late_prompts(cfg_t), Q.LATE_ITERS, decode=True)
    twin.close()
    assert np.array_equal(stepped, want)
    assert not stepped[1:16, 1].any() and not stepped[32:48, 1].any()  # slot 1: no word in block 0, none through block 2
    assert seen[16] == Q.WAITING and seen[32] == Q.WAITING and seen[48] == Q.WAITING
    eng.close()


def test_served_branch(gpu, dsm, fx):
    """cross_attention + cfg_rows: one guided slot, one with a source only, seeded top-k on two slots."""
    from dsm_amd import synth
    cfg_t, tts_path = Q.tts_setup(dsm, cross_attention=True, cfg_rows=True)
    setups = {
        0: lambda e, b: e.set_ca_src(b, synth.synth_ca_src(cfg_t, 20, 1), synth.synth_ca_src(cfg_t, 9, 99), 2.5),
        1: lambda e, b: e.set_sampling(b, 5, 0.8, 1234),
        2: lambda e, b: e.set_ca_src(b, synth.synth_ca_src(cfg_t, 8, 2)),
        3: lambda e, b: e.set_sampling(b, 3, 1.1, 77),
    }

    def gens():
        g = Q.whole_prompts(cfg_t)
        g[3]["max_seq_len"] = 40
        for x in g:
            x["setup"] = setups[x["slot"]]
        return g

    twin = _engine(dsm, cfg_t, tts_path, fx["mimi"])
    want, _ = Q.run(twin, cfg_t, B, gens(), 64, decode=True)
    twin.close()
    assert all(sum(r["valid"]) >= 1 for r in want[:2])
    eng = _engine(dsm, cfg_t, tts_path, fx["mimi"])
    got, _ = drive(eng, cfg_t, gens(), 5, 64)
    for b in range(B):
        same(got[b], want[b], f"served slot {b}")
    assert eng.metrics().capture_failures == 0
    eng.close()


def test_slots_come_and_go(gpu, dsm, fx):
    """A request begins in block 2 beside running ones; a DONE slot is reset and serves a second request: every generation
    equals a twin that runs it alone."""
    cfg_t = fx["cfg_t"]
    bos = cfg_t.text_bos_token
    gens = [
        dict(slot=0, words=Q.whole_prompts(cfg_t)[0]["words"], max_seq_len=64, extra_steps=2),
        dict(slot=1, words=[[bos, 8]], max_seq_len=64, extra_steps=0),
        dict(slot=2, at=16, words=[[bos, 10, 11], [12], [13, 14]], max_seq_len=64, extra_steps=1),
        dict(slot=1, at=32, reset=True, words=[[bos, 21, 22], [23]], max_seq_len=20, extra_steps=4),
    ]
    eng = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    got, _ = drive(eng, cfg_t, [dict(g) for g in gens], 16, 80)
    assert got[1]["status"] == Q.DONE and len(got[1]["text"]) < 16  # done before its slot is reused
    for i, g in enumerate(gens):
        alone = dict(g, at=0, reset=False)
        twin = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
        (want,), _ = Q.run(twin, cfg_t, B, [alone], 64, decode=True)
        twin.close()
        same(got[i], want, f"generation {i}")
    eng.close()


def _snapshot(eng):
    return ([eng.step_idx(b) for b in range(eng.B)], [eng.request_status(b) for b in range(eng.B)],
            [[eng.audio_tokens(b, i).tolist() for i in range(eng.step_idx(b))] for b in range(eng.B)])


def test_rules(gpu, dsm, lib, fx):
    """Every refused call leaves step indices, tables and statuses alone; step() serves an IDLE slot between blocks."""
    cfg_t = fx["cfg_t"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bare = dsm.TtsEngine(cfg_t, B, fx["tts_path"])
    bare.request_begin(0, 8, 0)
    assert lib.dsm_tts_run(bare.h, 1, 1) == DSM_ERR_STATE  # decode without a Mimi
    assert bare.step_idx(0) == 0 and bare.request_status(0) == Q.RUNNING
    bare.close()

    eng = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    twin = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    sched = schedule(cfg_t, B, 13)
    only3 = np.array([0, 0, 0, 1], dtype=np.uint8)
    toks, lens = np.array([1, 5, 6], dtype=np.uint32), np.array([2, 1], dtype=np.int32)
    big = np.zeros(200, dtype=np.uint32)
    biglen = np.array([200], dtype=np.int32)
    text, audio = np.zeros(B, dtype=np.uint32), np.zeros((B, eng.S), dtype=np.uint32)

    def step_raw(mask):
        prev, allowed, _ = sched[0]
        return lib.dsm_tts_step(eng.h, p(prev), p(allowed), p(np.ascontiguousarray(mask)), p(text), p(audio))

    def refused(rc, call):
        before = _snapshot(eng)
        assert call() == rc, call
        assert _snapshot(eng) == before

    # no request anywhere yet
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_push_words(eng.h, 0, p(toks), p(lens), 2))   # IDLE slot
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_close(eng.h, 0))
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_collect(eng.h, C.byref(dsm.TtsBlockC())))           # no block waits
    refused(DSM_ERR_INVALID, lambda: lib.dsm_tts_request_begin(eng.h, B, 8, 0))
    refused(DSM_ERR_INVALID, lambda: lib.dsm_tts_request_begin(eng.h, 0, 0, 0))
    refused(DSM_ERR_INVALID, lambda: lib.dsm_tts_request_begin(eng.h, 0, 8, -1))
    refused(DSM_ERR_INVALID, lambda: lib.dsm_tts_request_status(eng.h, -1))
    # slot 3 takes ordinary steps: it is not fresh any more
    for x in (eng, twin):
        t0, a0 = x.step(sched[0][0], sched[0][1], only3)
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_begin(eng.h, 3, 8, 0))
    g = Q.whole_prompts(cfg_t)[0]
    eng.request_begin(0, g["max_seq_len"], g["extra_steps"])
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_begin(eng.h, 0, 8, 0))                      # has a request already
    refused(DSM_ERR_INVALID, lambda: lib.dsm_tts_request_push_words(eng.h, 0, p(toks), p(np.array([2, -1], dtype=np.int32)), 2))
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_push_words(eng.h, 0, p(big), p(biglen), 1))  # does not fit
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_run(eng.h, 0, 0))
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_run(eng.h, dsm.TTS_RUN_MAX + 1, 0))
    refused(DSM_ERR_STATE, lambda: step_raw(np.array([1, 0, 0, 1], dtype=np.uint8)))               # mask on a slot with a request
    eng.push_words(0, g["words"])
    eng.request_close(0)
    refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_push_words(eng.h, 0, p(toks), p(lens), 2))   # closed
    got = dict(text=[], audio=[])
    for blk_i in range(4):
        # between blocks: step() on the IDLE slot 3, the same calls on the twin
        for s in range(1 + 3 * blk_i, 4 + 3 * blk_i):
            te, ae = eng.step(sched[s][0], sched[s][1], only3)
            tt, ta = twin.step(sched[s][0], sched[s][1], only3)
            assert te[3] == tt[3] and np.array_equal(ae[3], ta[3]), f"step() on the idle slot differs at {s}"
        eng.run(16, decode=True)
        # a block waits
        refused(DSM_ERR_STATE, lambda: lib.dsm_tts_run(eng.h, 1, 0))
        refused(DSM_ERR_STATE, lambda: step_raw(only3))
        refused(DSM_ERR_STATE, lambda: lib.dsm_tts_step_pcm(eng.h, p(sched[0][0]), p(sched[0][1]), p(only3), p(text), p(audio), None, None))
        refused(DSM_ERR_STATE, lambda: lib.dsm_tts_request_begin(eng.h, 1, 8, 0))
        refused(DSM_ERR_STATE, lambda: lib.dsm_tts_reset_slot(eng.h, 2))
        blk = eng.collect()
        for s in range(16):
            if blk.stepped[s, 0]:
                got["text"].append(int(blk.text_token[s, 0]))
                got["audio"].append(blk.audio[s, 0].copy())
        assert not blk.stepped[:, 1:].any()
    want = fx["ref"][0]
    assert got["text"] == want["text"] and all(np.array_equal(a, b) for a, b in zip(got["audio"], want["audio"]))
    assert eng.request_status(0) == Q.DONE and eng.step_idx(0) == want["step_idx"]
    assert eng.step_idx(3) == twin.step_idx(3) == 13
    for i in range(13):
        assert np.array_equal(eng.audio_tokens(3, i), twin.audio_tokens(3, i))
    eng.reset_batch_idx(0)
    assert eng.request_status(0) == Q.IDLE and eng.step_idx(0) == 0
    eng.close(); twin.close()


def test_blocks_replay_graphs(gpu, dsm, fx):
    """After warm-up a block adds graph launches and no eager bodies."""
    cfg_t = fx["cfg_t"]
    eng = _engine(dsm, cfg_t, fx["tts_path"], fx["mimi"])
    for g in Q.whole_prompts(cfg_t):
        eng.request_begin(g["slot"], g["max_seq_len"], g["extra_steps"])
        if g["words"]:
            eng.push_words(g["slot"], g["words"])
        eng.request_close(g["slot"])
    eng.run(16, decode=True)
    eng.collect()
    m0 = eng.metrics()
    eager0, graphs0 = m0.eager_bodies, m0.graph_launches
    eng.run(16, decode=True)
    blk = eng.collect()
    assert blk.stepped[:, 0].all()
    m = eng.metrics()
    assert m.capture_failures == 0, m.capture_error
    assert m.eager_bodies == eager0, (m.eager_bodies, eager0)
    assert m.graph_launches >= graphs0 + 32, (m.graph_launches, graphs0)  # the step's group and the decode, 16 times each
    eng.close()
