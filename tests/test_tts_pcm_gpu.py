"""GPU parity of dsm_tts_step_pcm — State::step + the audio_processing_loop's Mimi::decode_step of the frame the step
completed (srv/tts.rs:528-544) — against a reference built from the oracle alone (tests/tts_pcm_ref.py): every slot decodes
as a fresh B = 1 Mimi of its own.  PCM of emitting slots bit for bit, the valid flags, and tokens / step indices / token tables
identical to dsm_tts_step's."""
import numpy as np
import pytest

import tts_pcm_ref as R

pytestmark = pytest.mark.gpu
DSM_ERR_INVALID, DSM_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def fx(dsm, orc):
    """Inputs and the reference, computed once and left unchanged."""
    cfg_t, tts_path = R.tts_setup(dsm)
    mimi = R.mimi_setup(dsm)
    steps, resets = R.plan(cfg_t)
    ref = R.reference(orc, cfg_t, tts_path, mimi, steps, resets, R.B)
    R.check_inputs(cfg_t, ref, R.batched_module_pcm(orc, mimi, ref, resets, R.B))
    return dict(cfg_t=cfg_t, tts_path=tts_path, mimi=mimi, steps=steps, resets=resets, ref=ref)


def _check_pcm(ref, s, pcm, valid):
    want = ref["valid"][s]
    assert np.array_equal(valid, want), f"valid differs at step {s}: {valid} vs {want}"
    v = want.astype(bool)
    assert np.all(np.isfinite(pcm[v]))
    assert np.array_equal(pcm[v].view(np.uint32), ref["pcm"][s][v].view(np.uint32)), f"PCM bits differ at step {s}, slots {np.flatnonzero(v)}"


def _check_tables(eng, ref, nb):
    for b in range(nb):
        assert eng.step_idx(b) == ref["step_idx"][b]
        for i in range(eng.step_idx(b)):
            assert np.array_equal(eng.audio_tokens(b, i), ref["tables"][b][i])


def _serial(dsm, cfg_t, tts_path, mimi, steps, resets, ref, nb, setup=None):
    """step_pcm (serial) against the reference, and against a twin engine without Mimi running step()."""
    eng, twin = dsm.TtsEngine(cfg_t, nb, tts_path), dsm.TtsEngine(cfg_t, nb, tts_path)
    eng.attach_mimi(mimi[0].mimi, mimi[2])
    for x in (eng, twin):
        if setup:
            setup(x)
    emitted = 0
    for s, (prev, allowed, mask) in enumerate(steps):
        for slot in resets.get(s, []):
            eng.reset_batch_idx(slot)
            twin.reset_batch_idx(slot)
        text, audio, pcm, valid = eng.step_pcm(prev, allowed, mask)
        tt, ta = twin.step(prev, allowed, mask)
        act = mask.astype(bool)
        assert np.array_equal(text, tt) and np.array_equal(audio, ta), f"step_pcm and step disagree at step {s}"
        assert np.array_equal(text[act], ref["text"][s][act]) and np.array_equal(audio[act], ref["audio"][s][act]), f"tokens differ at step {s}"
        _check_pcm(ref, s, pcm, valid)
        emitted += int(valid.sum())
    _check_tables(eng, ref, nb)
    _check_tables(twin, ref, nb)
    m = eng.metrics()
    assert m.capture_failures == 0, m.capture_error
    assert eng.pcm_pending() == 0
    eng.close(); twin.close()
    return emitted


def test_serial_parity(gpu, dsm, lib, fx):
    n = _serial(dsm, fx["cfg_t"], fx["tts_path"], fx["mimi"], fx["steps"], fx["resets"], fx["ref"], R.B)
    assert n == int(np.sum(fx["ref"]["valid"]))


def test_deferred_parity(gpu, dsm, lib, fx):
    """defer=True with recv_pcm() after the following step: the decode of step n overlaps the LM of step n + 1."""
    cfg_t, ref, steps = fx["cfg_t"], fx["ref"], fx["steps"]
    eng = dsm.TtsEngine(cfg_t, R.B, fx["tts_path"])
    eng.attach_mimi(fx["mimi"][0].mimi, fx["mimi"][2])
    g0 = eng.metrics().graph_launches
    assert eng.pcm_pending() == 0 and eng.recv_pcm() is None
    for s, (prev, allowed, mask) in enumerate(steps):
        for slot in fx["resets"].get(s, []):
            eng.reset_batch_idx(slot)  # with step s - 1's frames still queued: they belong to the old generation and are delivered
        text, audio = eng.step_pcm(prev, allowed, mask, defer=True)
        act = mask.astype(bool)
        assert np.array_equal(text[act], ref["text"][s][act]) and np.array_equal(audio[act], ref["audio"][s][act]), f"tokens differ at step {s}"
        assert eng.pcm_pending() == (1 if s == 0 else 2)
        if s > 0:
            _check_pcm(ref, s - 1, *eng.recv_pcm())
            assert eng.pcm_pending() == 1
    _check_pcm(ref, len(steps) - 1, *eng.recv_pcm())
    assert eng.pcm_pending() == 0 and eng.recv_pcm() is None
    _check_tables(eng, ref, R.B)
    m = eng.metrics()
    assert m.graph_launches > g0 and m.capture_failures == 0, (m.graph_launches, m.capture_error)
    eng.close()


def test_guided_and_sampled(gpu, dsm, lib, orc, fx):
    """Two batch rows per slot (classifier-free guidance on slot 0) and the sampler variant of the step graph (slot 1)."""
    from dsm_amd import synth
    from tts_schedule import schedule
    cfg_t, tts_path = R.tts_setup(dsm, cross_attention=True, cfg_rows=True)
    nb = 3
    steps = [(p, a, np.ones(nb, dtype=np.uint8)) for p, a, _ in schedule(cfg_t, nb, 16)]

    def setup(x):
        x.set_ca_src(0, synth.synth_ca_src(cfg_t, 20, 1), synth.synth_ca_src(cfg_t, 9, 99), 2.5)
        x.set_ca_src(2, synth.synth_ca_src(cfg_t, 8, 2))
        x.set_sampling(1, 5, 0.8, 1234)

    ref = R.reference(orc, cfg_t, tts_path, fx["mimi"], steps, {}, nb, setup=setup)
    assert np.all(np.sum(ref["valid"], axis=0) >= 5)
    _serial(dsm, cfg_t, tts_path, fx["mimi"], steps, {}, ref, nb, setup=setup)


def test_errors(gpu, dsm, lib, fx):
    import ctypes as C
    cfg_t, ref, steps = fx["cfg_t"], fx["ref"], fx["steps"]
    cfg_a, _, mimi_path = fx["mimi"]
    eng = dsm.TtsEngine(cfg_t, R.B, fx["tts_path"])
    args = [np.ascontiguousarray(a) for a in steps[0]]
    text, audio = np.zeros(R.B, dtype=np.uint32), np.zeros((R.B, eng.S), dtype=np.uint32)
    pcm, valid = np.zeros((R.B, 1920), dtype=np.float32), np.zeros(R.B, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(s, serial):
        a = [np.ascontiguousarray(x) for x in steps[s]]
        return lib.dsm_tts_step_pcm(eng.h, p(a[0]), p(a[1]), p(a[2]), p(text), p(audio), p(pcm) if serial else None, p(valid) if serial else None)

    assert raw(0, True) == DSM_ERR_STATE and raw(0, False) == DSM_ERR_STATE  # no Mimi attached
    assert [eng.step_idx(b) for b in range(R.B)] == [0] * R.B
    t0, a0 = eng.step(*args)
    act = args[2].astype(bool)
    assert np.array_equal(t0[act], ref["text"][0][act]) and np.array_equal(a0[act], ref["audio"][0][act])
    bad = dsm.MimiConfig.from_buffer_copy(cfg_a.mimi)
    bad.quantizer_n_q = 4
    assert lib.dsm_tts_attach_mimi(eng.h, C.byref(bad), mimi_path.encode()) == DSM_ERR_INVALID
    eng.attach_mimi(cfg_a.mimi, mimi_path)
    assert lib.dsm_tts_attach_mimi(eng.h, C.byref(cfg_a.mimi), mimi_path.encode()) == DSM_ERR_STATE
    assert eng.recv_pcm() is None
    assert raw(1, False) == 0 and raw(2, False) == 0 and eng.pcm_pending() == 2
    idx = [eng.step_idx(b) for b in range(R.B)]
    assert raw(3, False) == DSM_ERR_STATE  # a third deferred step
    assert raw(3, True) == DSM_ERR_STATE   # a serial step while entries are pending
    assert [eng.step_idx(b) for b in range(R.B)] == idx and eng.pcm_pending() == 2
    for s in (1, 2):
        _check_pcm(ref, s, *eng.recv_pcm())
    assert eng.recv_pcm() is None and lib.dsm_tts_recv_pcm(eng.h, None, None) == 0
    assert raw(3, True) == 0  # and the run goes on
    _check_pcm(ref, 3, pcm, valid)
    eng.close()


def test_module_level_decode_is_untouched(gpu, dsm, lib, orc, fx):
    """dsm_mimi_decode_step keeps Mimi::decode_step's module-level first call (the kernels' NULL `started` path): a slot that
    starts late equals the BATCHED oracle bit for bit — including its first frame, which has the `(z + b) + (0 - b)` carry term."""
    cfg_a, lm_a, mimi_a = fx["mimi"]
    nb = 3
    eng, ora = dsm.AsrEngine(cfg_a, nb, lm_a, mimi_a), orc.OracleAsr(cfg_a, nb, lm_a, mimi_a)
    fresh = orc.OracleAsr(cfg_a, 1, lm_a, mimi_a)
    rng = np.random.default_rng(8)
    for s in range(6):
        codes = rng.integers(0, cfg_a.mimi.quantizer_bins, (nb, cfg_a.mimi.quantizer_n_q)).astype(np.uint32)
        mask = np.array([1, s >= 3, s != 1], dtype=np.uint8)
        act = mask.astype(bool)
        pe, po = eng.decode_step(codes, mask), ora.decode_step(codes, mask, side=0)
        assert np.array_equal(pe[act].view(np.uint32), po[act].view(np.uint32)), f"PCM bits differ at step {s}"
        if s == 3:  # the late slot's first frame is NOT what a fresh module gives: the two semantics are distinguishable here
            pf = fresh.decode_step(codes[1:2], [1], side=0)
            assert not np.array_equal(pf[0].view(np.uint32), po[1].view(np.uint32))
    eng.close(); ora.close(); fresh.close()
