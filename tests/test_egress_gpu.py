"""GPU parity of the TTS egress (dsm_tts_set_egress, dsm_tts_step_raw / _recv_raw / _collect_raw) against a plain engine — egress
off, the f32 frames of dsm_tts_step_pcm, which test_tts_pcm_gpu.py pins to the oracle — whose frames go through the host
function dsm_egress_host per slot: the host state is stepped on valid frames only and is new at a slot's reset and at a format
switch.  Rows are compared bit for bit in their first frame_bytes; everything behind a frame and the rows of slots that did not
emit keep the 0xA5 the test put there; valid flags, text tokens and audio tokens are the plain engine's.

Plan (tests/tts_pcm_ref.py): config_tts_tiny, the 6-codebook tiny Mimi, B = 4, 24 steps, slot 3 late, slot 2 reset before step 13.
Formats: slot 0 24000 / F32, slot 1 8000 / MULAW, slot 2 44100 / S16, slot 3 48000 / F32; slot 1 switches to 16000 / ALAW before
step 16."""
import numpy as np
import pytest

import egress_ref as E
import tts_pcm_ref as P
import tts_request_ref as Q

pytestmark = pytest.mark.gpu
DSM_ERR_INVALID, DSM_ERR_STATE = -1, -4
B, FILL, PITCH = P.B, 0xA5, 15360
FORMATS = {0: (24000, E.F32), 1: (8000, E.MULAW), 2: (44100, E.S16), 3: (48000, E.F32)}
SWITCH_STEP, SWITCH_SLOT, SWITCH_TO = 16, 1, (16000, E.ALAW)
# (rate, format): (frame_samples, frame_bytes, latency) by the definition's table
WANT_FORMAT = {(24000, E.F32): (1920, 7680, 0), (8000, E.MULAW): (640, 640, 34), (44100, E.S16): (3528, 7056, 62),
               (48000, E.F32): (3840, 15360, 68), (16000, E.ALAW): (1280, 1280, 34)}


def _engine(dsm, cfg_t, tts_path, mimi, egress):
    eng = dsm.TtsEngine(cfg_t, B, tts_path)
    eng.attach_mimi(mimi[0].mimi, mimi[2])
    if egress:
        eng.set_egress(True)
        for b, (rate, fmt) in FORMATS.items():
            eng.set_output_format(b, rate, fmt)
    return eng


def oracle_valid(orc, cfg_t, tts_path, steps, resets):
    """The emit flags of the plan from the CPU oracle's tokens alone (the predicate of tts_pcm_ref.reference, no decode)."""
    ora = orc.OracleTts(cfg_t, B, tts_path)
    ad, out = cfg_t.acoustic_delay, []
    for s, (prev, allowed, mask) in enumerate(steps):
        for slot in resets.get(s, []):
            ora.reset_batch_idx(slot)
        before = [ora.step_idx(b) for b in range(B)]
        ora.step(prev, allowed, mask)
        out.append([int(bool(mask[b]) and before[b] >= ad and P.emits(cfg_t, mask[b], before[b], ora.audio_tokens(b, before[b] - ad)))
                    for b in range(B)])
    ora.close()
    return np.array(out, dtype=np.uint8)


class HostSide:
    """The expected rows: one dsm_egress_host per slot, new at a reset and at a format switch, stepped on valid frames only."""

    def __init__(self, dsm):
        self.dsm, self.fmt = dsm, dict(FORMATS)
        self.h = {b: dsm.egress_host(*self.fmt[b]) for b in range(B)}

    def renew(self, b, fmt=None):
        self.fmt[b] = fmt or self.fmt[b]
        self.h[b].close()
        self.h[b] = self.dsm.egress_host(*self.fmt[b])

    def rows(self, pcm, valid):
        out = np.full((B, PITCH), FILL, dtype=np.uint8)
        for b in range(B):
            if valid[b]:
                out[b, :self.h[b].frame_bytes] = self.h[b].step(pcm[b])
        return out


@pytest.fixture(scope="module")
def fx(gpu, dsm, lib, orc):
    """The plain engine's run of the plan and the rows expected of it, computed once and left unchanged."""
    cfg_t, tts_path = P.tts_setup(dsm)
    mimi = P.mimi_setup(dsm)
    steps, resets = P.plan(cfg_t)
    # on the inputs, on the CPU: every slot emits at least 5 frames, slot 1 at least 3 after its switch
    ov = oracle_valid(orc, cfg_t, tts_path, steps, resets)
    assert np.all(ov.sum(axis=0) >= 5), ov.sum(axis=0)
    assert ov[SWITCH_STEP:, SWITCH_SLOT].sum() >= 3 and ov[:SWITCH_STEP, SWITCH_SLOT].sum() >= 2
    assert ov[P.RESET_STEP:, P.RESET_SLOT].sum() >= 3 and ov[:P.RESET_STEP, P.RESET_SLOT].sum() >= 1
    plain = _engine(dsm, cfg_t, tts_path, mimi, egress=False)
    host = HostSide(dsm)
    ref = dict(text=[], audio=[], valid=[], pcm=[], rows=[])
    for s, (prev, allowed, mask) in enumerate(steps):
        for slot in resets.get(s, []):
            plain.reset_batch_idx(slot)
            host.renew(slot)
        if s == SWITCH_STEP:
            host.renew(SWITCH_SLOT, SWITCH_TO)
        text, audio, pcm, valid = plain.step_pcm(prev, allowed, mask)
        for k, v in zip(("text", "audio", "valid", "pcm"), (text, audio, valid, pcm)):
            ref[k].append(v)
        ref["rows"].append(host.rows(pcm, valid))
    assert np.array_equal(np.array(ref["valid"]), ov)
    ref["step_idx"] = [plain.step_idx(b) for b in range(B)]
    plain.close()
    return dict(cfg_t=cfg_t, tts_path=tts_path, mimi=mimi, steps=steps, resets=resets, ref=ref)


def _check_rows(ref, s, rows, valid):
    assert np.array_equal(valid, ref["valid"][s]), f"valid differs at step {s}: {valid} vs {ref['valid'][s]}"
    bad = np.argwhere(rows != ref["rows"][s])
    assert bad.size == 0, f"step {s}: {len(bad)} bytes differ, the first at (slot, byte) {bad[:4].tolist()}"


def _between(eng, fx, s):
    for slot in fx["resets"].get(s, []):
        eng.reset_batch_idx(slot)
    if s == SWITCH_STEP:
        eng.set_output_format(SWITCH_SLOT, *SWITCH_TO)
        assert eng.output_format(SWITCH_SLOT) == SWITCH_TO + WANT_FORMAT[SWITCH_TO]


def test_serial_step_raw(dsm, fx):
    ref = fx["ref"]
    eng = _engine(dsm, fx["cfg_t"], fx["tts_path"], fx["mimi"], egress=True)
    for b, f in FORMATS.items():
        assert eng.output_format(b) == f + WANT_FORMAT[f]
    for s, (prev, allowed, mask) in enumerate(fx["steps"]):
        _between(eng, fx, s)
        text, audio, rows, valid = eng.step_raw(prev, allowed, mask, pitch=PITCH, fill=FILL)
        assert np.array_equal(text, ref["text"][s]) and np.array_equal(audio, ref["audio"][s]), f"tokens differ at step {s}"
        _check_rows(ref, s, rows, valid)
        if valid[0]:  # the pass-through slot: the plain engine's f32 frame, byte for byte
            assert rows[0, :7680].tobytes() == ref["pcm"][s][0].tobytes()
    assert [eng.step_idx(b) for b in range(B)] == ref["step_idx"]
    assert eng.metrics().capture_failures == 0 and eng.pcm_pending() == 0
    eng.close()


def test_deferred_step_raw_and_recv_raw(dsm, fx):
    """Queue depth 2: the rows of step n are received after step n + 1 was enqueued — across the reset of slot 2 and the format
    switch of slot 1, whose queued frames are still delivered in the format they were made in."""
    ref, steps = fx["ref"], fx["steps"]
    eng = _engine(dsm, fx["cfg_t"], fx["tts_path"], fx["mimi"], egress=True)
    assert eng.recv_raw() is None
    for s, (prev, allowed, mask) in enumerate(steps):
        _between(eng, fx, s)
        text, audio = eng.step_raw(prev, allowed, mask, defer=True)
        assert np.array_equal(text, ref["text"][s]) and np.array_equal(audio, ref["audio"][s]), f"tokens differ at step {s}"
        assert eng.pcm_pending() == (1 if s == 0 else 2)
        if s > 0:
            _check_rows(ref, s - 1, *eng.recv_raw(pitch=PITCH, fill=FILL))
    _check_rows(ref, len(steps) - 1, *eng.recv_raw(pitch=PITCH, fill=FILL))
    assert eng.pcm_pending() == 0 and eng.recv_raw() is None
    eng.close()


def test_requests_run_and_collect_raw(dsm, fx):
    """request_* / run(16, decode) / collect_raw against a plain engine's collect pushed through the host function."""
    cfg_t, tts_path = Q.tts_setup(dsm)
    plain = _engine(dsm, cfg_t, tts_path, fx["mimi"], egress=False)
    eng = _engine(dsm, cfg_t, tts_path, fx["mimi"], egress=True)
    host = HostSide(dsm)
    for x in (plain, eng):
        for g in Q.whole_prompts(cfg_t):
            x.request_begin(g["slot"], g["max_seq_len"], g["extra_steps"])
            x.push_words(g["slot"], g["words"])
            x.request_close(g["slot"])
    emitted = np.zeros(B, dtype=int)
    for block in range(4):
        if block == 1:
            eng.set_output_format(SWITCH_SLOT, *SWITCH_TO)
            host.renew(SWITCH_SLOT, SWITCH_TO)
        plain.run(16, decode=True)
        want = plain.collect()
        eng.run(16, decode=True)
        if block == 0:  # the f32 collect is refused on a decode block, and a pitch below an emitted frame: the block stays
            with pytest.raises(dsm.DsmError):
                eng.collect()
            eng._run = (16, True)
            with pytest.raises(dsm.DsmError):
                eng.collect_raw(pitch=640)
            eng._run = (16, True)
        got = eng.collect_raw(pitch=PITCH, fill=FILL)
        assert got.n_steps == want.n_steps == 16 and got.events == want.events
        for k in ("stepped", "text_token", "audio", "pcm_valid", "status"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), (block, k)
        for s in range(16):
            rows = host.rows(want.pcm[s], want.pcm_valid[s])
            bad = np.argwhere(got.pcm[s] != rows)
            assert bad.size == 0, f"block {block} step {s}: {len(bad)} bytes differ, the first at (slot, byte) {bad[:4].tolist()}"
        emitted += want.pcm_valid.sum(axis=0).astype(int)
    assert emitted.sum() >= 20 and emitted[SWITCH_SLOT] >= 3, emitted
    assert [eng.step_idx(b) for b in range(B)] == [plain.step_idx(b) for b in range(B)]
    plain.close(); eng.close()


def test_refusals_leave_the_following_step_unchanged(dsm, lib, fx):
    ref, steps = fx["ref"], fx["steps"]
    eng = dsm.TtsEngine(fx["cfg_t"], B, fx["tts_path"])
    p = lambda a: None if a is None else a.ctypes.data
    text, audio = np.zeros(B, dtype=np.uint32), np.zeros((B, eng.S), dtype=np.uint32)
    rows, valid = np.full((B, PITCH), FILL, dtype=np.uint8), np.zeros(B, dtype=np.uint8)
    pcm = np.zeros((B, 1920), dtype=np.float32)

    def raw(s, pitch, serial=True):
        a = [np.ascontiguousarray(x) for x in steps[s]]
        return lib.dsm_tts_step_raw(eng.h, p(a[0]), p(a[1]), p(a[2]), p(text), p(audio), p(rows) if serial else None, pitch, p(valid) if serial else None)

    def plain(s):
        a = [np.ascontiguousarray(x) for x in steps[s]]
        return lib.dsm_tts_step_pcm(eng.h, p(a[0]), p(a[1]), p(a[2]), p(text), p(audio), p(pcm), p(valid))

    idx = lambda: [eng.step_idx(b) for b in range(B)]
    assert not np.any(ref["valid"][:2])  # steps 0 and 1, taken around the refusals below, emit nothing: the streams start at step 2
    assert lib.dsm_tts_set_egress(eng.h, 1) == DSM_ERR_STATE  # no Mimi attached
    eng.attach_mimi(fx["mimi"][0].mimi, fx["mimi"][2])
    assert eng.output_format(2) == (24000, E.F32, 1920, 7680, 0)  # the default, before the section exists
    assert raw(0, PITCH) == DSM_ERR_STATE and lib.dsm_tts_recv_raw(eng.h, p(rows), PITCH, p(valid)) == DSM_ERR_STATE  # egress off
    assert lib.dsm_tts_set_output_format(eng.h, 0, 8000, E.MULAW) == DSM_ERR_STATE
    assert idx() == [0] * B and np.all(rows == FILL)
    # with an entry waiting the switch is refused
    a0 = [np.ascontiguousarray(x) for x in steps[0]]
    assert lib.dsm_tts_step_pcm(eng.h, p(a0[0]), p(a0[1]), p(a0[2]), p(text), p(audio), None, None) == 0 and eng.pcm_pending() == 1
    assert lib.dsm_tts_set_egress(eng.h, 1) == DSM_ERR_STATE
    assert eng.recv_pcm() is not None and eng.pcm_pending() == 0
    eng.set_egress(True)
    for b, (rate, fmt) in FORMATS.items():
        eng.set_output_format(b, rate, fmt)
    at = idx()
    assert plain(1) == DSM_ERR_STATE and lib.dsm_tts_recv_pcm(eng.h, p(pcm), p(valid)) == DSM_ERR_STATE  # the f32 calls while on
    assert raw(1, 15352) == DSM_ERR_INVALID and raw(1, 15376) == DSM_ERR_INVALID  # not a multiple of 16, above the largest row
    assert steps[1][2][0] and raw(1, 7664) == DSM_ERR_INVALID and raw(1, 16) == DSM_ERR_INVALID  # below the active slot 0's frame
    assert lib.dsm_tts_set_output_format(eng.h, 1, 12345, E.F32) == DSM_ERR_INVALID
    assert lib.dsm_tts_set_output_format(eng.h, 1, 8000, 4) == DSM_ERR_INVALID
    assert lib.dsm_tts_set_output_format(eng.h, B, 8000, E.F32) == DSM_ERR_INVALID
    assert eng.output_format(1) == FORMATS[1] + WANT_FORMAT[FORMATS[1]]
    assert idx() == at and np.all(rows == FILL) and eng.pcm_pending() == 0
    assert raw(1, 0, serial=False) == 0 and eng.pcm_pending() == 1   # a deferred step takes no pitch
    assert lib.dsm_tts_set_egress(eng.h, 0) == DSM_ERR_STATE          # an entry waits
    assert lib.dsm_tts_recv_raw(eng.h, p(rows), 100, p(valid)) == DSM_ERR_INVALID and eng.pcm_pending() == 1
    assert lib.dsm_tts_recv_raw(eng.h, p(rows), PITCH, p(valid)) == 1 and np.array_equal(valid, ref["valid"][1])
    # ... and the run goes on with the plan's results (the histories are at their start: nothing was emitted yet or the rows say so)
    for s in range(2, len(steps)):
        for slot in fx["resets"].get(s, []):
            eng.reset_batch_idx(slot)
        if s == SWITCH_STEP:
            eng.set_output_format(SWITCH_SLOT, *SWITCH_TO)
        rows[:] = FILL
        assert raw(s, PITCH) == 0
        assert np.array_equal(text, ref["text"][s]) and np.array_equal(audio, ref["audio"][s])
        _check_rows(ref, s, rows, valid)
    # off again: the f32 calls are back, formats and histories stay
    eng.set_egress(False)
    assert raw(0, PITCH) == DSM_ERR_STATE
    assert eng.output_format(1) == SWITCH_TO + WANT_FORMAT[SWITCH_TO]
    eng.close()
