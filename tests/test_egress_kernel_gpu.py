"""egress_resample_kernel alone (dsm_tts_debug_egress: no LM, no Mimi decode) against the host function dsm_egress_host, bit for
bit: all seven resampling rates x four sample formats — seven passes with the four formats across the four slots — over three
frames of adversarial input: full scale, values just past clip, NaN and infinities, a DC frame (every phase has unit DC gain),
and a frame whose valid flag is 0 in the middle, which must leave history and row alone.  11025 Hz (L = 147, M = 320, 148 taps)
is the largest table and has negative q with a wrapping phase.  The pass-through format rides along."""
import numpy as np
import pytest

import egress_ref as R
import tts_pcm_ref as P

pytestmark = pytest.mark.gpu
B, FILL = 4, 0xA5


@pytest.fixture(scope="module")
def eng(gpu, dsm, lib):
    cfg_t, tts_path = P.tts_setup(dsm)
    cfg_a, _, mimi_path = P.mimi_setup(dsm)
    e = dsm.TtsEngine(cfg_t, B, tts_path)
    e.attach_mimi(cfg_a.mimi, mimi_path)
    e.set_egress(True)
    yield e
    e.close()


def frames_for(rate):
    """[4 steps][B][1920] and valid [4][B]: per slot three valid frames and one that is not, at step 1 or 2."""
    rng = np.random.RandomState(rate)
    f = (rng.standard_normal((4, B, R.FRAME)) * 0.3).astype(np.float32)
    nan, inf = np.float32("nan"), np.float32("inf")
    # slot 0: full scale and just past clip, alternating signs, then noise
    f[0, 0, :64] = np.tile(np.array([1.0, -1.0, 1.0000001, -1.0000001, 0.99999994, -0.99999994, 2.0, -2.0], dtype=np.float32), 8)
    f[2, 0, -32:] = np.float32(1.0)
    # slot 1: a DC frame between noise frames, and the ties of the s16 rounding
    f[1, 1] = np.float32(0.5)
    f[3, 1, :4] = np.array([1.5, 2.5, -1.5, -2.5], dtype=np.float32) / np.float32(32768)
    # slot 2: NaN and infinities inside the frame, at its end (they reach the next frame through the history) and alone
    f[0, 2, 100] = nan
    f[0, 2, 900:902] = [inf, -inf]
    f[2, 2, -3:] = [inf, nan, -inf]
    f[3, 2, 5] = inf
    # slot 3: tiny values, signed zeros, a silent frame
    f[0, 3, :6] = np.array([1e-40, -1e-40, 0.0, -0.0, 1e-30, -1e-30], dtype=np.float32)
    f[2, 3] = 0.0
    valid = np.ones((4, B), dtype=np.uint8)
    valid[1, 0] = valid[2, 1] = valid[1, 2] = valid[1, 3] = 0  # the frame in the middle that does not count (noise, DC, noise, noise)
    return f, valid


@pytest.mark.parametrize("rate", R.RATES)
def test_kernel_rows_are_the_host_functions(dsm, eng, rate):
    fmts = [(b + R.RATES.index(rate)) % 4 for b in range(B)]  # the four formats across the slots, rotated per pass
    for b in range(B):
        eng.set_output_format(b, rate, fmts[b])
        assert eng.output_format(b) == (rate, fmts[b], R.TABLE[rate][4], R.TABLE[rate][4] * R.SAMPLE_BYTES[fmts[b]], R.TABLE[rate][5])
    host = [dsm.egress_host(rate, fmts[b]) for b in range(B)]
    frames, valid = frames_for(rate)
    pitch = (max(h.frame_bytes for h in host) + 15) & ~15
    for s in range(4):
        rows = eng.debug_egress(frames[s], valid[s], pitch=pitch, fill=FILL)
        for b in range(B):
            if not valid[s, b]:  # nothing written, and the history untouched: the next valid frame shows it
                assert np.all(rows[b] == FILL), (rate, s, b)
                continue
            want = host[b].step(frames[s, b])
            n = host[b].frame_bytes
            bad = np.flatnonzero(rows[b, :n] != want)
            assert bad.size == 0, f"{rate} Hz format {fmts[b]} step {s} slot {b}: {bad.size} bytes differ, the first at {bad[:6]}"
            assert np.all(rows[b, n:] == FILL), (rate, s, b)
    for h in host:
        h.close()


def test_pass_through_and_unfiltered_formats(dsm, eng):
    """24000 Hz: F32 copies the bits (NaN payloads included), the other formats encode without a filter."""
    for b in range(B):
        eng.set_output_format(b, R.IN_RATE, b)
    host = [dsm.egress_host(R.IN_RATE, b) for b in range(B)]
    frames, valid = frames_for(24000)
    odd = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0x80000000], dtype=np.uint32)
    frames[0, 0, :odd.size] = odd.view(np.float32)
    for s in (0, 3):
        rows = eng.debug_egress(frames[s], np.ones(B, dtype=np.uint8), pitch=7680, fill=FILL)
        for b in range(B):
            n = host[b].frame_bytes
            assert np.array_equal(rows[b, :n], host[b].step(frames[s, b])) and np.all(rows[b, n:] == FILL), (s, b)
    assert rows[0].tobytes() == frames[3, 0].tobytes()
    for h in host:
        h.close()


def test_refusals_leave_the_state_alone(dsm, lib, eng):
    for b in range(B):
        eng.set_output_format(b, 48000 if b == 1 else 8000, R.F32 if b == 1 else R.MULAW)
    host = [dsm.egress_host(48000 if b == 1 else 8000, R.F32 if b == 1 else R.MULAW) for b in range(B)]
    frames, _ = frames_for(5)
    ones = np.ones(B, dtype=np.uint8)
    eng.debug_egress(frames[0], ones)
    for h, f in zip(host, frames[0]):
        h.step(f)
    rows = np.full((B, 15360), FILL, dtype=np.uint8)
    p = lambda a: a.ctypes.data
    f1 = np.ascontiguousarray(frames[1])
    assert lib.dsm_tts_debug_egress(eng.h, p(f1), p(ones), p(rows), 15352) == -1   # not a multiple of 16
    assert lib.dsm_tts_debug_egress(eng.h, p(f1), p(ones), p(rows), 15376) == -1   # above the largest row
    assert lib.dsm_tts_debug_egress(eng.h, p(f1), p(ones), p(rows), 640) == -1     # below slot 1's frame
    assert np.all(rows == FILL)
    only = np.array([1, 0, 1, 1], dtype=np.uint8)  # ... which is fine while slot 1 does not emit
    got = eng.debug_egress(frames[1], only, pitch=640, fill=FILL)
    for b in (0, 2, 3):
        assert np.array_equal(got[b], host[b].step(frames[1, b]))
    assert np.all(got[1] == FILL)
    with pytest.raises(dsm.DsmError):
        eng.set_output_format(0, 12345, R.F32)
    with pytest.raises(dsm.DsmError):
        eng.set_output_format(0, 8000, 4)
    with pytest.raises(dsm.DsmError):
        eng.set_output_format(B, 8000, R.F32)
    assert eng.output_format(0)[:2] == (8000, R.MULAW)
    got = eng.debug_egress(frames[2], ones, fill=FILL)
    for b in range(B):  # histories went on through the refusals: slot 1's holds frame 0 only
        assert np.array_equal(got[b, :host[b].frame_bytes], host[b].step(frames[2, b])), b
