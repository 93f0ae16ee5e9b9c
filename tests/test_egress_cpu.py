"""Egress on the host (csrc/dsm_pcm_format.h; no GPU): every descriptor word is the restatement's (tests/egress_ref.py) and the
definition's table; D is the brute-force minimum and the kept history covers the brute-force reach; what is outside the
definition is refused; dsm_egress_host, streamed frame by frame as F32, delivers the whole-clip resampler's output delayed by D,
bit for bit, for every rate; the sample encoders over all 65536 16-bit values against the restatement and the standard library's
G.711; a stream switched to another format restarts with D zeros.  Floats are compared as uint32."""
import audioop
import os

import numpy as np
import pytest

import egress_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 6
ALL_S16 = np.arange(-32768, 32768, dtype=np.int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stream(dsm, rate, fmt, x):
    h = dsm.egress_host(rate, fmt)
    out = np.concatenate([h.step(x[e * R.FRAME:(e + 1) * R.FRAME]) for e in range(x.size // R.FRAME)])
    h.close()
    return out


@pytest.mark.parametrize("rate", R.RATES)
def test_descriptor_words_latency_and_reach(dsm, lib, rate):
    g = R.geometry(rate)
    D, reach = R.brute_force(rate)
    assert (g["L"], g["M"], g["half"], g["taps"], g["F_out"], D) == R.TABLE[rate]  # the restatement finds the definition's table again
    assert D == (g["half"] * g["L"]) // g["M"]
    assert reach < g["taps"] <= R.MAX_TAPS, (reach, g["taps"])
    for fmt in R.FORMATS:
        info = dsm.egress_describe(rate, fmt)
        want = dict(rate=rate, fmt=fmt, L=g["L"], M=g["M"], half=g["half"], taps=g["taps"], F_out=g["F_out"],
                    frame_bytes=g["F_out"] * R.SAMPLE_BYTES[fmt], D=D, table_words=g["L"] * g["taps"])
        assert info == want, (info, want)
        h = dsm.egress_host(rate, fmt)
        assert (h.frame_samples, h.frame_bytes, h.latency) == (g["F_out"], want["frame_bytes"], D)
        h.close()
    w = np.zeros(12, dtype=np.uint32)
    assert lib.dsm_egress_describe(rate, R.F32, w.ctypes.data) == 0
    assert w[9] == 0 and w[11] == 0 and list(w[:9]) == [rate, R.F32, *R.TABLE[rate][:5], 4 * g["F_out"], D]


def test_the_pass_through_format(dsm, lib):
    info = dsm.egress_describe(R.IN_RATE, R.F32)
    assert (info["L"], info["M"], info["half"], info["taps"], info["F_out"], info["frame_bytes"], info["D"], info["table_words"]) == (1, 1, 0, 0, 1920, 7680, 0, 0)
    odd = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0x00000001, 0x80000000], dtype=np.uint32)
    frame = np.zeros(R.FRAME, dtype=np.uint32)
    frame[:odd.size] = odd
    h = dsm.egress_host(R.IN_RATE, R.F32)
    assert h.latency == 0 and h.step(frame.view(np.float32)).tobytes() == frame.tobytes()  # NaN payloads and all
    x = R.signal(FRAMES, seed=24000)
    assert _stream(dsm, R.IN_RATE, R.F32, x).tobytes() == x.tobytes()
    assert dsm.EGRESS_MAX_FRAME_BYTES == R.MAX_FRAME_BYTES == 4 * 2 * 48000 // 25


def test_formats_outside_the_definition_are_refused(dsm, lib):
    for rate, fmt, word in ((7999, R.F32, "outside 8000"), (48001, R.F32, "outside 8000"), (12345, R.S16, "whole number"), (16000, 4, "sample format")):
        assert not R.supported(rate) or fmt not in R.FORMATS
        for make in (dsm.egress_describe, dsm.egress_host):
            with pytest.raises(dsm.DsmError) as ei:
                make(rate, fmt)
            assert word in str(ei.value), str(ei.value)
    for rate in (8025, 12000, 47975):  # every rate that gives whole frames is inside the definition, not only the common ones
        assert R.supported(rate) and dsm.egress_describe(rate, R.F32)["F_out"] == 2 * rate // 25


@pytest.mark.parametrize("rate", R.RATES + (R.IN_RATE,))
def test_stream_is_the_whole_clip_result_delayed_by_the_latency(dsm, lib, rate):
    x = R.signal(FRAMES, seed=rate)
    got = _stream(dsm, rate, R.F32, x).view(np.float32)
    g = R.geometry(rate)
    D = 0 if rate == R.IN_RATE else R.TABLE[rate][5]
    y = dsm.resample(x, R.IN_RATE, rate)
    want = R.stream_of(y, D, FRAMES, g["F_out"])
    assert got.size == want.size == FRAMES * g["F_out"]
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{rate} Hz: {bad.size} samples differ, the first at {bad[:5]}"
    assert np.any(want[D:] != 0) and not _bits(got[:D]).any()
    # the other formats are the encoders over the same samples
    for fmt in (R.S16, R.MULAW, R.ALAW):
        assert np.array_equal(_stream(dsm, rate, fmt, x[:2 * R.FRAME]), R.encode(fmt, want[:2 * g["F_out"]])), (rate, fmt)


def _encode_all(dsm, fmt):
    return np.array([dsm.egress_encode_sample(fmt, s / 32768.0) for s in ALL_S16], dtype=np.int32)


def test_s16_encoder(dsm, lib):
    assert np.array_equal(_encode_all(dsm, R.S16), ALL_S16)
    nan, inf = float("nan"), float("inf")
    edges = [(1.0, 32767), (-1.0, -32768), (1.5 / 32768, 2), (2.5 / 32768, 2), (0.5 / 32768, 0), (-0.5 / 32768, 0), (-1.5 / 32768, -2),
             (nan, 0), (inf, 32767), (-inf, -32768), (-0.0, 0), (32766.5 / 32768, 32766), (32767.5 / 32768, 32767),
             (-32767.5 / 32768, -32768), (3e38, 32767), (-3e38, -32768), (1e-40, 0)]
    for v, want in edges:
        assert dsm.egress_encode_sample(R.S16, v) == want == R.s16_of(v), (v, want)
        for fmt in (R.MULAW, R.ALAW):
            assert dsm.egress_encode_sample(fmt, v) == R.encode_s16(fmt, want), (v, fmt)
    assert dsm.egress_encode_sample(R.F32, -0.0) == 0x80000000 and dsm.egress_encode_sample(R.F32, 0.25) == 0x3E800000


def test_g711_encoders_over_every_16_bit_value(dsm, lib):
    lin = ALL_S16.astype("<i2").tobytes()
    a, u = _encode_all(dsm, R.ALAW), _encode_all(dsm, R.MULAW)
    assert np.array_equal(a, [R.alaw_of(int(s)) for s in ALL_S16]) and np.array_equal(u, [R.ulaw_of(int(s)) for s in ALL_S16])
    assert np.array_equal(a, np.frombuffer(audioop.lin2alaw(lin, 2), dtype=np.uint8))
    pos = ALL_S16 >= 0
    assert np.array_equal(u[pos], np.frombuffer(audioop.lin2ulaw(lin, 2), dtype=np.uint8)[pos])
    by = dict(zip(ALL_S16.tolist(), u.tolist()))
    assert all(by[-s] == by[s] ^ 0x80 for s in range(1, 32768))
    # monotone: the expansion of the code never decreases with the sample
    for fmt, codes in ((R.MULAW, u), (R.ALAW, a)):
        table = dsm.ingest_g711_table(fmt).astype(np.int32)
        assert np.all(np.diff(table[codes]) >= 0)
        back = np.array([dsm.egress_encode_sample(fmt, int(t) / 32768.0) for t in table])  # round trip over all 256 bytes
        want = np.arange(256)
        if fmt == R.MULAW:
            want[0x7F] = 0xFF  # negative zero decodes to 0, which encodes as positive zero
        assert np.array_equal(back, want)


def test_engine_calls_refuse_a_null_engine_without_a_device(dsm, lib):
    buf = np.zeros(16, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.dsm_tts_set_egress(None, 1) == -1 and lib.dsm_tts_set_output_format(None, 0, 8000, R.MULAW) == -1
    assert lib.dsm_tts_output_format(None, 0, None, None, None, None, None) == -1
    assert lib.dsm_tts_step_raw(None, p, p, p, None, None, p, 16, None) == -1 and lib.dsm_tts_recv_raw(None, p, 16, None) == -1
    assert lib.dsm_tts_collect_raw(None, p, p, 16) == -1 and lib.dsm_tts_debug_egress(None, p, p, p, 16) == -1
    assert lib.dsm_egress_host(None, p, p) == -1 and lib.dsm_egress_describe(8000, R.MULAW, None) == -1
    assert lib.dsm_egress_encode_sample(4, 0.0, p) == -1 and lib.dsm_egress_encode_sample(R.S16, 0.0, None) == -1
    header = open(os.path.join(ROOT, "include", "dsm.h")).read()
    for name in ("dsm_tts_set_egress", "dsm_tts_step_raw", "dsm_tts_recv_raw", "dsm_tts_collect_raw", "dsm_egress_host", "dsm_egress_encode_sample"):
        assert name + "(" in header and name in dsm.ABI_SYMBOLS


def test_a_started_stream_switched_to_another_format_restarts_with_d_zeros(dsm, lib):
    """A switch is a new state (dsm_tts_set_output_format clears the history): nothing of the frames before it is heard."""
    x = R.signal(5, seed=77)
    a = dsm.egress_host(8000, R.MULAW)
    for e in range(2):
        a.step(x[e * R.FRAME:(e + 1) * R.FRAME])
    a.close()
    rest = x[2 * R.FRAME:]
    got = _stream(dsm, 16000, R.F32, rest).view(np.float32)
    D, f_out = R.TABLE[16000][5], R.TABLE[16000][4]
    want = R.stream_of(dsm.resample(rest, R.IN_RATE, 16000), D, 3, f_out)
    assert not _bits(got[:D]).any() and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_stream(dsm, 16000, R.ALAW, rest), R.encode(R.ALAW, want))
