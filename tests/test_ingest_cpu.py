"""Ingest on the host (csrc/dsm_pcm_format.h; no GPU): dsm_ingest_host, streamed frame by frame, delivers the whole-clip resampler's
output delayed by the format's latency D, bit for bit, for every supported rate and sample format, extremes and the start of the
stream included; D is the brute-force minimum and the kept history covers the brute-force reach; the G.711 tables are the
standard library's; the pass-through format returns its input bytes; what is outside the definition is refused with a message;
dsm_resample still gives the bits it gave before its phase-table builder moved (tests/golden/ingest, written by the library of
the commit before).  Floats are compared as uint32."""
import audioop
import os

import numpy as np
import pytest

import ingest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 7


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("rate", R.RATES + (47975,))  # and the rate with the most phases (L = 960)
def test_stream_is_the_whole_clip_result_delayed_by_the_latency(dsm, lib, rate):
    g = R.geometry(rate)
    for fmt in R.FORMATS:
        raw = R.noise_clip(rate, fmt, FRAMES, seed=rate + fmt)
        fb = g["F_in"] * R.SAMPLE_BYTES[fmt]
        h = dsm.ingest_host(rate, fmt)
        assert (h.frame_samples, h.frame_bytes, h.latency) == (g["F_in"], fb, g["D"])
        got = np.concatenate([h.step(raw[t * fb:(t + 1) * fb]) for t in range(FRAMES)])
        h.close()
        x = R.decode(fmt, raw)
        y = dsm.resample(x, rate, R.OUT_RATE)
        want = R.stream_of(y, g["D"], FRAMES)
        bad = np.flatnonzero(_bits(got) != _bits(want))
        assert bad.size == 0, f"{rate} Hz format {fmt}: {bad.size} samples differ, the first at {bad[:5]}"
        if fmt == R.F32 and rate == R.OUT_RATE:  # the pass-through format: the input's bytes, NaN payloads and all
            odd = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0x00000001, 0x80000000], dtype=np.uint32)
            frame = np.zeros(R.FRAME, dtype=np.uint32)
            frame[:odd.size] = odd
            p = dsm.ingest_host(rate, fmt)
            assert p.step(frame.tobytes()).tobytes() == frame.tobytes()
            p.close()
    # a stream of silence is +0.0 throughout: the zeros of the history and of the input add +-0.0 to an accumulator that began at +0.0
    h = dsm.ingest_host(rate, R.S16)
    z = np.concatenate([h.step(bytes(2 * g["F_in"])) for _ in range(2)])
    assert not _bits(z).any()


@pytest.mark.parametrize("rate", R.RATES)
def test_latency_and_history_are_the_brute_force_minimum(dsm, lib, rate):
    """D: the smallest latency for which no tap of a frame reaches input not yet received.  The history a step reads: at most
    `taps` samples in front of its frame — the depth the state keeps — and, from D = floor(half L / M) and M / L <= 2, at least
    taps - 2, so no smaller round depth would do."""
    info = dsm.ingest_describe(rate, R.F32)
    g = R.geometry(rate)
    for k in ("L", "M", "half", "taps", "F_in", "D"):
        assert info[k] == g[k], (k, info[k], g[k])
    assert info["table_words"] == (g["L"] * g["taps"] if g["taps"] else 0)
    if rate == R.OUT_RATE:
        assert info["D"] == 0 and info["taps"] == 0
        return
    D, reach = R.brute_force(rate)
    assert info["D"] == D
    assert info["taps"] - 2 <= reach <= info["taps"], (reach, info["taps"])
    assert reach == -((-D * g["M"]) // g["L"]) + g["half"] - 1


def test_the_issue_latency_table(dsm, lib):
    assert [dsm.ingest_describe(r, R.F32)["D"] for r in (8000, 16000, 44100, 48000)] == [102, 51, 33, 34]
    assert [dsm.ingest_describe(r, R.F32)["taps"] for r in (8000, 16000, 44100, 48000)] == [68, 68, 124, 136]
    assert dsm.ingest_describe(8000, R.MULAW)["frame_bytes"] == 640 and dsm.ingest_describe(48000, R.F32)["frame_bytes"] == 15360


def test_g711_tables_are_the_standard_librarys(dsm, lib):
    every = bytes(range(256))
    for fmt, lin in ((R.MULAW, audioop.ulaw2lin), (R.ALAW, audioop.alaw2lin)):
        want = np.frombuffer(lin(every, 2), dtype="<i2")
        assert np.array_equal(dsm.ingest_g711_table(fmt), want)
        assert np.array_equal([(R.ulaw_to_s16 if fmt == R.MULAW else R.alaw_to_s16)(b) for b in range(256)], want)


def test_unsupported_rates_and_formats_are_refused_with_a_message(dsm, lib):
    for rate, fmt, word in ((7999, R.F32, "outside 8000"), (48025, R.F32, "outside 8000"), (8001, R.S16, "whole number"),
                            (44101, R.F32, "whole number"), (16000, 4, "sample format"), (16000, -1, "sample format"), (0, R.F32, "outside")):
        assert not R.supported(rate) or fmt not in R.FORMATS
        for make in (dsm.ingest_describe, dsm.ingest_host):
            with pytest.raises(dsm.DsmError) as ei:
                make(rate, fmt)
            assert word in str(ei.value), str(ei.value)
    h = dsm.ingest_host(8000, R.MULAW)
    with pytest.raises(dsm.DsmError):
        h.step(bytes(639))  # a frame shorter than the format's
    # every rate that gives whole frames is inside the definition, not only the common ones
    for rate in (8025, 12000, 47975):
        assert R.supported(rate) and dsm.ingest_describe(rate, R.F32)["F_in"] == 2 * rate // 25


@pytest.mark.parametrize("rate", (8000, 44100, 48000))
def test_dsm_resample_gives_the_bits_of_the_commit_before(dsm, lib, rate):
    rng = np.random.RandomState(20261021 + rate)
    x = (rng.standard_normal(3000) * 0.3).astype(np.float32)
    x[:4] = [1.0, -1.0, 0.0, 1e-40]
    want = np.fromfile(os.path.join(ROOT, "tests", "golden", "ingest", f"resample_{rate}_to_24000.f32"), dtype="<f4")
    got = dsm.resample(x, rate, R.OUT_RATE)
    assert got.size == want.size and np.array_equal(_bits(got), _bits(want))


def test_worker_with_a_callers_backend_takes_24_khz_only(dsm, lib):
    """dsm_worker_set_input_rate on a worker built with dsm_worker_create_with_backend: DSM_ERR_STATE, like dsm_worker_set_word_scores."""
    be = dsm.WorkerBackend()
    be.batch_size, be.asr_delay_in_tokens, be.extra_heads_num = 2, 2, 0
    cbs = (dsm.BE_ENCODE(lambda *_: 0), dsm.BE_RESET(lambda *_: 0), dsm.BE_STEP(lambda *_: 0), dsm.BE_POLL(lambda *_: 0))
    be.encode_step, be.reset_slot, be.step_tokens, be.poll_msgs = cbs
    w = dsm.Worker(backend=be)
    slot = w.open()
    with pytest.raises(dsm.DsmError) as ei:
        w.set_input_rate(slot, 8000)
    assert ei.value.code == -4 and "backend" in str(ei.value)
    w.close()


def test_python_constants_are_the_headers(dsm):
    header = open(os.path.join(ROOT, "include", "dsm.h")).read()
    for name, value in (("F32", dsm.PCM_F32), ("S16", dsm.PCM_S16), ("MULAW", dsm.PCM_MULAW), ("ALAW", dsm.PCM_ALAW)):
        assert "#define DSM_PCM_%s %d\n" % (name, value) in header
    assert (R.F32, R.S16, R.MULAW, R.ALAW) == (dsm.PCM_F32, dsm.PCM_S16, dsm.PCM_MULAW, dsm.PCM_ALAW)
    assert dsm.INGEST_MAX_FRAME_BYTES == 4 * 2 * 48000 // 25
