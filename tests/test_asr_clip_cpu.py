"""The clips section on the host (include/dsm.h "clips"; csrc/dsm_asr_clip.h), no device: dsm_asr_clip_frame_host against the
independent cut of tests/clip_ref.py for the four sample formats at 8000, 11025, 24000 and 44100 Hz and clips of 0 bytes, 1 byte,
one frame, one frame - 1 and + 1 byte, and 5 frames + 7 bytes; the two G.711 silence bytes through dsm_ingest_g711_table; and the
schedule dsm_asr_run goes through (dsm_asr_clip_host_*) — frame index, mask and status per step — for begin / push / close
sequences, WAITING included."""
import numpy as np
import pytest

import clip_ref as R

RATES = (8000, 11025, 24000, 44100)
FORMATS = (R.F32, R.S16, R.MULAW, R.ALAW)


def clip_lengths(fb):
    return (0, 1, fb, fb - 1, fb + 1, 5 * fb + 7)


def clip_of(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rate", RATES)
def test_frame_host_is_the_reference_cut(dsm, lib, rate, fmt):
    fb = R.frame_bytes(rate, fmt)
    assert dsm.ingest_describe(rate, fmt)["frame_bytes"] == fb
    for n in clip_lengths(fb):
        clip = clip_of(n, 31 * rate + fmt + n)
        for i in range(R.n_audio(n, rate, fmt) + 3):  # every audio frame and three of the silence behind it
            got = dsm.asr_clip_frame_host(clip, rate, fmt, i)
            assert len(got) == fb
            assert got == R.frame(clip, rate, fmt, i), (rate, fmt, n, i)
    # far behind the clip, where index * frame_bytes no longer fits 32 bits: silence
    assert dsm.asr_clip_frame_host(clip_of(fb + 1, 5), rate, fmt, (1 << 40) + 3) == bytes([R.SILENCE[fmt]]) * fb


def test_frame_host_refuses_what_is_no_format(dsm, lib):
    for rate, fmt in ((8001, R.F32), (7999, R.S16), (8000, 7), (96000, R.F32)):
        with pytest.raises(dsm.DsmError):
            dsm.asr_clip_frame_host(b"\0" * 16, rate, fmt, 0)


def test_g711_silence_bytes_expand_to_silence(dsm, lib):
    """0xFF is mu-law's zero; A-law has no zero and 0xD5, its idle code, is the smallest positive value, +8"""
    mu, al = dsm.ingest_g711_table(dsm.PCM_MULAW), dsm.ingest_g711_table(dsm.PCM_ALAW)
    assert R.SILENCE[R.MULAW] == 0xFF and mu[0xFF] == 0
    assert R.SILENCE[R.ALAW] == 0xD5 and al[0xD5] == 8 and min(abs(int(v)) for v in al) == 8
    for fmt, byte in ((dsm.PCM_MULAW, 0xFF), (dsm.PCM_ALAW, 0xD5), (dsm.PCM_S16, 0x00), (dsm.PCM_F32, 0x00)):
        assert dsm.asr_clip_frame_host(b"", 8000, fmt, 0) == bytes([byte]) * R.frame_bytes(8000, fmt)
    # a silent frame goes through ingest as a frame of zeros (A-law: of +8 / 32768)
    for fmt, want in ((dsm.PCM_MULAW, 0.0), (dsm.PCM_S16, 0.0), (dsm.PCM_F32, 0.0), (dsm.PCM_ALAW, 8 / 32768)):
        out = dsm.ingest_host(24000, fmt).step(dsm.asr_clip_frame_host(b"", 24000, fmt, 0))
        assert np.all(out == np.float32(want))


def both(dsm, B, cap):
    return dsm.asr_clip_host(B, cap), R.Schedule(B, cap)


def same_run(host, ref, n):
    (hf, hm), (rf, rm) = host.run(n), ref.run(n)
    assert np.array_equal(hm, rm), (hm, rm)
    assert np.array_equal(hf[rm == 1], rf[rm == 1])
    assert [host.status(b) for b in range(ref.B)] == [ref.status(b) for b in range(ref.B)]
    return rf, rm


def test_schedule_of_closed_clips(dsm, lib):
    """the four clips of the GPU scenario: 3 frames + 7 samples, exactly 2 frames, 5 frames + 1 byte, nothing"""
    B, flush = 4, 3
    host, ref = both(dsm, B, 1 << 20)
    clips = [(24000, R.F32, 3 * 7680 + 28), (8000, R.MULAW, 2 * 640), (11025, R.MULAW, 5 * 882 + 1), (44100, R.S16, 0)]
    for b, (rate, fmt, n) in enumerate(clips):
        for s in (host, ref):
            s.begin(b, rate, fmt, flush)
            s.push(b, n)
            s.close(b)
    assert [host.status(b) for b in range(B)] == [R.RUNNING] * B
    frame, mask = same_run(host, ref, 16)
    assert mask.sum(axis=0).tolist() == [4 + flush, 2 + flush, 6 + flush, 0 + flush]
    for b in range(B):
        taken = frame[mask[:, b] == 1, b]
        assert taken.tolist() == list(range(len(taken)))  # frames 0, 1, 2, ... in consecutive steps from the first
        assert mask[:len(taken), b].all()
    assert [host.status(b) for b in range(B)] == [R.DONE] * B
    _, mask = same_run(host, ref, 2)
    assert not mask.any()
    host.free()


def test_schedule_waits_for_whole_frames_and_resumes(dsm, lib):
    B, fb = 2, 640
    host, ref = both(dsm, B, 10 * fb)
    for s in (host, ref):
        s.begin(0, 8000, R.MULAW, 1)
        s.push(0, fb + fb // 2)  # one and a half frames, open
    _, mask = same_run(host, ref, 3)
    assert mask[:, 0].tolist() == [1, 0, 0] and host.status(0) == R.WAITING and host.status(1) == R.IDLE
    for s in (host, ref):
        s.push(0, 1)  # still no whole frame
    assert host.status(0) == R.RUNNING
    _, mask = same_run(host, ref, 1)
    assert mask[:, 0].tolist() == [0] and host.status(0) == R.WAITING
    for s in (host, ref):
        s.push(0, fb // 2)  # 2 frames + 1 byte
    frame, mask = same_run(host, ref, 2)
    assert mask[:, 0].tolist() == [1, 0] and frame[0, 0] == 1
    for s in (host, ref):
        s.close(0)  # the last byte's frame and one flush frame follow
    assert host.status(0) == R.RUNNING
    frame, mask = same_run(host, ref, 4)
    assert mask[:, 0].tolist() == [1, 1, 0, 0] and frame[:2, 0].tolist() == [2, 3] and host.status(0) == R.DONE
    host.free()


def test_schedule_refusals_change_nothing(dsm, lib):
    host, ref = both(dsm, 2, 1000)
    with pytest.raises(dsm.DsmError):
        host.push(0, 1)      # no clip
    with pytest.raises(dsm.DsmError):
        host.close(0)
    host.begin(0, 8000, R.MULAW, 0); ref.begin(0, 8000, R.MULAW, 0)
    with pytest.raises(dsm.DsmError):
        host.begin(0, 8000, R.MULAW, 0)  # has a clip already
    with pytest.raises(dsm.DsmError):
        host.begin(1, 8000, R.MULAW, -1)
    with pytest.raises(dsm.DsmError):
        host.begin(1, 8001, R.MULAW, 0)
    host.push(0, 700); ref.push(0, 700)
    with pytest.raises(dsm.DsmError):
        host.push(0, 301)    # beyond the cap
    host.push(0, 300); ref.push(0, 300)
    with pytest.raises(dsm.DsmError):
        host.run(0)
    with pytest.raises(dsm.DsmError):
        host.run(R.RUN_MAX + 1)
    host.close(0); ref.close(0)
    host.close(0)            # twice is fine
    with pytest.raises(dsm.DsmError):
        host.push(0, 1)      # closed
    _, mask = same_run(host, ref, 3)
    assert mask[:, 0].tolist() == [1, 1, 0]
    host.reset(0); ref.reset(0)
    assert host.status(0) == R.IDLE
    host.begin(0, 44100, R.S16, 2); ref.begin(0, 44100, R.S16, 2)
    host.close(0); ref.close(0)  # an empty clip: the flush alone
    _, mask = same_run(host, ref, 3)
    assert mask[:, 0].tolist() == [1, 1, 0] and host.status(0) == R.DONE
    host.free()


def test_abi_lists_the_section(dsm, lib):
    for name in ("dsm_asr_set_clips", "dsm_asr_clip_begin", "dsm_asr_clip_push", "dsm_asr_clip_close", "dsm_asr_run", "dsm_asr_collect",
                 "dsm_asr_clip_status", "dsm_asr_clip_frame_host"):
        assert name in dsm.ABI_SYMBOLS and hasattr(lib, name)
