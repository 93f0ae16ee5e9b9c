"""GPU tests of the speaker encoder: dsm_tts_attach_speaker_encoder / dsm_tts_encode_voice / dsm_tts_speaker_empty
(SpeakerEncoder::{new, encode, empty}, core/tts_streaming.rs:346-416).

The encoder is TOLERANCE-pinned (the oracle has only the streaming Mimi): with R64 the float64 whole-clip restatement and O the
streaming oracle of tests/speaker_ref.py, noise = max|O - R64| and the engine's rows and latents must satisfy
max|E - R64| <= 4 x noise (the engine's attention sums in a third order; f32 chains of this depth differ by small factors between
orders).  The normalised clip has a derivable bound: relative error against the float64 normalisation of at most
(log2(clip_len) + 4) x 2^-24.  Determinism is exact.

Measured on an MI355X (every case prints its figures before it asserts; DESIGN.md section 5.2 keeps the table):
  case                 rows: noise / engine      latent: noise / engine    pcm_norm rel. err (bound)
  tiny_full_window     6.303e-07 / 6.994e-07     7.701e-07 / 8.297e-07     1.560e-07 (1.027e-06)
  medium_ragged        8.222e-07 / 8.830e-07     8.599e-07 / 8.763e-07     1.683e-07 (1.109e-06)
  medium_real_length   8.363e-07 / 8.100e-07     7.891e-07 / 7.891e-07     1.748e-07 (1.304e-06)
speaker_empty: all 375 rows bit-equal to the reference table."""
import numpy as np
import pytest

import speaker_ref as SR
import tts_pcm_ref as R

pytestmark = pytest.mark.gpu
DSM_ERR_INVALID, DSM_ERR_IO, DSM_ERR_STATE = -1, -2, -4


def _engine(dsm, cs, B=1):
    eng = dsm.TtsEngine(cs.cfg_t, B, cs.tts_path)
    eng.attach_mimi(cs.cfg_a.mimi, cs.mimi_a)
    eng.attach_speaker_encoder(cs.n_speakers, cs.tts_path)
    return eng


@pytest.mark.parametrize("name", list(SR.CASES))
def test_encode_voice_against_the_two_references(gpu, dsm, lib, orc, name):
    """1 tiny, full window (head_dim 32, T = 10 = context, one padding block); 2 medium, ragged tile (head_dim 64, T = 26);
    3 medium at the real sequence length (T = 250 = context, 240 000-row convolutions, one clip of two speakers)."""
    cs = SR.case(name)
    assert cs.noise_rows > 0 and cs.noise_latent > 0
    eng = _engine(dsm, cs)
    rows = eng.encode_voice(cs.clips)
    c, r, dim, n = cs.n_clips, cs.frames, cs.cfg_a.mimi.dimension, cs.frames * SR.FRAME
    assert rows.shape == (cs.n_speakers * r, cs.cond) and np.all(np.isfinite(rows))
    pcm = eng.debug_read("spk.pcm_norm", c * n).reshape(c, n)
    lat = eng.debug_read("spk.latent", c * r * dim).reshape(c, r, dim)
    eng.close()
    bound = (np.log2(n) + 4) * 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(pcm - cs.r64_pcm) / np.abs(cs.r64_pcm)
    e_lat, e_rows = float(np.abs(lat - cs.r64_latent).max()), float(np.abs(rows - cs.r64_rows).max())
    print(f"{name}: pcm_norm rel err {np.nanmax(rel):.3e} (bound {bound:.3e}); latent noise {cs.noise_latent:.3e} engine {e_lat:.3e}; "
          f"rows noise {cs.noise_rows:.3e} engine {e_rows:.3e}")
    assert np.all(np.abs(pcm - cs.r64_pcm) <= bound * np.abs(cs.r64_pcm)), "spk.pcm_norm outside its bound"
    assert e_lat <= 4 * cs.noise_latent, f"spk.latent: {e_lat:.3e} > 4 x {cs.noise_latent:.3e}"
    assert e_rows <= 4 * cs.noise_rows, f"rows: {e_rows:.3e} > 4 x {cs.noise_rows:.3e}"


def test_speaker_empty(gpu, dsm, lib, orc):
    """n_speakers * 125 rows of learnt_padding + pos_emb: one f32 add of values both sides compute with the C library's f32
    functions, so equal to 1 ulp of the sum."""
    cs = SR.case("tiny_full_window")
    eng = _engine(dsm, cs)
    got = eng.speaker_empty()
    eng.close()
    n = cs.n_speakers * 125
    assert got.shape == (n, cs.cond)
    pos = SR.pos_table_f32(n, cs.cond)
    pad = np.broadcast_to(cs.pad.astype(np.float32)[None, :], pos.shape)
    want = pad + pos
    ulp = np.spacing(np.abs(want).astype(np.float32))
    print(f"speaker_empty: max |diff| {np.abs(got - want).max():.3e}, exact rows {int(np.all(got == want, axis=1).sum())} of {n}")
    assert np.all(np.abs(got - want) <= ulp)


def test_determinism_and_non_interference(gpu, dsm, lib, orc):
    """An engine with a Mimi attached runs the first half of tts_pcm_ref.plan's schedule through step_pcm, encodes a voice
    (twice), and runs the rest: tokens, valid flags and PCM equal a run without the encode bit for bit, and the two encodes are
    byte-identical."""
    cs = SR.case("tiny_full_window")
    steps, resets = R.plan(cs.cfg_t)
    runs = []
    for with_encode in (False, True):
        eng = _engine(dsm, cs, B=R.B)
        out = []
        for s, (prev, allowed, mask) in enumerate(steps):
            if with_encode and s == len(steps) // 2:
                a, b = eng.encode_voice(cs.clips), eng.encode_voice(cs.clips)
                assert a.tobytes() == b.tobytes(), "two encodes of the same clips differ"
                assert np.abs(a - cs.r64_rows).max() <= 4 * cs.noise_rows
            for slot in resets.get(s, []):
                eng.reset_batch_idx(slot)
            out.append(eng.step_pcm(prev, allowed, mask))
        assert eng.metrics().capture_failures == 0
        eng.close()
        runs.append(out)
    emitted = 0
    for s, (x, y) in enumerate(zip(*runs)):
        for k, (u, v) in enumerate(zip(x, y)):
            assert u.tobytes() == v.tobytes(), f"step {s}: output {k} (text, audio, pcm, valid) differs after an encode"
        emitted += int(x[3].sum())
    assert emitted >= 20  # (the comparison covers real frames)


def test_end_to_end_rows_feed_the_cross_attention(gpu, dsm, lib, orc):
    """encode_voice + speaker_empty -> set_ca_src(slot, rows, uncond, cfg_alpha) on a cfg_rows engine: six steps of tokens equal
    OracleTts.set_ca_src given the same arrays (the engine's own output): the plumbing and the row counts, not the encoder again."""
    from tts_schedule import schedule
    cs = SR.case("tiny_full_window")
    cfg, path = SR.tts_fixture(dsm, cs.cfg_a.mimi.dimension, ca_max_len=128, cfg_rows=True)
    B = 2
    eng, ora = dsm.TtsEngine(cfg, B, path), orc.OracleTts(cfg, B, path)
    eng.attach_mimi(cs.cfg_a.mimi, cs.mimi_a)
    eng.attach_speaker_encoder(1, path)
    rows, empty = eng.encode_voice(cs.clips), eng.speaker_empty()
    assert rows.shape == (cs.frames, cs.cond) and empty.shape == (125, cs.cond)
    for x in (eng, ora):
        x.set_ca_src(0, rows, empty, 2.0)
        x.set_ca_src(1, rows)
    for s, (prev, allowed, mask) in enumerate(schedule(cfg, B, 6)):
        (te, ae), (to, ao) = eng.step(prev, allowed, mask), ora.step(prev, allowed, mask)
        act = mask.astype(bool)
        assert np.array_equal(te[act], to[act]) and np.array_equal(ae[act], ao[act]), f"tokens differ at step {s}"
    eng.close(); ora.close()


def test_refusals_leave_the_engine_usable(gpu, dsm, lib, orc):
    from dsm_amd import synth
    cs = SR.case("tiny_full_window")
    lib_ = dsm.load_library()
    # no cross-attention
    plain_cfg, plain_path = R.tts_setup(dsm)
    plain = dsm.TtsEngine(plain_cfg, 1, plain_path)
    plain.attach_mimi(cs.cfg_a.mimi, cs.mimi_a)
    assert lib_.dsm_tts_attach_speaker_encoder(plain.h, 2, cs.tts_path.encode()) == DSM_ERR_STATE
    with pytest.raises(dsm.DsmError, match="cross_attention"):
        plain.attach_speaker_encoder(2, cs.tts_path)
    plain.close()
    eng = dsm.TtsEngine(cs.cfg_t, 1, cs.tts_path)
    # no Mimi
    assert lib_.dsm_tts_attach_speaker_encoder(eng.h, 2, cs.tts_path.encode()) == DSM_ERR_STATE
    with pytest.raises(dsm.DsmError, match="dsm_tts_attach_mimi"):
        eng.attach_speaker_encoder(2, cs.tts_path)
    eng.attach_mimi(cs.cfg_a.mimi, cs.mimi_a)
    with pytest.raises(dsm.DsmError, match="n_speakers"):
        eng.attach_speaker_encoder(0, cs.tts_path)
    # a checkpoint without the two keys
    _, no_keys = R.tts_setup(dsm, cross_attention=True)
    assert lib_.dsm_tts_attach_speaker_encoder(eng.h, 3, no_keys.encode()) == DSM_ERR_IO
    with pytest.raises(dsm.DsmError, match="speaker_wavs"):
        eng.attach_speaker_encoder(3, no_keys)
    with pytest.raises(dsm.DsmError, match="attach_speaker_encoder first"):
        eng.encode_voice(cs.clips)
    eng.attach_speaker_encoder(3, cs.tts_path)
    # second attach
    assert lib_.dsm_tts_attach_speaker_encoder(eng.h, 3, cs.tts_path.encode()) == DSM_ERR_STATE
    with pytest.raises(dsm.DsmError, match="attached already"):
        eng.attach_speaker_encoder(3, cs.tts_path)
    with pytest.raises(dsm.DsmError, match="multiple of 1920"):
        eng.encode_voice(cs.clips[:, :5 * 1920 - 7])
    with pytest.raises(dsm.DsmError, match="context"):  # T = 12 > context = 10
        eng.encode_voice(np.concatenate([cs.clips, cs.clips[:, :1920]], axis=1))
    out, rows = np.zeros((4, cs.cond), dtype=np.float32), dsm.C.c_int(0)
    a = np.ascontiguousarray(cs.clips)
    rc = lib_.dsm_tts_encode_voice(eng.h, a.ctypes.data_as(dsm.C.c_void_p), 2, a.shape[1], out.ctypes.data_as(dsm.C.c_void_p), 4,
                                   dsm.C.byref(rows))
    assert rc == DSM_ERR_INVALID and rows.value == 15 and b"15 rows" in lib_.dsm_tts_last_error(eng.h)
    rc = lib_.dsm_tts_encode_voice(eng.h, a.ctypes.data_as(dsm.C.c_void_p), 0, a.shape[1], out.ctypes.data_as(dsm.C.c_void_p), 4,
                                   dsm.C.byref(rows))
    assert rc == DSM_ERR_INVALID and b"empty speakers in encode" in lib_.dsm_tts_last_error(eng.h)
    silent = cs.clips.copy()
    silent[1] = 0.0
    with pytest.raises(dsm.DsmError, match="clip 1: standard deviation"):
        eng.encode_voice(silent)
    # ... and the engine still encodes
    rows = eng.encode_voice(cs.clips)
    assert np.abs(rows - cs.r64_rows).max() <= 4 * cs.noise_rows
    eng.close()
