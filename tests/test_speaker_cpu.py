"""CPU side of the speaker-encoder tests: the ABI of the three calls, the two references of tests/speaker_ref.py against each
other (so that the GPU test's reference is honest without a GPU), the properties of the fixtures without which the GPU test
could not tell right from wrong, the position table by hand, and the synthetic checkpoints left byte-identical."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest

import speaker_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsm_tts_attach_speaker_encoder", "dsm_tts_encode_voice", "dsm_tts_speaker_empty")
DSM_ERR_INVALID = -1


def test_the_three_calls_are_declared_exported_and_listed(dsm, lib):
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % s, hdr), f"{s} is not declared in include/dsm.h"
        assert s in dsm.ABI_SYMBOLS and hasattr(lib, s)
    assert "core/tts_streaming.rs:382-409" in hdr and "core/tts_streaming.rs:411-416" in hdr and "core/tts_streaming.rs:346-372" in hdr


def test_null_handles_are_refused_without_a_device(dsm, lib):
    buf, rows = np.zeros(8, dtype=np.float32), C.c_int(7)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.dsm_tts_attach_speaker_encoder(None, 2, b"x.safetensors") == DSM_ERR_INVALID
    assert lib.dsm_tts_encode_voice(None, p, 1, 1920, p, 1, C.byref(rows)) == DSM_ERR_INVALID
    assert lib.dsm_tts_speaker_empty(None, p, 1, C.byref(rows)) == DSM_ERR_INVALID
    assert rows.value == 7


@pytest.mark.parametrize("name", list(SR.CASES))
def test_r64_agrees_with_the_streaming_oracle(dsm, orc, name):
    """R64 against O within the project's own figure for this comparison (tests/test_oracle_vs_hf_mimi.py: 2e-4 * max(1, |x|max)
    on latents), and the input conditions of the fixture."""
    cs = SR.case(name)
    lat = cs.r64_latent
    print(f"{name}: latent noise {cs.noise_latent:.3e}, rows noise {cs.noise_rows:.3e}, |latent|max {np.abs(lat).max():.3f}")
    assert cs.noise_latent <= 2e-4 * max(1.0, float(np.abs(lat).max()))
    assert cs.noise_rows <= 2e-4 * max(1.0, float(np.abs(cs.r64_rows).max()))
    assert cs.noise_latent > 0 and cs.noise_rows > 0
    x = cs.clips.astype(np.float64)
    assert np.all(x.std(axis=1) > 0)
    r, c = cs.frames, cs.n_clips
    assert cs.r64_rows.shape == (cs.n_speakers * r, cs.cond)
    if cs.n_speakers > c:  # projected rows and padding rows differ (before the position table is added)
        pos = SR.pos_table_f64(cs.n_speakers * r, cs.cond)
        body = cs.r64_rows - pos
        assert np.abs(body[c * r:] - cs.pad[None, :]).max() < 1e-12
        assert np.abs(body[:c * r] - cs.pad[None, :]).max() > 0.1
    if c > 1:  # clips of different loudness and DC offset, both normalised to 0.08
        assert abs(x[0].std() / x[1].std() - 1) > 0.5 and abs(x[0].mean() - x[1].mean()) > 0.01
        assert np.allclose(cs.r64_pcm.std(axis=1), 0.08, rtol=1e-9)
        assert np.all(np.abs(cs.r64_pcm.mean(axis=1)) > 1e-4)  # the output is NOT mean-subtracted


def test_the_cases_cover_padding_and_no_padding():
    pads = [n_speakers > n_clips for (_, _, n_speakers, n_clips) in SR.CASES.values()]
    assert any(pads) and not all(pads)


def test_position_table_by_hand():
    """core/tts.rs:94-109 for rows 0, 1 and the last: pos_emb[j] = [cos(j f_i) | sin(j f_i)], f_i = 1 / 10000^(i / (half - 1)).
    cos(0) = 1 in the first half and sin(0) = 0 in the second catches a swapped concatenation."""
    rows, dim = 625, 128
    half = dim // 2
    t64, t32 = SR.pos_table_f64(rows, dim), SR.pos_table_f32(rows, dim)
    assert t64.shape == t32.shape == (rows, dim)
    assert np.all(t64[0, :half] == 1.0) and np.all(t64[0, half:] == 0.0)
    assert np.all(t32[0, :half] == 1.0) and np.all(t32[0, half:] == 0.0)
    for j in (1, rows - 1):
        for i in (0, 1, half // 2, half - 1):
            f = 1.0 / 10000.0 ** (i / (half - 1))
            # the table's angle is the f32 product of f32 factors: it is within j * 2^-22 of the exact one
            tol = j * 2.0 ** -22 + 2.0 ** -23
            assert abs(t64[j, i] - math.cos(j * f)) <= tol and abs(t64[j, half + i] - math.sin(j * f)) <= tol
            assert abs(float(t32[j, i]) - t64[j, i]) <= 2.0 ** -23 and abs(float(t32[j, half + i]) - t64[j, half + i]) <= 2.0 ** -23
    assert abs(t64[1, 0] - math.cos(1.0)) < 1e-15 and abs(t64[1, half] - math.sin(1.0)) < 1e-15  # f_0 = 1 exactly
    assert abs(t64[1, half - 1] - math.cos(1e-4)) < 1e-9                 # f_(half-1) = 1e-4


def test_synth_without_speaker_reproduces_the_existing_checkpoints(dsm, tmp_path):
    """Names are seeded per tensor and speaker=True only appends: tts_tiny / tts_tiny_ca keep the bytes they had before the
    speaker tensors existed (digests recorded from the previous synth.py)."""
    from dsm_amd import synth
    want = {"tts_tiny": "12c40a99996e29a8e78ccd6ca8176f02bd7fe6755d711fd6cc81e18112c88a89",
            "tts_tiny_ca": "d62d583776c4aaa57cfbce58d60dfebc423b4e3bf5d6505ad43e9d281a5c1985"}
    for tag, kw in (("tts_tiny", {}), ("tts_tiny_ca", {"cross_attention": True})):
        cfg = dsm.config_tts_tiny(**kw)
        path = synth.make_synth_tts_weights(cfg, str(tmp_path), tag=tag)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == want[tag], tag
        W = synth.read_safetensors(path)
        assert not any("speaker_wavs" in k for k in W)
    cfg = dsm.config_tts_tiny(cross_attention=True)
    spk = synth.make_synth_tts_weights(cfg, str(tmp_path), tag="tts_tiny_ca", speaker=True, mimi_dim=64)
    assert os.path.basename(spk) == "tts_tiny_ca_spk64.lm.safetensors"
    W, base = synth.read_safetensors(spk), synth.read_safetensors(os.path.join(str(tmp_path), "tts_tiny_ca.lm.safetensors"))
    p = "condition_provider.conditioners.speaker_wavs"
    assert W[p + ".output_proj.weight"].shape == (128, 64) and W[p + ".learnt_padding"].shape == (1, 1, 128)
    assert set(W) - set(base) == {p + ".output_proj.weight", p + ".learnt_padding"}
    for k in base:
        assert np.array_equal(W[k].view(np.uint32), base[k].view(np.uint32)), k
