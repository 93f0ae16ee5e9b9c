"""References and fixtures of the speaker-encoder tests (dsm_tts_encode_voice / dsm_tts_speaker_empty).

Two references, neither of which is the code under test:
  R64  a float64 torch restatement of the WHOLE-CLIP forward, written from the definitions: causal conv1d with zero / replicate
       left pad, ELU, resnet block, LayerNorm, interleaved RoPE, causal softmax attention, LayerScale, GELU MLP, downsample,
       projection, padding, position table.  It reads the synthetic safetensors through synth.read_safetensors.
  O    the existing CPU oracle driven as a stream (a fresh OracleAsr per clip, "mimi.latent" after every step) with numpy f32 for
       the normalisation, projection, padding and position table.  For T <= context a fresh stream and the whole-clip forward
       compute the same sums (tests/test_oracle_vs_hf_mimi.py explains why a ring wrap would not).
noise = max|O - R64| is the f32 rounding noise of an implementation already known good; the engine must stay within 4 x noise.

The position table is DEFINED in f32 (core/tts.rs:94-109: powf, an f32 quotient and product, cos / sin of the f32 angle), so both
references start from the same f32 angles, built with the C library's powf; R64 takes cos / sin of them in float64, the f32 table
uses the C library's cosf / sinf — the functions the engine's host code calls."""
import ctypes
import ctypes.util
import functools
import math
import os

import numpy as np

WDIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
FRAME = 1920
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("powf", "cosf", "sinf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * (2 if _n == "powf" else 1)


# ---------------------------------------------------------------------------------------------- position table
def pos_angles_f32(rows, dim):
    """freqs[j][i] = f32(j) * inv_freq[i], inv_freq[i] = 1f32 / 10000f32.powf(f32(i) / f32(half - 1)) — all f32."""
    half = dim // 2
    inv = np.array([np.float32(1.0) / np.float32(_libm.powf(10000.0, np.float32(i) / np.float32(half - 1))) for i in range(half)],
                   dtype=np.float32)
    return np.arange(rows, dtype=np.float32)[:, None] * inv[None, :]


def pos_table_f64(rows, dim):
    a = pos_angles_f32(rows, dim).astype(np.float64)
    return np.concatenate([np.cos(a), np.sin(a)], axis=1)  # cosines first


def pos_table_f32(rows, dim):
    a = pos_angles_f32(rows, dim)
    cos = np.array([_libm.cosf(float(v)) for v in a.ravel()], dtype=np.float32).reshape(a.shape)
    sin = np.array([_libm.sinf(float(v)) for v in a.ravel()], dtype=np.float32).reshape(a.shape)
    return np.concatenate([cos, sin], axis=1)


# ---------------------------------------------------------------------------------------------- R64
def normalize_f64(clips):
    x = np.asarray(clips, dtype=np.float64)
    sd = np.sqrt(np.mean((x - x.mean(axis=1, keepdims=True)) ** 2, axis=1, keepdims=True))
    return x * 0.08 / sd


def _conv(x, w, b, stride, replicate=False):
    """Causal conv1d of [C, T] (T a multiple of stride): left pad k - stride, zeros or the first frame repeated."""
    import torch
    import torch.nn.functional as F
    k = w.shape[2]
    pad = k - stride
    if pad > 0:
        left = x[:, :1].expand(-1, pad) if replicate else torch.zeros(x.shape[0], pad, dtype=x.dtype)
        x = torch.cat([left, x], dim=1)
    return F.conv1d(x[None], w, b, stride=stride)[0]


def _layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / (var + eps).sqrt() * w + b


def r64_latent(m, W, pcm_norm):
    """Mimi::encode_pre_quantize of one normalised clip [len] in float64, transposed: [r][dimension]."""
    import torch
    F = torch.nn.functional
    g = lambda name: torch.from_numpy(np.asarray(W[name], dtype=np.float64))
    conv = lambda x, p, stride: _conv(x, g(p + ".conv.conv.weight"), g(p + ".conv.conv.bias"), stride)
    x = torch.from_numpy(np.asarray(pcm_norm, dtype=np.float64))[None, :]  # [1, len]
    idx = 0
    x = conv(x, f"encoder.model.{idx}", 1)
    idx += 1
    for ratio in reversed([m.ratios[i] for i in range(m.n_ratios)]):
        assert m.n_residual_layers == 1
        y = conv(F.elu(x), f"encoder.model.{idx}.block.1", 1)
        x = x + conv(F.elu(y), f"encoder.model.{idx}.block.3", 1)
        idx += 1
        x = conv(F.elu(x), f"encoder.model.{idx + 1}", ratio)
        idx += 2
    x = conv(F.elu(x), f"encoder.model.{idx + 1}", 1)  # [dimension, T]
    t = m.transformer
    d, H = t.d_model, t.num_heads
    hd = d // H
    x = x.T.contiguous()  # [T, d]
    T = x.shape[0]
    assert T <= t.context and t.norm == 0 and not t.gating and t.positional_embedding == 1
    # RotaryEmbedding::new builds inv_freq in f32 (the definition); everything after it is float64 here
    inv = np.array([np.float32(1.0) / np.float32(_libm.powf(float(t.max_period), np.float32(i) / np.float32(hd))) for i in range(0, hd, 2)],
                   dtype=np.float32).astype(np.float64)
    ang = torch.from_numpy(np.arange(T, dtype=np.float64)[:, None] * inv[None, :])  # positions 0 .. T-1
    cos, sin = ang.cos()[:, None, :], ang.sin()[:, None, :]

    def rope(v):  # [T, H, hd], interleaved pairs
        a, b = v[..., 0::2], v[..., 1::2]
        return torch.stack([a * cos - b * sin, a * sin + b * cos], dim=-1).reshape(v.shape)

    causal = torch.ones(T, T, dtype=torch.bool).tril()
    for l in range(t.num_layers):
        p = f"encoder_transformer.transformer.layers.{l}"
        xn = _layer_norm(x, g(p + ".norm1.weight"), g(p + ".norm1.bias"))
        qkv = (xn @ g(p + ".self_attn.in_proj_weight").T).reshape(T, 3, H, hd)
        q, k, v = rope(qkv[:, 0]), rope(qkv[:, 1]), qkv[:, 2]
        s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(hd)
        s = s.masked_fill(~causal[None], float("-inf"))
        a = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v).reshape(T, d)
        x = x + (a @ g(p + ".self_attn.out_proj.weight").T) * g(p + ".layer_scale_1.scale")
        xn = _layer_norm(x, g(p + ".norm2.weight"), g(p + ".norm2.bias"))
        h = xn @ g(p + ".linear1.weight").T
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = x + (h @ g(p + ".linear2.weight").T) * g(p + ".layer_scale_2.scale")
    lat = _conv(x.T.contiguous(), g("downsample.conv.conv.conv.weight"), None, m.downsample_stride, replicate=True)
    return lat.T.numpy()  # [r, dimension]


def assemble(latents, proj, pad, n_speakers, pos):
    """[c][r][dim] latents -> [n_speakers * r][cond]: projected rows speaker-major, learnt_padding blocks, + pos_emb per flat row."""
    c, r = len(latents), latents[0].shape[0]
    rows = [lat @ proj.T for lat in latents]
    rows += [np.broadcast_to(pad.reshape(1, -1), (r, pad.size)).astype(proj.dtype)] * (n_speakers - c)
    out = np.concatenate(rows, axis=0)
    return out + pos[:out.shape[0]]


# ---------------------------------------------------------------------------------------------- fixtures
class Case:
    pass


def _clips(n, frames, seed):
    """Voice-like clips of different loudness and DC offset."""
    t = np.arange(frames * FRAME, dtype=np.float64) / 24000.0
    out = []
    for i in range(n):
        r = np.random.Generator(np.random.Philox(key=seed + i))
        x = (0.05 + 0.2 * i) * np.sin(2 * np.pi * (130 + 40 * i) * t) + (0.01 + 0.03 * i) * r.standard_normal(t.size) + (0.02 - 0.07 * i)
        out.append(x.astype(np.float32))
    return np.stack(out)


CASES = {  # name: (mimi fixture, frames, n_speakers, n_clips)
    "tiny_full_window": ("tiny", 5, 3, 2),
    "medium_ragged": ("medium", 13, 2, 2),
    "medium_real_length": ("medium", 125, 2, 1),
}


def mimi_fixture(dsm, which):
    """(AsrConfig whose Mimi has n_q = dep_num_slices of config_tts_tiny, lm path, mimi path)."""
    from dsm_amd import synth
    if which == "tiny":
        import tts_pcm_ref
        return tts_pcm_ref.mimi_setup(dsm)
    cfg = dsm.config_medium(mimi_context=250)
    cfg.mimi.quantizer_n_q = 6
    cfg.audio_codebooks = 6
    lm, mimi = synth.make_synth_weights(cfg, WDIR, tag="medium_nq6_ctx250")
    return cfg, lm, mimi


def tts_fixture(dsm, mimi_dim, ca_max_len=24, **kw):
    """config_tts_tiny with cross-attention (cond_dim = 128) and its checkpoint with the two speaker tensors."""
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny(cross_attention=True, **kw)
    cfg.ca_max_len = ca_max_len
    return cfg, synth.make_synth_tts_weights(cfg, WDIR, tag="tts_tiny_ca", speaker=True, mimi_dim=mimi_dim)


def speaker_tensors(tts_path):
    from dsm_amd import synth
    W = synth.read_safetensors(tts_path)
    p = "condition_provider.conditioners.speaker_wavs"
    return np.array(W[p + ".output_proj.weight"]), np.array(W[p + ".learnt_padding"]).reshape(-1)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and both references of one case, computed once per process."""
    import dsm_amd as dsm
    import oracle as orc
    from dsm_amd import synth
    orc.build()
    which, frames, n_speakers, n_clips = CASES[name]
    cs = Case()
    cs.name, cs.frames, cs.n_speakers, cs.n_clips = name, frames, n_speakers, n_clips
    cs.cfg_a, cs.lm_a, cs.mimi_a = mimi_fixture(dsm, which)
    m = cs.cfg_a.mimi
    cs.cfg_t, cs.tts_path = tts_fixture(dsm, m.dimension, ca_max_len=24 if which == "tiny" else 256)
    cs.cond = cs.cfg_t.ca_dim or cs.cfg_t.lm.d_model
    cs.clips = _clips(n_clips, frames, seed=77)
    proj, pad = speaker_tensors(cs.tts_path)
    cs.proj, cs.pad = proj, pad
    rows = n_speakers * frames
    # R64
    W = synth.read_safetensors(cs.mimi_a)
    cs.r64_pcm = normalize_f64(cs.clips)
    cs.r64_latent = np.stack([r64_latent(m, W, x) for x in cs.r64_pcm])  # [c][r][dim]
    cs.r64_rows = assemble(list(cs.r64_latent), proj.astype(np.float64), pad.astype(np.float64), n_speakers, pos_table_f64(rows, cs.cond))
    # O
    x = cs.clips
    sd = np.sqrt(np.mean((x - x.mean(axis=1, keepdims=True, dtype=np.float32)) ** 2, axis=1, keepdims=True, dtype=np.float32))
    cs.o_pcm = ((x * np.float32(0.08)) / sd).astype(np.float32)
    lat = np.zeros((n_clips, frames, m.dimension), dtype=np.float32)
    mask = np.ones(1, dtype=np.uint8)
    for i in range(n_clips):
        ora = orc.OracleAsr(cs.cfg_a, 1, cs.lm_a, cs.mimi_a)
        for s in range(frames):
            ora.encode_step(cs.o_pcm[i, s * FRAME:(s + 1) * FRAME][None, :], mask)
            lat[i, s] = ora.debug_read("mimi.latent", m.dimension)
        ora.close()
    cs.o_latent = lat
    cs.o_rows = assemble(list(lat), proj, pad, n_speakers, pos_table_f32(rows, cs.cond)).astype(np.float32)
    cs.noise_latent = float(np.abs(cs.o_latent - cs.r64_latent).max())
    cs.noise_rows = float(np.abs(cs.o_rows - cs.r64_rows).max())
    return cs
