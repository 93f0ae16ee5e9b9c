"""numpy reference for the TTS conditioners (core/conditioner.rs:31-176): the row a slot's Condition::AddToInput adds to the
input embedding sum, and that sum itself (core/tts_streaming.rs:126-158 input assembly, core/lm.rs:983-1000).

The engine's dot product is ONE f32 fma chain per output element over k ascending from 0.  chain() restates it as
acc = f32(acc + f32(a) * f32(w)): for a BF16 checkpoint a bf16 x bf16 product has at most 16 significant bits, so the f32
product is exact and the sum rounds once per term, exactly like the fma — the comparison is bit for bit."""
import json
import struct

import numpy as np

from dsm_amd import synth

CONDS = [
    dict(name="description", type="Lut", n_bins=31, dim=16, possible_values=["very_bad", "bad", "neutral", "good", "very_good"]),
    dict(name="tail", type="Lut", n_bins=4, dim=5, possible_values=["a", "b", "c", "d", "e"]),  # dim 5: no multiple of anything
    dict(name="speed", type="ContinuousAttribute", dim=8, scale_factor=10.0, max_period=100.0),
]


class Rows:
    """A [rows][width] table of a BF16 file, left on disk: t[i] is row i as f32 (the served embedding tables are 600 MB as f32)."""

    def __init__(self, bits):
        self.bits = bits

    def __getitem__(self, i):
        return synth.bf16_bits_to_f32(np.array(self.bits[i]))


def read_tensors(path, want, lazy=False):
    """{name: f32 ndarray} of the tensors whose name `want(name)` accepts (synth.read_safetensors converts a whole file).
    lazy: BF16 tensors come back as Rows."""
    with open(path, "rb") as f:
        (hlen,) = struct.unpack("<Q", f.read(8))
        header = json.loads(f.read(hlen))
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    out = {}
    for name, meta in header.items():
        if name == "__metadata__" or not want(name):
            continue
        a, b = meta["data_offsets"]
        raw = mm[8 + hlen + a:8 + hlen + b]
        if meta["dtype"] == "BF16":
            bits = raw.view(np.uint16).reshape(meta["shape"])
            out[name] = Rows(bits) if lazy else synth.bf16_bits_to_f32(np.array(bits))
        else:
            assert meta["dtype"] == "F32", meta["dtype"]
            out[name] = np.array(raw.view(np.float32)).reshape(meta["shape"])
    return out


def cond_tensors(path):
    return read_tensors(path, lambda n: n.startswith("condition_provider.conditioners."))


def bf16_round(a):
    """f32 -> bf16 (round to nearest even) -> f32."""
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(np.asarray(a, dtype=np.float32)))


def chain(x, W):
    """row[j] = fma chain over k ascending from 0 of x[k] * W[j][k], in f32."""
    x, W = np.asarray(x, dtype=np.float32), np.asarray(W, dtype=np.float32)
    acc = np.zeros(W.shape[0], dtype=np.float32)
    for k in range(W.shape[1]):
        acc = (acc + np.float32(x[k]) * W[:, k]).astype(np.float32)
    return acc


def _key(c, leaf):
    return f"condition_provider.conditioners.{c['name']}.{leaf}"


def lut_row(tensors, c, value):
    """condition_lut: embed.weight[position of value] through output_proj."""
    idx = c["possible_values"].index(value)
    return chain(tensors[_key(c, "embed.weight")][idx], tensors[_key(c, "output_proj.weight")])


def padding_row(tensors, c):
    return tensors[_key(c, "learnt_padding")].reshape(-1).astype(np.float32)


def sin_embedding(c, value):
    """create_sin_embeddings in float64: [cos(v a_i) ..., sin(v a_i) ...], v = value * scale_factor, a_i = max_period^(-i / (half - 1)).
    value and scale_factor are taken as the f32 numbers the C ABI carries."""
    half = c["dim"] // 2
    v = float(np.float32(value)) * float(np.float32(c["scale_factor"]))
    a = np.array([1.0 / float(np.float32(c["max_period"])) ** (i / (half - 1)) for i in range(half)], dtype=np.float64)
    return np.concatenate([np.cos(v * a), np.sin(v * a)])


def cont_row_f64(tensors, c, value):
    """condition_cont evaluated in float64 (no bf16 rounding of the embedding), and the bound of the engine's row on it, per
    element: sum_k |W[j][k]| |e_k| 2^-8 (one bf16 ulp on every input, in case a near-tie rounds the other way) +
    dim 2^-24 sum_k |W[j][k] e_k| (the f32 chain)."""
    e = sin_embedding(c, value)
    W = tensors[_key(c, "output_proj.weight")].astype(np.float64)
    terms = np.abs(W) * np.abs(e)[None, :]
    bound = terms.sum(axis=1) * 2.0 ** -8 + c["dim"] * 2.0 ** -24 * terms.sum(axis=1)
    return W @ e, bound


def cont_row_chain(tensors, c, value):
    """The engine's recipe: the float64 embedding rounded to f32, then to bf16, through the f32 chain."""
    return chain(bf16_round(sin_embedding(c, value).astype(np.float32)), tensors[_key(c, "output_proj.weight")])


def emb_tables(path, cfg):
    t = read_tensors(path, lambda n: n == "text_emb.weight" or (n.startswith("emb.") and n.endswith(".weight")), lazy=True)
    return t["text_emb.weight"], [t[f"emb.{i}.weight"] for i in range(cfg.audio_codebooks)]


def plain_input_row(cfg, tables, prev_text, step, audio_table):
    """The input embedding sum of State::step for a slot at step index `step`, without a condition: the text row, then the
    audio rows in codebook order, f32 adds; None entries are skipped.  audio_table(i) = the slot's audio_tokens[i]."""
    text_emb, audio_emb = tables
    S, nc, ad, tad = cfg.dep_num_slices, cfg.audio_codebooks, cfg.acoustic_delay, cfg.text_audio_delay_in_tokens
    pad = cfg.audio_vocab_size - 1
    e = text_emb[int(prev_text) if int(prev_text) < cfg.text_in_vocab_size else 0].astype(np.float32)
    for cb in range(min(S, nc)):
        if cb == 0:
            if step == 0:
                tok = pad
            elif step <= tad:
                continue
            else:
                tok = int(audio_table(step - 1)[0])
        elif step <= ad:
            tok = pad
        elif step <= tad + ad:
            continue
        else:
            tok = int(audio_table(step - ad - 1)[cb])
        e = (e + audio_emb[cb][tok]).astype(np.float32)
    return e
