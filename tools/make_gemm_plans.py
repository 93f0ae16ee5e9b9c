#!/usr/bin/env python3
"""Writes tests/golden/gemm_plans.json: matrix-product queries and the line dsm_debug_gemm_plan answers for each (no GPU needed).
(a) one query per branch of plan_gemm (csrc/dsm_gemm_plan.h) at the smallest shape that reaches it, (b) the products of the
shipped presets, shapes and row maps worked out from the configurations the way the engines' call sites do.  Run it after a
deliberate change of a gate and read the diff: every changed line is a shape that moved to another kernel or launch shape.
Importable: mimi_products(mimi, B, stt, dot_mode) returns the rows of one Mimi at any batch (tests/decoder_plans.py uses it)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsm_amd  # noqa: E402

STORE, QKV, GATE, RVQ = 0, 1, 2, 3
ALIGNED, Y, Y2, RES, BIAS, NORM, Y_OK4, Y2_OK4, RES_OK4, Y_PLAIN, MAY_DEFER = (1 << i for i in range(11))
OK = Y_OK4 | Y2_OK4 | RES_OK4          # unset row maps of base_args are all zero: ld % 4 == 0 holds
BASE = ALIGNED | OK | Y_PLAIN          # a linear on plain [M][ld] matrices


def add(rows, name, stt, dot_mode, bf16, epi, nt, M, N, K, flags):
    rows.append(dict(name=name, stt=stt, dot_mode=dot_mode, weight_bf16=bf16, epi=epi, nt=nt, M=M, N=N, K=K, flags=flags))


def branch_rows():
    """(a) one row per branch of plan_gemm."""
    rows = []
    add(rows, "generic: K % 32 != 0", 1, 0, 0, STORE, 1, 16, 64, 100, BASE | Y)
    add(rows, "one chunk f32: tile kernel, fused epilogue, separate row norm", 1, 0, 0, STORE, 1, 16, 64, 256, BASE | Y | NORM)
    add(rows, "two chunks mode 0: slabs left to the consumer", 1, 0, 1, STORE, 1, 16, 1024, 512, BASE | Y | MAY_DEFER)
    add(rows, "two chunks mode 0: reduce rows<1> with the norm, N = 1024", 1, 0, 1, STORE, 1, 16, 1024, 512, BASE | Y | RES | NORM)
    add(rows, "two chunks mode 0: reduce rows<2> with the norm, N = 2048", 1, 0, 1, STORE, 1, 16, 2048, 512, BASE | Y | RES | NORM)
    add(rows, "two chunks mode 0: reduce rows<4> with the norm, N = 4096", 1, 0, 1, STORE, 1, 16, 4096, 512, BASE | Y | RES | NORM)
    add(rows, "two chunks mode 0: tile reduce, no norm", 1, 0, 1, STORE, 1, 16, 1024, 512, BASE | Y)
    add(rows, "chunk loop at 384 tiles", 1, 0, 1, STORE, 1, 384 * 64, 64, 512, BASE | Y)
    add(rows, "no chunk loop at 383 tiles", 1, 0, 1, STORE, 1, 383 * 64, 64, 512, BASE | Y)
    add(rows, "STT mode 1: chunk loop at 192 tiles", 1, 1, 1, STORE, 1, 192 * 64, 64, 512, BASE | Y)
    add(rows, "STT mode 1: no chunk loop at 191 tiles", 1, 1, 1, STORE, 1, 191 * 64, 64, 512, BASE | Y)
    add(rows, "TTS mode 1: no chunk loop at 192 tiles", 0, 1, 1, STORE, 1, 192 * 64, 64, 512, BASE | Y)
    add(rows, "loop depth 2: f32 weights", 1, 0, 0, STORE, 1, 384 * 64, 64, 512, BASE | Y)
    add(rows, "loop depth 2: NT = 2 (gate)", 1, 0, 1, GATE, 2, 384 * 64, 64, 512, BASE | Y)
    add(rows, "loop depth 4: bf16 weights, NT = 1", 1, 0, 1, STORE, 1, 384 * 64, 64, 512, BASE | Y)
    add(rows, "smallk at 1024 tiles, MT 4", 1, 0, 0, STORE, 1, 1024 * 64, 64, 64, BASE | Y)
    add(rows, "no smallk at 1023 tiles, MT 4", 1, 0, 0, STORE, 1, 1023 * 64, 64, 64, BASE | Y)
    add(rows, "mode 1 split-K: M = 16 on bx3u<1>, 24 KB", 1, 1, 1, STORE, 1, 16, 2048, 2048, BASE | Y)
    add(rows, "mode 1 split-K: M = 17 on bx3u<2>, 48 KB", 1, 1, 1, STORE, 1, 17, 2048, 2048, BASE | Y)
    add(rows, "mode 1 split-K: M = 32 on bx3u<2>, 48 KB", 1, 1, 1, STORE, 1, 32, 2048, 2048, BASE | Y)
    add(rows, "mode 1 split-K: M = 65 on bx3 split", 1, 1, 1, STORE, 1, 65, 2048, 2048, BASE | Y)
    add(rows, "33..64-row override: 256 workgroups, M = 48 on two 32-row tiles", 1, 1, 1, STORE, 1, 48, 64, 256 * 256, BASE | Y)
    add(rows, "33..64-row override: 257 workgroups stay at MT 4", 1, 1, 1, STORE, 1, 48, 64, 257 * 256, BASE | Y)
    add(rows, "33..64-row override: not for the QKV epilogue", 1, 1, 1, QKV, 1, 48, 64, 256 * 256, BASE | Y)
    add(rows, "two-n-tile form at (N / 128) * grid.z = 256", 1, 1, 1, STORE, 1, 256 * 64, 128, 512, BASE | Y)
    add(rows, "no two-n-tile form at 255", 1, 1, 1, STORE, 1, 255 * 64, 128, 512, BASE | Y)
    add(rows, "whole-K gate: K = 1024, M = 64 taken", 0, 1, 1, GATE, 2, 64, 2048, 1024, BASE | Y)
    add(rows, "whole-K gate: M = 65 refused", 0, 1, 1, GATE, 2, 65, 2048, 1024, BASE | Y)
    add(rows, "whole-K gate: K = 2048 (eight chunks) refused", 0, 1, 1, GATE, 2, 64, 2048, 2048, BASE | Y)
    add(rows, "whole-K gate: N % 16 != 0 refused", 0, 1, 1, GATE, 2, 64, 2040, 1024, BASE | Y)
    add(rows, "whole-K gate: mode 0 refused", 0, 0, 1, GATE, 2, 64, 2048, 1024, BASE | Y)
    add(rows, "RVQ never on a bx3 kernel: split-K", 1, 1, 1, RVQ, 1, 64, 2048, 512, BASE | BIAS)
    add(rows, "RVQ never on a bx3 kernel: chunk loop", 1, 1, 1, RVQ, 1, 192 * 64, 2048, 512, BASE | BIAS)
    add(rows, "RVQ never on a bx3 kernel: generic", 1, 1, 1, RVQ, 1, 64, 2048, 100, BASE | BIAS)
    add(rows, "generic: chunk partials do not fit in LDS", 1, 0, 0, STORE, 1, 16, 64, 161 * 256 - 28, BASE | Y)
    return rows


# ---- (b) the shipped presets ----
def ok4(m):  # RowMap (bstride, ld)
    return m[0] % 4 == 0 and m[1] % 4 == 0


NONE = (0, 1)  # plain_map(1, 1): what the call sites pass for an unused map


def plain(ld):
    return (0, ld)


def map_flags(y, ymap, y2, y2map, res, rmap):
    f = (Y if y else 0) | (Y2 if y2 else 0) | (RES if res else 0)
    f |= (Y_OK4 if ok4(ymap) else 0) | (Y2_OK4 if ok4(y2map) else 0) | (RES_OK4 if ok4(rmap) else 0)
    return f | (Y_PLAIN if ymap[0] == 0 else 0)


class Conv:  # ConvGeom
    def __init__(self, in_c, out_c, k, stride, T_in, T_out):
        self.in_c, self.out_c, self.k, self.stride, self.T_in, self.T_out, self.S = in_c, out_c, k, stride, T_in, T_out, k - stride

    def cat_map(self):  # rows -> this conv's concat buffer
        return ((self.S + self.T_in) * self.in_c, self.in_c)


def conv(rows, name, B, c, y=None, y2=None, res=None, stt=1, dot_mode=1):  # run_conv; y / y2 / res: a RowMap or None
    bstride = (c.S + c.T_in) * c.in_c
    aligned = (c.stride * c.in_c) % 4 == 0 and bstride % 4 == 0
    f = map_flags(y is not None, y or NONE, y2 is not None, y2 or NONE, res is not None, res or NONE) | BIAS | (ALIGNED if aligned else 0)
    add(rows, name, stt, dot_mode, 0, STORE, 1, B * c.T_out, c.out_c, c.k * c.in_c, f)


def transformer(rows, name, stt, dot_mode, bf16, M, T, d, hidden, gating, last_map=None, post_norm=False, ca=False):
    """One middle layer and the last layer's ff_out of transformer_forward / transformer_layer_tail."""
    lin = BASE | Y
    add(rows, name + " QKV", stt, dot_mode, bf16, QKV, 1, M, 3 * d, d, lin | (MAY_DEFER if T == 1 else 0))
    add(rows, name + " out_proj + norm", stt, dot_mode, bf16, STORE, 1, M, d, d, lin | RES | NORM)
    if ca:
        add(rows, name + " ca_q", stt, dot_mode, bf16, STORE, 1, M, d, d, lin | MAY_DEFER)
        add(rows, name + " ca_out + norm2", stt, dot_mode, bf16, STORE, 1, M, d, d, lin | RES | NORM)
    if gating:
        add(rows, name + " gate", stt, dot_mode, bf16, GATE, 2, M, hidden, d, lin)
    else:
        add(rows, name + " ff_in", stt, dot_mode, bf16, STORE, 1, M, hidden, d, lin)
    add(rows, name + " ff_out + next norm1", stt, dot_mode, bf16, STORE, 1, M, d, hidden, lin | RES | NORM)
    if last_map is not None:  # the last layer writes the next conv's concat buffer, no norm
        add(rows, name + " ff_out, last layer", stt, dot_mode, bf16, STORE, 1, M, d, hidden,
            ALIGNED | RES | map_flags(True, last_map, False, (0, 0), True, plain(d)))
    elif not post_norm:
        add(rows, name + " ff_out, last layer", stt, dot_mode, bf16, STORE, 1, M, d, hidden, lin | RES)


def gating_hidden(t):
    return 11 * t.d_model // 4 if t.dim_feedforward == 4 * t.d_model else 2 * t.dim_feedforward // 3


DEC = "mimi dec"  # every decoder product's name starts with it


def mimi_products(m, B, stt=1, dot_mode=1):
    """The matrix products of one Mimi encode step and one decode step at batch B, as rows (the decoder's are named DEC ...).
    stt / dot_mode: the engine the Mimi belongs to (they choose the plan's default knobs, nothing else: the weights are f32)."""
    rows = []
    FRAME = 1920
    # encoder (load_mimi, seanet_encode)
    mult, T = 1, FRAME
    init = Conv(m.channels, mult * m.n_filters, m.kernel_size, 1, T, T)
    stages = []
    for i in range(m.n_ratios):
        ratio = m.ratios[m.n_ratios - 1 - i]
        dim = mult * m.n_filters
        ra, rb = Conv(dim, dim // m.compress, m.residual_kernel_size, 1, T, T), Conv(dim // m.compress, dim, 1, 1, T, T)
        dn = Conv(dim, 2 * dim, 2 * ratio, ratio, T, T // ratio)
        stages.append((ra, rb, dn))
        T //= ratio
        mult *= 2
    final = Conv(mult * m.n_filters, m.dimension, m.last_kernel_size, 1, T, T)
    down = Conv(m.dimension, m.dimension, 2 * m.downsample_stride, m.downsample_stride, T, T // m.downsample_stride)
    e = dict(stt=stt, dot_mode=dot_mode)
    conv(rows, "mimi enc init", B, init, y=plain(init.out_c), y2=stages[0][0].cat_map(), **e)
    for i, (ra, rb, dn) in enumerate(stages):
        conv(rows, "mimi enc stage %d ra" % i, B, ra, y2=rb.cat_map(), **e)
        conv(rows, "mimi enc stage %d rb" % i, B, rb, y2=dn.cat_map(), res=plain(rb.out_c), **e)
        if i + 1 < len(stages):
            conv(rows, "mimi enc stage %d down" % i, B, dn, y=plain(dn.out_c), y2=stages[i + 1][0].cat_map(), **e)
        else:
            conv(rows, "mimi enc stage %d down" % i, B, dn, y2=final.cat_map(), **e)
    conv(rows, "mimi enc final", B, final, y=plain(m.dimension), **e)
    t = m.transformer
    transformer(rows, "mimi enc tr", stt, dot_mode, 0, B * T, T, t.d_model, t.dim_feedforward, False, last_map=down.cat_map())
    f = map_flags(True, plain(m.dimension), False, NONE, False, NONE) | ALIGNED  # the downsample conv has no bias
    add(rows, "mimi enc downsample", stt, dot_mode, 0, STORE, 1, B * down.T_out, down.out_c, down.k * down.in_c, f)
    add(rows, "mimi rvq input_proj", stt, dot_mode, 0, STORE, 1, B, m.quantizer_dim, m.dimension, BASE | Y)
    add(rows, "mimi rvq codebook", stt, dot_mode, 0, RVQ, 1, B, m.quantizer_bins, m.quantizer_dim, BASE | BIAS)
    # decoder (load_mimi, mimi_decode_body)
    add(rows, DEC + " rvq output_proj first", stt, dot_mode, 0, STORE, 1, B, m.dimension, m.quantizer_dim, BASE | Y)
    add(rows, DEC + " rvq output_proj rest", stt, dot_mode, 0, STORE, 1, B, m.dimension, m.quantizer_dim, BASE | Y | RES)
    dec_init = Conv(m.dimension, mult * m.n_filters, m.kernel_size, 1, T, T)
    transformer(rows, DEC + " tr", stt, dot_mode, 0, B * T, T, t.d_model, t.dim_feedforward, False, last_map=dec_init.cat_map())
    conv(rows, DEC + " init", B, dec_init, y2=plain(dec_init.out_c), **e)
    dec = []
    for i in range(m.n_ratios):
        ratio = m.ratios[i]
        in_c = mult * m.n_filters
        out_c = in_c // 2
        add(rows, DEC + " stage %d convtr" % i, stt, dot_mode, 0, STORE, 1, B * T, 2 * ratio * out_c, in_c, BASE | Y)
        T *= ratio
        dec.append((Conv(out_c, out_c // m.compress, m.residual_kernel_size, 1, T, T), Conv(out_c // m.compress, out_c, 1, 1, T, T)))
        mult //= 2
    dec_final = Conv(m.n_filters, m.channels, m.last_kernel_size, 1, T, T)
    for i, (ra, rb) in enumerate(dec):
        conv(rows, DEC + " stage %d ra" % i, B, ra, y2=rb.cat_map(), **e)
        conv(rows, DEC + " stage %d rb" % i, B, rb, y2=plain(rb.out_c) if i + 1 < len(dec) else dec_final.cat_map(), res=plain(rb.out_c), **e)
    conv(rows, DEC + " final", B, dec_final, y=plain(m.channels), **e)
    return rows


def stt_lm_products(rows, name, cfg, M, dot_mode=1):
    """The LM products of one STT stream group of M rows: one layer, the text head, the extra heads where the preset has any."""
    d = cfg.lm.d_model
    transformer(rows, name + ":", 1, dot_mode, 1, M, 1, d, gating_hidden(cfg.lm), True, post_norm=True)
    add(rows, name + ": text linear", 1, dot_mode, 1, STORE, 1, M, cfg.text_out_vocab_size, d, BASE | Y)
    if cfg.extra_heads_num:
        add(rows, name + ": extra heads", 1, dot_mode, 1, STORE, 1, M, cfg.extra_heads_num * cfg.extra_heads_dim, d, BASE | Y)


def tts_lm_products(rows, name, cfg, M, dot_mode=1):
    """The products of one TTS stream group of M batch rows: one main-LM layer, the text head, the depformer."""
    d, D = cfg.lm.d_model, cfg.depformer.d_model
    transformer(rows, name + " main LM:", 0, dot_mode, 1, M, 1, d, gating_hidden(cfg.lm), True, post_norm=True, ca=True)
    add(rows, name + " text linear", 0, dot_mode, 1, STORE, 1, M, cfg.text_out_vocab_size, d, BASE | Y)
    add(rows, name + " depformer in_all", 0, dot_mode, 1, STORE, 1, M, cfg.dep_weight_groups * D, d, BASE | Y)
    transformer(rows, name + " depformer:", 0, dot_mode, 1, M, 1, D, gating_hidden(cfg.depformer), True)
    add(rows, name + " depformer linears.k", 0, dot_mode, 1, STORE, 1, M, cfg.audio_vocab_size - 1, D, BASE | Y | MAY_DEFER)


def stt_group_rows(B):
    """Rows per LM launch of an STT engine of B slots: two stream groups of whole 16-row blocks from B = 32 on (dsm_asr_create)."""
    G = min(2 if B >= 32 else 1, (B + 15) // 16)
    n16, out, b0 = (B + 15) // 16, [], 0
    for g in range(G):
        nb = min((n16 // G + (1 if g < n16 % G else 0)) * 16, B - b0)
        out.append(nb)
        b0 += nb
    return out


def tts_group_rows(B, rows_per_slot):
    """Rows per launch of a TTS engine of B slots: one stream group below 96 slots, two from there on (dsm_tts_create)."""
    G = min(2 if B >= 96 else 1, B)
    return [(B // G + (1 if g < B % G else 0)) * rows_per_slot for g in range(G)]


def preset_rows():
    """(b) the products of the shipped presets."""
    rows = []
    stt = dsm_amd.config_stt_1b_en_fr()
    stt_lm_products(rows, "stt-1b group of 32", stt, 32)
    rows += mimi_products(stt.mimi, 64)
    tts = dsm_amd.config_tts_v202501()
    tts_lm_products(rows, "tts B = 32", tts, 32)
    # the groups of 64 rows (batch 128, the batch BASELINE.json quotes stt-2.6b-en at) and the second STT preset
    stt_lm_products(rows, "stt-1b group of 64", stt, 64)
    big = dsm_amd.config_stt_2_6b_en()
    stt_lm_products(rows, "stt-2.6b group of 32", big, 32)
    stt_lm_products(rows, "stt-2.6b group of 64", big, 64)
    return rows


def plan_line(lib, r):
    """What dsm_debug_gemm_plan answers for a row."""
    buf = C.create_string_buffer(512)
    n = lib.dsm_debug_gemm_plan(r["stt"], r["dot_mode"], r["weight_bf16"], r["epi"], r["nt"], r["M"], r["N"], r["K"], r["flags"], buf, len(buf))
    assert n > 0, r
    return buf.value.decode()


def plan_line_knobs(lib, r, knobs):
    """The same under explicit knobs (dot_mode, chunk_loop_min_tiles, smallk_min_tiles, smallk_mt, loop_depth; -1 = the default of
    the row's engine kind): dsm_debug_gemm_plan_knobs.  knobs[0] decides the mode, not the row's dot_mode."""
    buf = C.create_string_buffer(512)
    n = lib.dsm_debug_gemm_plan_knobs(r["stt"], (C.c_int * 5)(*knobs), r["weight_bf16"], r["epi"], r["nt"], r["M"], r["N"], r["K"], r["flags"],
                                      buf, len(buf))
    assert n > 0, (r, knobs)
    return buf.value.decode()


if __name__ == "__main__":
    lib = dsm_amd.load_library()
    rows = branch_rows() + preset_rows()
    for r in rows:
        r["line"] = plan_line(lib, r)
    out = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(out, len(rows), "rows")
