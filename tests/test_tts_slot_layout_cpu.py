"""dsm_tts_slot_layout (csrc/dsm_tts_slot_layout.h) without a device: the section list of a TTS slot's device payload, worked out
here from DESIGN.md section 7.2's table of state and the configuration alone, against what the library answers — names, bytes
per slot, 16-byte-aligned offsets, slot_bytes and the signature's length — for config_tts_tiny with kv_bf16 on / off, cfg_rows
on / off, cross-attention on / off, with and without a Mimi configuration.  A blob built by the hand-builder of test_tts_slot_blob_cpu.py with that slot_bytes and
that signature reads back through dsm_tts_slot_blob_info."""
import itertools

import pytest

from test_tts_slot_blob_cpu import ITEMS, build_blob

FRAME = 1920


def align16(n):
    return (n + 15) & ~15


def expected_sections(cfg, mimi):
    """(name, bytes per slot) in blob order: every row of the table of state above "host"."""
    rps = 2 if cfg.cfg_rows else 1
    kv = 2 if cfg.kv_bf16 else 4
    S, d = cfg.dep_num_slices, cfg.lm.d_model
    out = [("lm.pos", 4 * rps), ("lm.idx", 4 * rps)]
    for l in range(cfg.lm.num_layers):
        out += [(f"lm.k.{l}", rps * d * cfg.lm.context * kv), (f"lm.v.{l}", rps * d * cfg.lm.context * kv)]
    if cfg.cross_attention:
        out.append(("ca.last", 4 * rps))
        for l in range(cfg.lm.num_layers):
            for j in range(rps):
                out += [(f"ca.k.{l}.{j}", d * cfg.ca_max_len * kv), (f"ca.v.{l}.{j}", d * cfg.ca_max_len * kv)]
    out += [("cfg.on", 1), ("cfg.fa", 4), ("cfg.fb", 4)]
    out += [("samp.k", 4), ("samp.invt", 4), ("rng.key", 32), ("rng.pos_text", 4), ("rng.pos_audio", 4)]
    out += [("text_token", 4), ("last", 4), ("lat", 4 * S), ("ring", 4 * (cfg.acoustic_delay + 1)), ("row0", 4 * S)]
    out += [("cond.row", 4 * d), ("cond.on", 1), ("req", 52)]
    if mimi is None:
        return out
    t = mimi.transformer
    out += [("dec.started", 1), ("dec.pos", 4), ("dec.idx", 4)]
    for l in range(t.num_layers):
        out += [(f"dec.k.{l}", t.d_model * t.context * 4), (f"dec.v.{l}", t.d_model * t.context * 4)]
    out.append(("dec.up_carry", 4 * mimi.downsample_stride * mimi.dimension))
    ratios = list(mimi.ratios)[:mimi.n_ratios]
    mult = 1 << mimi.n_ratios
    convs = [(mimi.kernel_size - 1, mimi.dimension)]  # (carried frames, channels) of every streaming conv of the decoder
    for i, r in enumerate(ratios):
        out_c = mult * mimi.n_filters // 2
        out.append((f"dec.carry.{i}", 4 * (2 * r - r) * out_c))  # conv-transpose: (k - stride) * out_c
        convs += [(mimi.residual_kernel_size - 1, out_c), (0, out_c // mimi.compress)]  # the residual block's k = 3 and k = 1 convs
        mult //= 2
    convs.append((mimi.last_kernel_size - 1, mimi.n_filters))
    for i, (s, c) in enumerate(x for x in convs if x[0] > 0):
        out.append((f"dec.conv.{i}", 4 * s * c))
    return out


CASES = list(itertools.product([0, 1], [0, 1], [0, 1], [0, 1]))


@pytest.mark.parametrize("kv_bf16,cfg_rows,cross,with_mimi", [c for c in CASES if c[2] or not c[1]])
def test_layout_is_the_table_of_state(dsm, lib, kv_bf16, cfg_rows, cross, with_mimi):
    cfg = dsm.config_tts_tiny(kv_bf16=kv_bf16, cross_attention=bool(cross), cfg_rows=bool(cfg_rows))
    mimi = None
    if with_mimi:
        mimi = dsm.config_tiny().mimi
        mimi.quantizer_n_q = cfg.dep_num_slices
    got = dsm.tts_slot_layout(cfg, mimi)
    want = expected_sections(cfg, mimi)
    assert [(n, b) for n, b, _ in got["sections"]] == want
    off = 0
    for name, nbytes, at in got["sections"]:
        assert at == off and at % 16 == 0, name
        off += align16(nbytes)
    assert got["slot_bytes"] == off and off % 16 == 0
    # 21 words for the model, 13 + n_ratios more for a Mimi with decode state
    assert len(got["signature"]) == 21 + ((13 + mimi.n_ratios) if with_mimi else 0)
    assert got["signature"][:5] == [cfg.lm.num_layers, cfg.lm.num_heads, cfg.lm.d_model // cfg.lm.num_heads, cfg.lm.context, kv_bf16]
    # without the Mimi the list is a prefix of the one with it, and so is the signature
    if with_mimi:
        base = dsm.tts_slot_layout(cfg)
        assert got["sections"][:len(base["sections"])] == base["sections"]
        assert got["signature"][:len(base["signature"])] == base["signature"]
    flags = dsm.TTS_SLOT_BLOB_HAS_MIMI_DEC if with_mimi else 0
    blob = build_blob(ITEMS, got["signature"], got["slot_bytes"], flags=flags, slices=cfg.dep_num_slices)
    info = dsm.tts_slot_blob_info(blob)
    assert info["slot_bytes"] == got["slot_bytes"] and info["sig_words"] == len(got["signature"]) and info["total_bytes"] == len(blob)


def test_layout_is_pure_and_checks_its_configuration(dsm, lib):
    cfg = dsm.config_tts_tiny(cross_attention=True, cfg_rows=True)
    assert dsm.tts_slot_layout(cfg) == dsm.tts_slot_layout(cfg)
    bad = dsm.config_tts_tiny()
    bad.cfg_rows = 1  # needs cross_attention
    with pytest.raises(dsm.DsmError, match="cfg_rows"):
        dsm.tts_slot_layout(bad)
    mimi = dsm.config_tiny().mimi
    mimi.ratios[0] = 7  # 1920 samples do not divide
    with pytest.raises(dsm.DsmError, match="ratios"):
        dsm.tts_slot_layout(cfg, mimi)
    # the odd sizes the transfer kernels' word and byte paths exist for
    sizes = {n: b for n, b, _ in dsm.tts_slot_layout(cfg)["sections"]}
    assert sizes["cfg.on"] == 1 and sizes["cond.on"] == 1 and sizes["req"] == 52 and sizes["ring"] == 4 * (cfg.acoustic_delay + 1)
