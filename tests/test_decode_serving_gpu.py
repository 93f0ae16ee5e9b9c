"""Mimi::decode_step (core/mimi.rs:217-225) at the batch sizes that are served, bit for bit against the CPU oracle.

Which kernel a decoder matrix product gets depends on M = B x rows per slot (plan_gemm, csrc/dsm_gemm_plan.h), and the tiny and
medium Mimi (n_filters = 4: K % 32 != 0 almost everywhere) take the generic kernel throughout, so the tiled kernels with the
decoder's own epilogues — the ELU copy into the next conv's concat buffer, residual + plain Y2, the N = 1 final conv without
16-byte stores, N = 32 with idle waves, Y2 behind a 14-chunk tile reduce — are reached only by the real Mimi, and the forms the
served batches take only by running those batches.  CASES is the table of them; tests/test_decoder_plan_coverage_cpu.py proves
on the CPU that it covers every class of (product, plan) that B = 32, 48 and 64 reach in either engine kind, and that no case of
it can go.

The reference is computed once: NS = 3 code streams stepped through OracleAsr.decode_step for 6 frames, one paused on frame 2,
one reset before frame 3.  Streams do not interact (every slot decodes with its own state), so every engine slot carries one of the
three streams (`owner`) and its PCM must equal the oracle's PCM of that stream, whatever the batch and wherever the slot sits in
it.  No tolerance: the decoder kernels follow the canonical reduction orders (dsm_numerics.h), as every other decode test demands.

The configuration is the tiny LM with the stt-1b-en_fr preset's Mimi, so that neither side loads the 1 B LM.  An STT engine is
enough for both knob families: the Mimi weights are f32, so dot_mode changes nothing for them except the chunk-loop threshold —
dot_mode 1 gives 192 tiles, dot_mode 0 gives 384, the same as a decoder attached to a TTS engine (gemm_default_knobs).

B = 64 in dot_mode 1 is the regression test of a fault (profiles/r09/decode_fault.txt): gemm_reduce_rows_kernel's idle threads read
2 KB past the end of the split-K workspace when d_model < 1024, and at B = 64 the decoder transformer's ff_out slabs fill a workspace of
exactly 2 MiB, so the read left the allocation's mapping — in either dot_mode, through either entry point."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")

# (engine kind, dot_mode, B), from the smallest batch up.  A plain list: the coverage test imports it.
CASES = [("stt", 1, 32), ("stt", 1, 48), ("stt", 0, 48), ("stt", 1, 64)]

NS, FRAMES = 3, 6          # source streams, oracle frames
PAUSED, PAUSE_AT = 1, 2    # stream 1 is inactive on frame 2
RESET, RESET_AT = 2, 3     # stream 2 gets mimi_reset_batch_idx before frame 3


def serving_config(dsm, dot_mode=0):
    """The tiny LM around the real Mimi."""
    cfg = dsm.config_tiny()
    cfg.mimi = dsm.config_stt_1b_en_fr().mimi
    cfg.audio_codebooks = cfg.mimi.quantizer_n_q
    cfg.audio_vocab_size = cfg.mimi.quantizer_bins + 1
    cfg.dot_mode = dot_mode
    return cfg


class Reference:
    pass


@pytest.fixture(scope="module")
def ref(dsm, orc):
    """codes [FRAMES][NS][n_q], mask [FRAMES][NS], pcm [FRAMES][NS][1920] of the oracle, read-only."""
    from dsm_amd import synth
    cfg = serving_config(dsm)
    r = Reference()
    r.lm, r.mimi = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="tinylm-mimi-v0_1")
    rng = np.random.default_rng(20250117)
    r.codes = rng.integers(0, cfg.mimi.quantizer_bins, (FRAMES, NS, cfg.mimi.quantizer_n_q)).astype(np.uint32)
    r.mask = np.ones((FRAMES, NS), dtype=np.uint8)
    r.mask[PAUSE_AT, PAUSED] = 0
    r.pcm = np.zeros((FRAMES, NS, 1920), dtype=np.float32)
    ora = orc.OracleAsr(cfg, NS, r.lm, r.mimi)
    orc.set_num_threads(orc.default_num_threads())  # OracleAsr sizes its team by the LM, which is tiny here; Mimi is not
    for s in range(FRAMES):
        if s == RESET_AT:
            ora.mimi_reset_batch_idx(RESET, side=0)
        r.pcm[s] = ora.decode_step(r.codes[s], r.mask[s], side=0)
    ora.close()
    assert np.all(np.isfinite(r.pcm)) and all(np.any(r.pcm[s][r.mask[s] == 1] != 0) for s in range(FRAMES))
    for a in (r.codes, r.mask, r.pcm):
        a.setflags(write=False)
    return r


def owners(B):
    """Which source stream a slot carries: random, with the first slots, the last slots and the slots around B / 2 pinned."""
    owner = np.random.default_rng(B).integers(0, NS, B)
    pins = [0, 1, 2, B // 2 - 1, B // 2, B // 2 + 1, B - 3, B - 2, B - 1]
    owner[pins] = [0, 1, 2, 0, 1, 2, 0, 1, 2]
    assert all((owner == k).any() for k in range(NS))
    return owner


def reset_slots(eng, owner):
    for b in np.nonzero(owner == RESET)[0]:
        eng.mimi_reset_batch_idx(int(b))


def check_frame(got, ref, owner, s, what):
    act = ref.mask[s][owner].astype(bool)
    g, w = got.reshape(len(owner), 1920).view(np.uint32), ref.pcm[s][owner].view(np.uint32)
    bad = np.nonzero((g != w).any(axis=1) & act)[0]
    print(f"{what} frame {s}: {act.sum()} active slots, {len(bad)} differ")
    assert len(bad) == 0, (f"{what}, frame {s}: PCM of {len(bad)} of {act.sum()} active slots differs from the oracle's; first: slot {bad[0]} "
                           f"(stream {owner[bad[0]]}), {(g[bad[0]] != w[bad[0]]).sum()} of 1920 samples, "
                           f"max |diff| {np.abs(got.reshape(len(owner), 1920)[bad[0]] - ref.pcm[s][owner[bad[0]]]).max():.3g}")


def run_host(dsm, ref, B, dot_mode, frames, what):
    """`frames` frames through decode_step (host codes in, host PCM out) on a B-slot engine."""
    eng = dsm.AsrEngine(serving_config(dsm, dot_mode), B, ref.lm, ref.mimi)
    owner = owners(B)
    try:
        for s in range(frames):
            if s == RESET_AT:
                reset_slots(eng, owner)
            pcm = eng.decode_step(np.ascontiguousarray(ref.codes[s][owner]), np.ascontiguousarray(ref.mask[s][owner]))
            assert pcm is not None and pcm.shape == (B, 1920)
            check_frame(pcm, ref, owner, s, what)
        assert eng.metrics().capture_failures == 0, eng.metrics().capture_error
    finally:
        eng.close()


@pytest.mark.parametrize("knobs", [{"DSM_SMALLK_MIN": "1", "DSM_SMALLK_MT": "4"}, {"DSM_SMALLK_MIN": "1", "DSM_SMALLK_MT": "2"},
                                   {"DSM_SMALLK_MIN": "1", "DSM_SMALLK_MT": "1"}, {"DSM_CHUNK_LOOP_MIN": "1"}],
                         ids=lambda k: ",".join(f"{n[4:]}={v}" for n, v in k.items()))
def test_small_batch_forced_forms_match_the_oracle(gpu, dsm, lib, ref, monkeypatch, knobs):
    """The real Mimi at B = 9, the smallest batch at which the 1920-row products keep MT = 4 (M = 17 280: 270 workgroups of 64
    rows cover the 256 CUs).  DSM_SMALLK_MIN=1 moves every one-chunk product to gemm_loop_kernel's two-block form — loop2<4> for the
    convtr of stages 2 and 3, ra3, rb3 and the N = 1 final conv, what B >= 35 takes by itself — with DSM_SMALLK_MT capping the rows
    per workgroup at 64, 32 and 16; DSM_CHUNK_LOOP_MIN=1 makes every multi-chunk product walk its chunks in the workgroup."""
    for name, value in knobs.items():
        monkeypatch.setenv(name, value)
    run_host(dsm, ref, 9, 0, 4, f"B=9 {knobs}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-dot%d-B%d" % c)
def test_served_batches_match_the_oracle(gpu, dsm, lib, ref, case):
    kind, dot_mode, B = case
    assert kind == "stt"
    run_host(dsm, ref, B, dot_mode, 4, f"B={B} dot_mode {dot_mode}")


def test_device_pointer_entry_and_graph_replay(gpu, dsm, lib, ref):
    """dsm_mimi_decode_step_dev the way bench.py --workload mimi-decode drives it: int32 device codes, a uint8 device mask, an f32
    device PCM buffer, no synchronisation inside the call.  All 6 frames: frame 0 grows the split-K workspace, which restarts
    the settling count, frames 1 and 2 settle, frame 3 is captured and launched as a graph, frames 4 and 5 are replays."""
    import torch
    kind, dot_mode, B = max(CASES, key=lambda c: (c[2], c[1]))
    eng = dsm.AsrEngine(serving_config(dsm, dot_mode), B, ref.lm, ref.mimi)
    owner = owners(B)
    dev = torch.device("cuda", 0)
    codes = torch.from_numpy(ref.codes[:, owner].astype(np.int32)).to(dev).contiguous()   # [FRAMES][B][n_q]
    mask = torch.from_numpy(np.ascontiguousarray(ref.mask[:, owner])).to(dev).contiguous()  # [FRAMES][B] uint8
    pcm = torch.zeros(B * 1920, dtype=torch.float32, device=dev)
    assert codes.dtype == torch.int32 and mask.dtype == torch.uint8
    torch.cuda.synchronize()
    try:
        for s in range(FRAMES):
            if s == RESET_AT:
                reset_slots(eng, owner)
            eng.decode_step_dev(codes[s].data_ptr(), mask[s].data_ptr(), pcm.data_ptr())
            eng.sync()
            check_frame(pcm.cpu().numpy(), ref, owner, s, f"decode_step_dev B={B} dot_mode {dot_mode}")
        m = eng.metrics()
        print("graph launches", m.graph_launches, "eager bodies", m.eager_bodies, "capture failures", m.capture_failures)
        assert m.capture_failures == 0, m.capture_error
        assert m.graph_launches >= 2, "the last frames must be replays of the captured decode graph"
    finally:
        eng.close()
