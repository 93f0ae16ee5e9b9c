"""The fused SEANet front end (`seanet_front_kernel`, the default; DSM_FUSE_FRONT=0 selects the three GEMM launches) under the
overlap that once disturbed it: `dsm_mimi_encode_step_dev` free-running beside `dsm_asr_step_tokens_dev`
that is fed a FIXED device code buffer, so the LM never waits for the encoder's hand-off and its dot_mode 1 kernels share the
CUs with the front kernel's 1 920 workgroups in every frame.  Before the fix nearly all of the 40 frames differed from the
synchronised run; they must be equal bit for bit, twice in a row.

stt-1b-en_fr, B = 64 (the smallest shape at which both LM groups' 32-row GEMMs are co-resident with the front kernel), dot_mode 1,
default environment, synthetic weights, 40 frames; every frame's codes stay in a device-side history so that read-backs do not
serialise the run.  The second test steps the fused kernel against the three launches at B = 2 over three frames: frames 1 and
2 read, in their first tile, what the last tile of the frame before left (the k-3 conv's carried frames).  (The `tiny` preset
has four SEANet filters and never takes the fused kernel.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
N, B = 40, 64


@pytest.fixture(scope="module")
def stt(gpu, dsm, lib):
    import torch
    from dsm_amd import synth
    cfg = dsm.config_stt_1b_en_fr()
    cfg.dot_mode = 1
    lm, mimi = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="stt-1b-en_fr")
    base = dsm.AsrEngine(cfg, 2, lm, mimi, device_id=0)
    try:
        yield cfg, base.weight_arena(), torch.device("cuda", 0)
    finally:
        base.close()


def _encode_beside_lm(dsm, torch, cfg, arena, pcm, mask, fixed_codes, sync_every_step):
    dev = pcm.device
    nq, nh = cfg.audio_codebooks, max(cfg.extra_heads_num, 1)
    eng = dsm.AsrEngine(cfg, B, device_id=0, arena=arena)
    try:
        codes = torch.zeros(N, B * nq, dtype=torch.int32, device=dev)
        text = torch.zeros(N, B, dtype=torch.int32, device=dev)
        prs = torch.zeros(N, nh * B, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the engine's streams are not ordered against torch's
        for i in range(N):
            eng.encode_step_dev(pcm[i % pcm.shape[0]].data_ptr(), mask.data_ptr(), codes[i].data_ptr())
            eng.step_tokens_dev(fixed_codes.data_ptr(), mask.data_ptr(), text[i].data_ptr(), prs[i].data_ptr())
            if sync_every_step:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert eng.metrics().capture_failures == 0
        return codes.cpu().numpy()
    finally:
        eng.close()


def test_fused_front_is_reproducible_beside_an_lm_that_never_waits(dsm, stt, monkeypatch):
    import torch
    from dsm_amd import synth
    monkeypatch.delenv("DSM_FUSE_FRONT", raising=False)  # the default: the fused kernel
    cfg, arena, dev = stt
    pcm = torch.from_numpy(synth.synth_pcm(B, 16, seed=1000)).to(dev)
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    fixed = torch.zeros(B * cfg.audio_codebooks, dtype=torch.int32, device=dev)
    ref = _encode_beside_lm(dsm, torch, cfg, arena, pcm, mask, fixed, True)
    assert len(np.unique(ref)) > 16, "the synchronised run's codes look degenerate"
    for attempt in range(2):
        got = _encode_beside_lm(dsm, torch, cfg, arena, pcm, mask, fixed, False)
        bad = np.nonzero((got != ref).reshape(N, -1).any(axis=1))[0]
        assert bad.size == 0, (f"free-running run {attempt}: Mimi codes differ from the synchronised run in {bad.size} of {N} "
                               f"frames ({int((got != ref).sum())} codes), first frames {bad.tolist()[:8]}")


def test_fused_front_equals_the_three_launches_across_the_carry(dsm, stt, monkeypatch):
    import torch
    from dsm_amd import synth
    cfg, arena, dev = stt
    b, frames = 2, 3
    pcm = torch.from_numpy(synth.synth_pcm(b, frames, seed=77)).to(dev)
    mask = torch.ones(b, dtype=torch.uint8, device=dev)
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("DSM_FUSE_FRONT", fuse)  # read when the engine is created
        eng = dsm.AsrEngine(cfg, b, device_id=0, arena=arena)
        try:
            codes = torch.zeros(frames, b * cfg.audio_codebooks, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for i in range(frames):
                eng.encode_step_dev(pcm[i].data_ptr(), mask.data_ptr(), codes[i].data_ptr())
            torch.cuda.synchronize()
            out[fuse] = codes.cpu().numpy()
        finally:
            eng.close()
    assert len(np.unique(out["0"])) > 8, "the three-launch codes look degenerate"
    assert np.array_equal(out["1"], out["0"]), "fused front end and three launches disagree"
