"""The overlapped device-pointer pipeline (`dsm_mimi_encode_step_dev` on the encoder stream beside
`dsm_asr_step_tokens_dev` on the LM streams: what bench.py times) must compute what the same calls compute when the device is
synchronised after every step, frame for frame and bit for bit, and twice in a row.

stt-1b-en_fr, B = 64, dot_mode 1 (the benchmarked mode), 40 frames, every output of every step kept in a device-side history
so that the free-running run is not disturbed by read-backs.  The oracle parity tests step synchronously; this one pins that
overlapping the streams changes nothing (with the fused SEANet front end it did)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
N, B = 40, 64


def _run(dsm, torch, cfg, arena, pcm, mask, sync_every_step):
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
            eng.step_tokens_dev(None, mask.data_ptr(), text[i].data_ptr(), prs[i].data_ptr())
            if sync_every_step:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        assert eng.metrics().capture_failures == 0
        return codes.cpu().numpy(), text.cpu().numpy(), prs.cpu().numpy().view(np.uint32)
    finally:
        eng.close()


def test_overlapped_pipeline_equals_the_synchronised_one(gpu, dsm, lib):
    import torch
    from dsm_amd import synth
    cfg = dsm.config_stt_1b_en_fr()
    cfg.dot_mode = 1
    lm, mimi = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="stt-1b-en_fr")
    dev = torch.device("cuda", 0)
    base = dsm.AsrEngine(cfg, B, lm, mimi, device_id=0)
    try:
        arena = base.weight_arena()
        pcm = torch.from_numpy(synth.synth_pcm(B, 16, seed=1000)).to(dev)
        mask = torch.ones(B, dtype=torch.uint8, device=dev)
        ref = _run(dsm, torch, cfg, arena, pcm, mask, True)
        for attempt in range(2):
            got = _run(dsm, torch, cfg, arena, pcm, mask, False)
            for name, a, b in zip(("codes", "text tokens", "VAD probabilities"), got, ref):
                bad = np.nonzero((a != b).reshape(N, -1).any(axis=1))[0]
                assert bad.size == 0, f"free-running run {attempt}: {name} differ from the synchronised run at frames {bad.tolist()}"
    finally:
        base.close()
