"""The deployment switches among the ten DSM_* variables (include/dsm.h) each pick another launch sequence for the same arithmetic:
under every one of them the engine must stay bit-exact against the oracle, like the default in test_parity_gpu.py.
  DSM_FUSE_QKV=0     the split-K QKV GEMM keeps its own reduce launch instead of the attention kernel's prologue
  DSM_STREAM_PRIO=1  LM streams high, encoder stream low
  DSM_GRAPHS=0       every launch sequence eager
  DSM_LM_GROUPS=1    one stream group
Shapes: the smallest with a split-K QKV GEMM (the only place DSM_FUSE_QKV matters) and with a bf16 ring — the tiny model (K = 352:
one full chunk plus a 3-block chunk) in dot_mode 0, and a medium model (d_model 512 = two chunks, head_dim 128, bf16 ring of 300)
in dot_mode 1.  B = 5, 12 frames, random masks with slot 0 always on, one reset."""
import os

import numpy as np
import pytest

from test_parity_gpu import run_pair

pytestmark = pytest.mark.gpu
WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
B, FRAMES = 5, 12


@pytest.mark.parametrize("model", ["tiny", "medium_bx3"])
@pytest.mark.parametrize("knob,value", [("DSM_FUSE_QKV", "0"), ("DSM_STREAM_PRIO", "1"), ("DSM_GRAPHS", "0"), ("DSM_LM_GROUPS", "1")])
def test_parity_under_each_deployment_switch(gpu, dsm, lib, orc, tiny_weights, model, knob, value, monkeypatch):
    from dsm_amd import synth
    monkeypatch.setenv(knob, value)
    if model == "tiny":
        cfg = dsm.config_tiny()
        lm, mimi = tiny_weights
    else:
        cfg = dsm.config_medium(lm_heads=4, lm_head_dim=128, lm_context=300, kv_bf16=1)
        cfg.dot_mode = 1
        lm, mimi = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="medium_bf16_hd128_ctx300")
    rng = np.random.default_rng(13)
    masks = (rng.random((FRAMES, B)) < 0.75).astype(np.uint8)
    masks[:, 0] = 1
    run_pair(dsm, orc, cfg, B, lm, mimi, steps=FRAMES, mask_fn=lambda s: masks[s], resets={6: [1]})
