"""Ownership and teardown of the TTS engine: the device context (csrc/dsm_device.h) hands out device memory, pinned memory,
events, streams and graph slots, and its destructor is the only place that releases them.  Create / attach_mimi / step /
close cycles — with a group stream, a decode left unreceived, and creates / attaches that fail half way — must neither fault nor
leak device memory; an STT engine in the same process then goes through its own create / step / close."""
import numpy as np
import pytest

import tts_pcm_ref as R

pytestmark = pytest.mark.gpu
CYCLES = 5


def test_tts_create_destroy_cycles(gpu, dsm, lib, tiny_weights, monkeypatch):
    import torch
    monkeypatch.setenv("DSM_TTS_GROUPS", "2")  # a group stream with its fork / done events
    cfg_t, tts_path = R.tts_setup(dsm)
    cfg_a, _, mimi_path = R.mimi_setup(dsm)
    steps, _ = R.plan(cfg_t)
    deeper = type(cfg_t).from_buffer_copy(cfg_t)  # one layer more than the checkpoint has: fails after the device and streams are open
    deeper.lm.num_layers += 1
    first = None
    free0 = torch.cuda.mem_get_info()[0]
    for cycle in range(CYCLES):
        with pytest.raises(dsm.DsmError, match="cannot find tensor"):
            dsm.TtsEngine(deeper, R.B, tts_path)
        eng = dsm.TtsEngine(cfg_t, R.B, tts_path)
        if cycle == 0:
            with pytest.raises(dsm.DsmError, match="cannot open"):
                eng.attach_mimi(cfg_a.mimi, mimi_path + ".missing")
        eng.attach_mimi(cfg_a.mimi, mimi_path)
        text, audio, pcm, valid = eng.step_pcm(*steps[0])  # serial
        text1, audio1 = eng.step_pcm(*steps[1], defer=True)  # deferred, never received: the decode is pending at close()
        assert eng.pcm_pending() == 1
        got = (text, audio, valid, text1, audio1)
        if first is None:
            first = got
        for a, b in zip(got, first):  # every engine starts from the same clean state
            assert np.array_equal(a, b), f"cycle {cycle} differs from cycle 0"
        m = eng.metrics()
        assert m.capture_failures == 0, m.capture_error
        eng.close()
    used = free0 - torch.cuda.mem_get_info()[0]
    assert used < 64 << 20, f"device memory leaked across TTS create/destroy: {used} bytes"
    # the two engine types share the device context type, not a destructor path
    cfg = dsm.config_tiny()
    stt = dsm.AsrEngine(cfg, 8, *tiny_weights)
    stt.step_pcm(np.zeros((8, 1920), dtype=np.float32), np.ones(8, dtype=np.uint8))
    m = stt.metrics()
    assert m.capture_failures == 0, m.capture_error
    stt.close()
