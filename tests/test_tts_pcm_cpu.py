"""TTS-to-PCM without a GPU: the four entry points are declared, exported and listed; NULL handles are refused before any
device work; and the fixture of tests/test_tts_pcm_gpu.py — built from the oracle alone — still has the properties that test
relies on (so an edit of tts_schedule.py cannot silently empty it)."""
import ctypes as C
import os
import re

import numpy as np

import tts_pcm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsm_tts_attach_mimi", "dsm_tts_step_pcm", "dsm_tts_recv_pcm", "dsm_tts_pcm_pending")


def test_symbols_are_declared_exported_and_listed(dsm, lib):
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    declared = set(re.findall(r"\b(dsm_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in declared and s in dsm.ABI_SYMBOLS and hasattr(lib, s), s


def test_null_handles_are_refused_without_a_device(dsm, lib):
    cfg = dsm.config_tiny()
    assert lib.dsm_tts_attach_mimi(None, C.byref(cfg.mimi), b"/nonexistent.safetensors") == -1  # DSM_ERR_INVALID
    pcm, valid = np.zeros(1920, dtype=np.float32), np.zeros(1, dtype=np.uint8)
    assert lib.dsm_tts_recv_pcm(None, pcm.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p)) == -1
    assert lib.dsm_tts_pcm_pending(None) == -1
    assert lib.dsm_tts_step_pcm(None, None, None, None, None, None, None, None) == -1


def test_reference_fixture_meets_its_input_conditions(dsm, orc):
    cfg_t, tts_path = R.tts_setup(dsm)
    mimi = R.mimi_setup(dsm)
    steps, resets = R.plan(cfg_t)
    ref = R.reference(orc, cfg_t, tts_path, mimi, steps, resets, R.B)
    batched = R.batched_module_pcm(orc, mimi, ref, resets, R.B)
    per_slot, differ = R.check_inputs(cfg_t, ref, batched)
    print("emitted frames per slot", per_slot, "frames where the batched module differs", differ)
    # slots 0 and 1 are active from the module's first call and never reset: both semantics agree on them
    assert differ[0] == 0 and differ[1] == 0
    assert all(np.isfinite(p).all() for p in ref["pcm"])
    assert max(int(f.max()) for f in ref["frames"]) < cfg_t.audio_vocab_size - 1 <= mimi[0].mimi.quantizer_bins
