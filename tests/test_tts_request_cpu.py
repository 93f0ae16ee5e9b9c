"""The request loop without a GPU: the reference loop of tests/tts_request_ref.py over the oracle's TTS step walks every
branch with the prompts the GPU tests use (conditions on the inputs, not on the code under test), and the six entry points
of the device-side request loop exist in the built library and in include/dsm.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tts_pcm_ref as R
import tts_request_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSM_ERR_INVALID = -1
SYMBOLS = ["dsm_tts_request_begin", "dsm_tts_request_push_words", "dsm_tts_request_close", "dsm_tts_run", "dsm_tts_collect",
           "dsm_tts_request_status"]


@pytest.fixture(scope="module")
def ref(dsm, orc):
    cfg_t, tts_path = Q.tts_setup(dsm)
    ora = orc.OracleTts(cfg_t, R.B, tts_path)
    results, stepped = Q.run(ora, cfg_t, R.B, Q.whole_prompts(cfg_t), 64)
    ora.close()
    return cfg_t, results, stepped


def test_prompts_walk_every_branch(ref):
    cfg_t, results, stepped = ref
    n = Q.check_branches(cfg_t, results)
    print(n, [(r["status"], r["step_idx"]) for r in results])
    # the slot built for it ends by max_seq_len, the others by the tail rule, all within the 64 iterations
    assert [r["status"] for r in results] == [Q.DONE, Q.DONE, Q.DONE, Q.DONE_LIMIT]
    assert results[3]["step_idx"] == 9
    # the tail is extra_steps + text_audio_delay_in_tokens Pad steps
    for r, g in zip(results[:3], Q.whole_prompts(cfg_t)):
        assert r["kind"][-(g["extra_steps"] + cfg_t.text_audio_delay_in_tokens):] == ["pad"] * (g["extra_steps"] + cfg_t.text_audio_delay_in_tokens)
        assert r["kind"].count("pad") == g["extra_steps"] + cfg_t.text_audio_delay_in_tokens
    # the empty prompt: the empty word's end-of-pad, then the tail; its last end-of-pad became a pad in the text table
    assert results[2]["events"][0][0] == -1 and len(results[2]["events"]) == 1
    assert len(results[2]["overwritten"]) == 1
    # a Text token with the end-of-pad value ends its word: word 1 of slot 1 stops after two tokens
    ev = {w: (a, b) for w, a, b in results[1]["events"]}
    w1 = [i for i, k in enumerate(results[1]["kind"]) if k == "text"]
    assert 1 in ev and results[1]["text"][ev[1][1]] == cfg_t.text_eop_token and results[1]["kind"][ev[1][1]] == "text"
    assert 21 not in [results[1]["text"][i] for i in w1]
    # every word of the finished prompts has its event, in push order, with growing steps
    for r, g in zip(results[:3], Q.whole_prompts(cfg_t)):
        assert [e[0] for e in r["events"]] == list(range(-1, len(g["words"])))
        assert all(a <= b for _, a, b in r["events"])


def test_words_arriving_late_only_delay(dsm, orc, ref):
    """A script that holds words back changes when a slot steps, not what it computes."""
    cfg_t, results, _ = ref
    _, tts_path = Q.tts_setup(dsm)
    ora = orc.OracleTts(cfg_t, R.B, tts_path)
    late, stepped = Q.run(ora, cfg_t, R.B, Q.late_prompts(cfg_t), Q.LATE_ITERS)
    ora.close()
    for a, b in zip(late, results):
        assert a["text"] == b["text"] and a["events"] == b["events"] and a["status"] == b["status"]
        assert all(np.array_equal(x, y) for x, y in zip(a["audio"], b["audio"]))
        assert all(np.array_equal(x, y) for x, y in zip(a["table"], b["table"]))
    assert (stepped[:32, 0] == 0).sum() > 0 and not stepped[1:16, 1].any() and not stepped[32:48, 1].any()  # slot 1 waits through block 2


def test_abi(lib):
    """Fails without the feature: the symbols, their declarations, and DSM_ERR_INVALID for a NULL engine."""
    header = open(os.path.join(ROOT, "include", "dsm.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(dsm_tts\*" % name, header), f"{name} is not declared in dsm.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert "#define DSM_TTS_RUN_MAX 16" in header
    assert lib.dsm_tts_request_begin(None, 0, 8, 0) == DSM_ERR_INVALID
    assert lib.dsm_tts_request_push_words(None, 0, None, None, 0) == DSM_ERR_INVALID
    assert lib.dsm_tts_request_close(None, 0) == DSM_ERR_INVALID
    assert lib.dsm_tts_run(None, 1, 0) == DSM_ERR_INVALID
    assert lib.dsm_tts_collect(None, None) == DSM_ERR_INVALID
    assert lib.dsm_tts_request_status(None, 0) == DSM_ERR_INVALID
