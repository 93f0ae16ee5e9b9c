"""Shared fixture of the TTS-to-PCM tests: the inputs, and the reference built from the existing oracle only.

Reference semantics (srv/tts.rs:499-500,528-544): every generation decodes with a Mimi of its own — OracleTts produces the
tokens, the emit rule of dsm_tts_step_pcm picks the frames, and each emitted frame goes to that slot's own B = 1 OracleAsr
decoder, replaced by a new instance when the slot is reset."""
import os

import numpy as np

from tts_schedule import schedule

WDIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
B, STEPS, LATE_SLOT, LATE_UNTIL, RESET_SLOT, RESET_STEP = 4, 24, 3, 7, 2, 13


def mimi_setup(dsm):
    """config_tiny with a 6-codebook Mimi (n_q = dep_num_slices of config_tts_tiny) and its synthetic weights."""
    from dsm_amd import synth
    cfg_a = dsm.config_tiny()
    cfg_a.mimi.quantizer_n_q = 6
    cfg_a.audio_codebooks = 6
    lm_a, mimi_a = synth.make_synth_weights(cfg_a, WDIR, tag="tiny_nq6")
    return cfg_a, lm_a, mimi_a


def tts_setup(dsm, **kw):
    from dsm_amd import synth
    cfg_t = dsm.config_tts_tiny(**kw)
    tag = "tts_tiny" + ("_ca" if kw.get("cross_attention") else "")
    return cfg_t, synth.make_synth_tts_weights(cfg_t, WDIR, tag=tag)


def plan(cfg_t):
    """24 steps of the shared schedule; slot 3 starts late (masked off for steps 0-6); slot 2 is reset before step 13."""
    out = []
    for s, (prev, allowed, mask) in enumerate(schedule(cfg_t, B, STEPS)):
        mask = mask.copy()
        if s < LATE_UNTIL:
            mask[LATE_SLOT] = 0
        out.append((prev, allowed, mask))
    return out, {RESET_STEP: [RESET_SLOT]}


def emits(cfg_t, active, s, row):
    """The predicate of dsm_tts_step_pcm: s = the slot's step index before the step, row = audio_tokens[s - acoustic_delay]
    after it (last_audio_tokens, core/tts_streaming.rs:275-287, and the test at srv/tts.rs:537)."""
    return bool(active) and s >= cfg_t.text_audio_delay_in_tokens + cfg_t.acoustic_delay and bool(np.all(row < cfg_t.audio_vocab_size - 1))


def reference(orc, cfg_t, tts_path, mimi, steps, resets, nb, setup=None):
    """Drives OracleTts over `steps` [(prev, allowed, mask)] and decodes per slot.  Returns a dict of per-step lists:
    text, audio, valid [nb], frames [nb][S], pcm [nb][1920] (rows of slots that did not emit are zero), plus the final
    step indices and token tables."""
    cfg_a, lm_a, mimi_a = mimi
    ora = orc.OracleTts(cfg_t, nb, tts_path)
    if setup:
        setup(ora)
    dec = [orc.OracleAsr(cfg_a, 1, lm_a, mimi_a) for _ in range(nb)]
    S, ad = cfg_t.dep_num_slices, cfg_t.acoustic_delay
    out = dict(text=[], audio=[], valid=[], frames=[], pcm=[])
    for s, (prev, allowed, mask) in enumerate(steps):
        for slot in resets.get(s, []):
            ora.reset_batch_idx(slot)
            dec[slot].close()
            dec[slot] = orc.OracleAsr(cfg_a, 1, lm_a, mimi_a)
        before = [ora.step_idx(b) for b in range(nb)]
        text, audio = ora.step(prev, allowed, mask)
        valid = np.zeros(nb, dtype=np.uint8)
        frames = np.zeros((nb, S), dtype=np.uint32)
        pcm = np.zeros((nb, 1920), dtype=np.float32)
        for b in range(nb):
            if not mask[b] or before[b] < ad:
                continue
            row = ora.audio_tokens(b, before[b] - ad)
            if emits(cfg_t, mask[b], before[b], row):
                valid[b], frames[b] = 1, row
                pcm[b] = dec[b].decode_step(row[None], [1], side=0)[0]
        for k, v in zip(("text", "audio", "valid", "frames", "pcm"), (text, audio, valid, frames, pcm)):
            out[k].append(v)
    out["step_idx"] = [ora.step_idx(b) for b in range(nb)]
    out["tables"] = [[ora.audio_tokens(b, i).copy() for i in range(ora.step_idx(b))] for b in range(nb)]
    ora.close()
    for d in dec:
        d.close()
    return out


def batched_module_pcm(orc, mimi, ref, resets, nb):
    """The same frames through ONE batched oracle module with Mimi::reset_batch_idx — the semantics the TTS path avoids."""
    cfg_a, lm_a, mimi_a = mimi
    ora = orc.OracleAsr(cfg_a, nb, lm_a, mimi_a)
    out = []
    for s, (valid, frames) in enumerate(zip(ref["valid"], ref["frames"])):
        for slot in resets.get(s, []):
            ora.mimi_reset_batch_idx(slot, side=0)
        out.append(ora.decode_step(frames, valid, side=0) if valid.any() else np.zeros((nb, 1920), dtype=np.float32))
    ora.close()
    return out


def check_inputs(cfg_t, ref, batched):
    """Properties of the inputs (not of the code under test) without which the GPU test could not tell the two decode
    semantics apart or would run empty."""
    valid = np.array(ref["valid"])
    per_slot = valid.sum(axis=0)
    assert np.all(per_slot >= 5), per_slot
    assert valid[RESET_STEP:, RESET_SLOT].sum() >= 3
    assert np.flatnonzero(valid[:, LATE_SLOT])[0] > 7
    differ = np.zeros(B, dtype=int)
    for s in range(len(valid)):
        for b in range(B):
            if valid[s, b] and not np.array_equal(batched[s][b].view(np.uint32), ref["pcm"][s][b].view(np.uint32)):
                differ[b] += 1
    assert differ[RESET_SLOT] >= 1 and differ[LATE_SLOT] >= 1, differ
    return per_slot, differ
