"""The kernels that hold, or held, a packed-f32 result read by the next vector instruction (tools/packed_f32_hazards.py), run
BESIDE other kernels' vector work and compared bit for bit with themselves on an idle device.  seanet_front_kernel lost taps of
such a chain only while the dot_mode 1 LM shared its SIMDs; alone it was bit-exact, so no parity test sees
that kind of error.

The amplifier is the one that exposed the front end (tests/test_front_overlap_gpu.py): an stt-1b-en_fr engine, dot_mode 1,
B = 64, synthetic weights, stepping `step_tokens_dev` on a fixed device code buffer, enqueued without a synchronise.  Everything
that synchronises the device (engine creation, attach_mimi, attach_speaker_encoder) happens before it starts.  After the last
compared call of a pass the amplifier must still have work outstanding — its `sync()` takes longer than one LM step as timed in
this file — or the pass fails with "no overlap": the front-end record shows that whatever ran after the LM's queue had drained was
always clean.

  spk_attn_kernel<32|64>         (class L until its chains were made scalar) through dsm_tts_encode_voice: eight encodes beside the
                                 amplifier, twice, each byte-identical to the encode on the idle device;
  attn_small_kernel<float, 64>   (class H: reads the high half only; the DepFormer's attention on its f32 ring and, with kv_bf16 = 0
                                 and head_dim 64, the tiny main LM's self- and cross-attention) through 20 dsm_tts_step calls at B = 4
                                 (after four on the idle device, which capture the engine's graphs): text tokens, audio tokens and
                                 lm.hidden bits equal those of the idle run."""
import os
import time

import numpy as np
import pytest

import speaker_ref as SR
from tts_schedule import schedule

pytestmark = pytest.mark.gpu
WEIGHTS_DIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")
B_AMP = 64
N_AMP = 40      # LM steps enqueued in front of a pass: 57 ms of work on an MI355X; eight encodes take 10 ms of it, 20 TTS steps 20 ms
N_ENCODES = 8
N_TTS_WARM = 4  # steps of a fresh TTS engine on the idle device in every run: its graphs are captured and instantiated in them
N_TTS_STEPS = 20


@pytest.fixture(scope="module")
def stt(gpu, dsm, lib):
    from dsm_amd import synth
    cfg = dsm.config_stt_1b_en_fr()
    cfg.dot_mode = 1
    lm, mimi = synth.make_synth_weights(cfg, WEIGHTS_DIR, tag="stt-1b-en_fr")
    base = dsm.AsrEngine(cfg, 2, lm, mimi, device_id=0)
    try:
        yield cfg, base.weight_arena()
    finally:
        base.close()


class Amplifier:
    """A B = 64 LM that steps on fixed codes.  Created (and warmed: the steps replay as graphs once two have run) before the pass;
    start() only enqueues, outstanding_ms() is the time its sync() then takes."""

    def __init__(self, dsm, stt):
        import torch
        cfg, arena = stt
        dev = torch.device("cuda", 0)
        self.eng = dsm.AsrEngine(cfg, B_AMP, device_id=0, arena=arena)
        self.mask = torch.ones(B_AMP, dtype=torch.uint8, device=dev)
        self.codes = torch.zeros(B_AMP * cfg.audio_codebooks, dtype=torch.int32, device=dev)
        self.text = torch.zeros(B_AMP, dtype=torch.int32, device=dev)
        self.prs = torch.zeros(max(cfg.extra_heads_num, 1) * B_AMP, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # the engine's streams are not ordered against torch's
        self.start(4)
        self.eng.sync()
        t0 = time.perf_counter()
        self.start(8)
        self.eng.sync()
        self.step_ms = (time.perf_counter() - t0) * 1e3 / 8

    def start(self, n):
        for _ in range(n):
            self.eng.step_tokens_dev(self.codes.data_ptr(), self.mask.data_ptr(), self.text.data_ptr(), self.prs.data_ptr())

    def outstanding_ms(self):
        t0 = time.perf_counter()
        self.eng.sync()
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.eng.sync()
        assert self.eng.metrics().capture_failures == 0
        self.eng.close()


def _assert_overlapped(amp, left_ms, what):
    print(f"{what}: amplifier outstanding for {left_ms:.2f} ms after the last compared call (one LM step: {amp.step_ms:.2f} ms)")
    assert left_ms > amp.step_ms, (f"no overlap: {what} ended with {left_ms:.2f} ms of amplifier work outstanding, less than one LM step "
                                   f"({amp.step_ms:.2f} ms): raise N_AMP")


@pytest.mark.parametrize("name", ["tiny_full_window", "medium_ragged"])
def test_encode_voice_beside_the_lm_equals_encode_voice_alone(gpu, dsm, lib, orc, stt, name):
    """tiny_full_window: head_dim 32, T = 10; medium_ragged: head_dim 64, T = 26 (a ragged query block, one partial key tile): the
    smallest shapes that run every chain of spk_attn_kernel (the rotation, the QK dot, the PV sums)."""
    cs = SR.case(name)
    eng = dsm.TtsEngine(cs.cfg_t, 1, cs.tts_path)
    eng.attach_mimi(cs.cfg_a.mimi, cs.mimi_a)
    eng.attach_speaker_encoder(cs.n_speakers, cs.tts_path)
    amp = Amplifier(dsm, stt)
    try:
        alone = eng.encode_voice(cs.clips)
        assert np.abs(alone - cs.r64_rows).max() <= 4 * cs.noise_rows, "the encode on the idle device is off its float64 reference"
        assert eng.encode_voice(cs.clips).tobytes() == alone.tobytes(), "two encodes on the idle device differ"
        for attempt in range(2):
            amp.start(N_AMP)
            got = [eng.encode_voice(cs.clips) for _ in range(N_ENCODES)]
            left = amp.outstanding_ms()
            bad = [(i, int((g.view(np.uint32) != alone.view(np.uint32)).sum())) for i, g in enumerate(got) if g.tobytes() != alone.tobytes()]
            worst = max((float(np.abs(g - alone).max()) for g in got), default=0.0)
            print(f"{name}, pass {attempt}: {len(bad)} of {N_ENCODES} encodes differ from the idle one "
                  f"(values per encode: {[n for _, n in bad]} of {alone.size}; max |diff| {worst:.3e})")
            assert not bad, (f"pass {attempt}: {len(bad)} of {N_ENCODES} encodes beside the LM differ from the encode alone "
                             f"(encode, values): {bad}; max |diff| {worst:.3e}")
            _assert_overlapped(amp, left, f"{name}, pass {attempt}")
    finally:
        amp.close()
        eng.close()


def _tts_hd64_f32(dsm):
    """config_tts_tiny with cross-attention at head_dim 64 and f32 rings: the depformer (one head, context 6) and the main LM
    (two heads, context 16, sources of at most 24 rows) all dispatch attn_small_kernel<float, 64> (T == 1, head_dim 64, context <= 32)."""
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny(cross_attention=True)
    cfg.lm.num_heads, cfg.depformer.num_heads = 2, 1
    cfg.kv_bf16 = 0
    return cfg, synth.make_synth_tts_weights(cfg, WEIGHTS_DIR, tag="tts_tiny_ca_hd64")


def _tts_run(dsm, cfg, path, B, after_warm=None):
    """A fresh engine with sources of 24, 1, 0 and 13 rows, N_TTS_WARM + N_TTS_STEPS of the schedule: per step the active slots'
    text tokens, audio tokens and lm.hidden bits, and the milliseconds the last N_TTS_STEPS took.  after_warm() runs in front of
    those: after everything that synchronises the device, and after the steps in which the engine captures its graphs.  (Measured:
    a fresh engine's first 20 steps beside a queue that was kept full took 293 ms, as long as the whole queue, and left nothing
    outstanding; after four idle steps and with dsm_tts_debug_read's copy on the model stream, 20 steps take 21 ms beside it,
    10 ms alone, and 31 ms of the queue are left.)"""
    from dsm_amd import synth
    eng = dsm.TtsEngine(cfg, B, path)
    try:
        for b, n in enumerate([24, 1, 0, 13]):
            if n:
                eng.set_ca_src(b, synth.synth_ca_src(cfg, n, 50 + b))
        d, out = cfg.lm.d_model, []
        for s, (prev, allowed, mask) in enumerate(schedule(cfg, B, N_TTS_WARM + N_TTS_STEPS)):
            if s == N_TTS_WARM:
                if after_warm:
                    after_warm()
                t0 = time.perf_counter()
            text, audio = eng.step(prev, allowed, mask)
            act = mask.astype(bool)
            hidden = eng.debug_read("lm.hidden", B * d).reshape(B, d)
            out.append((text[act].copy(), audio[act].copy(), hidden[act].view(np.uint32).copy()))
        return eng, out, (time.perf_counter() - t0) * 1e3
    except Exception:
        eng.close()
        raise


def test_depformer_f32_ring_attention_beside_the_lm(gpu, dsm, lib, stt):
    cfg, path = _tts_hd64_f32(dsm)
    B = 4
    eng, idle, idle_ms = _tts_run(dsm, cfg, path, B)
    assert eng.metrics().capture_failures == 0
    eng.close()
    assert len(np.unique(np.concatenate([audio.ravel() for _, audio, _ in idle]))) > 8, "the idle run's audio tokens look degenerate"
    amp = Amplifier(dsm, stt)
    try:
        for attempt in range(2):
            eng, got, ms = _tts_run(dsm, cfg, path, B, after_warm=lambda: amp.start(N_AMP))
            left = amp.outstanding_ms()
            assert eng.metrics().capture_failures == 0
            eng.close()
            bad = [s for s, (x, y) in enumerate(zip(got, idle)) if any(not np.array_equal(u, v) for u, v in zip(x, y))]
            print(f"pass {attempt}: {len(bad)} of {N_TTS_WARM + N_TTS_STEPS} steps differ from the idle run ({N_TTS_STEPS} steps: {ms:.1f} ms, idle {idle_ms:.1f} ms)")
            for s in bad[:1]:
                (te, ae, he), (ti, ai, hi) = got[s], idle[s]
                assert np.array_equal(he, hi), f"pass {attempt}, step {s}: {int((he != hi).sum())} lm.hidden values differ beside the LM (steps {bad})"
                assert np.array_equal(te, ti), f"pass {attempt}, step {s}: text tokens differ beside the LM: {te} vs {ti} (steps {bad})"
                assert np.array_equal(ae, ai), f"pass {attempt}, step {s}: depformer tokens differ beside the LM (steps {bad})"
            assert not bad
            _assert_overlapped(amp, left, f"TTS steps, pass {attempt}")
    finally:
        amp.close()
