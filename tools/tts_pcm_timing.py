#!/usr/bin/env python3
"""ms per step of the TTS product call, three ways (config_tts_v202501, synthetic weights, Mimi v0_1 with n_q = dep_num_slices):

  step          dsm_tts_step: tokens only
  serial        dsm_tts_step_pcm with a PCM buffer: every step waits for its frame's decode
  deferred      dsm_tts_step_pcm(NULL) + dsm_tts_recv_pcm one step behind: the decode of step n overlaps the LM of step n + 1

Every slot is active at every step and the timed steps lie past both delay windows, so every slot emits a frame per step.
Prints one JSON line.  Not part of bench.py: this times a call sequence, the headline workloads stay as they are."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    ap.add_argument("--tiny", action="store_true", help="the tiny test configurations instead (a quick check of the tool itself)")
    args = ap.parse_args()
    import ctypes as C
    import dsm_amd
    from dsm_amd import synth
    B = args.batch
    if args.tiny:
        cfg = dsm_amd.config_tts_tiny(cross_attention=True)
        path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts_tiny_ca")
        mcfg = dsm_amd.config_tiny().mimi
        mcfg.quantizer_n_q = cfg.dep_num_slices
        src_rows, mtag = 20, "tiny_nq%d" % cfg.dep_num_slices
    else:
        cfg = dsm_amd.config_tts_v202501()
        path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts-v202501-ca")  # the file bench.py --workload tts uses
        mcfg = dsm_amd.MimiConfig()
        dsm_amd.load_library().dsm_mimi_config_v0_1(C.byref(mcfg), cfg.dep_num_slices)
        src_rows, mtag = 125, "mimi-v0_1-nq%d" % cfg.dep_num_slices
    mimi_path = os.path.join(args.weights_dir, mtag + ".mimi.safetensors")
    if not os.path.exists(mimi_path):
        synth.write_safetensors(mimi_path, synth.mimi_spec(mcfg), "F32", synth.SEED)
    fill = cfg.text_audio_delay_in_tokens + cfg.acoustic_delay + 3
    assert fill + args.warmup + args.steps < cfg.max_steps, "the run must fit one generation (max_steps)"
    mask = np.ones(B, dtype=np.uint8)

    def leg(mode):
        rng = np.random.default_rng(3)
        eng = dsm_amd.TtsEngine(cfg, B, path)
        for b in range(B):
            eng.set_ca_src(b, synth.synth_ca_src(cfg, src_rows, 100 + b))
        if mode != "step":
            eng.attach_mimi(mcfg, mimi_path)
        frames = [0]

        def step():
            prev = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.uint32)
            allowed = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.int32)
            if mode == "step":
                eng.step(prev, allowed, mask)
            elif mode == "serial":
                frames[0] += int(eng.step_pcm(prev, allowed, mask)[3].sum())
            else:
                eng.step_pcm(prev, allowed, mask, defer=True)
                if eng.pcm_pending() == 2:
                    frames[0] += int(eng.recv_pcm()[1].sum())

        for _ in range(fill + args.warmup):
            step()
        frames[0] = 0
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        while mode == "deferred" and eng.pcm_pending():  # the last decode belongs to the timed work
            frames[0] += int(eng.recv_pcm()[1].sum())
        ms = (time.perf_counter() - t0) / args.steps * 1000
        m = eng.metrics()
        eng.close()
        if mode != "step":
            assert frames[0] >= (args.steps - 1) * B, f"{mode}: only {frames[0]} frames in {args.steps} steps of {B} slots"
        return ms, int(m.capture_failures)

    out = {"tool": "tts_pcm_timing", "config": "tiny" if args.tiny else "tts_v202501 + Mimi v0_1 n_q=%d" % cfg.dep_num_slices,
           "batch": B, "steps": args.steps, "warmup": args.warmup}
    for mode in ("step", "serial", "deferred"):
        ms, fails = leg(mode)
        out["ms_per_step_" + mode] = round(ms, 4)
        out["capture_failures_" + mode] = fails
    print(json.dumps(out))


if __name__ == "__main__":
    main()
