#!/usr/bin/env python3
"""ms per step of a batch of TTS generations, host-driven against device-scheduled (config_tts_v202501, synthetic weights, a
cross-attention source on every slot as bench.py's TTS leg builds them, Mimi v0_1 with n_q = dep_num_slices):

  --leg step_pcm   dsm_tts_step_pcm(NULL) + dsm_tts_recv_pcm one step behind: every step is a host round trip
  --leg run --k K  dsm_tts_run(K, decode) + dsm_tts_collect over requests with a long prompt: K steps per visit

One leg per process (run each under its own time limit).  Every slot steps at every timed step and the timed steps lie past
both delay windows, so every slot emits a frame per step.  Prints one JSON line.  The step_pcm leg only uses calls that exist
before the request loop did: run on the parent commit it is the baseline."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["step_pcm", "run"], required=True)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=96, help="timed steps (a multiple of 16)")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    ap.add_argument("--tiny", action="store_true", help="the tiny test configurations instead (a quick check of the tool itself)")
    args = ap.parse_args()
    import dsm_amd
    from dsm_amd import synth
    B = args.batch
    if args.tiny:
        cfg = dsm_amd.config_tts_tiny(cross_attention=True)
        cfg.max_steps = 512
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
    fill = (cfg.text_audio_delay_in_tokens + cfg.acoustic_delay + 3 + 15) // 16 * 16  # whole blocks of 16, past both delay windows
    total = fill + args.warmup + args.steps
    assert args.steps % 16 == 0 and args.warmup % 16 == 0 and total < cfg.max_steps, "whole blocks that fit one generation"
    eng = dsm_amd.TtsEngine(cfg, B, path)
    for b in range(B):
        eng.set_ca_src(b, synth.synth_ca_src(cfg, src_rows, 100 + b))
    eng.attach_mimi(mcfg, mimi_path)
    rng = np.random.default_rng(3)
    frames = 0
    if args.leg == "step_pcm":
        mask = np.ones(B, dtype=np.uint8)

        def step():
            prev = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.uint32)
            allowed = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.int32)
            eng.step_pcm(prev, allowed, mask, defer=True)
            return int(eng.recv_pcm()[1].sum()) if eng.pcm_pending() == 2 else 0

        for _ in range(fill + args.warmup):
            step()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            frames += step()
        while eng.pcm_pending():  # the last decode belongs to the timed work
            frames += int(eng.recv_pcm()[1].sum())
        ms = (time.perf_counter() - t0) / args.steps * 1000
    else:
        K = args.k
        assert 16 % K == 0
        for b in range(B):  # a prompt that outlasts the run: words of three tokens, none of them a special id
            eng.request_begin(b, total + 16, 0)
            eng.push_words(b, [[cfg.text_bos_token] + rng.integers(4, cfg.text_in_vocab_size - 1, 2).tolist()] +
                           [rng.integers(4, cfg.text_in_vocab_size - 1, 3).tolist() for _ in range(total // 3)])
        for _ in range((fill + args.warmup) // K):
            eng.run(K, decode=True)
            eng.collect()
        t0 = time.perf_counter()
        for _ in range(args.steps // K):
            eng.run(K, decode=True)
            blk = eng.collect()
            assert blk.stepped.all(), "a slot sat a timed step out"
            frames += int(blk.pcm_valid.sum())
        ms = (time.perf_counter() - t0) / args.steps * 1000
    m = eng.metrics()
    eng.close()
    assert frames >= (args.steps - 1) * B, f"only {frames} frames in {args.steps} steps of {B} slots"
    print(json.dumps({"tool": "tts_run_timing", "leg": args.leg if args.leg == "step_pcm" else "run%d" % args.k,
                      "config": "tiny" if args.tiny else "tts_v202501 + Mimi v0_1 n_q=%d" % cfg.dep_num_slices, "batch": B,
                      "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 4), "frames": frames,
                      "capture_failures": int(m.capture_failures)}))


if __name__ == "__main__":
    main()
