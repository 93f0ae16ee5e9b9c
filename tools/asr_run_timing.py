#!/usr/bin/env python3
"""ms per step of a batch of STT streams fed from the host frame by frame against clips resident on the device (stt-1b-en_fr,
synthetic weights, as bench.py builds them):

  --leg ticket     dsm_mimi_encode_step_raw_async + dsm_asr_step_tokens_ticket per step: every step uploads a raw row per slot
                   and is a host round trip.  Only calls that exist without the clips section: run on the parent commit it is
                   the baseline.
  --leg run --k K  dsm_asr_run(K) + dsm_asr_collect over clips pushed beforehand: K steps per visit

--format mulaw8k (8 kHz mu-law, 640 bytes a frame) or f32 (24 kHz f32, 7680 bytes a frame).  One leg per process (run each under
its own time limit).  Every slot steps at every timed step.  Prints one JSON line."""
import argparse
import audioop
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["ticket", "run"], required=True)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--format", choices=["mulaw8k", "f32"], default="mulaw8k")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=96, help="timed steps (a multiple of 16)")
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    ap.add_argument("--tiny", action="store_true", help="the tiny test configuration instead (a quick check of the tool itself)")
    args = ap.parse_args()
    import dsm_amd
    from dsm_amd import synth
    B = args.batch
    assert args.steps % 16 == 0 and args.warmup % 16 == 0 and 16 % args.k == 0, "whole blocks"
    cfg = dsm_amd.config_tiny() if args.tiny else dsm_amd.config_stt_1b_en_fr()
    lm_path, mimi_path = synth.make_synth_weights(cfg, args.weights_dir, tag="tiny" if args.tiny else "stt-1b-en_fr")
    rate, fmt = (8000, dsm_amd.PCM_MULAW) if args.format == "mulaw8k" else (24000, dsm_amd.PCM_F32)
    fb = dsm_amd.ingest_describe(rate, fmt)["frame_bytes"]
    total = args.warmup + args.steps
    # one clip of `total` frames, every slot its own rotation of it
    t = np.arange(total * fb // (1 if fmt == dsm_amd.PCM_MULAW else 4)) / rate
    x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.05 * np.random.default_rng(5).standard_normal(t.size)
    clip = audioop.lin2ulaw(np.round(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes(), 2) if fmt == dsm_amd.PCM_MULAW else x.astype("<f4").tobytes()
    assert len(clip) == total * fb
    clips = [clip[(b % total) * fb:] + clip[:(b % total) * fb] for b in range(B)]
    eng = dsm_amd.AsrEngine(cfg, B, lm_path, mimi_path, device_id=0)
    mask = np.ones(B, dtype=np.uint8)
    stepped = 0
    if args.leg == "ticket":
        eng.set_ingest(True)
        for b in range(B):
            eng.set_input_format(b, rate, fmt)
        pitch = (fb + 15) // 16 * 16
        rows = np.zeros((total, B, pitch), dtype=np.uint8)
        for b in range(B):
            rows[:, b, :fb] = np.frombuffer(clips[b], dtype=np.uint8).reshape(total, fb)

        def step(s):
            eng.step_tokens_ticket(eng.encode_step_raw_async(rows[s], mask, pitch), mask)
            return B

        for s in range(args.warmup):
            step(s)
        t0 = time.perf_counter()
        for s in range(args.warmup, total):
            stepped += step(s)
        ms = (time.perf_counter() - t0) / args.steps * 1000
    else:
        K = args.k
        eng.set_clips(True, total * fb)
        for b in range(B):
            eng.clip_begin(b, rate, fmt, 0)
            eng.clip_push(b, clips[b])
            eng.clip_close(b)
        eng.sync()  # the uploads are not part of a step
        for _ in range(args.warmup // K):
            eng.run(K)
            eng.collect()
        t0 = time.perf_counter()
        for _ in range(args.steps // K):
            eng.run(K)
            stepped += int(eng.collect().stepped.sum())
        ms = (time.perf_counter() - t0) / args.steps * 1000
    m = eng.metrics()
    eng.close()
    assert stepped == args.steps * B, f"{stepped} slot steps in {args.steps} steps of {B} slots"
    print(json.dumps({"tool": "asr_run_timing", "leg": "ticket" if args.leg == "ticket" else "run%d" % args.k, "format": args.format,
                      "config": "tiny" if args.tiny else "stt-1b-en_fr", "batch": B, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(ms, 4), "capture_failures": int(m.capture_failures)}))


if __name__ == "__main__":
    main()
