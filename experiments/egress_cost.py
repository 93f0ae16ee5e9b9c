"""What does the TTS egress (dsm_tts_set_egress) cost per step?  The setup of tools/tts_run_timing.py: config_tts_v202501 with
synthetic weights, a cross-attention source on every slot, Mimi v0_1 with n_q = dep_num_slices, B = 32; every leg is a generation
of its own (slots reset, requests begun again with a prompt that outlasts the leg), so that all legs cover the same step indices
— a step's time grows with the slot's context; blocks of dsm_tts_run(16, decode = 1) run to their collect, timed with the host
clock (collect ends in the device synchronise).  Every slot steps at every timed step and the timed steps lie past both delay windows, so every slot
emits a frame per step.  Legs: egress off (dsm_tts_collect with the f32 frames: what the parent commit does); egress on with
every slot at 8000 / MULAW; egress on with every slot at 48000 / F32 (dsm_tts_collect_raw) — in alternating order, --repeats
times, in ONE process on one engine.  On a tree without the calls (the parent commit) only the first leg runs: the same script,
copied there.
    python experiments/egress_cost.py [--out FILE]
One JSON line per leg, then a summary line (mean and min .. max of each setting, in ms per step, and the bytes a step downloads
for the frames)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dsm_amd
from dsm_amd import synth

K = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=96, help="timed steps per leg (a multiple of 16)")
    ap.add_argument("--warmup", type=int, default=16, help="steps in front of every leg (a multiple of 16)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    args = ap.parse_args()
    B = args.batch
    cfg = dsm_amd.config_tts_v202501()
    path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts-v202501-ca")  # the file bench.py --workload tts uses
    mcfg = dsm_amd.MimiConfig()
    dsm_amd.load_library().dsm_mimi_config_v0_1(C.byref(mcfg), cfg.dep_num_slices)
    mimi_path = os.path.join(args.weights_dir, "mimi-v0_1-nq%d.mimi.safetensors" % cfg.dep_num_slices)
    if not os.path.exists(mimi_path):
        synth.write_safetensors(mimi_path, synth.mimi_spec(mcfg), "F32", synth.SEED)
    eng = dsm_amd.TtsEngine(cfg, B, path)
    eng.attach_mimi(mcfg, mimi_path)
    has = hasattr(eng, "set_egress")
    settings = [("off (f32 frames)", None)]
    if has:
        settings += [("on, 8000 / MULAW", (8000, dsm_amd.PCM_MULAW)), ("on, 48000 / F32", (48000, dsm_amd.PCM_F32))]
    fill = (cfg.text_audio_delay_in_tokens + cfg.acoustic_delay + 3 + K - 1) // K * K  # whole blocks, past both delay windows
    total = fill + args.warmup + args.steps
    assert args.steps % K == 0 and args.warmup % K == 0 and total < cfg.max_steps, "whole blocks that fit one generation"
    src = [synth.synth_ca_src(cfg, 125, 100 + b) for b in range(B)]

    def begin():
        """Every leg is a generation of its own over the same step indices: a step's time grows with the slot's context."""
        rng = np.random.default_rng(3)
        for b in range(B):  # a prompt that outlasts the leg: words of three tokens, none of them a special id
            eng.reset_batch_idx(b)
            eng.set_ca_src(b, src[b])
            eng.request_begin(b, total + K, 0)
            eng.push_words(b, [[cfg.text_bos_token] + rng.integers(4, cfg.text_in_vocab_size - 1, 2).tolist()] +
                           [rng.integers(4, cfg.text_in_vocab_size - 1, 3).tolist() for _ in range(total // 3)])

    def blocks(n, fmt):
        """n steps in blocks of 16; returns (frames emitted, bytes downloaded for frames per step)"""
        frames, pitch = 0, dsm_amd.FRAME_SIZE * 4
        if fmt is not None:
            pitch = (eng.output_format(0)[3] + 15) // 16 * 16
        for _ in range(n // K):
            eng.run(K, decode=True)
            blk = eng.collect() if fmt is None else eng.collect_raw(pitch=pitch)
            assert blk.stepped.all(), "a slot sat a step out"
            frames += int(blk.pcm_valid.sum())
        return frames, B * pitch

    lines, per, down = [], {name: [] for name, _ in settings}, {}
    for r in range(args.repeats):
        for name, fmt in (settings if r % 2 == 0 else settings[::-1]):
            if has:
                eng.set_egress(fmt is not None)
                if fmt is not None:
                    for b in range(B):
                        eng.set_output_format(b, *fmt)
            begin()
            blocks(fill + args.warmup, fmt)
            t0 = time.perf_counter()
            frames, down[name] = blocks(args.steps, fmt)
            ms = 1e3 * (time.perf_counter() - t0) / args.steps
            assert frames == args.steps * B, f"only {frames} frames in {args.steps} steps of {B} slots"
            per[name].append(ms)
            lines.append({"tree": args.tag, "leg": name, "repeat": r, "ms_per_step": round(ms, 4), "steps": args.steps, "batch": B,
                          "frame_bytes_downloaded_per_step": down[name], "capture_failures": int(eng.metrics().capture_failures)})
            print(json.dumps(lines[-1]), flush=True)
    summary = {"tree": args.tag, "summary_ms_per_step": {k: {"mean": round(float(np.mean(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                                            "frame_bytes_downloaded_per_step": down[k]} for k, v in per.items()}}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
