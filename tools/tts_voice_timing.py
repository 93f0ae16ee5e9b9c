#!/usr/bin/env python3
"""Voices against private rows at the shapes a deployment uses: config_tts_v202501 with ca_max_len = 640 and cfg_rows = 1,
synthetic weights, B slots that are all guided, sources of 625 rows (5 speakers x 125), no Mimi.

  --leg private   every slot takes its own rows and its own copy of the unconditional rows through set_ca_src: admission is
                  the wall time of one set_ca_src(625 + 625 rows), mean over the slots
  --leg voice     one voice and one unconditional voice for all slots: voice_create once each, admission is one set_voice

then ms per step of dsm_tts_step with every slot stepping.  One leg per process (run each under its own time limit); prints one
JSON line.  --tree imports the package from another built checkout: the parent commit's is the baseline of the private leg (it
only uses calls that exist without voices)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["private", "voice"], required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, default=625)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--tree", default=ROOT, help="the built checkout to import dsm_amd from")
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    ap.add_argument("--tiny", action="store_true", help="the tiny test configuration instead (a quick check of the tool itself)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import dsm_amd
    from dsm_amd import synth
    B = args.batch
    if args.tiny:
        cfg = dsm_amd.config_tts_tiny(cross_attention=True, cfg_rows=True)
        cfg.max_steps = 512
        path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts_tiny_ca")
        n = min(args.rows, cfg.ca_max_len)
    else:
        cfg = dsm_amd.config_tts_v202501()
        cfg.cross_attention, cfg.ca_norm, cfg.ca_dim, cfg.ca_max_len, cfg.cfg_rows = 1, 0, 0, 640, 1
        path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts-v202501-ca")  # the file bench.py --workload tts uses
        n = args.rows
    assert args.warmup + args.steps < cfg.max_steps and n <= cfg.ca_max_len
    eng = dsm_amd.TtsEngine(cfg, B, path)
    empty = synth.synth_ca_src(cfg, n, 9)
    out = {"tool": "tts_voice_timing", "leg": args.leg, "config": "tiny" if args.tiny else "tts_v202501, ca_max_len 640, cfg_rows",
           "tree": os.path.relpath(args.tree, ROOT), "batch": B, "rows": n, "steps": args.steps, "warmup": args.warmup}
    elem = 2 if cfg.kv_bf16 else 4
    out["private_block_bytes_per_row"] = 2 * cfg.lm.num_layers * cfg.lm.d_model * cfg.ca_max_len * elem
    if args.leg == "private":
        srcs = [synth.synth_ca_src(cfg, n, 100 + b) for b in range(B)]
        t0 = time.perf_counter()
        for b in range(B):
            eng.set_ca_src(b, srcs[b], empty, 2.0)
        out["admit_ms_per_slot"] = round((time.perf_counter() - t0) / B * 1000, 3)
    else:
        rows = synth.synth_ca_src(cfg, n, 100)
        t0 = time.perf_counter()
        v = eng.voice_create(rows)
        t1 = time.perf_counter()
        u = eng.voice_create(empty)
        t2 = time.perf_counter()
        for b in range(B):
            eng.set_voice(b, v, u, 2.0)
        t3 = time.perf_counter()
        out["voice_create_ms"] = [round((t1 - t0) * 1000, 3), round((t2 - t1) * 1000, 3)]
        out["admit_ms_per_slot"] = round((t3 - t2) / B * 1000, 3)
        info = eng.voice_info(v)
        assert info[:2] == (n, B) and eng.voice_info(u)[:2] == (n, B)
        out["voice_device_bytes"] = info[2]
    rng = np.random.default_rng(3)
    mask = np.ones(B, dtype=np.uint8)

    def step():
        prev = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.uint32)
        allowed = rng.integers(4, cfg.text_in_vocab_size - 1, B).astype(np.int32)
        eng.step(prev, allowed, mask)

    for _ in range(args.warmup):
        step()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    out["ms_per_step"] = round((time.perf_counter() - t0) / args.steps * 1000, 4)
    out["capture_failures"] = int(eng.metrics().capture_failures)
    assert all(eng.step_idx(b) == args.warmup + args.steps for b in range(B)), "a slot sat a step out"
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
