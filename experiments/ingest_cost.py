"""What does the ingest (dsm_asr_set_ingest) cost per Mimi encode?  The setup of text_bias_cost.py: stt-1b-en_fr shapes with
synthetic weights, B = 64; after a warm-up --steps encode calls of the dsm_mimi_encode_step_dev class on device-resident input,
timed with the host clock from a synchronised engine to the dsm_sync behind the last call.  Legs: plain
(dsm_mimi_encode_step_dev); raw (dsm_mimi_encode_step_raw_dev) with every slot on the pass-through format, at 8000 / MULAW, and
at 48000 / F32 — the most taps and the largest frames — in alternating order, --repeats times, in ONE process on one engine.  On
a tree without the calls (the parent commit) only the plain leg runs: the same script, copied there.
    python experiments/ingest_cost.py [--out FILE]
One JSON line per leg, then a summary line (mean and min .. max of each setting, in us per encode)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import dsm_amd
from dsm_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = dsm_amd.config_stt_1b_en_fr()
    B = args.batch
    lm, mimi = synth.make_synth_weights(cfg, os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"), tag="stt-1b-en_fr")
    eng = dsm_amd.AsrEngine(cfg, B, lm, mimi)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pcm = torch.from_numpy(synth.synth_pcm(B, 8, seed=1000)).to(dev)
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    codes = torch.zeros(B * cfg.mimi.quantizer_n_q, dtype=torch.int32, device=dev)
    has = hasattr(eng, "set_ingest")
    settings = [("plain", None)]
    raw = {}
    if has:
        eng.set_ingest(True)
        pitch = dsm_amd.INGEST_MAX_FRAME_BYTES
        # 8 frames of rows per format: the 24 kHz frames' bytes, random mu-law bytes, 48 kHz noise
        rows = np.zeros((8, B, pitch), dtype=np.uint8)
        rows[:, :, :7680] = synth.synth_pcm(B, 8, seed=1000).view(np.uint8).reshape(8, B, 7680)
        raw["raw, 24000 / F32 (pass-through)"] = (24000, dsm_amd.PCM_F32, torch.from_numpy(rows).to(dev))
        rows = np.zeros((8, B, pitch), dtype=np.uint8)
        rows[:, :, :640] = rng.integers(0, 256, (8, B, 640), dtype=np.uint8)
        raw["raw, 8000 / MULAW"] = (8000, dsm_amd.PCM_MULAW, torch.from_numpy(rows).to(dev))
        rows = (0.1 * rng.standard_normal((8, B, 3840))).astype(np.float32).view(np.uint8).reshape(8, B, pitch)
        raw["raw, 48000 / F32"] = (48000, dsm_amd.PCM_F32, torch.from_numpy(rows).to(dev))
        settings += [(name, name) for name in raw]
    torch.cuda.synchronize()

    def run(n, leg):
        for i in range(n):
            if leg is None:
                eng.encode_step_dev(pcm[i % 8].data_ptr(), mask.data_ptr(), codes.data_ptr())
            else:
                eng.encode_step_raw_dev(raw[leg][2][i % 8].data_ptr(), pitch, mask.data_ptr(), codes.data_ptr())
        eng.sync()

    lines, per = [], {name: [] for name, _ in settings}
    for r in range(args.repeats):
        for name, leg in (settings if r % 2 == 0 else settings[::-1]):
            if leg is not None:
                for b in range(B):
                    eng.set_input_format(b, raw[leg][0], raw[leg][1])
            run(args.warmup, leg)
            g0 = eng.metrics().graph_launches
            t0 = time.perf_counter()
            run(args.steps, leg)
            us = 1e6 * (time.perf_counter() - t0) / args.steps
            m = eng.metrics()
            per[name].append(us)
            lines.append({"tree": args.tag, "leg": name, "repeat": r, "us_per_encode": round(us, 2), "steps": args.steps, "batch": B,
                          "graph_launches_in_window": int(m.graph_launches - g0), "capture_failures": int(m.capture_failures)})
            print(json.dumps(lines[-1]), flush=True)
    summary = {"tree": args.tag, "summary_us_per_encode": {k: {"mean": round(float(np.mean(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                                           for k, v in per.items()}}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
