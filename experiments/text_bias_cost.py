"""What does the text bias (dsm_asr_set_text_bias) cost per LM step?  The setup of token_scores_cost.py: stt-1b-en_fr shapes with
synthetic weights, B = 64, every ring full; after a warm-up (the switch is part of the LM step's capture key, so each change
settles into a graph again) --steps dsm_asr_step_tokens_dev calls on device-resident codes, timed with the host clock from a
synchronised engine to the dsm_sync behind the last step.  Legs: off; on with nothing attached; on with every slot attached to
one set of 1000 keywords and 100 token biases — in alternating order, --repeats times, in ONE process on one engine.  On a tree
without the call (the parent commit) only the "off" leg runs: the same script, copied there.
    python experiments/text_bias_cost.py [--out FILE]
One JSON line per leg, then a summary line (mean and min .. max of each setting, in us per step)."""
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


def big_set(V, rng):
    """1000 keywords of 1 .. 6 pieces over a 400-piece alphabet (so that prefixes are shared) and 100 token biases."""
    alphabet = np.array([p for p in range(1, 404) if p != 3])
    kws = [(rng.choice(alphabet, size=int(rng.integers(1, 7))).tolist(), float(rng.uniform(0.5, 4.0))) for _ in range(1000)]
    toks = [(int(t), float(v)) for t, v in zip(rng.choice(V, 100, replace=False), rng.standard_normal(100))]
    return toks, kws


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
    codes = torch.from_numpy(rng.integers(0, cfg.audio_vocab_size - 1, (8, B, cfg.audio_codebooks)).astype(np.int32)).to(dev)
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    text = torch.zeros(B, dtype=torch.int32, device=dev)
    prs = torch.zeros(max(cfg.extra_heads_num, 1) * B, device=dev)
    torch.cuda.synchronize()
    eng.debug_set_positions(3 * cfg.lm.context + 11, 0)  # steady state: every ring row is read

    def run(n):
        for i in range(n):
            eng.step_tokens_dev(codes[i % 8].data_ptr(), mask.data_ptr(), text.data_ptr(), prs.data_ptr())
        eng.sync()

    has = hasattr(eng, "set_text_bias")
    settings = [("off", None)]
    info = None
    if has:
        handle = eng.bias_create(*big_set(cfg.text_out_vocab_size, np.random.default_rng(1)))
        info = eng.bias_info(handle)
        settings = [("off", (False, 0)), ("on, nothing attached", (True, 0)), ("on, 1000 keywords + 100 token biases on every slot", (True, handle))]
    lines, per = [], {name: [] for name, _ in settings}
    for r in range(args.repeats):
        for name, how in (settings if r % 2 == 0 else settings[::-1]):
            if how is not None:
                eng.set_text_bias(how[0])
                for b in range(B):
                    eng.set_bias(b, how[1])
            run(args.warmup)
            g0 = eng.metrics().graph_launches
            t0 = time.perf_counter()
            run(args.steps)
            us = 1e6 * (time.perf_counter() - t0) / args.steps
            m = eng.metrics()
            per[name].append(us)
            lines.append({"tree": args.tag, "leg": name, "repeat": r, "us_per_step": round(us, 2), "steps": args.steps, "batch": B,
                          "graph_launches_in_window": int(m.graph_launches - g0), "capture_failures": int(m.capture_failures)})
            print(json.dumps(lines[-1]), flush=True)
    summary = {"tree": args.tag, "set": info, "summary_us_per_step": {k: {"mean": round(float(np.mean(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                                                      for k, v in per.items()}}
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
