"""`bench.py` plain run, `--full` and `--dump-outputs` on the tiny configuration (a few seconds on the GPU).

A plain run prints the headline fields only and does nothing after the timed steps; `--full` adds the separate passes
(roofline, per-class breakdown); `--dump-outputs DIR` writes what the last timed step returned, one float32 / float64 .npy per
array, and the single-stream step (`--no-overlap`) writes the same arrays when it is run again with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
B = 4


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--batch", str(B),
                        "--steps", "5", "--warmup", "2"] + extra, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(gpu, dsm, lib, tmp_path):
    cfg = dsm.config_tiny()
    dumps = []
    for name in ("a", "b"):
        out = _bench(["--no-overlap", "--dump-outputs", str(tmp_path / name)])
        for k in HEADLINE:
            assert k in out, k
        assert out["steps"] == 5 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert abs(out["value"] - B * 80.0 / out["ms_per_step"]) <= 1e-9 * out["value"]
        for k in ("roofline", "step_breakdown_us_single_stream", "capacity", "cpu_baseline", "other_dot_mode", "other_configs"):
            assert k not in out, k
        d = {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
        assert sorted(d) == ["codes", "text_tokens", "vad_probs"]
        assert d["codes"].shape == (B, cfg.audio_codebooks) and d["text_tokens"].shape == (B,)
        assert d["vad_probs"].shape == (max(cfg.extra_heads_num, 1), B)
        assert all(a.dtype in (np.float32, np.float64) for a in d.values())
        assert (d["codes"] >= 0).all() and (d["codes"] < cfg.audio_vocab_size).all() and (d["codes"] == np.round(d["codes"])).all()
        assert (d["text_tokens"] >= 0).all() and (d["text_tokens"] < cfg.text_out_vocab_size).all()
        assert np.isfinite(d["vad_probs"]).all() and (d["vad_probs"] >= 0).all() and (d["vad_probs"] <= 1).all()
        dumps.append(d)
    for k in dumps[0]:  # same arguments, same inputs, same single-stream arithmetic: the same arrays
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_full_run_adds_the_separate_passes(gpu, dsm, lib):
    out = _bench(["--full", "--no-cpu-baseline"])
    for k in HEADLINE + ("roofline", "step_breakdown_us_single_stream", "whole_step"):
        assert k in out, k
    assert out["steps"] == 5 and "timed_region" in out["config"]
