#!/usr/bin/env python3
"""bench.py — per-80 ms-frame batched STT step on MI355X (Mimi encode + delayed-streams LM decode).

One "step" = one 80 ms frame for every stream slot of the batch: dsm_asr_step_pcm_dev = SEANet
encoder + Mimi transformer + RVQ encode + LM step (16 layers over the full ring KV cache) + argmax,
with PCM, mask and every state tensor resident in HBM.  Workload: stt-1b-en_fr, bf16 weights / bf16
KV, batch 64 per GPU (BASELINE.json configs[1]); synthetic Philox weights and PCM (no checkpoints
offline).  Before the warmup an UNTIMED fill of `context` steps brings every slot's ring cache to
steady state, so each timed step streams the whole 750-frame KV cache.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
      A plain run sets up, fills the rings, warms up, times K steps and prints the headline line; --dump-outputs also
      writes what the last timed step returned as DIR/<name>.npy.  --full adds every other measurement (roofline passes,
      capacity / host-path / other-configuration legs, dot_mode agreement, CPU baseline) to the line.
      N > 1 without a launcher: spawns N ranks itself (python -m torch.distributed.run ... bench.py, as child
      processes, before this process imports torch); under a launcher (WORLD_SIZE set) it is one of the ranks.

Prints ONE JSON line on rank 0.  Multi-GPU: independent stream batches per GPU (weak scaling), no
per-step collective; the shared weights are fanned out once at load with an RCCL broadcast.
"""
import argparse
import ctypes as C
import json
import subprocess
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="stream slots per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything that is not the headline figure: the roofline / per-class profiling "
                         "passes, capacity and host-path legs, the other dot_mode, the other configurations, the dot_mode agreement pass, "
                         "the CPU baseline and (--workload tts) the guided leg; the options below that select or skip those legs only "
                         "matter with --full")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step returned (stt: codes, text_tokens, vad_probs; "
                         "mimi-decode: pcm; tts: text_tokens, audio_tokens) as DIR/<name>.npy (float32; integer tokens and codes as float64); inputs are seeded, so two "
                         "builds run with the same arguments can be compared array for array")
    ap.add_argument("--config", default="stt-1b-en_fr", choices=["stt-1b-en_fr", "stt-2.6b-en", "tiny"])
    ap.add_argument("--dot-mode", type=int, default=1, choices=[0, 1],
                    help="dsm_asr_config.dot_mode of the timed engine.  1 (bench default): the LM's bf16-weight GEMMs on v_mfma_f32_16x16x32_bf16 "
                         "over the exact three-way bf16 split of the f32 activations; 0 (the config constructors' default): the f32 fmaf "
                         "chain on v_mfma_f32_16x16x4_f32.  Each mode is bit-exact against the oracle run in the same mode; the other "
                         "mode's step time is reported beside the headline as `other_dot_mode`")
    ap.add_argument("--spawn-check-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)      # tests: this rank raises mid-run
    ap.add_argument("--spawn-check-arena-skew-rank", type=int, default=-1, help=argparse.SUPPRESS)  # tests: this rank reports another arena size
    ap.add_argument("--host-path-legs", default="400,2048,2560",
                    help="batch sizes for the end-to-end host-path legs (tools/host_path_bench: msgpack in, worker threads, H2D, "
                         "msgpack out); empty = skip")
    ap.add_argument("--host-path-frames", type=int, default=16)
    ap.add_argument("--workload", default="stt", choices=["stt", "mimi-decode", "tts"],
                    help="stt = Mimi encode + LM decode (the headline metric); mimi-decode = Mimi::decode_step only (config 5)")
    ap.add_argument("--no-fill", action="store_true", help="skip the untimed ring-cache fill (debug only)")
    ap.add_argument("--fast-fill", action="store_true",
                    help="profiling aid: jump the ring positions to steady state instead of running `context` fill steps")
    ap.add_argument("--no-overlap", action="store_true", help="single-stream step_pcm instead of the encoder/model stream pipeline")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=4, help="oracle frames timed for cpu_baseline (a full-ring frame of 64 streams takes a few seconds on 16 cores)")
    ap.add_argument("--capacity-legs", default="400,2048,2304,2560,2688",
                    help="comma-separated larger batches timed after the headline run (N = 1 only; '' to skip)")
    ap.add_argument("--part", default="all", choices=["all", "lm", "enc"],
                    help="experiment: time only the LM step (codes fed from a fixed device buffer) or only the Mimi encode")
    ap.add_argument("--spawn-check", action="store_true",
                    help="CPU rehearsal of the multi-rank control path (gloo): no engine, no GPU")
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    ap.add_argument("--other-configs", default="stt-2.6b-en:128,tts:32",
                    help="the other single-GPU BASELINE.json configurations, run as short legs after the headline (N = 1, stt-1b-en_fr at "
                         "B = 64 only) and reported under `other_configs`: `<config>:<batch>` with config stt-2.6b-en or tts; '' to skip")
    ap.add_argument("--no-agreement", action="store_true", help="skip the dot_mode 1 vs dot_mode 0 agreement pass (`dot_mode_agreement`)")
    ap.add_argument("--tts-guided-leg", type=int, default=1, help="--workload tts: also time the cfg_rows = 1 engine (two batch rows per slot, guidance on)")
    return ap.parse_args()


def dump_outputs(args, world, rank, arrays):
    """--dump-outputs: one .npy per returned array, float32 for floating-point outputs and float64 for integer tokens /
    codes (exact for every uint32); with several ranks each writes its own `<name>.rank<r>.npy`."""
    if not args.dump_outputs:
        return
    os.makedirs(args.dump_outputs, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(args.dump_outputs, name + ("" if world == 1 else ".rank%d" % rank) + ".npy"),
                a.astype(np.float32 if a.dtype == np.float32 else np.float64))


def other_config_leg(args, spec):
    """One of the other BASELINE.json configurations as a child `bench.py` run on the same GPU (its own engine and a synthetic
    checkpoint in a scratch directory that is deleted afterwards); returns the fields VERDICT r03 #4 asks for."""
    import shutil
    import tempfile
    name, batch = spec.split(":")
    wd = tempfile.mkdtemp(prefix="dsm_other_", dir=os.path.dirname(args.weights_dir.rstrip("/")) or "/tmp")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--batch", batch, "--steps", "30", "--warmup", "5", "--no-cpu-baseline",
           "--capacity-legs", "", "--host-path-legs", "", "--other-configs", "", "--no-agreement", "--dot-mode", str(args.dot_mode), "--weights-dir", wd]
    cmd += ["--workload", "tts"] if name == "tts" else ["--config", name, "--fast-fill"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": (r.stderr or r.stdout)[-300:]}
        j = json.loads(lines[-1])
        out = {"metric": j["metric"], "ms_per_step": j["ms_per_step"], "rtf": j["rtf"], "value": j["value"], "dot_mode": j.get("dot_mode"),
               "workload": j["config"]["workload"],
               "roofline": {k: j["roofline"].get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_us", "algorithmic_bytes_per_launch")}}
        if "isolated_single_stream" in j["roofline"]:
            out["roofline"]["isolated_frac"] = j["roofline"]["isolated_single_stream"]["frac"]
        if "whole_step" in j:
            out["whole_step_frac_of_hbm_peak"] = j["whole_step"]["frac_of_hbm_peak"]
        for k in ("guided_leg", "pipelined"):
            if k in j:
                out[k] = j[k]
        out["how"] = "child run of bench.py on the same GPU after the headline: 30 timed steps" + ("" if name == "tts" else ", ring positions jumped to the wrapped steady state (--fast-fill)")
        return out
    except Exception as ex:
        return {"error": str(ex)[:300]}
    finally:
        shutil.rmtree(wd, ignore_errors=True)


def cpu_baseline(cfg, B, lm_path, mimi_path, n_steps):
    """The oracle (CPU restatement, kind "port") timed on the host cores on a bounded sample of the same workload:
    n_steps frames of the same batch with every ring jumped to the wrapped steady state the GPU is timed in
    (full-length attention; the cache contents do not change the arithmetic count)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from dsm_amd import synth
    oracle.build()
    # timed in dot_mode 0 whatever the GPU line runs: mode 0 is plain f32 fused multiply-adds, what a CPU implementation of the
    # reference path does; mode 1's restatement emulates the GPU's bf16 matrix instruction in integers — a checker, not a baseline
    cfg = type(cfg).from_buffer_copy(cfg)
    cfg.dot_mode = 0
    t0 = time.time()
    o = oracle.OracleAsr(cfg, B, lm_path, mimi_path)
    load_s = time.time() - t0
    pcm = synth.synth_pcm(B, n_steps + 1, seed=1000)
    mask = np.ones(B, dtype=np.uint8)
    o.step_pcm(pcm[0], mask)  # untimed first touch
    o.debug_set_positions(3 * cfg.lm.context + 11, 3 * cfg.mimi.transformer.context + 5)
    t0 = time.time()
    for s in range(n_steps):
        o.step_pcm(pcm[1 + s], mask)
    dt = (time.time() - t0) / n_steps
    o.close()
    cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    return {"value": B * 0.08 / dt, "unit": "x realtime (stream-seconds of audio per wall second)",
            "cores": cores, "kind": "port", "dot_mode": 0,
            "sample": f"{n_steps} frame(s) x {B} streams on full rings ({cfg.lm.context} LM / {cfg.mimi.transformer.context} Mimi frames, "
                      f"the steady state the GPU line is timed in), {dt * 1000:.0f} ms/step, oracle load {load_s:.0f} s; "
                      "dot_mode 0 (f32 fma dot products); Candle itself cannot be built offline"}


def bench_decode(args, eng, cfg, B, dev, world, rank, dist, torch):
    """BASELINE.json configs[4] (TTS path, Mimi decode side only): codes -> PCM for B slots per 80 ms frame."""
    rng = np.random.default_rng(1 + rank)
    n_q = cfg.mimi.quantizer_n_q
    codes = torch.from_numpy(rng.integers(0, cfg.mimi.quantizer_bins, (16, B, n_q)).astype(np.int32)).to(dev)
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    pcm = torch.zeros(B * 1920, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    it = 0
    if args.fast_fill or not args.no_fill:
        for _ in range(cfg.mimi.transformer.context // 2 + 4):  # decoder transformer ring (250 @ 25 Hz) full
            eng.decode_step_dev(codes[it % 16].data_ptr(), mask.data_ptr(), pcm.data_ptr())
            it += 1
    for _ in range(args.warmup):
        eng.decode_step_dev(codes[it % 16].data_ptr(), mask.data_ptr(), pcm.data_ptr())
        it += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.decode_step_dev(codes[it % 16].data_ptr(), mask.data_ptr(), pcm.data_ptr())
        it += 1
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1000
    dump_outputs(args, world, rank, {"pcm": pcm.cpu().numpy().reshape(B, 1920)})
    if rank == 0:
        print(json.dumps({"metric": "Mimi decode_step real-time stream throughput @ bs=%d" % B, "value": world * B * 0.08 / (ms / 1000),
                          "unit": "x realtime (stream-seconds of audio per wall second)", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "f32", "data": "synthetic", "rtf": 80.0 / ms,
                          "config": {"workload": "Mimi v0_1 decode_step (32 codebooks -> 1920 samples), batch=%d" % B}}))
    eng.close()


def bench_tts(args, world, rank, local_rank):
    """BASELINE.json configs[4], LM side: tts_streaming::State::step (main LM + 32-slice depformer, greedy) for B
    generations per 80 ms frame.  Host-pointer ABI (the step's inputs are B tokens); every step synchronises, as the
    reference's does when it reads the sampled tokens back."""
    import torch
    import dsm_amd
    from dsm_amd import synth
    cfg = dsm_amd.config_tts_v202501()  # cross-attention in every main-LM layer, as the reference's tts_202501 (core/lm.rs:392-396)
    cfg.dot_mode = args.dot_mode
    B = args.batch
    path = synth.make_synth_tts_weights(cfg, args.weights_dir, tag="tts-v202501-ca" + ("" if world == 1 else f".rank{rank}"))
    rng = np.random.default_rng(3 + rank)
    mask = np.ones(B, dtype=np.uint8)
    fill = cfg.text_audio_delay_in_tokens + cfg.acoustic_delay + 3  # past both delay windows: every codebook feeds back
    SRC_ROWS = 125  # speaker_cond_n_speakers (5) x 2 s at 12.5 Hz: what the server's conditioner hands State::new (srv/tts.rs:426-441)

    last = [None]  # what the latest step returned: (text tokens, audio tokens)

    def run(c, guided, steps, warmup):
        eng = dsm_amd.TtsEngine(c, B, path, device_id=local_rank)
        empty = synth.synth_ca_src(c, SRC_ROWS, 9)
        for b in range(B):  # the branch the server runs: every generation has a conditioning source
            if guided:
                eng.set_ca_src(b, synth.synth_ca_src(c, SRC_ROWS, 100 + b), empty, 2.0)
            else:
                eng.set_ca_src(b, synth.synth_ca_src(c, SRC_ROWS, 100 + b))

        def step():
            prev = rng.integers(4, c.text_in_vocab_size - 1, B).astype(np.uint32)
            allowed = rng.integers(4, c.text_in_vocab_size - 1, B).astype(np.int32)
            last[0] = eng.step(prev, allowed, mask)

        for _ in range(fill + warmup):
            step()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=torch.device("cuda", local_rank))
        if world > 1:
            dist.barrier()
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        m = eng.metrics()
        eng.close()
        return float(dt.item()) / steps * 1000, m

    ms, m = run(cfg, False, args.steps, args.warmup)
    dump_outputs(args, world, rank, {"text_tokens": last[0][0], "audio_tokens": last[0][1]})
    guided = None
    if args.full and args.tts_guided_leg and world == 1:
        gcfg = type(cfg).from_buffer_copy(cfg)
        gcfg.cfg_rows = 1
        gms, _ = run(gcfg, True, min(args.steps, 20), 3)
        guided = {"ms_per_step": gms, "rtf": 80.0 / gms, "batch_rows": 2 * B,
                  "what": "cfg_rows = 1: every slot runs a conditional and an unconditional row, logits mixed l0 * a - l1 * (a - 1) "
                          "(core/tts_streaming.rs:164-173,207-214), alpha 2.0 on every slot"}
    if world > 1:
        os.remove(path)
    if rank == 0:
        wbytes = m.algorithmic_bytes_lm
        achieved = wbytes / (ms * 1e-3) / 1e9
        print(json.dumps({"metric": "TTS step real-time generation throughput @ bs=%d" % B, "value": world * B * 0.08 / (ms / 1000),
                          "unit": "x realtime (seconds of audio tokens per wall second)", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": ("bf16 weights, f32 activations as three exact bf16 pieces, f32 accumulate" if args.dot_mode == 1
                                    else "bf16 weights, f32 activations/accumulate"),
                          "data": "synthetic", "rtf": 80.0 / ms, "dot_mode": args.dot_mode,
                          "config": {"workload": "tts v202501 State::step (2048-d x 16 LM with cross-attention to a %d-row source per slot + "
                                                 "32-slice depformer, greedy), batch=%d, KV fill %d frames" % (SRC_ROWS, B, fill + args.warmup)},
                          "guided_leg": guided,
                          # the step is one dependent chain of ~1400 launches of 4-7 us (profiles/r03/tts_kernel_trace_summary.txt):
                          # no kernel dominates, so the roofline object prices the WHOLE step against the bytes it has to stream
                          "roofline": {"bound": "hbm", "kernel": "whole step (launch-bound chain: 16 LM layers + 32 depformer slices x 4 layers, "
                                                                  "every GEMM / reduce / attention launch 4-22 us at %d rows)" % B,
                                       "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                                       "algorithmic_bytes_per_launch": wbytes,
                                       "what": "bf16 weight matrices multiplied per step, each counted once (dsm_tts_get_metrics); "
                                               "embedding rows and the short KV reads left out",
                                       "avg_launch_us": ms * 1000.0, "timer": "host wall clock over the timed steps (each step synchronises)",
                                       "traffic": None},
                          "graphs": {"graph_launches": int(m.graph_launches), "eager_bodies": int(m.eager_bodies),
                                     "capture_failures": int(m.capture_failures)}}))


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N fresh ranks (one per GPU) with torch.distributed.run and
    let rank 0's JSON line through.  This parent has not imported torch nor touched the GPU, and it never execs: the
    ranks are child processes and their exit code becomes ours."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def rank_report(dist, torch, dev, ms_per_step, arena_bytes):
    """Every rank's step time and arena size on every rank (all_gather): rank 0 prints them, and ANY rank that sees a
    disagreement about the weight arena exits non-zero (a rank that attached to different bytes would serve different
    weights: SURVEY.md §8(e))."""
    mine = torch.tensor([ms_per_step, float(arena_bytes)], dtype=torch.float64, device=dev)
    allr = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(allr, mine)
    per_rank_ms = [float(t[0].item()) for t in allr]
    arenas = [int(t[1].item()) for t in allr]
    if len(set(arenas)) != 1:
        raise SystemExit("ranks disagree about the weight arena: %s bytes" % arenas)
    return per_rank_ms


def spawn_check(args, world, rank):
    """CPU rehearsal of the N > 1 control path (tests/test_bench_spawn_cpu.py): gloo process group, the load-time
    broadcast of a byte blob, barrier-bracketed timing with a MAX over ranks, one JSON line on rank 0.  No engine."""
    import torch
    import torch.distributed as dist
    from dsm_amd import sharding
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    blob = torch.arange(1 << 16, dtype=torch.int64).to(torch.uint8) if rank == 0 else torch.zeros(1 << 16, dtype=torch.uint8)
    sharding.broadcast_tensor_(blob, 0, dist, chunk_bytes=10000)
    ok = bool((blob == torch.arange(1 << 16, dtype=torch.int64).to(torch.uint8)).all())
    dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    if rank == args.spawn_check_fail_rank:
        # a rank dying mid-run: the launcher (torch.distributed.run's agent) must take the others down from their barrier and
        # hand a non-zero exit code to `bench.py --gpus N` — no hang, no JSON line that looks like a result
        raise RuntimeError("spawn-check: rank %d fails on purpose" % rank)
    dist.barrier()
    own = time.perf_counter() - t0
    dt = torch.tensor([own], dtype=torch.float64)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    flags = torch.tensor([1 if ok else 0], dtype=torch.int64)
    dist.all_reduce(flags, op=dist.ReduceOp.MIN)
    per_rank = rank_report(dist, torch, torch.device("cpu"), own * 1000.0, (1 << 16) + (1 if rank == args.spawn_check_arena_skew_rank else 0))
    if rank == 0:
        print(json.dumps({"metric": "spawn-check", "n_gpus": world, "value": float(dt.item()), "unit": "s", "steps": args.steps,
                          "warmup": args.warmup, "broadcast_ok": bool(flags.item()), "backend": "gloo", "per_rank_ms": per_rank}))
    dist.destroy_process_group()


def timed_steps(step, n, barrier):
    barrier()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    barrier()
    return time.perf_counter() - t0


def capacity_leg(dsm_amd, synth, cfg, B, arena, dev, local_rank, steps, torch):
    """One extra engine of B slots attached to the already loaded weight arena, ring positions jumped to steady state
    (cache content is whatever HBM holds: same traffic, same arithmetic), a short warmup and `steps` timed frames of the
    two-stream pipeline.  Returns ms per step."""
    ptr, nbytes, manifest = arena
    eng = dsm_amd.AsrEngine(cfg, B, device_id=local_rank, arena=(ptr, nbytes, manifest))
    try:
        n_pcm = 4
        pcm = torch.from_numpy(synth.synth_pcm(64, n_pcm, seed=77)).to(dev).repeat(1, (B + 63) // 64, 1)[:, :B].contiguous()
        mask = torch.ones(B, dtype=torch.uint8, device=dev)
        text = torch.zeros(B, dtype=torch.int32, device=dev)
        prs = torch.zeros(max(cfg.extra_heads_num, 1) * B, dtype=torch.float32, device=dev)
        codes = torch.zeros(B * cfg.audio_codebooks, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.debug_set_positions(4 * cfg.lm.context, 4 * cfg.mimi.transformer.context)
        it = [0]

        def step():
            eng.encode_step_dev(pcm[it[0] % n_pcm].data_ptr(), mask.data_ptr(), codes.data_ptr())
            eng.step_tokens_dev(None, mask.data_ptr(), text.data_ptr(), prs.data_ptr())
            it[0] += 1

        for _ in range(3):
            step()
        dt = timed_steps(step, steps, torch.cuda.synchronize)
        return dt / steps * 1000.0
    finally:
        eng.close()


def headline(args, cfg, B, world, ms_per_step, fill, groups, fan, per_rank_ms):
    """The fields of the result line that the timed steps alone determine (a plain run prints exactly these)."""
    return {
        "metric": "real-time stream throughput, %s @ bs=%d per GPU (Mimi encode + LM decode per 80 ms frame)" % (args.config, B),
        "value": world * B * 0.08 / (ms_per_step / 1000.0),
        "unit": "x realtime (stream-seconds of audio per wall second)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "weak",
        # BASELINE.md's published figure for this metric: 64 streams @ 3x real time = 192 x realtime at batch_size 64,
        # on 1x NVIDIA L40S (reference README.md:73-74) — other hardware, quoted for scale only
        "vs_baseline": (B * 0.08 / (ms_per_step / 1000.0)) / 192.0 if (args.config == "stt-1b-en_fr" and B == 64) else None,
        "baseline": "64 streams @ 3x real time (192 x realtime) on 1x L40S, per GPU (BASELINE.md)",
        "dtype": ("bf16 weights + bf16 KV, f32 activations as three exact bf16 pieces, f32 accumulate (v_mfma_f32_16x16x32_bf16)"
                  if args.dot_mode == 1 else "bf16 weights + bf16 KV, f32 activations/accumulate (v_mfma_f32_16x16x4_f32)"),
        "data": "synthetic", "dot_mode": args.dot_mode,
        "rtf": 80.0 / ms_per_step,
        "config": {"workload": "%s batch=%d streaming, ring KV cache full (%d frames), Mimi encode + LM decode HIP path"
                               % (args.config, B, fill),
                   "streams_per_gpu": B, "parallelism": "replicas x%d (independent stream batches, no per-step collective)" % world,
                   "streams": "single stream" if args.no_overlap else "encoder stream || %d LM group stream(s)" % len(groups),
                   "rccl_ranks": world if world > 1 else None,
                   "weights_broadcast_ms": fan["broadcast_ms"] if fan else None,
                   "weights_broadcast_bytes": fan["arena_bytes"] if fan else None,
                   "weights_broadcast_gbps": (fan["arena_bytes"] / (fan["broadcast_ms"] * 1e-3) / 1e9) if fan and fan["broadcast_ms"] > 0 else None,
                   "per_rank_ms_per_step": per_rank_ms,
                   "weights_broadcast": "packed device weight arena, rank 0 -> all, RCCL over xGMI, once at load" if fan else None},
    }


def main():
    args = parse()
    world_env = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and world_env is None:
        sys.exit(spawn_ranks(args))  # before torch is imported or the GPU touched in this process
    world = int(world_env or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_env is not None and args.gpus != world and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks; reporting n_gpus = {world}", file=sys.stderr)
    if args.spawn_check:
        return spawn_check(args, world, rank)
    import torch
    import torch.distributed as dist
    import dsm_amd
    from dsm_amd import synth, sharding

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the engine has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)  # "nccl" is RCCL on ROCm
    if args.workload == "tts":
        return bench_tts(args, world, rank, local_rank)

    cfg = {"stt-1b-en_fr": dsm_amd.config_stt_1b_en_fr, "stt-2.6b-en": dsm_amd.config_stt_2_6b_en,
           "tiny": dsm_amd.config_tiny}[args.config]()
    cfg.dot_mode = args.dot_mode
    B = args.batch
    tag = args.config
    # rank 0 writes + loads the synthetic checkpoint; the other ranks receive the packed device weight arena over RCCL
    # (the only collective of the whole path) and attach to it
    lm_path = mimi_path = None
    if rank == 0:
        lm_path, mimi_path = synth.make_synth_weights(cfg, args.weights_dir, tag=tag)
    fan = None
    if world > 1:
        eng, fan = sharding.fan_out_engine(dsm_amd, cfg, B, lm_path, mimi_path, dist, dev, src=0)
    else:
        eng = dsm_amd.AsrEngine(cfg, B, lm_path, mimi_path, device_id=local_rank)

    if args.workload == "mimi-decode":
        return bench_decode(args, eng, cfg, B, dev, world, rank, dist, torch)
    if args.no_overlap:
        eng.debug_serialize_groups(True)  # one stream for everything: kernels run alone (profiling runs)
    ctx = cfg.lm.context
    n_pcm = 16
    pcm = torch.from_numpy(synth.synth_pcm(B, n_pcm, seed=1000 + 7919 * rank)).to(dev)  # [n_pcm, B, 1920]
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    text = torch.zeros(B, dtype=torch.int32, device=dev)
    prs = torch.zeros(max(cfg.extra_heads_num, 1) * B, dtype=torch.float32, device=dev)
    codes = torch.zeros(B * cfg.audio_codebooks, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # uploads above ran on torch's stream; the engine's streams are not ordered against it
    it = [0]

    def step():
        i = it[0]
        it[0] += 1
        if args.part == "lm":
            eng.step_tokens_dev(codes.data_ptr(), mask.data_ptr(), text.data_ptr(), prs.data_ptr())
        elif args.part == "enc":
            eng.encode_step_dev(pcm[i % n_pcm].data_ptr(), mask.data_ptr(), codes.data_ptr())
        elif args.no_overlap:  # everything on one stream (asr::State::step_pcm)
            eng.step_pcm_dev(pcm[i % n_pcm].data_ptr(), mask.data_ptr(), codes.data_ptr(), text.data_ptr(), prs.data_ptr())
        else:
            # the reference's two-thread pipeline (srv/batched_asr.rs:314-522): Mimi encode on the encoder stream, LM
            # step on the model stream; encode of frame i+1 overlaps the LM step of frame i, codes handed over on-device
            eng.encode_step_dev(pcm[i % n_pcm].data_ptr(), mask.data_ptr(), codes.data_ptr())
            eng.step_tokens_dev(None, mask.data_ptr(), text.data_ptr(), prs.data_ptr())

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if args.fast_fill:
        eng.debug_set_positions(4 * ctx, 4 * cfg.mimi.transformer.context)
    elif not args.no_fill:
        for _ in range(ctx):
            step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    # ---- timed region: exactly K steps, no instrumentation of any kind inside it ----
    eng.prof_enable([])
    dt = timed_steps(step, args.steps, barrier)
    dt_t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(dt_t, op=dist.ReduceOp.MAX)
    own_ms = dt / args.steps * 1000.0
    dt = float(dt_t.item())
    ms_per_step = dt / args.steps * 1000.0
    per_rank_ms = rank_report(dist, torch, dev, own_ms, eng.weight_arena()[1]) if world > 1 else [own_ms]
    # what the last timed step handed back, copied out before any later pass steps over the same buffers
    dump_outputs(args, world, rank, {"codes": codes.cpu().numpy().reshape(B, cfg.audio_codebooks), "text_tokens": text.cpu().numpy(),
                                     "vad_probs": prs.cpu().numpy().reshape(-1, B)} if args.dump_outputs else {})
    fill = ctx if not args.no_fill else min(it[0], ctx)
    if not args.full:  # a plain run ends here: the headline line and nothing that takes steps of its own
        if rank == 0:
            print(json.dumps(headline(args, cfg, B, world, ms_per_step, fill, eng.stream_groups(), fan, per_rank_ms)))
        eng.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- separate pass (not part of `value`): the dominant kernel bracketed live, i.e. with the other streams running
    # beside it — HIP events on the stream it is launched on + the in-kernel device-clock bracket ----
    n_prof = min(args.steps, 20)
    eng.prof_enable(["attn_lm"])
    eng.prof_read()
    eng.prof_read_device()
    dt_prof = timed_steps(step, n_prof, torch.cuda.synchronize)
    prof = eng.prof_read()
    prof_dev = eng.prof_read_device()
    eng.prof_enable([])

    # one extra single-stream pass: per-class device time of a step, and the dominant kernel timed without a concurrent
    # stream competing for HBM
    overlap = not args.no_overlap
    args.no_overlap = True
    torch.cuda.synchronize()
    eng.debug_serialize_groups(True)  # stream groups one after the other: nothing overlaps in this pass
    eng.prof_enable(dsm_amd.PROF_TAGS)
    eng.prof_read()
    eng.prof_read_device()
    for _ in range(5):
        step()
    iso = eng.prof_read()
    iso_dev = eng.prof_read_device()
    breakdown = {k: round(v[0] / 5.0, 1) for k, v in iso.items()}
    eng.prof_enable([])
    eng.debug_serialize_groups(not overlap)
    args.no_overlap = not overlap
    groups = eng.stream_groups()

    # ---- capacity legs (N = 1 only): larger batches attached to the same weight arena.  BASELINE.json's north star is
    # ">= 400 concurrent real-time streams per MI355X at RTF > 1" ----
    legs = {}
    if world == 1 and args.capacity_legs and args.config != "tiny":
        arena = eng.weight_arena()
        for Bl in [int(x) for x in args.capacity_legs.split(",") if x]:
            try:
                ms = capacity_leg(dsm_amd, synth, cfg, Bl, arena, dev, local_rank, 20 if Bl <= 512 else 8, torch)
                legs[Bl] = {"ms_per_step": ms, "rtf": 80.0 / ms, "x_realtime": Bl * 80.0 / ms}
            except Exception as ex:  # e.g. another tenant's memory on the card: report, do not lose the headline line
                legs[Bl] = {"error": str(ex)[:200]}
            torch.cuda.empty_cache()

    # the same batch in the other dot_mode (same weight arena, steady-state ring positions, 30 timed steps)
    other_mode = None
    if world == 1 and args.config != "tiny" and args.part == "all" and not args.no_overlap:
        try:
            ocfg = type(cfg).from_buffer_copy(cfg)
            ocfg.dot_mode = 1 - args.dot_mode
            oms = capacity_leg(dsm_amd, synth, ocfg, B, eng.weight_arena(), dev, local_rank, 30, torch)
            other_mode = {"dot_mode": ocfg.dot_mode, "ms_per_step": oms, "value": B * 80.0 / oms}
        except Exception as ex:
            other_mode = {"error": str(ex)[:200]}
        torch.cuda.empty_cache()

    # ---- host-path legs (N = 1 only): the same batches driven end to end from HOST audio through the worker — per-channel
    # msgpack InMsg::Audio decode, the reference's encoder / model thread split with run-ahead, pinned staging + H2D, LM step,
    # OutMsg::Step fan-out and drain (tools/host_path_bench.cpp).  VERDICT r02 #5: the device-resident legs above say nothing
    # about the host side at 2 048 slots. ----
    host_legs = {}
    if world == 1 and args.host_path_legs and args.config == "stt-1b-en_fr" and args.part == "all" and not args.no_overlap:
        exe = os.path.join(ROOT, "tools", "host_path_bench")
        for Bl in [int(x) for x in args.host_path_legs.split(",") if x]:
            try:
                if not os.path.exists(exe):
                    raise RuntimeError("tools/host_path_bench is not built (__graft_entry__.build())")
                r = subprocess.run([exe, lm_path, mimi_path, str(Bl), str(args.host_path_frames), "8", str(args.dot_mode)], capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    raise RuntimeError((r.stderr or r.stdout)[-200:])
                host_legs[Bl] = json.loads(r.stdout.strip().splitlines()[-1])
            except Exception as ex:
                host_legs[Bl] = {"error": str(ex)[:200]}

    # dot_mode 1 against dot_mode 0 on this build, these weights, full rings (delayed-streams-modeling_amd/agreement.py)
    agree = None
    if world == 1 and args.config == "stt-1b-en_fr" and args.part == "all" and not args.no_overlap and not args.no_agreement:
        try:
            from dsm_amd import agreement
            agree = agreement.asr_agreement(dsm_amd, cfg, 8, lm_path, mimi_path, arena=eng.weight_arena(), steps=30, device_id=local_rank)
            agree.pop("flips", None)
        except Exception as ex:
            agree = {"error": str(ex)[:200]}
        torch.cuda.empty_cache()
    others = {}
    if world == 1 and args.config == "stt-1b-en_fr" and B == 64 and args.part == "all" and not args.no_overlap and args.other_configs:
        for spec in [x for x in args.other_configs.split(",") if x]:
            others[spec] = other_config_leg(args, spec)

    if rank == 0:
        H, hd, L = cfg.lm.num_heads, cfg.lm.d_model // cfg.lm.num_heads, cfg.lm.num_layers
        kv_b = 2 if cfg.kv_bf16 else 4
        # algorithmic bytes of the attention launches of ONE layer: K and V of every (slot, head) once + q in + out.
        # The LM step runs the batch as len(groups) stream groups, each with its own attention launch per layer, so a
        # launch covers B / len(groups) slots on average and `achieved` is bytes of all timed launches / their time.
        # Fused prologue (default, DSM_FUSE_QKV): the launch also sums the QKV GEMM's split-K slabs for its 3*hd values
        # (chunks = d/256 partials each, f32) and writes the new K/V row, instead of reading q.
        fused = os.environ.get("DSM_FUSE_QKV", "1") != "0"
        chunks = (cfg.lm.d_model + 255) // 256
        per_head = 2 * fill * hd * kv_b + hd * 4 + ((3 * hd * 4 * chunks + 2 * hd * kv_b) if fused else hd * 4)
        attn_bytes_layer = B * H * per_head
        attn_bytes = attn_bytes_layer / len(groups)
        # HBM traffic of the same kernel from the committed rocprofv3 PMC passes (bench.py cannot run under --pmc and
        # time itself): 2 x FETCH_SIZE (gfx950 counts 64 B per 128-B request) + WRITE_SIZE, per dispatch
        traffic, traffic_src = None, None
        for rnd in ("r04", "r03", "r02", "r01"):
            try:
                pmc = json.load(open(os.path.join(ROOT, "profiles", rnd, "pmc_hbm_traffic.json")))
                for k in pmc["kernels"]:
                    if ("attn_kernel<unsigned short, %d, 1" % hd in k["kernel"] and args.config == "stt-1b-en_fr"
                            and B == 64 and k.get("slots_per_dispatch", 64) * len(groups) == B):
                        traffic = (2 * k["FETCH_SIZE_KB_per_dispatch"] + k["WRITE_SIZE_KB_per_dispatch"]) * 1024
                        traffic_src = f"profiles/{rnd}/pmc_hbm_traffic.json (rocprofv3 --pmc, separate passes; not measured in this run)"
            except Exception:
                pass
            if traffic:
                break
        m = eng.metrics()
        step_bytes = m.algorithmic_bytes_lm + m.algorithmic_bytes_encode
        # launch duration = in-kernel device-clock bracket (first workgroup in -> last out), the quantity rocprofv3's
        # kernel trace reports; the HIP-event bracket on the launching stream is kept beside it: with three streams in
        # flight it also contains the time the launch queues behind the other streams' kernels
        attn_us, attn_n = prof_dev["attn_lm"]
        attn_avg_us = attn_us / max(attn_n, 1) or float("nan")
        ev_us, ev_n = prof["attn_lm"]
        achieved = attn_bytes / (attn_avg_us * 1e-6) / 1e9 if attn_n else 0.0
        iso_avg_us = iso_dev["attn_lm"][0] / max(iso_dev["attn_lm"][1], 1) or float("nan")  # --part enc: no LM attention ran
        ok_legs = [b for b, v in legs.items() if "rtf" in v and v["rtf"] >= 1.0]
        out = {
            **headline(args, cfg, B, world, ms_per_step, fill, groups, fan, per_rank_ms),
            "other_dot_mode": other_mode,
            "roofline": {"bound": "hbm", "kernel": "attn_kernel<bf16,hd%d,T1> (LM ring-cache attention%s, %d launches/step: %d layers x %d stream groups of %s slots)"
                                                    % (hd, " with the fused QKV reduce + RoPE + ring scatter prologue" if fused else "", L * len(groups), L, len(groups), "/".join(str(n) for _, n in groups)),
                         "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                         "algorithmic_bytes_per_launch": attn_bytes, "avg_launch_us": attn_avg_us,
                         "launches_timed": int(attn_n), "timer": "device wall clock inside the kernel (agrees with rocprofv3 --kernel-trace)",
                         "hip_event_bracket_avg_us": ev_us / max(ev_n, 1), "traffic": traffic,
                         "traffic_source": traffic_src,
                         "isolated_single_stream": {"avg_launch_us": iso_avg_us,
                                                    "achieved": attn_bytes / (iso_avg_us * 1e-6) / 1e9,
                                                    "frac": attn_bytes / (iso_avg_us * 1e-6) / 1e9 / 8000.0}},
            "step_breakdown_us_single_stream": breakdown,
            "whole_step": {"algorithmic_bytes": step_bytes, "achieved": step_bytes / (ms_per_step * 1e-3) / 1e9, "unit": "GB/s",
                           "frac_of_hbm_peak": step_bytes / (ms_per_step * 1e-3) / 1e9 / 8000.0},
        }
        out["config"]["timed_region"] = ("instrumentation off; roofline brackets come from a separate %d-step pass (%.3f ms/step with the brackets on)"
                                         % (n_prof, dt_prof / n_prof * 1000.0))
        if legs:
            out["capacity"] = {"legs": {str(b): v for b, v in legs.items()},
                               "streams_at_rtf_ge_1": max(ok_legs) if ok_legs else None,
                               "rtf_b400": legs.get(400, {}).get("rtf"),
                               "note": "same engine build and weight arena, ring positions jumped to steady state, two-stream pipeline, "
                                       "timed without instrumentation; north star: >= 400 real-time streams per MI355X"}
            if host_legs:
                # what can be promised: the largest measured batch whose RTF keeps a 10 % margin on BOTH the device-resident step
                # and (where it was driven) the whole host path
                safe = [b for b in legs if legs[b].get("rtf", 0.0) >= 1.10 and host_legs.get(b, {}).get("rtf", 0.0) >= 1.10]
                out["capacity"]["host_path"] = {
                    "legs": {str(b): v for b, v in host_legs.items()},
                    "what": "end to end from host audio: msgpack InMsg::Audio per channel (8 feeder threads) -> dsm_worker_send -> "
                            "dsm_worker_step_encode (pre_process, pinned staging, H2D, Mimi encode; run-ahead) || dsm_worker_step_model "
                            "(LM step, post_process, OutMsg::Step per channel) -> dsm_worker_recv; free-running, rtf = 80 ms / ms_per_frame",
                    "streams_at_rtf_ge_1p10_device_and_host": max(safe) if safe else None}
        if agree is not None:
            out["dot_mode_agreement"] = agree
        if others:
            out["other_configs"] = others
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg, B, lm_path, mimi_path, args.cpu_steps)
        print(json.dumps(out))
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
