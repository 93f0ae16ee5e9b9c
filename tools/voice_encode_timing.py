#!/usr/bin/env python3
"""Device time of dsm_tts_encode_voice at the real Mimi v0_1 shapes (synthetic weights), 1 and 5 clips of 240 000 samples, against
the only route the library offered before it: an STT engine with B = n_clips running 125 x dsm_mimi_encode_step_dev on the same
audio.  Prints a table and one JSON line.

  encode_voice   HIP events around the call's enqueue on the model stream ("spk.stats": upload, normalise, the host's wait for
                 the standard deviations, the whole-clip encode, download), median and minimum over --reps calls after --warmup
                 calls; the scratch bytes come from the same tap, launches per encode from "spk.launches" (kernel nodes of a
                 discarded stream capture of the device side, asked for once per shape).
  streaming      a host clock around 125 steps that ends in dsm_sync (the steps replay as one hipGraph each once two have run, so
                 the loop is device-bound); PCM is already on the device; warmed by one full pass.
The two sides are timed differently (events that span one host wait against a host clock that ends in a synchronise): the ratio
compares two complete calls as a caller sees them, not kernel time against kernel time.

usage: tools/voice_encode_timing.py [--reps 10] [--warmup 3] [--clips 1,5] [--weights DIR]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES = 125  # the shipped 10 s clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", default="1,5")
    ap.add_argument("--weights", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    args = ap.parse_args()
    import torch
    import dsm_amd as dsm
    from dsm_amd import synth
    if not torch.cuda.is_available():
        sys.exit("voice_encode_timing: no HIP device (timings are taken on the GPU only)")
    lib = dsm.load_library()
    # the real Mimi (n_q = 6 codebooks: the tiny TTS model's dep_num_slices) under tiny language models
    cfg_a = dsm.config_tiny()
    lib.dsm_mimi_config_v0_1(C.byref(cfg_a.mimi), 6)
    cfg_a.audio_codebooks = 6
    lm_a, mimi_a = synth.make_synth_weights(cfg_a, args.weights, tag="tiny_mimi_v0_1_nq6")
    cfg_t = dsm.config_tts_tiny(cross_attention=True)
    n_speakers = 5
    cfg_t.ca_max_len = n_speakers * FRAMES
    tts_path = synth.make_synth_tts_weights(cfg_t, args.weights, tag="tts_tiny_ca", speaker=True, mimi_dim=cfg_a.mimi.dimension)
    rng = np.random.default_rng(5)
    t = np.arange(FRAMES * dsm.FRAME_SIZE) / 24000.0
    voices = np.stack([(0.1 * np.sin(2 * np.pi * (120 + 30 * i) * t) + 0.03 * rng.standard_normal(t.size)).astype(np.float32)
                       for i in range(n_speakers)])
    out = {"frames": FRAMES, "n_speakers": n_speakers, "cases": []}
    eng = dsm.TtsEngine(cfg_t, 1, tts_path)
    eng.attach_mimi(cfg_a.mimi, mimi_a)
    eng.attach_speaker_encoder(n_speakers, tts_path)
    for c in [int(x) for x in args.clips.split(",")]:
        clips = voices[:c]
        for _ in range(args.warmup):
            rows = eng.encode_voice(clips)
        ms, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            again = eng.encode_voice(clips)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert again.tobytes() == rows.tobytes(), "encode_voice is not deterministic"
            ms.append(float(eng.debug_read("spk.stats", 2)[1]))
        scratch_mib = float(eng.debug_read("spk.stats", 2)[0])
        launches = float(eng.debug_read("spk.launches", 1)[0])
        # the streaming route on the same audio (normalised on the host: the streaming engine has no normalise kernel)
        x = clips.astype(np.float64)
        norm = (x * 0.08 / x.std(axis=1, keepdims=True)).astype(np.float32)
        asr = dsm.AsrEngine(cfg_a, c, lm_a, mimi_a)
        d_pcm = torch.from_numpy(np.ascontiguousarray(norm.reshape(c, FRAMES, dsm.FRAME_SIZE).transpose(1, 0, 2))).cuda()
        d_mask = torch.ones(c, dtype=torch.uint8, device="cuda")
        d_codes = torch.zeros((c, 6), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def stream_pass():
            for s in range(FRAMES):
                asr.encode_step_dev(d_pcm[s].data_ptr(), d_mask.data_ptr(), d_codes.data_ptr())
            asr.sync()

        stream_pass()
        sms = []
        for _ in range(max(3, args.reps // 2)):
            t0 = time.perf_counter()
            stream_pass()
            sms.append((time.perf_counter() - t0) * 1e3)
        m = asr.metrics()
        asr.close()
        case = dict(n_clips=c, encode_ms_median=float(np.median(ms)), encode_ms_min=float(np.min(ms)), encode_wall_ms_median=float(np.median(wall)),
                    launches=int(launches), scratch_mib=scratch_mib, streaming_ms_median=float(np.median(sms)), streaming_ms_min=float(np.min(sms)),
                    streaming_graph_launches=int(m.graph_launches), ratio=float(np.median(sms) / np.median(ms)))
        out["cases"].append(case)
    eng.close()
    print(f"{'clips':>5s} {'encode_voice ms (median / min)':>32s} {'wall ms':>8s} {'launches':>9s} {'scratch MiB':>12s} {'125 streaming steps ms (median / min)':>38s} {'ratio':>6s}")
    for k in out["cases"]:
        print(f"{k['n_clips']:5d} {k['encode_ms_median']:21.3f} / {k['encode_ms_min']:8.3f} {k['encode_wall_ms_median']:8.3f} {k['launches']:9d} {k['scratch_mib']:12.1f} "
              f"{k['streaming_ms_median']:27.3f} / {k['streaming_ms_min']:8.3f} {k['ratio']:6.2f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
