"""Slot snapshot timings at a served shape (DESIGN.md "Slot snapshots" quotes this probe's output).

    python experiments/slot_move_probe.py [--preset stt-1b-en_fr] [--batch 64] [--reps 11]

Two engines of the preset on one device (the second a replica of the first), rings full.  Measured, wall clock around calls
that return with their streams drained, median of --reps after 3 warm-up calls:
  * dsm_asr_move_slots for n = 1 and n = 8 (one pack launch, one unpack launch, no host copy);
  * dsm_asr_export_slots and dsm_asr_import_slots for n = 1 (through pinned staging and the caller's buffer);
  * the baseline the kernels replace: one hipMemcpyAsync per section and slot — the same section sizes, read from the blob's
    signature, between buffers of this probe's own laid out [slot][section bytes] like the engine's — enqueued on one stream
    and drained once.
GB/s figures count the bytes once (a copy reads and writes them: HBM traffic is twice that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def section_sizes(cfg, blob, has1):
    """Per-slot section sizes in blob order, from the configuration and the blob's signature (conv (S, C) list)."""
    nsig = struct.unpack_from("<I", blob, 16)[0]
    sig = struct.unpack_from(f"<{nsig}I", blob, 48)
    n_conv = sig[14]
    convs = [4 * sig[15 + 2 * i] * sig[16 + 2 * i] for i in range(n_conv)]
    lm_ring = cfg.lm.d_model * cfg.lm.context * (2 if cfg.kv_bf16 else 4)
    mt = cfg.mimi.transformer
    mimi_ring = mt.d_model * mt.context * 4
    lm = [4, 4, 4, 1, 8, 32, 4 * cfg.audio_codebooks] + [lm_ring] * (2 * cfg.lm.num_layers)
    side = [4, 4] + [mimi_ring] * (2 * mt.num_layers) + convs
    return lm + side * (2 if has1 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="stt-1b-en_fr")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--weights-dir", default=os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dsm_amd
    from dsm_amd import synth
    cfg = {"stt-1b-en_fr": dsm_amd.config_stt_1b_en_fr, "stt-2.6b-en": dsm_amd.config_stt_2_6b_en, "tiny": dsm_amd.config_tiny}[args.preset]()
    lm_path, mimi_path = synth.make_synth_weights(cfg, args.weights_dir, tag=args.preset)
    B = args.batch
    src = dsm_amd.AsrEngine(cfg, B, lm_path, mimi_path)
    dst = dsm_amd.AsrEngine.replica(src, 0)
    out = {"preset": args.preset, "batch": B, "reps": args.reps}
    out["slot_bytes_without_model_mimi"] = dsm_amd.slot_blob_info(src.export_slots([0]))["slot_bytes"]
    pcm = synth.synth_pcm(B, 3)
    ones = np.ones(B, dtype=np.uint8)
    for e in (src, dst):
        for s in range(3):
            e.step_pcm(pcm[s], ones)  # both Mimi sides of the model path exist, graphs settle
        e.debug_set_positions(4 * cfg.lm.context, 4 * cfg.mimi.transformer.context)  # rings full
    blob = src.export_slots([0])
    sb = dsm_amd.slot_blob_info(blob)["slot_bytes"]
    out["slot_bytes"] = sb
    for n in (1, 8):
        a, b = list(range(n)), list(range(B - n, B))
        med, lo, hi = median_ms(lambda: src.move_slots(a, dst, b), args.reps)
        out[f"move_n{n}_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3), "GBps": round(n * sb / med / 1e6, 1)}
    med, lo, hi = median_ms(lambda: src.export_slots([0]), args.reps)
    out["export_n1_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3), "GBps": round(sb / med / 1e6, 1)}
    med, lo, hi = median_ms(lambda: dst.import_slots([B - 1], blob), args.reps)
    out["import_n1_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3), "GBps": round(sb / med / 1e6, 1)}
    # the same two calls at the C ABI, into / out of a buffer that exists already (no allocation, no Python copy)
    cbuf = (C.c_char * len(blob))()
    one, last, need = (C.c_int * 1)(0), (C.c_int * 1)(B - 1), C.c_size_t(0)
    med, lo, hi = median_ms(lambda: src.lib.dsm_asr_export_slots(src.h, one, 1, cbuf, len(blob), C.byref(need)), args.reps)
    assert need.value == len(blob)
    out["export_n1_abi_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3), "GBps": round(sb / med / 1e6, 1)}
    med, lo, hi = median_ms(lambda: dst.lib.dsm_asr_import_slots(dst.h, last, 1, cbuf, len(blob)), args.reps)
    out["import_n1_abi_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3), "GBps": round(sb / med / 1e6, 1)}
    # ---- baseline: a chain of per-section hipMemcpyAsync calls ----
    sizes = section_sizes(cfg, blob, True)
    assert sum((s + 15) & ~15 for s in sizes) == sb, "the probe's section list does not add up to the blob's slot_bytes"
    rows = 8
    bufs_a = [torch.empty(rows * s, dtype=torch.uint8, device="cuda") for s in sizes]
    bufs_b = [torch.empty(rows * s, dtype=torch.uint8, device="cuda") for s in sizes]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = torch.cuda.Stream()
    sh = C.c_void_p(stream.cuda_stream)
    pa, pb = [t.data_ptr() for t in bufs_a], [t.data_ptr() for t in bufs_b]

    def chain(n):
        for j in range(n):
            for i, s in enumerate(sizes):
                rc = hip.hipMemcpyAsync(pb[i] + j * s, pa[i] + (rows - 1 - j) * s, s, 3, sh)  # hipMemcpyDeviceToDevice
                assert rc == 0
        stream.synchronize()

    out["baseline_sections"] = len(sizes)
    for n in (1, 8):
        med, lo, hi = median_ms(lambda: chain(n), args.reps)
        t0 = time.perf_counter()
        for j in range(n):
            for i, s in enumerate(sizes):
                hip.hipMemcpyAsync(pb[i] + j * s, pa[i] + (rows - 1 - j) * s, s, 3, sh)
        enq = (time.perf_counter() - t0) * 1e3
        stream.synchronize()
        out[f"memcpy_chain_n{n}_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3),
                                        "GBps": round(n * sb / med / 1e6, 1), "host_enqueue_ms": round(enq, 3)}
    src.close()
    dst.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
