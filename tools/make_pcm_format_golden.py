#!/usr/bin/env python3
"""tests/golden/pcm_format.json: SHA-256 digests of what the host functions of the PCM format section (csrc/dsm_pcm_format.h:
dsm_ingest_host, dsm_egress_host, the two describe calls, dsm_resample) give for seeded inputs — a pin that a change of the
code did not move a bit of them.  The GPU tests prove kernel == host; this proves host == the host of the commit the file was
made from.  No GPU, a few seconds.  The digests depend on libm's sin / sqrt through the phase table, as tests/golden/ingest/*.f32
do.

  tools/make_pcm_format_golden.py [--lib PATH]           write the file from a library (default: the tree's)
  tools/make_pcm_format_golden.py --check [--lib PATH]   recompute, compare with the file, exit 1 on a difference

To pin a refactor, write the file with --lib pointing at the library built from the commit before it, then --check this tree's.

What is recorded (inputs from tests/ingest_ref.py and tests/egress_ref.py):
  ingest    3 frames of noise_clip(rate, fmt, 3, seed) through dsm_ingest_host, every rate of ingest_ref.RATES and 8025, 12000,
            47975, every format.  No NaN goes in: what it gives is undefined on purpose.
  egress    3 frames of signal(3, seed) with the extremes in front (+-1, +-1.5, NaN, +-inf, a denormal, -0.0) through
            dsm_egress_host, every rate of egress_ref.RATES and 24000, 8025, 47975, every format; and one stream that changes its
            format behind the second frame.
  describe  per direction, one digest over the return code and the twelve words of every rate 8000, 8025, .. 48000 x format.
  refused   the return codes of a handful of rates and formats outside the definition.
  resample  dsm_resample on the seven resampling rates, both ways."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import egress_ref  # noqa: E402
import ingest_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pcm_format.json")
LIB = os.path.join(ROOT, "delayed-streams-modeling_amd", "libdsm_mi355x.so")
FRAMES, FRAME = 3, 1920
INGEST_RATES = ingest_ref.RATES + (8025, 12000, 47975)
EGRESS_RATES = egress_ref.RATES + (24000, 8025, 47975)
EXTREMES = np.array([1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 1e-40, -0.0], dtype=np.float32)
REFUSED = ((7999, 0), (48001, 0), (12345, 1), (16000, 4), (16000, -1), (0, 0), (24000, 7), (-8000, 2))


def load(path=LIB):
    """A handle of its own on the library (its own argtypes: nothing here depends on the package's declarations)."""
    lib = C.CDLL(path)
    for side in ("ingest", "egress"):
        getattr(lib, f"dsm_{side}_host_new").restype = C.c_void_p
        getattr(lib, f"dsm_{side}_host_new").argtypes = [C.c_int, C.c_int]
        getattr(lib, f"dsm_{side}_host_free").restype = None
        getattr(lib, f"dsm_{side}_host_free").argtypes = [C.c_void_p]
        getattr(lib, f"dsm_{side}_host").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(lib, f"dsm_{side}_describe").argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.dsm_resample.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t)]
    lib.dsm_free.restype = None
    lib.dsm_free.argtypes = [C.c_void_p]
    return lib


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p)
    return h.hexdigest()


def _host(lib, side, rate, fmt, frames_in, out_bytes):
    """the bytes `side`'s host function delivers for the frames (each a bytes object), one state"""
    h = getattr(lib, f"dsm_{side}_host_new")(rate, fmt)
    assert h, (side, rate, fmt)
    step, got = getattr(lib, f"dsm_{side}_host"), []
    for f in frames_in:
        out = C.create_string_buffer(out_bytes)
        rc = step(h, f, out)
        assert rc == 0, (side, rate, fmt, rc)
        got.append(out.raw)
    getattr(lib, f"dsm_{side}_host_free")(h)
    return b"".join(got)


def _egress_frames(seed):
    x = egress_ref.signal(FRAMES, seed=seed).astype(np.float32)
    x[:EXTREMES.size] = EXTREMES
    return [x[e * FRAME:(e + 1) * FRAME].tobytes() for e in range(FRAMES)]


def _describe(lib, side):
    h = hashlib.sha256()
    for rate in range(8000, 48001, 25):
        for fmt in range(4):
            w = np.zeros(12, dtype="<u4")
            rc = getattr(lib, f"dsm_{side}_describe")(rate, fmt, w.ctypes.data)
            h.update(np.array([rc], dtype="<i4").tobytes() + w.tobytes())
    return h.hexdigest()


def _resample(lib, x, rin, rout):
    x = np.ascontiguousarray(x, dtype=np.float32)
    ptr, n = C.POINTER(C.c_float)(), C.c_size_t(0)
    rc = lib.dsm_resample(x.ctypes.data, x.size, rin, rout, C.byref(ptr), C.byref(n))
    assert rc == 0, (rin, rout, rc)
    y = np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()
    lib.dsm_free(ptr)
    return _sha(np.array([n.value], dtype="<u8").tobytes(), y.tobytes())


def compute(lib):
    g = {"ingest": {}, "egress": {}, "describe": {}, "refused": {}, "resample": {}}
    for rate in INGEST_RATES:
        fb = 2 * rate // 25
        for fmt in ingest_ref.FORMATS:
            raw, n = ingest_ref.noise_clip(rate, fmt, FRAMES, seed=4 * rate + fmt), fb * ingest_ref.SAMPLE_BYTES[fmt]
            g["ingest"][f"{rate}/{fmt}"] = _sha(_host(lib, "ingest", rate, fmt, [raw[t * n:(t + 1) * n] for t in range(FRAMES)], 4 * FRAME))
    for rate in EGRESS_RATES:
        for fmt in egress_ref.FORMATS:
            row = (2 * rate // 25) * egress_ref.SAMPLE_BYTES[fmt]
            g["egress"][f"{rate}/{fmt}"] = _sha(_host(lib, "egress", rate, fmt, _egress_frames(4 * rate + fmt), row))
    f = _egress_frames(1)  # 16000 / S16 for two frames, then 44100 / mu-law: a new format starts a new stream
    g["egress"]["switch"] = _sha(_host(lib, "egress", 16000, egress_ref.S16, f[:2], 1280 * 2), _host(lib, "egress", 44100, egress_ref.MULAW, f[2:], 3528))
    w = np.zeros(12, dtype="<u4")
    for side in ("ingest", "egress"):
        g["describe"][side] = _describe(lib, side)
        g["refused"][side] = {f"{rate}/{fmt}": getattr(lib, f"dsm_{side}_describe")(rate, fmt, w.ctypes.data) for rate, fmt in REFUSED}
    for rate in egress_ref.RATES:
        x = ingest_ref.decode(ingest_ref.F32, ingest_ref.noise_clip(rate, ingest_ref.F32, 2, seed=rate))
        g["resample"][f"{rate}->24000"] = _resample(lib, x, rate, 24000)
        g["resample"][f"24000->{rate}"] = _resample(lib, egress_ref.signal(2, seed=rate), 24000, rate)
    return g


def differences(want, got, at=""):
    """the keys (as paths) at which two nested dicts differ"""
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(want.get(k), got.get(k), f"{at}/{k}")]
    return [] if want == got else [at]


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else LIB
    got = compute(load(path))
    if "--check" in sys.argv:
        bad = differences(json.load(open(OUT)), got)
        print(f"{OUT}: {len(bad)} difference(s) against {path}" + "".join("\n  " + b for b in bad))
        sys.exit(1 if bad else 0)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT} from {path}")
