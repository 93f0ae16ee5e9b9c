"""Python restatement of the ingest definition (csrc/dsm_pcm_format.h), written from the definition and not from the code: the G.711
expansions by the ITU-T formulas, the frame and latency arithmetic with its brute-force counterparts, the decoding of a raw
frame, and the streaming cut of a whole-clip result.  The filter itself is not restated: the definition names the whole-clip
function dsm_resample as the signal, and the tests compare against it."""
import math

import numpy as np

F32, S16, MULAW, ALAW = 0, 1, 2, 3
FORMATS = (F32, S16, MULAW, ALAW)
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
OUT_RATE, FRAME = 24000, 1920
SAMPLE_BYTES = {F32: 4, S16: 2, MULAW: 1, ALAW: 1}


def ulaw_to_s16(byte):
    u = ~byte & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return 0x84 - t if u & 0x80 else t - 0x84


def alaw_to_s16(byte):
    a = (byte ^ 0x55) & 0xFF
    e, m = (a & 0x70) >> 4, a & 0x0F
    t = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return t if a & 0x80 else -t


def decode(fmt, raw):
    """bytes of a frame (or a clip) -> f32 samples"""
    raw = bytes(raw)
    if fmt == F32:
        return np.frombuffer(raw, dtype="<f4").copy()
    if fmt == S16:
        return np.frombuffer(raw, dtype="<i2").astype(np.float32) * np.float32(1.0 / 32768)
    table = np.array([(ulaw_to_s16 if fmt == MULAW else alaw_to_s16)(b) for b in range(256)], dtype=np.float32) * np.float32(1.0 / 32768)
    return table[np.frombuffer(raw, dtype=np.uint8)]


def supported(rate):
    return 8000 <= rate <= 48000 and (2 * rate) % 25 == 0 and OUT_RATE // math.gcd(rate, OUT_RATE) <= 4096


def geometry(rate):
    """L, M, half, taps, F_in, D by the definition's formulas (rate 24000: no filter)"""
    f_in = 2 * rate // 25
    if rate == OUT_RATE:
        return dict(L=1, M=1, half=0, taps=0, F_in=f_in, D=0)
    g = math.gcd(rate, OUT_RATE)
    L, M = OUT_RATE // g, rate // g
    fc = 0.95 * (OUT_RATE / rate if OUT_RATE < rate else 1.0)
    half = int(math.ceil(32 / fc))
    return dict(L=L, M=M, half=half, taps=2 * half, F_in=f_in, D=(half * L) // M)


def brute_force(rate, frames=4):
    """(the smallest latency D for which no tap of a frame reaches input the slot has not received, how many samples in front
    of its frame a step then reads at most) by walking every output of `frames` frames.  Output j sits at input j M / L and
    reads input i0 - half + 1 .. i0 + half, i0 = floor(j M / L)."""
    g = geometry(rate)
    L, M, half, f_in = g["L"], g["M"], g["half"], g["F_in"]

    at = np.arange(frames * FRAME, dtype=np.int64)
    t = at // FRAME  # the frame an output is delivered in

    def fits(D):
        j = at - D
        return not np.any((j >= 0) & ((j * M) // L + half > f_in * (t + 1) - 1))

    D = 0
    while not fits(D):
        D += 1
    j = at - D
    first_tap = (j * M) // L - half + 1
    reach = int(np.max(np.where((j >= 0) & (t >= 1), f_in * t - first_tap, 0)))
    return D, reach


def stream_of(y, D, frames):
    """the frames a stream delivers, concatenated: D zeros, then the whole-clip result"""
    y = np.asarray(y, dtype=np.float32)
    assert y.size >= frames * FRAME - D
    return np.concatenate([np.zeros(D, dtype=np.float32), y[:frames * FRAME - D]])


def noise_clip(rate, fmt, frames, seed):
    """raw bytes of `frames` frames of seeded noise with the format's extremes in front: every G.711 byte; s16 +-32767 and
    -32768; f32 +-1, a denormal and signed zeros"""
    rng = np.random.RandomState(seed)
    n = frames * (2 * rate // 25)
    if fmt == F32:
        x = (rng.standard_normal(n) * 0.25).astype("<f4")
        x[:6] = np.array([1.0, -1.0, 1e-40, -0.0, 0.0, 0.999999], dtype="<f4")
        return x.tobytes()
    if fmt == S16:
        x = rng.randint(-32768, 32768, size=n).astype("<i2")
        x[:5] = np.array([32767, -32767, -32768, 0, -1], dtype="<i2")
        return x.tobytes()
    x = rng.randint(0, 256, size=n).astype(np.uint8)
    x[:256] = np.arange(256, dtype=np.uint8)
    return x.tobytes()
