"""Python restatement of the egress definition, written from the definition and not from csrc/dsm_pcm_format.h: the frame and
filter geometry of an output rate, the whole-clip resampler's indexing with the brute-force search for the latency D and for the
history a step reads, the three sample encoders, and the streaming cut of a whole-clip result.  The filter coefficients are not
restated: the definition names the whole-clip function dsm_resample(x, 24000, rate) as the signal, and the tests compare with it."""
import math

import numpy as np

F32, S16, MULAW, ALAW = 0, 1, 2, 3
FORMATS = (F32, S16, MULAW, ALAW)
SAMPLE_BYTES = {F32: 4, S16: 2, MULAW: 1, ALAW: 1}
IN_RATE, FRAME = 24000, 1920
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)  # the resampling rates of the definition's table
# rate: (L, M, half, taps, F_out, D) as the definition's table states them
TABLE = {
    8000: (1, 3, 102, 204, 640, 34),
    11025: (147, 320, 74, 148, 882, 33),
    16000: (2, 3, 51, 102, 1280, 34),
    22050: (147, 160, 37, 74, 1764, 33),
    32000: (4, 3, 34, 68, 2560, 45),
    44100: (147, 80, 34, 68, 3528, 62),
    48000: (2, 1, 34, 68, 3840, 68),
}
MAX_TAPS, MAX_FRAME_BYTES = 204, 15360


def supported(rate):
    return 8000 <= rate <= 48000 and (2 * rate) % 25 == 0


def geometry(rate):
    """L, M, half, taps, F_out of 24000 -> rate: L / M = rate / 24000 in lowest terms; the filter is cut off at 0.95 x the lower
    Nyquist with 32 zero crossings each side, so half = ceil(32 / fc) with fc relative to the input's Nyquist.  24000: no filter."""
    f_out = 2 * rate // 25
    if rate == IN_RATE:
        return dict(L=1, M=1, half=0, taps=0, F_out=f_out)
    g = math.gcd(rate, IN_RATE)
    L, M = rate // g, IN_RATE // g
    fc = 0.95 * (rate / IN_RATE if rate < IN_RATE else 1.0)
    half = int(math.ceil(32 / fc))
    return dict(L=L, M=M, half=half, taps=2 * half, F_out=f_out)


def brute_force(rate, frames=4):
    """(the smallest delay D for which no tap of an emitted frame reaches past the 1920 (e + 1) input samples produced so far,
    how many samples in front of its frame's first input sample a step then reads at most) by walking every output of `frames`
    frames.  Output j of the whole-clip result sits at input j M / L and reads input i0 - half + 1 .. i0 + half,
    i0 = floor(j M / L); frame e delivers j = F_out e + n - D for n = 0 .. F_out - 1."""
    g = geometry(rate)
    L, M, half, f_out = g["L"], g["M"], g["half"], g["F_out"]
    at = np.arange(frames * f_out, dtype=np.int64)
    e = at // f_out  # the frame an output is delivered in

    def fits(D):
        j = at - D
        return not np.any((j >= 0) & ((j * M) // L + half > FRAME * (e + 1) - 1))

    D = 0
    while not fits(D):
        D += 1
    j = at - D
    first_tap = (j * M) // L - half + 1
    reach = int(np.max(np.where(j >= 0, FRAME * e - first_tap, 0)))
    return D, reach


def stream_of(y, D, frames, f_out):
    """the frames a stream delivers, concatenated: D zeros, then the whole-clip result"""
    y = np.asarray(y, dtype=np.float32)
    assert y.size >= frames * f_out - D
    return np.concatenate([np.zeros(D, dtype=np.float32), y[:frames * f_out - D]])


def signal(frames, seed):
    """a seeded sine plus noise, amplitude <= 0.4, `frames` frames at 24 kHz"""
    rng = np.random.RandomState(seed)
    n = frames * FRAME
    t = np.arange(n, dtype=np.float64)
    x = 0.25 * np.sin(2 * np.pi * 437.0 * t / IN_RATE + 0.3) + np.clip(0.05 * rng.standard_normal(n), -0.15, 0.15)
    assert np.max(np.abs(x)) <= 0.4
    return x.astype(np.float32)


# ---- the sample encoders ----

def s16_of(v):
    """f32 -> the 16-bit value: round half to even of v * 32768, NaN 0, clamped"""
    v = np.float32(v)
    if np.isnan(v):
        return 0
    r = float(v) * 32768.0  # exact: a power of two (an overflow to inf clamps below)
    if r >= 32767.0:
        return 32767
    if r <= -32768.0:
        return -32768
    fl = math.floor(r)
    d = r - fl
    if d > 0.5 or (d == 0.5 and fl % 2 == 1):
        fl += 1
    return int(fl)


def ulaw_of(s):
    sign = 1 if s < 0 else 0
    mag = min(abs(s), 32635) + 0x84
    e = mag.bit_length() - 1 - 7
    assert 0 <= e <= 7
    m = (mag >> (e + 3)) & 0xF
    return ~(sign << 7 | e << 4 | m) & 0xFF


def alaw_of(s):
    sign = 1 if s < 0 else 0
    mag = -s - 1 if sign else s
    e = 0 if mag < 256 else mag.bit_length() - 1 - 7
    m = (mag >> 4) & 0xF if e == 0 else (mag >> (e + 3)) & 0xF
    return ((0 if sign else 0x80) | e << 4 | m) ^ 0x55


def encode_s16(fmt, s):
    """the value a 16-bit sample encodes to: itself, or its G.711 byte"""
    return s if fmt == S16 else ulaw_of(s) if fmt == MULAW else alaw_of(s)


def encode(fmt, y):
    """f32 samples -> the bytes of a frame (uint8 array)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    if fmt == F32:
        return y.view(np.uint8).copy()
    s = [s16_of(v) for v in y]
    if fmt == S16:
        return np.array(s, dtype="<i2").view(np.uint8).copy()
    return np.array([encode_s16(fmt, v) for v in s], dtype=np.uint8)
