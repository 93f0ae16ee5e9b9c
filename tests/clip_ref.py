"""An independent Python statement of the clips section (include/dsm.h "clips"; csrc/dsm_asr_clip.h): the cut of a clip into
frames and the schedule of begin / push / close / run, written from the section's text and sharing no code with the library.
The tests compare dsm_asr_clip_frame_host, dsm_asr_clip_host_* and the engine's blocks against it."""
import numpy as np

F32, S16, MULAW, ALAW = 0, 1, 2, 3
SAMPLE_BYTES = {F32: 4, S16: 2, MULAW: 1, ALAW: 1}
SILENCE = {F32: 0x00, S16: 0x00, MULAW: 0xFF, ALAW: 0xD5}
IDLE, RUNNING, WAITING, DONE = 0, 1, 2, 3
RUN_MAX = 16


def frame_bytes(rate, fmt):
    assert (2 * rate) % 25 == 0
    return (2 * rate // 25) * SAMPLE_BYTES[fmt]


def frame(clip, rate, fmt, index):
    """frame `index` of the clip followed by endless silence, as bytes"""
    fb = frame_bytes(rate, fmt)
    endless = bytes(clip) + bytes([SILENCE[fmt]]) * (fb * (index + 1))
    return endless[index * fb:(index + 1) * fb]


def n_audio(clip_bytes, rate, fmt):
    return -(-clip_bytes // frame_bytes(rate, fmt))


class Schedule:
    """B slots; run(n) gives frame [n][B] and mask [n][B] and advances the slots"""

    def __init__(self, B, cap):
        self.B, self.cap = B, cap
        self.slots = [None] * B

    def begin(self, b, rate, fmt, flush):
        if self.slots[b] is not None:
            return False
        self.slots[b] = dict(fb=frame_bytes(rate, fmt), bytes=0, closed=False, cursor=0, flush=flush, status=RUNNING)
        return True

    def push(self, b, n):
        s = self.slots[b]
        if s is None or s["closed"] or s["bytes"] + n > self.cap:
            return False
        s["bytes"] += n
        if s["status"] == WAITING:
            s["status"] = RUNNING
        return True

    def _total(self, s):
        return -(-s["bytes"] // s["fb"]) + s["flush"]

    def close(self, b):
        s = self.slots[b]
        if s is None:
            return False
        if not s["closed"]:
            s["closed"] = True
            s["status"] = DONE if s["cursor"] >= self._total(s) else RUNNING
        return True

    def reset(self, b):
        self.slots[b] = None

    def status(self, b):
        return IDLE if self.slots[b] is None else self.slots[b]["status"]

    def run(self, n):
        frame_idx = np.zeros((n, self.B), dtype=np.uint32)
        mask = np.zeros((n, self.B), dtype=np.uint8)
        for k in range(n):
            for b, s in enumerate(self.slots):
                if s is None or s["status"] == DONE:
                    continue
                if s["closed"]:
                    take = s["cursor"] < self._total(s)
                else:
                    take = (s["cursor"] + 1) * s["fb"] <= s["bytes"]
                    if not take:
                        s["status"] = WAITING
                if take:
                    frame_idx[k, b], mask[k, b] = s["cursor"], 1
                    s["cursor"] += 1
                if s["closed"] and s["cursor"] >= self._total(s):
                    s["status"] = DONE
        return frame_idx, mask
