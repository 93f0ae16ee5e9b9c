"""Ingest on the GPU (dsm_asr_set_ingest; csrc/dsm_pcm_format.h): ingest_resample_kernel hands Mimi the frames of the host function
dsm_ingest_host, bit for bit, per slot and step — four slots with four formats, a masked stretch, a format switched in
mid-stream —, and everything downstream (codes, text tokens, VAD values, messages) is what a plain engine computes from the host
function's 24 kHz frames, through the synchronous, the ticket, the device-pointer and the model-side entry points; the
pass-through format and an engine that only turned the switch on give the plain calls' results; resets clear one side's history
and keep the format; what must be refused is refused with nothing changed.  config_tiny, B = 4, 6 steps, pitch 15360.
Floats are compared as uint32."""
import audioop
import os

import numpy as np
import pytest

import ingest_ref as R

pytestmark = pytest.mark.gpu

B, STEPS, PITCH = 4, 6, 15360
FORMATS = [(24000, R.F32), (8000, R.MULAW), (44100, R.S16), (48000, R.F32)]
SWITCH_STEP, SWITCH_SLOT, SWITCH_TO = 4, 1, (16000, R.S16)  # slot 1 changes its format after step 3
MASKS = np.ones((STEPS, B), dtype=np.uint8)
MASKS[2:4, 2] = 0  # slot 2 is masked off in steps 2 and 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def audio_bytes(rate, fmt, first, n, slot):
    """samples first .. first + n of the slot's signal at `rate`, in `fmt`"""
    t = (first + np.arange(n)) / rate
    rng = np.random.RandomState(7 * slot + first % 9973)
    x = 0.3 * np.sin(2 * np.pi * (180 + 45 * slot) * t) + 0.05 * (2 * rng.random_sample(n) - 1)
    if fmt == R.F32:
        return x.astype("<f4").tobytes()
    s16 = np.round(x * 32767).astype("<i2").tobytes()
    return s16 if fmt == R.S16 else (audioop.lin2ulaw if fmt == R.MULAW else audioop.lin2alaw)(s16, 2)


def format_at(slot, step):
    return SWITCH_TO if (slot == SWITCH_SLOT and step >= SWITCH_STEP) else FORMATS[slot]


@pytest.fixture(scope="module")
def scenario(dsm, lib):
    """rows [STEPS][B][PITCH] uint8 and the host function's frames [STEPS][B][1920] (zeros where the slot is masked off: the
    host state is not stepped there)"""
    rows = np.zeros((STEPS, B, PITCH), dtype=np.uint8)
    frames = np.zeros((STEPS, B, R.FRAME), dtype=np.float32)
    for b in range(B):
        host, sent = None, 0
        for s in range(STEPS):
            rate, fmt = format_at(b, s)
            if host is None or (b == SWITCH_SLOT and s == SWITCH_STEP):
                host, sent = dsm.ingest_host(rate, fmt), 0
            raw = audio_bytes(rate, fmt, sent, host.frame_samples, b)
            rows[s, b, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
            rows[s, b, len(raw):] = 0xA5  # what lies behind a frame in its row is not read
            sent += host.frame_samples
            if MASKS[s, b]:
                frames[s, b] = host.step(raw)
    return rows, frames


def make_engine(dsm, tiny_weights, ingest=True, formats=True):
    eng = dsm.AsrEngine(dsm.config_tiny(), B, *tiny_weights, device_id=0)
    if ingest:
        eng.set_ingest(True)
        if formats:
            for b, (rate, fmt) in enumerate(FORMATS):
                eng.set_input_format(b, rate, fmt)
    return eng


def before_step(eng, s):
    if s == SWITCH_STEP:
        eng.set_input_format(SWITCH_SLOT, *SWITCH_TO)


@pytest.fixture(scope="module")
def plain(gpu, dsm, lib, tiny_weights, scenario):
    """what plain engines compute from the host function's frames, once: encode_step codes; encode_step_async +
    step_tokens_ticket tokens, VAD values and messages; step_pcm codes, tokens, VAD values and messages"""
    _, frames = scenario
    out = {"codes": [], "ticket": [], "pcm": []}
    eng = make_engine(dsm, tiny_weights, ingest=False)
    for s in range(STEPS):
        out["codes"].append(eng.encode_step(frames[s], MASKS[s]))
    eng.close()
    eng = make_engine(dsm, tiny_weights, ingest=False)
    for s in range(STEPS):
        text, prs = eng.step_tokens_ticket(eng.encode_step_async(frames[s], MASKS[s]), MASKS[s])
        out["ticket"].append((text, prs, eng.poll_msgs()))
    eng.close()
    eng = make_engine(dsm, tiny_weights, ingest=False)
    for s in range(STEPS):
        codes, text, prs = eng.step_pcm(frames[s], MASKS[s])
        out["pcm"].append((codes, text, prs, eng.poll_msgs()))
    eng.close()
    return out


def same_step(s, got, want, what):
    act = MASKS[s].astype(bool)
    for name, g, w in zip(what, got, want):
        if name == "messages":
            assert g == w, (s, name, g, w)
        elif name == "VAD values":
            assert np.array_equal(bits(g)[:, act], bits(w)[:, act]), (s, name)
        else:
            assert np.array_equal(np.asarray(g)[act], np.asarray(w)[act]), (s, name)


def test_kernel_frames_are_the_host_functions_and_codes_the_plain_engines(gpu, dsm, lib, tiny_weights, scenario, plain):
    rows, frames = scenario
    eng = make_engine(dsm, tiny_weights)
    try:
        assert [eng.input_format(b) for b in range(B)] == [(24000, 0, 1920, 7680, 0), (8000, 2, 640, 640, 102), (44100, 1, 3528, 7056, 33),
                                                           (48000, 0, 3840, 15360, 34)]
        for s in range(STEPS):
            before_step(eng, s)
            codes = eng.encode_step_raw(rows[s], MASKS[s], PITCH)
            got = eng.debug_ingest_read(0)
            act = MASKS[s].astype(bool)
            for b in np.flatnonzero(act):
                bad = np.flatnonzero(bits(got[b]) != bits(frames[s, b]))
                assert bad.size == 0, f"step {s} slot {b}: {bad.size} samples differ from dsm_ingest_host, the first at {bad[:4]}"
            for b in np.flatnonzero(~act):  # a masked-off slot writes nothing: its last frame still stands
                assert np.array_equal(bits(got[b]), bits(frames[1, b]))
            same_step(s, (codes,), (plain["codes"][s],), ("codes",))
        assert eng.input_format(SWITCH_SLOT) == (16000, 1, 1280, 2560, 51)
    finally:
        eng.close()


def test_device_pointer_entry_point(gpu, dsm, lib, tiny_weights, scenario, plain):
    import torch
    rows, frames = scenario
    dev = torch.device("cuda", 0)
    eng = make_engine(dsm, tiny_weights)
    try:
        d_rows = torch.from_numpy(rows).to(dev)
        d_masks = torch.from_numpy(MASKS).to(dev)
        d_codes = torch.zeros(STEPS, B * eng.n_q, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()  # the engine's streams are not ordered against torch's
        for s in range(STEPS):
            before_step(eng, s)
            eng.encode_step_raw_dev(d_rows[s].data_ptr(), PITCH, d_masks[s].data_ptr(), d_codes[s].data_ptr())
            got = eng.debug_ingest_read(0)
            for b in np.flatnonzero(MASKS[s]):
                assert np.array_equal(bits(got[b]), bits(frames[s, b])), (s, b)
        eng.sync()
        codes = d_codes.cpu().numpy().view(np.uint32).reshape(STEPS, B, eng.n_q)
        for s in range(STEPS):
            same_step(s, (codes[s],), (plain["codes"][s],), ("codes",))
    finally:
        eng.close()


def test_ticket_and_model_side_entry_points(gpu, dsm, lib, tiny_weights, scenario, plain):
    rows, frames = scenario
    eng = make_engine(dsm, tiny_weights)
    try:
        for s in range(STEPS):
            before_step(eng, s)
            text, prs = eng.step_tokens_ticket(eng.encode_step_raw_async(rows[s], MASKS[s], PITCH), MASKS[s])
            same_step(s, (text, prs, eng.poll_msgs()), plain["ticket"][s], ("text tokens", "VAD values", "messages"))
    finally:
        eng.close()
    eng = make_engine(dsm, tiny_weights)
    try:
        for s in range(STEPS):
            before_step(eng, s)
            codes, text, prs = eng.step_raw(rows[s], MASKS[s], PITCH)
            got = eng.debug_ingest_read(1)
            for b in np.flatnonzero(MASKS[s]):
                assert np.array_equal(bits(got[b]), bits(frames[s, b])), (s, b)
            same_step(s, (codes, text, prs, eng.poll_msgs()), plain["pcm"][s], ("codes", "text tokens", "VAD values", "messages"))
    finally:
        eng.close()


def test_pass_through_and_switch_alone_give_the_plain_results(gpu, dsm, lib, tiny_weights, scenario, plain):
    _, frames = scenario
    raw_eng = make_engine(dsm, tiny_weights, formats=False)  # every slot on 24000 / F32, the default
    on_eng = make_engine(dsm, tiny_weights, formats=False)   # ingest on, plain calls only
    try:
        assert raw_eng.input_format(2) == (24000, 0, 1920, 7680, 0)
        for s in range(STEPS):
            codes = raw_eng.encode_step_raw(frames[s].view(np.uint8), MASKS[s], 7680)
            same_step(s, (codes,), (plain["codes"][s],), ("codes",))
            act = MASKS[s].astype(bool)
            assert np.array_equal(bits(raw_eng.debug_ingest_read(0))[act], bits(frames[s])[act])
            same_step(s, (on_eng.encode_step(frames[s], MASKS[s]),), (plain["codes"][s],), ("codes",))
        on_eng.close()
        on_eng = make_engine(dsm, tiny_weights, formats=False)
        for s in range(STEPS):
            codes, text, prs = on_eng.step_pcm(frames[s], MASKS[s])
            same_step(s, (codes, text, prs, on_eng.poll_msgs()), plain["pcm"][s], ("codes", "text tokens", "VAD values", "messages"))
    finally:
        raw_eng.close()
        on_eng.close()


def test_resets_clear_one_sides_history_and_keep_the_format(gpu, dsm, lib, tiny_weights, scenario):
    rows, frames = scenario
    ones = np.ones(B, dtype=np.uint8)
    eng = make_engine(dsm, tiny_weights)
    try:
        for s in range(2):  # both sides in step on the same raw rows
            eng.encode_step_raw(rows[s], ones, PITCH)
            eng.step_raw(rows[s], ones, PITCH)
        eng.mimi_reset_batch_idx(1)  # encoder side, slot 1
        eng.reset_batch_idx(3)       # model side, slot 3
        assert eng.input_format(1)[:2] == FORMATS[1] and eng.input_format(3)[:2] == FORMATS[3]
        eng.encode_step_raw(rows[2], ones, PITCH)
        eng.step_raw(rows[2], ones, PITCH)
        enc, mod = eng.debug_ingest_read(0), eng.debug_ingest_read(1)
        fresh, cont = {}, {}
        for b in (1, 3):
            rate, fmt = FORMATS[b]
            h, c = dsm.ingest_host(rate, fmt), dsm.ingest_host(rate, fmt)
            nb = h.frame_bytes
            fresh[b] = h.step(rows[2, b, :nb].tobytes())
            for s in range(3):
                cont[b] = c.step(rows[s, b, :nb].tobytes())
            assert not np.array_equal(bits(fresh[b]), bits(cont[b]))
        assert np.array_equal(bits(enc[1]), bits(fresh[1])) and np.array_equal(bits(mod[1]), bits(cont[1]))
        assert np.array_equal(bits(enc[3]), bits(cont[3])) and np.array_equal(bits(mod[3]), bits(fresh[3]))
    finally:
        eng.close()


def test_refusals_change_nothing(gpu, dsm, lib, tiny_weights, scenario, plain):
    rows, frames = scenario
    off = make_engine(dsm, tiny_weights, ingest=False)
    eng = make_engine(dsm, tiny_weights)
    try:
        for call in (lambda: off.encode_step_raw(rows[0], MASKS[0], PITCH), lambda: off.step_raw(rows[0], MASKS[0], PITCH),
                     lambda: off.encode_step_raw_async(rows[0], MASKS[0], PITCH), lambda: off.set_input_format(0, 8000, R.MULAW)):
            with pytest.raises(dsm.DsmError, match="ingest is off"):
                call()
        same_step(0, (off.encode_step(frames[0], MASKS[0]),), (plain["codes"][0],), ("codes",))
        small = np.zeros((B, 7680), dtype=np.uint8)
        for call in (lambda: eng.encode_step_raw(small, MASKS[0], 7680),        # slot 3's frame has 15360 bytes
                     lambda: eng.step_raw(small, MASKS[0], 7680),
                     lambda: eng.encode_step_raw_async(small, MASKS[0], 7680),
                     lambda: eng.encode_step_raw(rows[0][:, :15352].copy(), MASKS[0], 15352),  # not a multiple of 16
                     lambda: eng.encode_step_raw(np.zeros((B, 15376), dtype=np.uint8), MASKS[0], 15376)):  # above the largest
            with pytest.raises(dsm.DsmError, match="raw frames"):
                call()
        with pytest.raises(dsm.DsmError, match="whole number"):
            eng.set_input_format(0, 8001, R.F32)
        with pytest.raises(dsm.DsmError, match="sample format"):
            eng.set_input_format(0, 8000, 7)
        assert eng.input_format(0) == (24000, 0, 1920, 7680, 0)
        # a pitch that is too small only for a masked-off slot is fine: that row is not read
        m = np.array([1, 1, 1, 0], dtype=np.uint8)
        eng.encode_step_raw(rows[0][:, :7680].copy(), m, 7680)
        got = eng.debug_ingest_read(0)
        for b in range(3):  # and the refused calls left the histories at the start of the stream
            assert np.array_equal(bits(got[b]), bits(frames[0, b])), b
    finally:
        off.close()
        eng.close()
