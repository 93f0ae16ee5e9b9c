"""dsm_worker_set_input_rate on the GPU: a worker with an 8 kHz channel beside a 24 kHz channel delivers, per channel, the
messages of a second worker whose two 24 kHz channels get the host function's output (dsm_ingest_host on the same 8 kHz frames)
and the same 24 kHz audio — except Step.buffered_pcm, which counts the channel's own samples and is checked on its own, and the
8 kHz channel's markers, which come one step later.  Closing the channel and reopening the slot gives a 24 kHz channel again."""
import numpy as np
import pytest

import ingest_ref as R

pytestmark = pytest.mark.gpu

EXTRA = 16  # each Audio message of the 8 kHz channel carries a frame and 16 samples more: its queue grows by 16 a step


def without(msgs, kind):
    return [{k: v for k, v in m.items() if k != "buffered_pcm"} for m in msgs if m["type"] != kind]


def marker_steps(msgs):
    """marker id -> how many Step messages the channel had received when the marker came"""
    out, steps = {}, 0
    for m in msgs:
        steps += m["type"] == "Step"
        if m["type"] == "Marker":
            out[m["id"]] = steps
    return out


def test_a_channel_at_8_khz_beside_one_at_24_khz(gpu, dsm, lib, tiny_weights):
    cfg = dsm.config_tiny()
    B, passes = 2, 26 + cfg.asr_delay_in_tokens
    rng = np.random.default_rng(11)
    t8 = np.arange(passes * (640 + EXTRA)) / 8000.0
    audio8 = (0.3 * np.sin(2 * np.pi * 220 * t8) + 0.03 * rng.standard_normal(t8.size)).astype(np.float32)
    audio24 = (0.1 * rng.standard_normal(passes * 1920)).astype(np.float32)
    host = dsm.ingest_host(8000, R.F32)
    host24 = [host.step(audio8[640 * f:640 * (f + 1)]) for f in range(passes)]  # the frames the worker cuts from the 8 kHz queue

    ea = dsm.AsrEngine(cfg, B, *tiny_weights)
    wa = dsm.Worker(ea)
    a8, a24 = wa.open(), wa.open()
    wa.set_input_rate(a8, 8000)
    assert ea.input_format(a8) == (8000, 0, 640, 2560, 102) and ea.input_format(a24) == (24000, 0, 1920, 7680, 0)
    with pytest.raises(dsm.DsmError):
        wa.set_input_rate(a24, 8001)
    eb = dsm.AsrEngine(cfg, B, *tiny_weights)
    wb = dsm.Worker(eb)
    b8, b24 = wb.open(), wb.open()
    try:
        for f in range(passes):
            wa.send(a8, dsm.encode_in_msg("Audio", pcm=audio8[(640 + EXTRA) * f:(640 + EXTRA) * (f + 1)]))
            wa.send(a24, dsm.encode_in_msg("Audio", pcm=audio24[1920 * f:1920 * (f + 1)]))
            wb.send(b8, dsm.encode_in_msg("Audio", pcm=host24[f]))
            wb.send(b24, dsm.encode_in_msg("Audio", pcm=audio24[1920 * f:1920 * (f + 1)]))
            if f in (4, 13, 22):
                for w, slots in ((wa, (a8, a24)), (wb, (b8, b24))):
                    for s in slots:
                        w.send(s, dsm.encode_in_msg("Marker", id=100 + f))
            assert wa.step() and wb.step()
            if f == 1:  # once its audio has been cut into frames a channel keeps its rate
                with pytest.raises(dsm.DsmError):
                    wa.set_input_rate(a8, 16000)
        got8, got24, want8, want24 = wa.recv(a8), wa.recv(a24), wb.recv(b8), wb.recv(b24)
        assert got24 == want24 and sum(m["type"] == "Step" for m in got24) == passes
        assert without(got8, "Marker") == without(want8, "Marker")
        # buffered_pcm: the channel's own samples — what is left in the 8 kHz queue when the step's frame was cut
        assert [m["buffered_pcm"] for m in got8 if m["type"] == "Step"] == [EXTRA * (f + 1) for f in range(passes)]
        assert all(m["buffered_pcm"] == 0 for m in want8 if m["type"] == "Step")
        m8, m24 = marker_steps(got8), marker_steps(want8)
        assert sorted(m8) == sorted(m24) == [104, 113, 122]
        assert all(m8[i] == m24[i] + 1 for i in m8), (m8, m24)
        # close, recycle the slot, reopen: a 24 kHz channel again, stepping through the plain entry point
        wa.close_channel(a8)
        wa.send(a24, dsm.encode_in_msg("Audio", pcm=audio24[:1920]))
        assert wa.step()
        assert ea.input_format(a8) == (24000, 0, 1920, 7680, 0)
        again = wa.open()
        assert again == a8
        wa.send(again, dsm.encode_in_msg("Audio", pcm=audio24[:1920]))
        assert wa.step()
        msgs = wa.recv(again)
        assert [m["type"] for m in msgs][:2] == ["Ready", "Step"] and msgs[1]["buffered_pcm"] == 0
    finally:
        wa.close(); wb.close(); ea.close(); eb.close()
