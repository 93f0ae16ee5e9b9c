"""The TTS slot blob's documented layout (csrc/dsm_tts_slot_blob.h) against dsm_tts_slot_blob_info, without a
device: a blob built here by hand, field by field, must read back; bad magic, bad version, inconsistent sizes, counts over
their bounds, unknown flags and short buffers are refused; an STT blob is refused by the TTS reader and a TTS blob by the STT one."""
import struct

import pytest

MAGIC, VERSION = 0x42535444, 1
STT_MAGIC = 0x424C5344
S = 6


def align16(n):
    return (n + 15) & ~15


def item_bytes(it):
    step_idx, cpads, samp_k, cfg_on, cond_on, ca_len, req_flags, req_status, text, audio, q_tok, q_end = it
    assert len(text) == step_idx and len(audio) == step_idx * S
    out = struct.pack("<QQiIIIIIiIIIII", step_idx, cpads, samp_k, cfg_on, cond_on, ca_len[0], ca_len[1], req_flags, req_status,
                      len(q_end), len(q_tok), 0, 0, 0)
    assert len(out) == 64
    out += struct.pack(f"<{len(text)}I", *text) + struct.pack(f"<{len(audio)}I", *audio)
    out += struct.pack(f"<{len(q_tok)}I", *q_tok) + struct.pack(f"<{len(q_end)}i", *q_end)
    return out


def build_blob(items, sig, slot_bytes, flags=0, slices=S, payload_fill=0xAB, magic=MAGIC):
    host = b"".join(item_bytes(it) for it in items)
    host += b"\0" * (align16(len(host)) - len(host))
    sigb = struct.pack(f"<{len(sig)}I", *sig)
    sigb += b"\0" * (align16(len(sigb)) - len(sigb))
    total = 48 + len(sigb) + len(host) + len(items) * slot_bytes
    head = struct.pack("<IIIIIIQQQ", magic, VERSION, len(items), flags, len(sig), slices, len(host), slot_bytes, total)
    assert len(head) == 48
    return head + sigb + host + bytes([payload_fill]) * (len(items) * slot_bytes)


UNG = 0xFFFFFFFF
ITEMS = [
    # a request in the middle of its second word: 3 steps done, 5 queued tokens in 2 words
    (3, 1, 0, 0, 0, (0, 0), 1 | 4, 1, [3, 0, 7], list(range(3 * S)), [1, 9, 11, 4, 5], [3, 5]),
    # a fresh slot
    (0, 0, 0, 0, 0, (0, 0), 0, 0, [], [], [], []),
    # a guided, sampling, conditioned slot without a request; its newest audio row is partly ungenerated
    (2, 0, 25, 1, 1, (5, 3), 0, 0, [0, 3], list(range(S)) + [1] + [UNG] * (S - 1), [], []),
]
SIG = list(range(29))
HOST_OFF = 48 + align16(4 * len(SIG))
ITEM0 = len(item_bytes(ITEMS[0]))


def test_hand_built_blob_reads_back(dsm, lib):
    blob = build_blob(ITEMS, SIG, 4096 + 16, flags=dsm.TTS_SLOT_BLOB_HAS_MIMI_DEC)
    info = dsm.tts_slot_blob_info(blob)
    host = align16(sum(len(item_bytes(it)) for it in ITEMS))
    assert info == {"version": 1, "n_slots": 3, "flags": 1, "sig_words": len(SIG), "slices": S, "host_bytes": host,
                    "slot_bytes": 4112, "total_bytes": len(blob)}
    assert info["total_bytes"] == HOST_OFF + host + 3 * 4112
    # trailing bytes behind the blob are not its business; a one-slot blob of a fresh slot with no signature is the smallest
    assert dsm.tts_slot_blob_info(blob + b"xyz")["total_bytes"] == len(blob)
    small = build_blob([ITEMS[1]], [], 0)
    assert len(small) == 48 + 64 and dsm.tts_slot_blob_info(small)["n_slots"] == 1


def patched(blob, offset, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


@pytest.mark.parametrize("name,mutate,msg", [
    ("magic", lambda b: patched(b, 0, "<I", MAGIC ^ 1), "bad magic"),
    ("version", lambda b: patched(b, 4, "<I", 2), "version"),
    ("version0", lambda b: patched(b, 4, "<I", 0), "version"),
    ("no_slots", lambda b: patched(b, 8, "<I", 0), "slot count"),
    ("too_many_slots", lambda b: patched(b, 8, "<I", (1 << 20) + 1), "slot count"),
    ("flags", lambda b: patched(b, 12, "<I", 2), "unknown flags"),
    ("sig_too_long", lambda b: patched(b, 16, "<I", (1 << 12) + 1), "signature too long"),
    ("no_slices", lambda b: patched(b, 20, "<I", 0), "slice count"),
    ("too_many_slices", lambda b: patched(b, 20, "<I", (1 << 10) + 1), "slice count"),
    ("slot_bytes_unaligned", lambda b: patched(b, 32, "<Q", 4100), "payload size"),
    ("total", lambda b: patched(b, 40, "<Q", len(b) - 16), "total size"),
    ("host_bytes", lambda b: patched(b, 24, "<Q", 16), "host section"),
    ("host_bytes_unaligned", lambda b: patched(b, 24, "<Q", 1000), "host section"),
    # more steps than the section has bytes for: the tables run out inside the item
    ("steps_run_out", lambda b: patched(b, HOST_OFF, "<Q", 4000), "inside an item's tables"),
    ("steps_over_bound", lambda b: patched(b, HOST_OFF, "<Q", (1 << 20) + 1), "step index too large"),
    ("n_words_over_bound", lambda b: patched(b, HOST_OFF + 44, "<I", (1 << 20) + 1), "queue too long"),
    ("n_tok_over_bound", lambda b: patched(b, HOST_OFF + 48, "<I", (1 << 20) + 1), "queue too long"),
    ("n_tok_runs_out", lambda b: patched(b, HOST_OFF + 48, "<I", 40000), "inside an item's tables"),
    ("cfg_on", lambda b: patched(b, HOST_OFF + 20, "<I", 2), "cfg_on"),
    ("cond_on", lambda b: patched(b, HOST_OFF + 24, "<I", 7), "cond_on"),
    ("req_flags", lambda b: patched(b, HOST_OFF + 36, "<I", 8), "request flags"),
    ("reserved", lambda b: patched(b, HOST_OFF + 56, "<I", 1), "reserved"),
    # the last item (behind the first and the 64 bytes of the fresh one) claims no steps: the section is longer than its items
    ("host_len", lambda b: patched(b, HOST_OFF + ITEM0 + 64, "<Q", 0), "does not match"),
])
def test_malformed_blobs_are_refused(dsm, lib, name, mutate, msg):
    blob = build_blob(ITEMS, SIG, 4112)
    with pytest.raises(dsm.DsmError, match=msg):
        dsm.tts_slot_blob_info(mutate(blob))


def test_host_section_ending_inside_an_item(dsm, lib):
    """A consistent header whose host section is one 16-byte unit short of its three items: the reader stops inside the last."""
    blob = build_blob(ITEMS, SIG, 0)
    host = align16(sum(len(item_bytes(it)) for it in ITEMS))
    short = bytearray(blob[:len(blob) - 16])
    struct.pack_into("<Q", short, 24, host - 16)
    struct.pack_into("<Q", short, 40, len(short))
    with pytest.raises(dsm.DsmError, match="ends inside"):
        dsm.tts_slot_blob_info(bytes(short))
    # 176 bytes of the first item, then 16 of the second one's 64: the section ends inside an item's fixed part
    two = bytearray(build_blob([ITEMS[0], ITEMS[1]], [], 0)[:48 + 192])
    struct.pack_into("<Q", two, 24, 192)
    struct.pack_into("<Q", two, 40, len(two))
    with pytest.raises(dsm.DsmError, match="ends inside an item$"):
        dsm.tts_slot_blob_info(bytes(two))
    # four slots need at least 4 * 64 bytes
    fresh = bytearray(build_blob([ITEMS[1]] * 3, [], 0))
    struct.pack_into("<I", fresh, 8, 4)  # four slots announced, three present
    struct.pack_into("<Q", fresh, 24, 192)
    with pytest.raises(dsm.DsmError, match="too short for its slots"):
        dsm.tts_slot_blob_info(bytes(fresh))


def test_short_buffers_are_refused(dsm, lib):
    blob = build_blob(ITEMS, SIG, 4112)
    for n in (0, 1, 47):
        with pytest.raises(dsm.DsmError, match="shorter than its header"):
            dsm.tts_slot_blob_info(blob[:n])
    for n in (48, 49, 200, len(blob) - 4112, len(blob) - 1):
        with pytest.raises(dsm.DsmError, match="truncated"):
            dsm.tts_slot_blob_info(blob[:n])
    dsm.tts_slot_blob_info(blob)


def test_the_two_blob_kinds_refuse_each_other(dsm, lib):
    """An STT blob (csrc/dsm_slot_blob.h: magic "DSLB", 32-byte host items) is "bad magic" to dsm_tts_slot_blob_info, and a
    TTS blob is "bad magic" to dsm_slot_blob_info."""
    host = struct.pack("<QdIIII", 7, 0.32, 1, 0, 0, 0)
    stt = struct.pack("<IIIIIIQQQ", STT_MAGIC, 1, 1, 0, 0, 0, len(host), 16, 48 + len(host) + 16) + host + b"\0" * 16
    assert dsm.slot_blob_info(stt)["n_slots"] == 1
    with pytest.raises(dsm.DsmError, match="bad magic"):
        dsm.tts_slot_blob_info(stt)
    tts = build_blob(ITEMS, SIG, 16)
    assert dsm.tts_slot_blob_info(tts)["n_slots"] == 3
    with pytest.raises(dsm.DsmError, match="bad magic"):
        dsm.slot_blob_info(tts)
