"""The slot blob's documented layout (csrc/dsm_slot_blob.h) against dsm_slot_blob_info, without a device: a blob
built here by hand, field by field, must read back; bad magic, bad version, inconsistent sizes and short buffers are refused."""
import struct

import pytest

MAGIC, VERSION = 0x424C5344, 1


def align16(n):
    return (n + 15) & ~15


def build_blob(items, sig, slot_bytes, flags=0, payload_fill=0xAB):
    """items: (step_idx, last_stop_time, unended_word, side_flags, [word tokens]) per slot."""
    host = b""
    for step_idx, stop, unended, side_flags, toks in items:
        host += struct.pack("<QdIIII", step_idx, stop, unended, side_flags, len(toks), 0)
        host += struct.pack(f"<{len(toks)}I", *toks)
    host += b"\0" * (align16(len(host)) - len(host))
    sigb = struct.pack(f"<{len(sig)}I", *sig)
    sigb += b"\0" * (align16(len(sigb)) - len(sigb))
    total = 48 + len(sigb) + len(host) + len(items) * slot_bytes
    head = struct.pack("<IIIIIIQQQ", MAGIC, VERSION, len(items), flags, len(sig), 0, len(host), slot_bytes, total)
    assert len(head) == 48
    return head + sigb + host + bytes([payload_fill]) * (len(items) * slot_bytes)


ITEMS = [(7, 0.32, 1, 0, [5, 9, 11]), (0, 0.0, 0, 3, []), (123456789012, 1.5, 0, 1, list(range(40)))]
SIG = [2, 4, 32, 12, 1, 2, 2, 32, 10, 4, 65, 64, 33, 2, 1, 6, 1]


def test_hand_built_blob_reads_back(dsm, lib):
    blob = build_blob(ITEMS, SIG, 4096 + 16, flags=dsm.SLOT_BLOB_HAS_MODEL_MIMI)
    info = dsm.slot_blob_info(blob)
    host = align16(sum(32 + 4 * len(t[4]) for t in ITEMS))
    assert info == {"version": 1, "n_slots": 3, "flags": 1, "sig_words": len(SIG), "host_bytes": host,
                    "slot_bytes": 4112, "total_bytes": len(blob)}
    assert info["total_bytes"] == 48 + align16(4 * len(SIG)) + host + 3 * 4112
    # trailing bytes behind the blob are not its business; a one-slot blob with no words and no signature is the smallest
    assert dsm.slot_blob_info(blob + b"xyz")["total_bytes"] == len(blob)
    small = build_blob([(0, 0.0, 0, 0, [])], [], 0)
    assert len(small) == 48 + 32 and dsm.slot_blob_info(small)["n_slots"] == 1


def patched(blob, offset, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


@pytest.mark.parametrize("name,mutate,msg", [
    ("magic", lambda b: patched(b, 0, "<I", MAGIC ^ 1), "magic"),
    ("version", lambda b: patched(b, 4, "<I", 2), "version"),
    ("version0", lambda b: patched(b, 4, "<I", 0), "version"),
    ("no_slots", lambda b: patched(b, 8, "<I", 0), "slot count"),
    ("flags", lambda b: patched(b, 12, "<I", 2), "flags"),
    ("slot_bytes_unaligned", lambda b: patched(b, 32, "<Q", 4100), "payload size"),
    ("total", lambda b: patched(b, 40, "<Q", len(b) - 16), "total size"),
    ("host_bytes", lambda b: patched(b, 24, "<Q", 16), "host section"),
    ("word_runs_out", lambda b: patched(b, 48 + align16(4 * len(SIG)) + 24, "<I", 4000), "inside a word"),
    ("word_too_long", lambda b: patched(b, 48 + align16(4 * len(SIG)) + 24, "<I", 1 << 20), "word too long"),
    ("unended", lambda b: patched(b, 48 + align16(4 * len(SIG)) + 16, "<I", 2), "unended_word"),
    # the last item (behind 32 + 12 and 32 bytes) four tokens shorter: the section is then 16 bytes longer than its items
    ("host_len", lambda b: patched(b, 48 + align16(4 * len(SIG)) + 76 + 24, "<I", 36), "does not match"),
])
def test_malformed_blobs_are_refused(dsm, lib, name, mutate, msg):
    blob = build_blob(ITEMS, SIG, 4112)
    with pytest.raises(dsm.DsmError, match=msg):
        dsm.slot_blob_info(mutate(blob))


def test_short_buffers_are_refused(dsm, lib):
    blob = build_blob(ITEMS, SIG, 4112)
    for n in (0, 1, 47):
        with pytest.raises(dsm.DsmError, match="shorter than its header"):
            dsm.slot_blob_info(blob[:n])
    for n in (48, 49, 200, len(blob) - 4112, len(blob) - 1):
        with pytest.raises(dsm.DsmError, match="truncated"):
            dsm.slot_blob_info(blob[:n])
    dsm.slot_blob_info(blob)
