"""The TTS slot blob's header and host-section parser (csrc/dsm_tts_slot_blob.h) under AddressSanitizer + UBSan: a stand-alone
program (tests/sanitize_slot/slot_blob_fuzz.cpp, which runs both blob kinds; its own main, nothing preloaded, no Python inside) reads valid blobs
back and feeds seeded mutations and truncations of them to the parser — each is accepted or refused cleanly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tts_slot_blob_parser_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_slot")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tts_slot_blob_fuzz ok" in r.stdout
