"""The host-side validation an import of a TTS slot blob has to make (csrc/dsm_tts_slot_layout.h: the layout and check_slot) under AddressSanitizer
+ UBSan: a stand-alone program (tests/sanitize_tts_xfer/tts_xfer_fuzz.cpp; its own main, nothing preloaded, no Python inside) feeds
seeded mutations of valid payloads and host items to the index checks — each is accepted or refused cleanly, no read leaves the
payload, and every accepted slot satisfies every bound restated in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tts_import_validation_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_tts_xfer")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tts_xfer_fuzz ok" in r.stdout
