"""The ingest section's host code (csrc/dsm_pcm_format.h: the descriptor of an input format, its checked reader, the streaming host
function) under AddressSanitizer + UBSan: a stand-alone program (tests/sanitize_ingest/ingest_fuzz.cpp, its own main, nothing
preloaded, no Python inside) streams every common rate and format from heap frames of exactly the declared length, feeds random
rates and formats, random and mutated descriptors and frames shorter than declared — each is accepted or refused cleanly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ingest_host_code_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_ingest")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ingest_fuzz ok" in r.stdout
