"""The text bias's host code (csrc/dsm_text_bias.h: the compiler of a bias set, the checked reader of its table, the host pick)
under AddressSanitizer + UBSan: a stand-alone program (tests/sanitize_bias/bias_fuzz.cpp, its own main, nothing preloaded, no
Python inside) compiles seeded random and malformed sets and feeds mutated, truncated and random tables with random nodes and
rows to the pick — each is accepted or refused cleanly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_text_bias_host_code_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_bias")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "bias_fuzz ok" in r.stdout
