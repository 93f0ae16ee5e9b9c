"""The egress section's host code (csrc/dsm_pcm_format.h: the descriptor of an output format, its checked reader, the sample
encoders, the streaming host function) under AddressSanitizer + UBSan: a stand-alone program (tests/sanitize_egress/egress_fuzz.cpp,
its own main, nothing preloaded, no Python inside) streams every admitted rate and format into heap rows of exactly the declared
length with extreme sample values among the input, mutates every descriptor word — each is refused — moves table offsets to and
past the arena's end, and feeds random rates, formats and descriptors: each is accepted or refused cleanly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_egress_host_code_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_egress")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "egress_fuzz ok" in r.stdout
