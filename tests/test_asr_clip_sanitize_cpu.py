"""The host half of the clips section (csrc/dsm_asr_clip.h: the cut, the schedule, the records' reader and the message replay of
dsm_asr_collect) under AddressSanitizer + UBSan: a stand-alone program (tests/sanitize_clip/clip_fuzz.cpp; its own main, nothing
preloaded, no Python inside) drives them with seeded random and mutated lengths, tables and capacities — every buffer a heap block
of exactly its size, every outcome checked against a restatement in the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_host_code_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_clip")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "clip_fuzz ok" in r.stdout
