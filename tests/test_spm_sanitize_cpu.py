"""The SentencePiece model reader and tokenizer (csrc/dsm_spm.h) under AddressSanitizer + UBSan: a stand-alone program
(tests/sanitize_spm/spm_fuzz.cpp, its own main, nothing preloaded, no Python inside) replays the golden vectors, loads
seeded mutations of every golden model — each load fails cleanly or the model is then used — and tokenizes random bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_reader_and_tokenizer_under_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize_spm")
    r = subprocess.run(["make", "-s", "-C", d, "run"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "spm_fuzz ok" in r.stdout
