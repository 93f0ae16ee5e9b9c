"""The packed-f32 instruction pattern that lost taps in seanet_front_kernel under overlap, pinned over the
whole library from the device assembly (no GPU; tools/packed_f32_hazards.py states the classes).  No parity test that runs a
kernel alone can see the defect, so the pattern is the check:

  class L  a v_pk_{fma,mul,add}_f32 result whose LOW register the next vector instruction reads, with nothing or only s_waitcnt
           in between: must not occur anywhere.
  class H  the next vector instruction reads only the HIGH register (never seen wrong): allowed per kernel and count, each entry
           of H_ALLOWED naming the GPU test that runs that kernel under overlap and compares bits."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "packed_f32_hazards.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "packed_f32_fixture.s")
needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc (device assembly)")

# kernel: (instances, the GPU test that runs it beside other kernels' vector work)
H_ALLOWED = {
    "attn_small_kernel<float, 64>": (9, "tests/test_packed_chains_overlap_gpu.py::test_depformer_f32_ring_attention_beside_the_lm"),
}


def _run(*args):
    out = subprocess.run([sys.executable, TOOL, "--json", *args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def _show(h):
    return "\n".join([f"{h['kernel']} (class {h['cls']}, {h['form']}; assembly line {h['line']}):", "    " + h["producer"]] +
                     ["    " + l for l in h["between"]] + ["    " + h["consumer"]])


@pytest.fixture(scope="module")
def library():
    return _run()


def test_parser_on_the_hand_written_fixture():
    """One instance each of waited L, adjacent L and H, and a pair behind an `s_nop` that is none; the adjacent L's consumer is a
    producer itself, and the `s_nop` behind it clears it."""
    rep = _run("--asm", FIXTURE)
    assert rep["kernels_with_packed_f32"] == 1 and rep["packed_f32_instructions"] == 5
    got = [(h["kernel"], h["cls"], h["form"], h["producer"].split()[1].rstrip(","), h["consumer"].split()[0], h["between"]) for h in rep["hazards"]]
    assert got == [
        ("fixture_kernel", "L", "waited", "v[6:7]", "v_fmac_f32_e32", ["s_waitcnt lgkmcnt(2)"]),
        ("fixture_kernel", "L", "adjacent", "v[8:9]", "v_pk_add_f32", []),
        ("fixture_kernel", "H", "adjacent", "v[32:33]", "v_cndmask_b32_e64", []),
    ], got


@needs_hipcc
def test_the_scan_sees_the_library(library):
    """A parser that stopped matching would find nothing and pass the two tests below."""
    per = library["packed_f32_per_kernel"]
    assert library["kernels_with_packed_f32"] >= 200, f"only {library['kernels_with_packed_f32']} kernels hold a packed-f32 instruction"
    assert "gemm_bx3u_kernel<bf16, 2, 2, 2, 8, 0, 4>" in per, "kernel names no longer demangle as expected"
    assert "seanet_front_kernel<64>" not in per, f"seanet_front_kernel<64> holds {per.get('seanet_front_kernel<64>')} packed-f32 instructions again"


@needs_hipcc
def test_no_packed_f32_result_is_read_in_its_low_half_by_the_next_vector_instruction(library):
    bad = [h for h in library["hazards"] if h["cls"] == "L"]
    assert not bad, (f"{len(bad)} packed-f32 results whose low register the next vector instruction reads (the sequence that lost taps "
                     "under overlap; keep the chain scalar with dsm_unpaired):\n" + "\n".join(_show(h) for h in bad))


@needs_hipcc
def test_high_half_readers_are_the_listed_ones_and_each_has_an_overlap_test(library):
    got = {}
    for h in library["hazards"]:
        if h["cls"] == "H":
            got.setdefault(h["kernel"], []).append(h)
    problems = []
    for k in sorted(set(got) | set(H_ALLOWED)):
        have, want = len(got.get(k, [])), H_ALLOWED.get(k, (0, None))[0]
        if have != want:
            problems.append(f"{k}: {have} instances, the table has {want}: remove the pattern (dsm_unpaired) or add a test that runs "
                            "this kernel under overlap and list it in H_ALLOWED\n" + "\n".join(_show(h) for h in got.get(k, [])))
    assert not problems, "\n".join(problems)
    for k, (_, test_id) in H_ALLOWED.items():
        path, name = test_id.split("::")
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(r"^def %s\(" % re.escape(name), src, re.M), f"{k}: its overlap test {test_id} does not exist"
