"""Register / scratch budget of the speaker encoder's kernels, from the device assembly (no GPU), in the style of
tests/test_kernel_resources_cpu.py: the new kernels must not spill, use no scratch, and allocate no padded registers."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("spk_attn_kernel<32>", "spk_attn_kernel<64>", "spk_normalize_kernel", "spk_rope_table_kernel", "spk_pad_rows_kernel")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="needs hipcc (device assembly)")
def test_speaker_kernels_do_not_spill():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "spk_"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {l[:64].strip(): l for l in out.stdout.splitlines()[1:] if l.strip()}
    print(out.stdout)
    for k in KERNELS:
        assert k in rows, f"{k} is not in the library:\n{out.stdout}"
        used, alloc, lds, scratch, occ = (int(v) for v in rows[k][64:].split()[:5])
        assert scratch == 0 and not rows[k].endswith("SPILLS"), rows[k]
        assert not rows[k].endswith("PADDED"), rows[k]
        assert alloc <= 128, rows[k]  # at least four waves per SIMD
