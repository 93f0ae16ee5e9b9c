"""The device assembly of libdsm_mi355x.so, as tools/kernel_resources.py and tools/packed_f32_hazards.py read it: one hipcc
device-only compile of csrc/dsm_engine.hip with the flags of delayed-streams-modeling_amd/build.py (no GPU needed, 30-80 s)."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "delayed-streams-modeling_amd", "csrc", "dsm_engine.hip")


def compile_device_asm(src=SRC):
    """The gfx950 assembly text of `src`, compiled as build.py compiles the library."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "dsm.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                        "-S", "--cuda-device-only", "-o", asm, src], check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def kernel_name(mangled):
    """`spk_attn_kernel<64>` from the mangled symbol: demangled, bf16 for its storage type, no return type, no argument list."""
    try:
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip() or mangled
    except FileNotFoundError:  # no binutils: the mangled name still identifies the kernel
        name = mangled
    name = name.replace("unsigned short", "bf16").replace("void ", "")
    return re.sub(r"\(.*", "", name)
