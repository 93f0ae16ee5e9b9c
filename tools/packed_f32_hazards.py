#!/usr/bin/env python3
"""Packed-f32 results read by the next vector instruction, per kernel of libdsm_mi355x.so, from the device assembly (no GPU).

seanet_front_kernel once lost taps of an FMA chain while other kernels' vector work shared its SIMDs: the
compiler had paired two scalar chains into dependent v_pk_fma_f32 with only an `s_waitcnt` between a result and its reader, and
the reader got the LOW half of the accumulator pair from before the write.  No parity test that runs a kernel alone sees that, so
the instruction pattern itself is pinned (tests/test_packed_f32_hazards_cpu.py).  The pattern, not a rule about the hardware:

  producer  v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 writing v[a:a+1]
  consumer  the next instruction in the text, `s_waitcnt` lines skipped (one whose count is met takes no issue cycle); a label,
            a branch, an `s_nop`, an assembler directive or any other instruction ends the window
  class L   the consumer is a vector ALU instruction (v_*) that reads v[a]: as a source operand, as the accumulator of a
            v_fmac / v_mac form, or inside a source pair of a packed consumer.  `waited`: s_waitcnt lines lay in between (the
            form measured bad); `adjacent`: nothing did
  class H   the consumer reads v[a+1] and not v[a] (the half never seen wrong; allowed per kernel beside an overlap test)

usage: tools/packed_f32_hazards.py [--asm FILE] [--json] [-v] [substring ...]
  --asm FILE  scan this assembly text instead of compiling the library (about 40 s)
  --json      one JSON object: {"kernels_with_packed_f32": n, "packed_f32_instructions": n, "hazards": [...]}
  -v          print every instance (kernel, line, producer, what lay between, consumer) under the table"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_asm import compile_device_asm, kernel_name

PRODUCERS = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")
_REG = re.compile(r"\bv(?:(\d+)\b|\[(\d+):(\d+)\])")
_FUNC = re.compile(r"^([A-Za-z_$][\w$.]*):")  # a function's own label; basic blocks are .LBB*


def _regs(text):
    """The VGPR numbers an operand text names: v7, -v7, |v7|, v[8:9] -> {8, 9}."""
    out = set()
    for m in _REG.finditer(text):
        lo, hi = (int(m.group(1)),) * 2 if m.group(1) else (int(m.group(2)), int(m.group(3)))
        out.update(range(lo, hi + 1))
    return out


def _split(ins):
    mn, _, rest = ins.partition(" ")
    return mn, [o.strip() for o in rest.split(",")] if rest.strip() else []


def reads(ins):
    """VGPRs a vector ALU instruction reads: every operand but the first; the first too where the destination is also an input
    (v_fmac / v_mac / v_pk_fmac accumulate on it, v_writelane and DPP forms keep its old lanes, v_swap exchanges)."""
    mn, ops = _split(ins)
    src = _regs(",".join(ops[1:]))
    if re.match(r"v_(pk_)?(fmac|mac)_|v_dot\w*c_|v_writelane|v_swap", mn) or mn.endswith("_dpp"):
        src |= _regs(ops[0]) if ops else set()
    return src


def scan(asm):
    """(hazards, packed-f32 instruction count per function).  hazards: dicts with function (mangled), line (1-based, of the
    producer), cls 'L' or 'H', form 'waited' or 'adjacent', producer, between (list of s_waitcnt lines), consumer."""
    hazards, packed = [], {}
    func = None
    pending = None  # (line, instruction, low register, waits)
    for no, raw in enumerate(asm.splitlines(), 1):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue  # comment lines (`; %bb.3:` names a fall-through block, not a branch target) and blanks
        m = _FUNC.match(line)
        if m and not line.startswith(".L"):
            func, pending = m.group(1), None
            continue
        if func is None:
            continue
        if line.startswith(".Lfunc_end"):
            func, pending = None, None
            continue
        if line.startswith(".") or line.endswith(":"):
            pending = None  # a label (branch target) or a directive (.p2align pads with s_nop)
            continue
        mn = line.split(None, 1)[0]
        if pending and mn == "s_waitcnt":
            pending[3].append(line)
            continue
        if pending and mn.startswith("v_"):
            pline, pins, a, waits = pending
            r = reads(line)
            cls = "L" if a in r else ("H" if a + 1 in r else None)
            if cls:
                hazards.append(dict(function=func, line=pline, cls=cls, form="waited" if waits else "adjacent", producer=pins,
                                    between=list(waits), consumer=line))
        pending = None
        if mn in PRODUCERS:
            packed[func] = packed.get(func, 0) + 1
            dst = _REG.search(_split(line)[1][0])
            pending = (no, line, int(dst.group(2) if dst.group(2) else dst.group(1)), [])
    return hazards, packed


def report(asm):
    hazards, packed = scan(asm)
    names = {f: kernel_name(f) for f in set(packed) | {h["function"] for h in hazards}}
    for h in hazards:
        h["kernel"] = names[h["function"]]
    return dict(kernels_with_packed_f32=len(packed), packed_f32_instructions=sum(packed.values()),
                packed_f32_per_kernel={names[f]: n for f, n in packed.items()}, hazards=hazards)


def main(argv):
    as_json, verbose, path, subs = False, False, None, []
    it = iter(argv)
    for a in it:
        if a == "--json": as_json = True
        elif a == "-v": verbose = True
        elif a == "--asm": path = next(it)
        else: subs.append(a)
    rep = report(open(path).read() if path else compile_device_asm())
    hz = [h for h in rep["hazards"] if not subs or any(s in h["kernel"] for s in subs)]
    if as_json:
        rep["hazards"] = hz
        print(json.dumps(rep))
        return 0
    print(f"{rep['packed_f32_instructions']} v_pk_{{fma,mul,add}}_f32 in {rep['kernels_with_packed_f32']} kernels")
    print(f"{'kernel':64s} {'L waited':>8s} {'L adjacent':>10s} {'H':>4s}")
    count = {}
    for h in hz:
        key = "H" if h["cls"] == "H" else "L " + h["form"]
        count.setdefault(h["kernel"], {}).setdefault(key, 0)
        count[h["kernel"]][key] += 1
    for k in sorted(count):
        c = count[k]
        print(f"{k[:64]:64s} {c.get('L waited', 0):8d} {c.get('L adjacent', 0):10d} {c.get('H', 0):4d}")
    tot = lambda key: sum(c.get(key, 0) for c in count.values())
    print(f"{'total':64s} {tot('L waited'):8d} {tot('L adjacent'):10d} {tot('H'):4d}")
    if verbose:
        for h in hz:
            print(f"\n{h['kernel']}  class {h['cls']} ({h['form']}), assembly line {h['line']}")
            for l in [h["producer"]] + h["between"] + [h["consumer"]]:
                print("    " + l)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
