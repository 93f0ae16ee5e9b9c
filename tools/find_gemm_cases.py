#!/usr/bin/env python3
"""Writes tests/golden/gemm_cases.json: the products tests/test_gemm_kernels_gpu.py runs through dsm_debug_gemm (no GPU needed).

(a) For every class (tests/gemm_classes.py: gemm_class) of a served product (tests/gemm_cases.py: SERVED) that dsm_debug_gemm
offers, the shape of least M N K that reaches the class under explicit knobs, found by asking dsm_debug_gemm_plan_knobs over a grid
of shapes and knob settings.  chunk_loop_min_tiles and the small-K knobs are lowered (or raised out of reach) to get the whole-K
forms and their split-K counterparts at small shapes; everything else that selects a kernel is the shape's own.  (b) The edge
cases beyond serving, written out below and tagged "edge".  Every row carries the plan line it must get; run the tool again after
a deliberate change of a gate in plan_gemm and read the diff (--edges: keep the file's served cases, rewrite only the edge cases)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsm_amd  # noqa: E402
import gemm_cases as G  # noqa: E402
import gemm_classes as GC  # noqa: E402

P = GC.plans
OFF = 1 << 30  # a tile count no shape reaches: the knob's path is never taken

M_GRID = sorted({1, 2, 16, 17, 32, 33, 48, 64, 65, 96, 128} | {64 * j for j in (3, 4, 6, 8, 16, 32, 64, 128, 256, 512)} |
                {64 * j - 31 for j in (2, 3, 4, 6, 8, 16, 32, 64, 128, 256, 512)})
N_GRID = (8, 16, 24, 32, 40, 64, 96, 128, 160, 256, 288, 512, 544, 1024, 1056, 1088, 2048, 2080, 2112, 4096, 4128, 8192, 8224)
K_GRID = (7, 8, 24, 32, 40, 64, 96, 256, 288, 512, 544, 800, 1024, 1056, 1312, 1568, 1824, 2048, 2080, 2304, 3872, 4096)


def knob_grid(dot_mode):
    out = []
    for cl in (1, OFF):
        for sk, mt in ((OFF, 4), (1, 1), (1, 2), (1, 4)):
            for depth in (4, 2):
                out.append((dot_mode, cl, sk, mt, depth))
    return out


def r4(n):
    return (n + 3) // 4 * 4


def out_ld(N, ok4, exact=False):
    """A row stride for an output of N columns: wider than N where it may be, a multiple of 4 floats or not as the flags say."""
    if exact:
        return N
    if ok4:
        return r4(N) + 4
    return N + 1 if (N + 1) % 4 else N + 2


def maps_for(flags, M, N, K, norm):
    """Row maps that give launch_gemm the flag bits of a served row: (xmap, ymap, y2map, rmap) as (bstride, rpb, ld, toff) or None."""
    if flags & P.ALIGNED:
        xmap = (0, M, K + 8, 0)
    else:
        xmap = (0, M, K + 1 if (K + 1) % 4 else K + 2, 0)

    def omap(present, ok4, plain, toff):
        if not present:
            return None
        ld = out_ld(N, ok4, exact=bool(norm) and plain and toff == 0)
        if plain:
            return (0, M, ld, 0)
        return ((4 + toff) * ld, 4, ld, toff)  # rows in blocks of four behind `toff` carried rows: a concat buffer

    ymap = omap(flags & P.Y, flags & P.Y_OK4, flags & P.Y_PLAIN, 0 if flags & P.Y_PLAIN else 2)
    y2map = omap(flags & P.Y2, flags & P.Y2_OK4, False, 2)
    rmap = omap(flags & P.RES, flags & P.RES_OK4, True, 0)
    if rmap and norm:
        rmap = (0, M, r4(N) + 4, 0)
    return xmap, ymap, y2map, rmap


def case_row(lib, cid, edge, knobs, bf16, epi, M, N, K, xmap, ymap, y2map, rmap, bias=0, scale=0, act=0, norm=0, may_defer=0):
    c = dict(id=cid, edge=edge, knobs=list(knobs), weight_bf16=int(bool(bf16)), epi=epi, M=M, N=N, K=K, xmap=xmap, ymap=ymap, y2map=y2map,
             rmap=rmap, bias=bias, scale=scale, act=act, norm=norm, may_defer=may_defer)
    c["line"] = G.case_plan_line(lib, c)
    assert not c["line"].startswith("error"), c
    return c


def served_cases(lib):
    targets = {}  # class -> a served row that has it
    for r in G.served_rows(dsm_amd):
        line = P.plan_line(lib, r)
        if G.offered(r, line):
            targets.setdefault(GC.gemm_class(r, line), r)
    # one search per query signature: the grid is walked once and every class it reaches keeps its cheapest shape
    sigs = {}
    for cls, r in targets.items():
        sigs.setdefault((r["dot_mode"], r["weight_bf16"], r["epi"], r["nt"], r["flags"]), set()).add(cls)
    best = {}
    for (dot_mode, bf16, epi, nt, flags), wanted in sorted(sigs.items()):
        for M in M_GRID:
            for N in N_GRID:
                if flags & P.NORM and N % 4:
                    continue
                for K in K_GRID:
                    mnk = M * N * K
                    if mnk > G.CASE_MNK_CAP:
                        continue
                    row = dict(stt=1, dot_mode=dot_mode, weight_bf16=bf16, epi=epi, nt=nt, M=M, N=N, K=K, flags=flags)
                    for knobs in knob_grid(dot_mode):
                        line = P.plan_line_knobs(lib, row, knobs)
                        if line.startswith("error") or int(GC.plan_fields(line)["lds"]) > 65536:
                            continue
                        cls = GC.gemm_class(row, line)
                        if cls in wanted and (cls not in best or mnk < best[cls][0]):
                            best[cls] = (mnk, row, knobs)
    missing = set(targets) - set(best)
    assert not missing, "no shape of the grid reaches:\n" + "\n".join(" ".join(c) + "   e.g. " + targets[c]["name"] for c in sorted(missing))
    cases = []
    for i, cls in enumerate(sorted(best)):
        _, row, knobs = best[cls]
        flags, norm = row["flags"], 0
        if flags & P.NORM:
            norm = 1 + i % 2  # LayerNorm and RmsNorm take turns over the classes with a norm
        xmap, ymap, y2map, rmap = maps_for(flags, row["M"], row["N"], row["K"], norm)
        cid = "%s-%s-%s-m%dn%dk%d-%03d" % (cls[0].replace("<", "").replace(">", "").replace(",al=0", ""), GC.EPI_NAMES[row["epi"]][4:].lower(),
                                          "bf16" if row["weight_bf16"] else "f32", row["M"], row["N"], row["K"], i)
        c = case_row(lib, cid, 0, knobs, row["weight_bf16"], row["epi"], row["M"], row["N"], row["K"], xmap, ymap, y2map, rmap,
                     bias=int(bool(flags & P.BIAS)), norm=norm, may_defer=int(bool(flags & P.MAY_DEFER)))
        assert GC.gemm_class(G.case_query_row(c), c["line"]) == cls, (c, cls)
        cases.append(c)
    return cases


def edge_cases(lib):
    D0, D1 = (0, -1, -1, -1, -1), (1, -1, -1, -1, -1)  # an STT engine's own knobs in either mode
    S, GATE = P.STORE, P.GATE
    out = []

    def add(cid, knobs, bf16, epi, M, N, K, xmap=None, ymap=None, y2map=None, rmap=None, **kw):
        xmap = xmap or (0, M, K + 8, 0)
        if ymap is None and y2map is None:
            ymap = (0, M, r4(N) + 4, 0)
        knobs = G.explicit_knobs(knobs)
        out.append(case_row(lib, "edge-" + cid, 1, knobs, bf16, epi, M, N, K, xmap, ymap, y2map, rmap, **kw))

    for tag, knobs, bf16 in (("f32", D0, 0), ("bf16-mode0", D0, 1), ("bf16-mode1", D1, 1)):
        add(f"n8-{tag}", knobs, bf16, S, 16, 8, 512)                     # N < 16: one ragged 16-column tile
        add(f"n40-{tag}", knobs, bf16, S, 33, 40, 512, bias=1)           # N in 17..63: the workgroup's fourth wave idles
        add(f"n7-{tag}", knobs, bf16, S, 17, 7, 512, rmap=(0, 17, 9, 0))               # N % 4 != 0: the last lane group stores part of its four
        add(f"n30-{tag}", knobs, bf16, S, 33, 30, 512, ymap=(0, 33, 36, 0), y2map=(6 * 36, 4, 36, 2))
        add(f"k24-{tag}", knobs, bf16, S, 17, 72, 24)                    # K < 32 on the generic kernel
        add(f"k40-{tag}", knobs, bf16, S, 17, 72, 40, bias=1)            # a K tail behind one whole block
        add(f"k4360-{tag}", knobs, bf16, S, 33, 40, 17 * 256 + 8)        # 18 chunks: several chunks per wave, summed through LDS
        add(f"xodd-{tag}", knobs, bf16, S, 33, 96, 512, xmap=(0, 33, 513, 0))          # rows off a 16-byte boundary, K % 32 == 0
        add(f"yld-{tag}", knobs, bf16, S, 17, 64, 512, ymap=(0, 17, 67, 0))            # Y's ld % 4 != 0: vec = 0
        add(f"y2toff-{tag}", knobs, bf16, S, 33, 64, 512, ymap=(0, 33, 68, 0), y2map=(7 * 64, 4, 64, 3), bias=1)
        add(f"m1-{tag}", knobs, bf16, S, 1, 96, 512)
        add(f"m65-{tag}", knobs, bf16, S, 65, 96, 512, rmap=(0, 65, 100, 0))           # M = 16 k + 1
        add(f"gate-m17-{tag}", knobs, bf16, GATE, 17, 80, 288)
        # a convolution over its concat buffer: three taps of 32 channels, rows overlap (K > ld)
        add(f"conv-{tag}", knobs, bf16, S, 30, 64, 96, xmap=(34 * 32, 10, 32, 0), bias=1, y2map=(14 * 64, 10, 64, 4))
        # everything the store epilogue has at once: bias, gelu, LayerScale, residual, Y and Y2
        add(f"epi-all-{tag}", knobs, bf16, S, 33, 72, 512, ymap=(0, 33, 76, 0), y2map=(6 * 76, 4, 76, 2), rmap=(0, 33, 72, 0), bias=1, scale=1, act=1)
        # the separate norm every shipped model runs (row_norm_kernel, N <= 4096): behind the generic kernel, behind a whole-K
        # loop form at N = 2048 (chunk_loop_min_tiles = 1), behind a one-chunk product, behind a tile reduce (Y2 keeps the norm out of it)
        loop = (knobs[0], 1, -1, -1, -1)
        for norm, nn in ((1, "ln"), (2, "rms")):
            add(f"norm-generic-{nn}-{tag}", knobs, bf16, S, 17, 512, 40, ymap=(0, 17, 512, 0), rmap=(0, 17, 516, 0), norm=norm, bias=1)
            add(f"norm-loop-{nn}-{tag}", loop, bf16, S, 33, 2048, 288, ymap=(0, 33, 2048, 0), rmap=(0, 33, 2052, 0), norm=norm)
            add(f"norm-onechunk-{nn}-{tag}", knobs, bf16, S, 65, 1024, 256, ymap=(0, 65, 1024, 0), norm=norm, scale=1)
            add(f"norm-y2-{nn}-{tag}", knobs, bf16, S, 17, 4096, 512, ymap=(0, 17, 4096, 0), y2map=(6 * 4096, 4, 4096, 2), rmap=(0, 17, 4096, 0), norm=norm)
        for n, kind in ((1024, "rows1"), (2048, "rows2"), (4096, "rows4"), (4100, "separate")):
            for norm, nn in ((1, "ln"), (2, "rms")):
                add(f"norm-{kind}-{nn}-{tag}", knobs, bf16, S, 17, n, 512, ymap=(0, 17, n, 0), rmap=(0, 17, n + 4, 0), norm=norm, scale=1)
    return out


if __name__ == "__main__":
    lib = dsm_amd.load_library()
    if "--edges" in sys.argv:  # keep the served cases of the file as they are (the search takes two minutes), rewrite the edge cases
        cases = [c for c in G.load_cases() if not c["edge"]] + edge_cases(lib)
    else:
        cases = served_cases(lib) + edge_cases(lib)
    assert len({c["id"] for c in cases}) == len(cases)
    out = os.path.join(ROOT, "tests", "golden", "gemm_cases.json")
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    print(out, len(cases), "cases,", sum(c["edge"] for c in cases), "of them edge cases; largest M N K", max(G.case_mnk(c) for c in cases))
