#!/usr/bin/env python3
"""Reads longer than 1024 bases on the affine kernels (option "long_reads", swmi_affine.hip): sweep and traceback times of the
strip sweeps next to the wide kernel's, one JSON line per shape.

  wide1024      1000 x (1024 x 2000), local, gap_open = -6: the wide kernel (the same line on a library without the option)
  long1025/2048/4096   1000 x (m x 2000), local, gap_open = -6: rows computed = 1024 * ceil(m / 1024)
  c4_local / c4_global 64 x (10,000 x 10,000)
  blosum62      1000 x (1500 x 2000), BLOSUM62, gap_open = -11, gap = -1

Per line: `steps` runs with option "profiling" = 1 (HIP events around the sweep and the traceback) after `warmup`; the median,
the minimum and the maximum of the sweep times; GCUPS over the m x n cells and over the cells the sweep computes (rows padded
to whole strips).  --lib-note labels the lines (SWMI_LIB selects another build of the library)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import matrix as M  # noqa: E402


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def measure(name, refs, reads, steps, warmup, scores=(5, -3, -2), gap_open=-6, mode=0, mat=None, note=""):
    ctx = sw.Context(0)
    try:
        m = max(len(r) for r in reads)
        ctx.set_option("gap_open", gap_open)
        if m > 1024:
            ctx.set_option("long_reads", 1)
        if mode:
            ctx.set_option("align_mode", mode)
        if mat is not None:
            ctx.set_score_matrix(mat)
        ctx.set_option("profiling", 1)
        b = ctx.upload(refs, reads)
        p = sw.make_params(scores)
        for _ in range(warmup):
            b.run(p)
        fill, tb = [], []
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
        cells = b.timing().cells
        rows = 1024 * ((m + 1023) // 1024) if m > 1024 else m
        computed = sum(len(r) for r in refs) * sum(rows for _ in reads)
        sc, na = b.pair_results()
        med = statistics.median(fill)
        out = {"shape": name, "lib": note, "pairs": len(refs) * len(reads), "read": m, "mode": b.pipeline_mode(), "align_mode": mode,
               "sweep_ms": round(med, 4), "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "cells": int(cells), "gcups": round(cells / (med * 1e-3) / 1e9, 1),
               "computed_cells": int(computed), "gcups_computed": round(computed / (med * 1e-3) / 1e9, 1),
               "launches": int(b.timing().fill_launches), "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="wide1024,long1025,long2048,long4096,c4_local,c4_global,blosum62")
    ap.add_argument("--lib-note", default="")
    args = ap.parse_args()
    rng = random.Random(2024)
    refs = [_rand(rng, 2000) for _ in range(1000)]
    for name in args.shapes.split(","):
        kw = dict(steps=args.steps, warmup=args.warmup, note=args.lib_note)
        if name == "wide1024" or name.startswith("long"):
            m = 1024 if name == "wide1024" else int(name[4:])
            read = _rand(rng, m)
            read = read[:m - 200] + refs[7][500:650] + read[m - 50:]
            out = measure(name, refs, [read], **kw)
        elif name in ("c4_local", "c4_global"):
            big = [_rand(rng, 10000) for _ in range(8)]
            out = measure(name, big, [_rand(rng, 10000) for _ in range(8)], mode=2 if name == "c4_global" else 0, **kw)
        elif name == "blosum62":
            amino = "ARNDCQEGHILKMFPSTWYV"
            prefs = [_rand(rng, 2000, amino) for _ in range(1000)]
            out = measure(name, prefs, [_rand(rng, 1300, amino) + prefs[3][400:600]], scores=(5, -4, -1), gap_open=-11, mat=M.BLOSUM62, **kw)
        else:
            raise SystemExit("unknown shape %s" % name)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
