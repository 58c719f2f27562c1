#!/usr/bin/env python3
"""End-to-end alignment modes (option "align_mode", swmi_affine.hip) on the GPU: sweep and traceback times of the local, fit and
global kernels on the same batches, one JSON line per (shape, mode).

  headline      1000 x (150 x 2000), gap_open = -6 (the batch of tools/affine_bench.py)
  engineerdata  40,000 x (80 x 400): 100 references of 400 bases x 400 reads of 80, gap_open = -6

Per line: `steps` timed runs after `warmup` (wall time of swmi_batch_run, results in host memory), then the same runs with
option "profiling" = 1 for the kernels' own times (HIP events around the sweep and the traceback).  --modes picks the modes
(default all three)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import synth       # noqa: E402

MODES = {"local": 0, "fit": 1, "global": 2}


def measure(name, refs, reads, mode, steps, warmup, gap_open=-6, scores=(5, -3, -4)):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", gap_open)
        if mode != "local":                     # (a library without the option still runs the local line)
            ctx.set_option("align_mode", MODES[mode])
        b = ctx.upload(refs, reads)
        p = sw.make_params(scores)
        for _ in range(warmup):
            b.run(p)
        wall = []
        for _ in range(steps):
            t = time.perf_counter()
            b.run(p)
            wall.append((time.perf_counter() - t) * 1e3)
        sc, na = b.pair_results()
        ctx.set_option("profiling", 1)
        fill, tb = [], []
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
        cells = b.timing().cells
        ms = statistics.median(wall)
        n_al, n_ch = b.materialise_all() if hasattr(b, "materialise_all") else (int(na.sum()), 0)
        out = {"shape": name, "align_mode": mode, "pairs": len(refs) * len(reads), "gap_open": gap_open, "mode": b.pipeline_mode(),
               "ms_per_run": round(ms, 4), "sweep_ms": round(statistics.median(fill), 4), "sweep_ms_min": round(min(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "cells": int(cells),
               "gcups_sweep": round(cells / (statistics.median(fill) * 1e-3) / 1e9, 1),
               "score_sum": int(sc.astype("int64").sum()), "alignments": int(n_al), "aligned_chars": int(n_ch)}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="local,fit,global")
    ap.add_argument("--shapes", default="headline,engineerdata")
    args = ap.parse_args()
    shapes = {}
    if "headline" in args.shapes:
        shapes["headline"] = synth.config_1k(n_refs=1000, ref_len=2000, read_len=150)
    if "engineerdata" in args.shapes:
        erefs, _ = synth.config_1k(n_refs=100, ref_len=400, read_len=80, seed=7)
        shapes["engineerdata"] = (erefs, [synth.config_1k(n_refs=1, ref_len=400, read_len=80, seed=100 + k)[1][0] for k in range(400)])
    for name, (refs, reads) in shapes.items():
        for mode in args.modes.split(","):
            print(json.dumps(measure(name, refs, reads, mode, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
