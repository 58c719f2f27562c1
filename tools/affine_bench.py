#!/usr/bin/env python3
"""Affine-gap path (swmi_affine.hip) on the GPU: sweep and traceback times and GCUPS of the full path, one JSON line per shape.

  headline      1000 x (150 x 2000), gap_open = -6
  reduction     the same batch on the affine kernels at gap_open = 0 ("affine" = 1), and on the linear path (mode 1)
  engineerdata  40,000 x (80 x 400): 100 references of 400 bases x 400 reads of 80, gap_open = -6

Per shape: `steps` timed runs after `warmup` (wall time of swmi_batch_run, results in host memory), then the same runs with
option "profiling" = 1 for the kernels' own times (HIP events around the sweep and the traceback)."""
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


def measure(name, refs, reads, gap_open, affine, steps, warmup, scores=(5, -3, -4)):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", gap_open)
        ctx.set_option("affine", affine)
        b = ctx.upload(refs, reads)
        p = sw.make_params(scores)
        for _ in range(warmup):
            b.run(p)
        wall = []
        for _ in range(steps):
            t = time.perf_counter()
            b.run(p)
            wall.append((time.perf_counter() - t) * 1e3)
        mode = b.pipeline_mode()
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
        out = {"shape": name, "pairs": len(refs) * len(reads), "gap_open": gap_open, "mode": mode,
               "ms_per_run": round(ms, 4), "sweep_ms": round(statistics.median(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "cells": int(cells),
               "gcups_full_path": round(cells / (ms * 1e-3) / 1e9, 1),
               "gcups_sweep": round(cells / (statistics.median(fill) * 1e-3) / 1e9, 1),
               "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    refs, reads = synth.config_1k(n_refs=1000, ref_len=2000, read_len=150)
    for name, o, aff in (("headline", -6, -1), ("reduction-affine", 0, 1), ("reduction-linear", 0, -1)):
        print(json.dumps(measure(name, refs, reads, o, aff, args.steps, args.warmup)), flush=True)
    erefs, _ = synth.config_1k(n_refs=100, ref_len=400, read_len=80, seed=7)
    ereads = [synth.config_1k(n_refs=1, ref_len=400, read_len=80, seed=100 + k)[1][0] for k in range(400)]
    print(json.dumps(measure("engineerdata", erefs, ereads, -6, -1, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
