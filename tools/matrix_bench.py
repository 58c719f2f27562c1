#!/usr/bin/env python3
"""Score matrices (swmi_set_score_matrix, the matrix sweeps of swmi_affine.hip) on the GPU: sweep and traceback times and GCUPS,
one JSON line per shape, each DNA shape with and without a matrix that gives the same scores.

  dna           1000 x (150 x 2000), gap_open -6 and 0 ("affine" = 1: both on the affine kernels), match 5 / mismatch -3 / gap -4,
                without a matrix and with the identity matrix over ACGT (5 on the diagonal, -3 off it)
  engineerdata  40,000 x (80 x 400): 100 references of 400 bases x 400 reads of 80, gap_open -6, without and with the matrix
  protein       1000 x (300 x 2000) random residues, BLOSUM62, gap_open -11, gap -1

Per shape: `steps` timed runs after `warmup` (wall time of swmi_batch_run, results in host memory), then the same runs with
option "profiling" = 1 for the kernels' own times (HIP events around the sweep and the traceback)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import matrix as M  # noqa: E402
from sparksmithwaterman_amd import synth       # noqa: E402


def measure(name, refs, reads, gap_open, matrix, steps, warmup, scores=(5, -3, -4)):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", gap_open)
        ctx.set_option("affine", 1)
        if matrix is not None:
            ctx.set_score_matrix(matrix)
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
        out = {"shape": name, "pairs": len(refs) * len(reads), "gap_open": gap_open, "matrix": matrix is not None, "mode": mode,
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
    ident = M.uniform("ACGT", 5, -3)
    refs, reads = synth.config_1k(n_refs=1000, ref_len=2000, read_len=150)
    for o in (-6, 0):
        for mat in (None, ident):
            print(json.dumps(measure("dna", refs, reads, o, mat, args.steps, args.warmup)), flush=True)
    erefs, _ = synth.config_1k(n_refs=100, ref_len=400, read_len=80, seed=7)
    ereads = [synth.config_1k(n_refs=1, ref_len=400, read_len=80, seed=100 + k)[1][0] for k in range(400)]
    for mat in (None, ident):
        print(json.dumps(measure("engineerdata", erefs, ereads, -6, mat, args.steps, args.warmup)), flush=True)
    rng = random.Random(7)
    aa = "ARNDCQEGHILKMFPSTWYV"
    prefs = ["".join(rng.choice(aa) for _ in range(2000)) for _ in range(1000)]
    preads = ["".join(rng.choice(aa) for _ in range(300))]
    print(json.dumps(measure("protein", prefs, preads, -11, M.BLOSUM62, args.steps, args.warmup, scores=(1, -1, -1))), flush=True)


if __name__ == "__main__":
    main()
