#!/usr/bin/env python3
"""Per-read score profiles (swmi_batch_set_read_profiles, the profile sweeps of swmi_affine.hip) on the GPU against the plain and the
matrix sweep of the same batch and scores: one JSON line per shape, variant and repetition, three repetitions each.

  dna           1000 x (150 x 2000), gap_open -6, match 5 / mismatch -3 / gap -4; the matrix is the identity over ACGT
  protein       1000 x (300 x 2000) random residues, BLOSUM62, gap_open -11, gap -1 (no plain variant: it would score otherwise)
  engineerdata  40,000 x (80 x 400): 100 references of 400 bases x 400 reads of 80, gap_open -6, the identity matrix

Variants: "plain" (no matrix), "matrix", "profile" = matrix.profile_from_matrix of that matrix for every read, which scores the same
(the line carries the score sum and the alignment count of each, so the three can be compared), and "set" = the
Batch.set_read_profiles call itself (host time, median of `steps` calls).  Per run: `steps` timed runs after `warmup` (wall time of
swmi_batch_run), then the same with option "profiling" = 1 for the kernels' own times."""
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


def measure(shape, variant, rep, refs, reads, gap_open, scores, matrix, steps, warmup):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", gap_open)
        ctx.set_option("affine", 1)
        if variant == "matrix":
            ctx.set_score_matrix(matrix)
        b = ctx.upload(refs, reads)
        out = {"shape": shape, "variant": variant, "rep": rep, "pairs": len(refs) * len(reads), "gap_open": gap_open}
        if variant in ("profile", "set"):
            profiles = [M.profile_from_matrix(q, matrix, None, scores[1]) for q in reads]
            t_set = []
            for _ in range(steps if variant == "set" else 1):
                t = time.perf_counter()
                b.set_read_profiles(matrix.alphabet, profiles)
                t_set.append((time.perf_counter() - t) * 1e3)
            out["set_ms"] = round(statistics.median(t_set), 4)
            if variant == "set":
                out["entries"] = sum(len(q) for q in reads) * len(matrix.alphabet)
                b.free()
                return out
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
        out.update({"mode": b.pipeline_mode(), "ms_per_run": round(ms, 4), "sweep_ms": round(statistics.median(fill), 4),
                    "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
                    "traceback_ms": round(statistics.median(tb), 4), "cells": int(cells),
                    "gcups_sweep": round(cells / (statistics.median(fill) * 1e-3) / 1e9, 1),
                    "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())})
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="dna,protein,engineerdata")
    args = ap.parse_args()
    ident = M.uniform("ACGT", 5, -3)
    shapes = {}
    refs, reads = synth.config_1k(n_refs=1000, ref_len=2000, read_len=150)
    shapes["dna"] = (refs, reads, -6, (5, -3, -4), ident, ("plain", "matrix", "profile", "set"))
    rng = random.Random(7)
    aa = "ARNDCQEGHILKMFPSTWYV"
    prefs = ["".join(rng.choice(aa) for _ in range(2000)) for _ in range(1000)]
    preads = ["".join(rng.choice(aa) for _ in range(300))]
    shapes["protein"] = (prefs, preads, -11, (1, -1, -1), M.BLOSUM62, ("matrix", "profile", "set"))
    erefs, _ = synth.config_1k(n_refs=100, ref_len=400, read_len=80, seed=7)
    ereads = [synth.config_1k(n_refs=1, ref_len=400, read_len=80, seed=100 + k)[1][0] for k in range(400)]
    shapes["engineerdata"] = (erefs, ereads, -6, (5, -3, -4), ident, ("plain", "matrix", "profile", "set"))
    for name in args.shapes.split(","):
        refs, reads, gap_open, scores, matrix, variants = shapes[name]
        for rep in range(args.reps):
            for variant in variants:
                print(json.dumps(measure(name, variant, rep, refs, reads, gap_open, scores, matrix, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
