#!/usr/bin/env python3
"""Banded alignment of long reads (option "band", the banded strip sweeps of swmi_affine.hip): sweep and traceback times, field
bytes and the rate per computed cell, one JSON line per shape.

  c4_global_w0 / _w128 / _w512 / _w2048    64 x (10,000 x 10,000), global, gap_open = -6; w0 is the unbanded run
  c4_local_w0 / ...                        the same pairs, local
  fit4096_w256                             1000 x (4096 x 4300), fit

The reads are mutated copies of the references, so the pairs are collinear and the banded results are the unbanded ones for a
band that holds the path.  Per line: `steps` runs with option "profiling" = 1 after `warmup`; the median, minimum and maximum
sweep time; the traceback's median; the direction field's bytes; the computed steps per pair (strips x (window + 63)) and cells
(1024 rows x window per strip) and the rate over them.  A w0 line runs on a library without the option as well (SWMI_LIB selects
another build; --lib-note labels the lines)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, n):
    """a copy of s with 3 % substitutions and a few single-base indels, cut or padded to n bases"""
    out = []
    for c in s:
        x = rng.random()
        if x < 0.001:
            continue
        if x < 0.002:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if rng.random() < 0.03 else c)
    out = "".join(out)[:n]
    return out + _rand(rng, n - len(out))


def _windows(m, n, w):
    if not w:
        return [n] * ((m + 1023) // 1024)
    return [min(n, 1024 * (s + 1) + w) - max(1, 1024 * s + 1 - w) + 1 for s in range((m + 1023) // 1024)]


def measure(name, refs, reads, mode, w, steps, warmup, note):
    """the batch is refs x reads: pass one read per run for pair lists, or equal-length sets for a cross product"""
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", -6)
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", mode)
        if w:
            ctx.set_option("band", w)
        ctx.set_option("profiling", 1)
        b = ctx.upload(refs, reads)
        p = sw.make_params((5, -3, -2))
        for _ in range(warmup):
            b.run(p)
        fill, tb = [], []
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
        t = b.timing()
        steps_pair = cells = 0
        for ref in refs:
            for read in reads:
                win = _windows(len(read), len(ref), w)
                steps_pair = max(steps_pair, sum(x + 63 for x in win))
                cells += sum(1024 * x for x in win)
        sc, na = b.pair_results()
        med = statistics.median(fill)
        out = {"shape": name, "lib": note, "pairs": len(refs) * len(reads), "align_mode": mode, "band": w, "mode": b.pipeline_mode(),
               "sweep_ms": round(med, 4), "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches),
               "steps_per_pair": int(steps_pair), "computed_cells": int(cells), "gcups_computed": round(cells / (med * 1e-3) / 1e9, 2),
               "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="c4_global_w0,c4_global_w128,c4_global_w512,c4_global_w2048,"
                                        "c4_local_w0,c4_local_w128,c4_local_w512,c4_local_w2048,fit4096_w256")
    ap.add_argument("--lib-note", default="")
    args = ap.parse_args()
    rng = random.Random(2025)
    base = _rand(rng, 10000)
    # 8 x 8 = 64 pairs, every read and every reference a mutated copy of one sequence: all 64 pairs are collinear
    c4_refs = [_mutate(rng, base, 10000) for _ in range(8)]
    c4_reads = [_mutate(rng, base, 10000) for _ in range(8)]
    fit_base = _rand(rng, 4300)
    fit_refs = None
    for name in args.shapes.split(","):
        kind, wtag = name.rsplit("_w", 1)
        w = int(wtag)
        kw = dict(steps=args.steps, warmup=args.warmup, note=args.lib_note)
        if kind in ("c4_global", "c4_local"):
            out = measure(name, c4_refs, c4_reads, 2 if kind == "c4_global" else 0, w, **kw)
        elif kind == "fit4096":
            if fit_refs is None:
                fit_refs = [_mutate(rng, fit_base, 4300) for _ in range(1000)]
            out = measure(name, fit_refs, [_mutate(rng, fit_base[100:4196], 4096)], 1, w, **kw)
        else:
            raise SystemExit("unknown shape %s" % name)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
