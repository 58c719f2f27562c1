#!/usr/bin/env python3
"""Two-piece affine gaps (options "gap_open2" / "gap2", the sw_affine_sweep2_* kernels of swmi_affine.hip) against the one-piece
run on the same build: sweep and traceback times and field bytes, one JSON line per run.

  one_piece    64 x (10,000 x 10,000), global, band 500, scores (2, -4, -2), gap_open -4
  two_piece    the same pairs with gap2 -1, gap_open2 -24

The reads are mutated copies of the references, so the pairs are collinear and the band holds the path.  Per line: `steps` runs
with option "profiling" = 1 after `warmup`; the median, minimum and maximum sweep time; the traceback's median, minimum and
maximum; the direction field's bytes; the score sum.  The two-piece line also carries the ratios of its medians to the one-piece
line's.  On a library without the option only the one-piece line is printed (SWMI_LIB selects another build; --lib-note labels
the lines)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import _capi       # noqa: E402

SCORES = (2, -4, -2, -4, -1, -24)
BAND = 500


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


def measure(name, refs, reads, two, steps, warmup, note):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", SCORES[3])
        if two:
            ctx.set_option("gap2", SCORES[4])
            ctx.set_option("gap_open2", SCORES[5])
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", sw.ALIGN_GLOBAL)
        ctx.set_option("band", BAND)
        ctx.set_option("profiling", 1)
        b = ctx.upload(refs, reads)
        p = sw.make_params(SCORES[:3])
        for _ in range(warmup):
            b.run(p)
        fill, tb = [], []
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
        t = b.timing()
        sc, na = b.pair_results()
        out = {"run": name, "lib": note, "pairs": len(refs) * len(reads), "band": BAND, "mode": b.pipeline_mode(), "steps": steps,
               "sweep_ms": round(statistics.median(fill), 4), "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "traceback_ms_min": round(min(tb), 4), "traceback_ms_max": round(max(tb), 4),
               "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches),
               "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib-note", default="")
    args = ap.parse_args()
    rng = random.Random(2026)
    base = _rand(rng, 10000)
    # 8 x 8 = 64 pairs, every read and every reference a mutated copy of one sequence: all 64 pairs are collinear
    refs = [_mutate(rng, base, 10000) for _ in range(8)]
    reads = [_mutate(rng, base, 10000) for _ in range(8)]
    kw = dict(steps=args.steps, warmup=args.warmup, note=args.lib_note)
    one = measure("one_piece", refs, reads, False, **kw)
    print(json.dumps(one), flush=True)
    try:
        two = measure("two_piece", refs, reads, True, **kw)
    except _capi.SwmiError as e:
        if "unknown option" not in str(e):
            raise
        return                                  # (a library without the option: the one-piece line is the yardstick)
    two["sweep_ratio"] = round(two["sweep_ms"] / one["sweep_ms"], 3)
    two["traceback_ratio"] = round(two["traceback_ms"] / one["traceback_ms"], 3)
    print(json.dumps(two), flush=True)


if __name__ == "__main__":
    main()
