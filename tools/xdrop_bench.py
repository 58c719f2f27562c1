#!/usr/bin/env python3
"""The drop-off rule of seed extension (option "xdrop", the xdrop sweeps of swmi_affine.hip) next to the plain extend run on the
same build: sweep and traceback times and the strips swept, one JSON line per shape, read kind, variant and repetition.

  c4_w0       64 x (10,000 x 10,000)     unbanded, 10 strips
  c4_w512     the same pairs at band 512
  b4096_w256  1000 x (4096 x 4300) at band 256, 4 strips

Two kinds of reads per shape: `collinear` reads are mutated copies of the head of the references, so nothing ever drops;
`diverging` reads are such a copy for their first 2,000 bases and unrelated after that.  Scores are (2, -4, -2, -4): under them
unrelated DNA loses score row after row (under 5 / -3 it keeps gaining in global mode, and nothing would drop).  Every (shape,
kind) is run with xdrop = 0 -- the parent's kernels -- and with xdrop = --xdrop (default 400: above what 48 unrelated rows lose up
to row 2048, below what 1,072 lose up to row 3072, so a diverging read is swept for three strips), the variants alternating
within one invocation, each `reps` times in a context of its own, so that the run-to-run spread of a line is known before two
variants are compared.  Per line: `steps` runs with option "profiling" = 1 after `warmup`; the median, minimum and maximum
sweep time; the traceback's median; the strips swept over the strips there are, from swmi_pair_rows_swept.  The sweep time of the
diverging reads is to be read against that ratio, the one of the collinear reads against the xdrop = 0 line of the same shape."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402

SCORES = (2, -4, -2, -4)


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


def measure(name, kind, xdrop, rep, refs, reads, w, steps, warmup):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", SCORES[3])
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", sw.ALIGN_GLOBAL)
        ctx.set_option("extend", 1)
        ctx.set_option("xdrop", xdrop)
        ctx.set_option("band", w)
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
        strips = lambda rows: (rows + 1023) // 1024
        swept = sum(strips(b.rows_swept(r * len(reads) + q)) for r in range(len(refs)) for q in range(len(reads)))
        total = len(refs) * sum(strips(len(q)) for q in reads)
        stopped = sum(b.rows_swept(r * len(reads) + q) < len(reads[q]) for r in range(len(refs)) for q in range(len(reads)))
        med = statistics.median(fill)
        out = {"shape": name, "kind": kind, "xdrop": xdrop, "rep": rep, "pairs": len(refs) * len(reads), "band": w,
               "mode": b.pipeline_mode(), "sweep_ms": round(med, 4), "sweep_ms_min": round(min(fill), 4),
               "sweep_ms_max": round(max(fill), 4), "traceback_ms": round(statistics.median(tb), 4),
               "strips_swept": swept, "strips": total, "strips_ratio": round(swept / total, 4), "pairs_stopped": stopped,
               "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches), "nominal_cells": int(t.cells),
               "score_sum": int(sc.astype("int64").sum()), "alignments": int(na.sum())}
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shapes", default="c4_w0,c4_w512,b4096_w256")
    ap.add_argument("--kinds", default="collinear,diverging")
    ap.add_argument("--xdrop", type=int, default=400)
    ap.add_argument("--common", type=int, default=2000, help="the bases a diverging read shares with the references")
    args = ap.parse_args()
    rng = random.Random(2027)
    c4 = None
    for name in args.shapes.split(","):
        w = int(name.rsplit("_w", 1)[1])
        if name.startswith("c4_w"):
            if c4 is None:                                        # (the same 64 pairs for every band)
                base = _rand(rng, 10000)
                c4 = ([_mutate(rng, base, 10000) for _ in range(8)],
                      {"collinear": [_mutate(rng, base, 10000) for _ in range(8)],
                       "diverging": [_mutate(rng, base[:args.common], args.common) + _rand(rng, 10000 - args.common) for _ in range(8)]})
            refs, reads = c4
        elif name.startswith("b4096_w"):
            base = _rand(rng, 4300)
            refs = [_mutate(rng, base, 4300) for _ in range(1000)]
            reads = {"collinear": [_mutate(rng, base[:4096], 4096)],
                     "diverging": [_mutate(rng, base[:args.common], args.common) + _rand(rng, 4096 - args.common)]}
        else:
            raise SystemExit("unknown shape %s" % name)
        for kind in args.kinds.split(","):
            for rep in range(args.reps):
                for xdrop in (0, args.xdrop):
                    print(json.dumps(measure(name, kind, xdrop, rep, refs, reads[kind], w, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
