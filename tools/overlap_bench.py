#!/usr/bin/env python3
"""Overlap alignment (option "overlap", the overlap sweeps and walks of swmi_affine.hip) next to fit mode and seed extension on the
same build: sweep and traceback times and field bytes, one JSON line per shape, variant and repetition.

  r150      1000 x (150 x 2000)         1000 references, one read
  r80       40,000 x (80 x 400)         200 references x 200 reads
  c4        64 x (10,000 x 10,000)      unbanded

The reads are mutated copies of the TAIL of the references followed by bases of their own, so that the reference's end continues
into the read: the overlap run ends in the last column, the fit run forces the read's tail in and the extend run starts at the
wrong end -- the sweeps cost the same whatever the alignment, the walks differ in length.  Every shape is run as overlap, fit and
extend (--variants), each `reps` times in a context of its own, so that the run-to-run spread of a line is known before two
variants are compared.  Per line: `steps` runs with option "profiling" = 1 after `warmup`; the median, minimum and maximum sweep
time; the traceback's median; the direction field's bytes.  The overlap sweep is fit mode's cell plus extend's list loop over
fewer cells: its time is to be read against those two lines of the same shape, its walk against fit's."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402

VARIANTS = {"overlap": (1, 0, 1), "fit": (1, 0, 0), "extend": (2, 1, 0)}        # (align_mode, extend, overlap)


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


def measure(name, variant, rep, refs, reads, steps, warmup):
    mode, extend, overlap = VARIANTS[variant]
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", -6)
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", mode)
        ctx.set_option("extend", extend)
        ctx.set_option("overlap", overlap)
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
        sc, na = b.pair_results()
        cells = sum(len(r) for r in refs) * sum(len(q) for q in reads)
        med = statistics.median(fill)
        out = {"shape": name, "variant": variant, "rep": rep, "pairs": len(refs) * len(reads), "mode": b.pipeline_mode(),
               "sweep_ms": round(med, 4), "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "traceback_ms_min": round(min(tb), 4), "traceback_ms_max": round(max(tb), 4),
               "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches), "rerun_pairs": int(t.rerun_pairs),
               "gcups_full_matrix": round(cells / (med * 1e-3) / 1e9, 2),
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
    ap.add_argument("--shapes", default="r150,r80,c4")
    ap.add_argument("--variants", default="overlap,fit,extend")
    args = ap.parse_args()
    rng = random.Random(2027)
    for name in args.shapes.split(","):
        if name == "r150":
            base = _rand(rng, 2000)
            refs, reads = [_mutate(rng, base, 2000) for _ in range(1000)], [_mutate(rng, base[1900:] + _rand(rng, 50), 150)]
        elif name == "r80":
            base = _rand(rng, 400)
            refs, reads = [_mutate(rng, base, 400) for _ in range(200)], [_mutate(rng, base[350:] + _rand(rng, 30), 80) for _ in range(200)]
        elif name == "c4":
            base = _rand(rng, 15000)
            refs, reads = [_mutate(rng, base[:10000], 10000) for _ in range(8)], [_mutate(rng, base[5000:], 10000) for _ in range(8)]
        else:
            raise SystemExit("unknown shape %s" % name)
        for rep in range(args.reps):
            for variant in args.variants.split(","):
                print(json.dumps(measure(name, variant, rep, refs, reads, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
