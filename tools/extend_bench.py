#!/usr/bin/env python3
"""Seed extension (option "extend", the extend sweeps of swmi_affine.hip) next to global and local mode on the same build: sweep
and traceback times and field bytes, one JSON line per shape, variant and repetition.

  r150      1000 x (150 x 2000)         1000 references, one read
  r80       40,000 x (80 x 400)         200 references x 200 reads
  c4_w0     64 x (10,000 x 10,000)      unbanded
  c4_w512   the same pairs at band 512
  b4096_w256  1000 x (4096 x 4300) at band 256

The reads are mutated copies of the head of the references, so an extension anchored at the start runs through the read.  Every
shape is run as extend, global and local (--variants), each `reps` times in a context of its own, so that the run-to-run spread of
a line is known before two variants are compared.  Per line: `steps` runs with option "profiling" = 1 after `warmup`; the median,
minimum and maximum sweep time; the traceback's median; the direction field's bytes.  The extend sweep is global mode's cell
plus local mode's maximum tracking: its time is to be read against those two lines of the same shape."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402

VARIANTS = {"extend": (2, 1), "global": (2, 0), "local": (0, 0)}        # (align_mode, extend)


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


def measure(name, variant, rep, refs, reads, w, steps, warmup):
    mode, extend = VARIANTS[variant]
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", -6)
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", mode)
        ctx.set_option("extend", extend)
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
        sc, na = b.pair_results()
        cells = sum(len(r) for r in refs) * sum(len(q) for q in reads)
        med = statistics.median(fill)
        out = {"shape": name, "variant": variant, "rep": rep, "pairs": len(refs) * len(reads), "band": w, "mode": b.pipeline_mode(),
               "sweep_ms": round(med, 4), "sweep_ms_min": round(min(fill), 4), "sweep_ms_max": round(max(fill), 4),
               "traceback_ms": round(statistics.median(tb), 4), "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches),
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
    ap.add_argument("--shapes", default="r150,r80,c4_w0,c4_w512,b4096_w256")
    ap.add_argument("--variants", default="extend,global,local")
    args = ap.parse_args()
    rng = random.Random(2026)
    c4 = None
    for name in args.shapes.split(","):
        w = int(name.rsplit("_w", 1)[1]) if "_w" in name else 0
        if name == "r150":
            base = _rand(rng, 2000)
            refs, reads = [_mutate(rng, base, 2000) for _ in range(1000)], [_mutate(rng, base[:150], 150)]
        elif name == "r80":
            base = _rand(rng, 400)
            refs, reads = [_mutate(rng, base, 400) for _ in range(200)], [_mutate(rng, base[:80], 80) for _ in range(200)]
        elif name.startswith("c4_w"):
            if c4 is None:                                        # (the same 64 pairs for every band)
                base = _rand(rng, 10000)
                c4 = [_mutate(rng, base, 10000) for _ in range(8)], [_mutate(rng, base, 10000) for _ in range(8)]
            refs, reads = c4
        elif name.startswith("b4096_w"):
            base = _rand(rng, 4300)
            refs, reads = [_mutate(rng, base, 4300) for _ in range(1000)], [_mutate(rng, base[:4096], 4096)]
        else:
            raise SystemExit("unknown shape %s" % name)
        for rep in range(args.reps):
            for variant in args.variants.split(","):
                print(json.dumps(measure(name, variant, rep, refs, reads, w, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
