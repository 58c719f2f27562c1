#!/usr/bin/env python3
"""The adaptive band of seed extension (option "band_adapt", the band_adapt kernels of swmi_affine.hip) next to the static band of
the same build (band_adapt = 0): sweep and traceback times, one JSON line per shape, variant and repetition.

  collinear   64 x (10,000 x 10,000), reads and references mutated copies of one sequence, band 512: adaptive against static.
              The windows have the same sizes, so the difference is the cost of the seam pass and the window table.
  drift       64 x (10,000 x 10,700): every reference holds 40 extra bases per 1,000 bases of the reads' common ancestor.  First
              the unbanded extend run gives the scores to reach; then the static band is run at half-widths 64, 128, ... until
              its scores equal them (the smallest such power of two is reported as `static_w`); then that static band and the
              adaptive band at --adapt-band (default 64) are measured, alternating.

Scores are (5, -3, -2, -6).  Each variant is run `reps` times in a context of its own, the variants alternating within one
invocation, so that the run-to-run spread of a line is known before two variants are compared.  Per line: `steps` runs with
option "profiling" = 1 after `warmup`; the median, minimum and maximum sweep time; the traceback's median; the field bytes; the
sum of the scores and whether it equals the unbanded run's; the sweep's dependent chain in steps per strip, 1087 + 2 w."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402

SCORES = (5, -3, -2, -6)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, n=None):
    """a copy of s with 3 % substitutions and a few single-base indels (cut or padded to n bases when n is given)"""
    out = []
    for c in s:
        x = rng.random()
        if x < 0.001:
            continue
        if x < 0.002:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if rng.random() < 0.03 else c)
    out = "".join(out)
    if n is None:
        return out
    out = out[:n]
    return out + _rand(rng, n - len(out))


def _with_extra(rng, s, every=1000, first=500, extra=40):
    """s with `extra` random bases inserted after bases first, first + every, ..."""
    out, at = [], 0
    for cut in list(range(first, len(s), every)) + [len(s)]:
        out.append(s[at:cut])
        if cut < len(s):
            out.append(_rand(rng, extra))
        at = cut
    return "".join(out)


def measure(shape, variant, w, adapt, rep, refs, reads, steps, warmup, want=None):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", SCORES[3])
        ctx.set_option("long_reads", 1)
        ctx.set_option("align_mode", sw.ALIGN_GLOBAL)
        ctx.set_option("extend", 1)
        ctx.set_option("band", w)
        ctx.set_option("band_adapt", adapt)
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
        scores = [int(x) for x in sc]
        out = {"shape": shape, "variant": variant, "band": w, "band_adapt": adapt, "rep": rep, "pairs": len(refs) * len(reads),
               "mode": b.pipeline_mode(), "sweep_ms": round(statistics.median(fill), 4), "sweep_ms_min": round(min(fill), 4),
               "sweep_ms_max": round(max(fill), 4), "traceback_ms": round(statistics.median(tb), 4),
               "steps_per_strip": 1087 + 2 * w if w else None, "field_bytes": int(t.dir_bytes), "launches": int(t.fill_launches),
               "score_sum": sum(scores), "alignments": int(na.sum())}
        if want is not None:
            out["equals_unbanded"] = scores == want
        if adapt:
            last = (len(reads[0]) - 1) // 1024
            out["last_window_of_pair_0"] = list(b.band_window(0, last))
        b.free()
        return out, scores
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="collinear,drift")
    ap.add_argument("--adapt-band", type=int, default=64)
    ap.add_argument("--length", type=int, default=10000, help="bases per read")
    args = ap.parse_args()
    rng = random.Random(2028)
    m = args.length
    base = _rand(rng, m)
    for shape in args.shapes.split(","):
        if shape == "collinear":
            refs = [_mutate(rng, base, m) for _ in range(8)]
            reads = [_mutate(rng, base, m) for _ in range(8)]
            for rep in range(args.reps):
                for adapt in (0, 1):
                    out, _ = measure(shape, "adaptive" if adapt else "static", 512, adapt, rep, refs, reads, args.steps, args.warmup)
                    print(json.dumps(out), flush=True)
        elif shape == "drift":
            refs = [_mutate(rng, _with_extra(rng, base)) + _rand(rng, 300) for _ in range(8)]
            reads = [_mutate(rng, base, m) for _ in range(8)]
            out, want = measure(shape, "unbanded", 0, 0, 0, refs, reads, 1, 0)
            print(json.dumps(out), flush=True)
            static_w = None
            for w in (64, 128, 256, 512, 1024, 2048):
                out, scores = measure(shape, "static_search", w, 0, 0, refs, reads, 1, 0, want)
                print(json.dumps(out), flush=True)
                if scores == want:
                    static_w = w
                    break
            if static_w is None:
                raise SystemExit("no static band up to 2048 reaches the unbanded scores")
            for rep in range(args.reps):
                for variant, w, adapt in (("static", static_w, 0), ("adaptive", args.adapt_band, 1)):
                    out, _ = measure(shape, variant, w, adapt, rep, refs, reads, args.steps, args.warmup, want)
                    out["static_w"] = static_w
                    print(json.dumps(out), flush=True)
        else:
            raise SystemExit("unknown shape %s" % shape)


if __name__ == "__main__":
    main()
