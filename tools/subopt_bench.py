#!/usr/bin/env python3
"""Option "subopt" (the SUBOPT sweeps of swmi_affine.hip, sw_subopt_kernel of swmi_subopt.hip) next to the same local run without it:
sweep time, traceback time and workspace, one JSON line per run.

  shapes     short      4,096 x (150 x 400) = 64 references x 64 reads, local, scores (5, -4, -3), gap_open -5
             long       64 x (10,000 x 10,000) = 8 x 8 mutated copies of one sequence, local, long_reads, scores (2, -4, -2), gap_open -4
             long_band  the same under band 500
  subopt     0 and SWMI_SUBOPT_AUTO (-1)

Per line: `steps` runs with option "profiling" = 1 after `warmup`; [median, minimum, maximum] of the sweep time -- the device events
bracket the sweep kernels AND, under subopt, the reduce kernel that follows them on the stream -- and of the traceback time;
workspace_bytes = the direction-field workspace of the run's launches (swmi_timing.dir_bytes: under subopt it includes the rows of
column maxima), launches, and the sums of score and score2 as a check.  The subopt lines carry the ratio of their sweep median to
the subopt = 0 line's and the added workspace.  The reduce kernel alone is not bracketed by an event of its own: its time is read
from a kernel trace of this tool (profiles/r16/subopt.md).  On a library without the option the subopt lines are left out
(SWMI_LIB selects another build; --lib-note labels the lines)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import _capi       # noqa: E402


def _load_any_build():
    """binds what the library at SWMI_LIB exports: a build from before the option lacks swmi_pair_subopt, and is measured all the same"""
    lib = C.CDLL(_capi.LIB_PATH)
    _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(lib, s[0])]
    return any(s[0] == "swmi_pair_subopt" for s in _capi.SYMBOLS)


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


def shapes():
    rng = random.Random(2028)
    base = _rand(rng, 10000)
    lrefs, lreads = [_mutate(rng, base, 10000) for _ in range(8)], [_mutate(rng, base, 10000) for _ in range(8)]
    long_ = dict(refs=lrefs, reads=lreads, scores=(2, -4, -2, -4), options=dict(long_reads=1))
    band = dict(refs=lrefs, reads=lreads, scores=(2, -4, -2, -4), options=dict(long_reads=1, band=500))
    refs = [_rand(rng, 400) for _ in range(64)]
    reads = [_mutate(rng, refs[k][rng.randrange(0, 250):][:150], 150) for k in range(64)]
    short = dict(refs=refs, reads=reads, scores=(5, -4, -3, -5), options={})
    return {"short": short, "long": long_, "long_band": band}


def _spread(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def measure(shape, case, subopt, steps, warmup, note):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", case["scores"][3])
        for name, v in case["options"].items():
            ctx.set_option(name, v)
        if subopt:
            ctx.set_option("subopt", subopt)
        ctx.set_option("profiling", 1)
        b = ctx.upload(case["refs"], case["reads"])
        p = sw.make_params(case["scores"][:3])
        for _ in range(warmup):
            b.run(p)
        fill, tb = [], []
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
        t = b.timing()
        out = {"shape": shape, "subopt": subopt, "lib": note, "pairs": len(case["refs"]) * len(case["reads"]), "mode": b.pipeline_mode(),
               "steps": steps, "sweep_ms": _spread(fill), "traceback_ms": _spread(tb), "workspace_bytes": int(t.dir_bytes),
               "launches": int(t.fill_launches), "score_sum": int(b.scores().astype("int64").sum())}
        if subopt:
            s2, e2 = b.subopts()
            out["score2_sum"] = int(s2.astype("int64").sum())
            out["pairs_with_score2"] = int((s2 > 0).sum())
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib-note", default="")
    ap.add_argument("--shapes", default="short,long_band,long")
    ap.add_argument("--subopt", default="0,-1", help="the values to run, 0 first (the ratio's base)")
    args = ap.parse_args()
    has_subopt = _load_any_build()
    cases = shapes()
    for shape in args.shapes.split(","):
        off = None
        for subopt in [int(v) for v in args.subopt.split(",")]:
            if subopt and not has_subopt:
                continue
            out = measure(shape, cases[shape], subopt, args.steps, args.warmup, args.lib_note)
            if not subopt:
                off = out
            elif off:
                out["sweep_ratio_to_off"] = round(out["sweep_ms"][0] / off["sweep_ms"][0], 4)
                out["workspace_added_bytes"] = out["workspace_bytes"] - off["workspace_bytes"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
