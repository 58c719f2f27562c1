#!/usr/bin/env python3
"""Option "hits" (the HITS sweeps of swmi_affine.hip, sw_hits_kernel of swmi_subopt.hip) next to the same local run under option "subopt"
alone, and next to the run without either: sweep time, traceback time and workspace, one JSON line per run.

  shapes     those of tools/subopt_bench.py: short 4,096 x (150 x 400), long 64 x (10,000 x 10,000), long_band the same under band 500
  runs       (subopt, hits) = (0, 0), (AUTO, 0), (AUTO, 2), (AUTO, 16)

Per line: `steps` runs with option "profiling" = 1 after `warmup`; [median, minimum, maximum] of the sweep time -- the device events
bracket the sweep kernels AND the reduce or pick kernel that follows them on the stream -- and of the traceback time;
workspace_bytes = the direction-field workspace of the run's launches (swmi_timing.dir_bytes: it includes the rows of column maxima
and, under hits, of their rows), launches, and the sums of score, score2 and of the hits' scores and counts as a check.  The hits
lines carry the ratio of their sweep median to the (AUTO, 0) line's of the same process and the added workspace.  The pick kernel
alone is not bracketed by an event of its own: its time is read from a kernel trace of this tool (profiles/r18/hits.md).  On a
library without the option the hits lines are left out (SWMI_LIB selects another build; --lib-note labels the lines): the parent
commit's (AUTO, 0) line is the yardstick."""
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
    """binds what the library at SWMI_LIB exports: a build from before the option lacks swmi_pair_hits, and is measured all the same"""
    lib = C.CDLL(_capi.LIB_PATH)
    _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(lib, s[0])]
    return any(s[0] == "swmi_pair_hits" for s in _capi.SYMBOLS)


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


def measure(shape, case, subopt, hits, steps, warmup, note):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", case["scores"][3])
        for name, v in case["options"].items():
            ctx.set_option(name, v)
        if subopt:
            ctx.set_option("subopt", subopt)
        if hits:
            ctx.set_option("hits", hits)
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
        out = {"shape": shape, "subopt": subopt, "hits": hits, "lib": note, "pairs": len(case["refs"]) * len(case["reads"]), "mode": b.pipeline_mode(),
               "steps": steps, "sweep_ms": _spread(fill), "traceback_ms": _spread(tb), "workspace_bytes": int(t.dir_bytes),
               "launches": int(t.fill_launches), "score_sum": int(b.scores().astype("int64").sum())}
        if subopt:
            s2, e2 = b.subopts()
            out["score2_sum"] = int(s2.astype("int64").sum())
            out["pairs_with_score2"] = int((s2 > 0).sum())
        if hits:
            cnt, sc, _, _ = b.hits_all()
            out["hits_sum"] = int(cnt.astype("int64").sum())
            out["hit_score_sum"] = int(sc.astype("int64").sum())
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
    ap.add_argument("--runs", default="0:0,-1:0,-1:2,-1:16", help="subopt:hits of the runs, in order; the ratio's base is the last run with hits = 0")
    args = ap.parse_args()
    has_hits = _load_any_build()
    cases = shapes()
    for shape in args.shapes.split(","):
        base = None
        for subopt, hits in [tuple(int(x) for x in v.split(":")) for v in args.runs.split(",")]:
            if hits and not has_hits:
                continue
            out = measure(shape, cases[shape], subopt, hits, args.steps, args.warmup, args.lib_note)
            if not hits:
                base = out
            elif base:
                out["sweep_ratio_to_hits_0"] = round(out["sweep_ms"][0] / base["sweep_ms"][0], 4)
                out["workspace_added_bytes"] = out["workspace_bytes"] - base["workspace_bytes"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
