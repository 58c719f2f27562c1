#!/usr/bin/env python3
"""Option "end_bonus" (the ENDB sweeps of swmi_affine.hip) next to the same extend run without it: sweep time and traceback time,
one JSON line per run.

  shapes     short      4,096 x (150 x 400) = 64 references x 64 reads, extend, scores (5, -4, -3), gap_open -5
             long       64 x (10,000 x 10,000) = 8 x 8 mutated copies of one sequence, extend, long_reads, scores (2, -4, -2), gap_open -4
             long_band  the same under band 500
  end_bonus  0 (off), 1 (the smallest bonus: it takes only the pairs whose best cell lies in row m anyway) and 2^30 (every pair)

Per line: `steps` runs with option "profiling" = 1 after `warmup`; [median, minimum, maximum] of the sweep time -- the device events
bracket the sweep kernels -- and of the traceback time (a pair taken to the end has ONE alignment, so the traceback of the 2^30 line
walks other and possibly fewer cells than the line without the option); launches; the sum of the scores as a check, and under the
option the number of pairs taken and the sums of max_score and end_score.  The end_bonus lines carry the ratio of their sweep median
to the end_bonus = 0 line's.  On a library without the option the end_bonus lines are left out (SWMI_LIB selects another build;
--lib-note labels the lines): alternate rounds of this tool on the parent commit's library and on this one give the yardstick, the
parent's extend sweep of the same shape, and its spread between rounds (profiles/r17/end_bonus.md)."""
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
    """binds what the library at SWMI_LIB exports: a build from before the option lacks swmi_pair_end_score, and is measured all the same"""
    lib = C.CDLL(_capi.LIB_PATH)
    _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(lib, s[0])]
    return any(s[0] == "swmi_pair_end_score" for s in _capi.SYMBOLS)


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
    rng = random.Random(2029)
    base = _rand(rng, 10000)
    # every read ends in a random tail (100 and 20 bases): where the read matches its reference the best cell lies before the tail and
    # row m well below, so the smallest bonus leaves those pairs alone.  No bonus >= 1 leaves EVERY pair alone -- among random pairs
    # some have their best cell in row m -- so the lines report how many pairs were taken
    lrefs, lreads = [_mutate(rng, base, 10000) for _ in range(8)], [_mutate(rng, base, 9900) + _rand(rng, 100) for _ in range(8)]
    ext = dict(align_mode=sw.ALIGN_GLOBAL, extend=1)
    long_ = dict(refs=lrefs, reads=lreads, scores=(2, -4, -2, -4), options=dict(ext, long_reads=1))
    band = dict(refs=lrefs, reads=lreads, scores=(2, -4, -2, -4), options=dict(ext, long_reads=1, band=500))
    # an extend run is anchored at both starts: every read is a mutated copy of the start of its own reference, and meets the other
    # 63 references as random sequence
    refs = [_rand(rng, 400) for _ in range(64)]
    reads = [_mutate(rng, refs[k][:130], 130) + _rand(rng, 20) for k in range(64)]
    short = dict(refs=refs, reads=reads, scores=(5, -4, -3, -5), options=dict(ext))
    return {"short": short, "long": long_, "long_band": band}


def _spread(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def measure(shape, case, bonus, steps, warmup, note):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", case["scores"][3])
        for name, v in case["options"].items():
            ctx.set_option(name, v)
        if bonus:
            ctx.set_option("end_bonus", bonus)
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
        n_pairs = len(case["refs"]) * len(case["reads"])
        out = {"shape": shape, "end_bonus": bonus, "lib": note, "pairs": n_pairs, "mode": b.pipeline_mode(),
               "steps": steps, "sweep_ms": _spread(fill), "traceback_ms": _spread(tb), "launches": int(t.fill_launches),
               "rerun_pairs": int(t.rerun_pairs), "score_sum": int(b.scores().astype("int64").sum())}
        if bonus:
            ms, es, _ = b.end_scores()
            out["max_score_sum"] = int(ms.astype("int64").sum())
            out["end_score_sum"] = int(es.astype("int64").sum())
            out["pairs_taken"] = sum(1 for k in range(n_pairs) if b.n_alignments(k)[1] & sw.PAIR_TO_END)
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
    ap.add_argument("--end-bonus", default="0,1,%d" % (1 << 30), help="the values to run, 0 first (the ratio's base)")
    args = ap.parse_args()
    has_option = _load_any_build()
    cases = shapes()
    for shape in args.shapes.split(","):
        off = None
        for bonus in [int(v) for v in args.end_bonus.split(",")]:
            if bonus and not has_option:
                continue
            out = measure(shape, cases[shape], bonus, args.steps, args.warmup, args.lib_note)
            if not bonus:
                off = out
            elif off:
                out["sweep_ratio_to_off"] = round(out["sweep_ms"][0] / off["sweep_ms"][0], 4)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
