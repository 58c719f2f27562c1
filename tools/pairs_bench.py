#!/usr/bin/env python3
"""Pair lists (swmi_batch_upload_pairs, sw_gather_kernel) against the only way a library without them aligns the same list: one
upload + run per read over strings the caller cut.  One JSON line per shape.

  extend4096    4,096 extend pairs: 512 reads of 150 bases x 8 overlapping windows of 190 columns, cut from one 1 Mbp reference;
                every other read is a left extension (both segments reversed); gap_open = -6
  long64        64 pairs of 10 kbp reads against 10 kbp windows of the same reference: long_reads, global, band 500

Per line, host wall times in ms around calls of the C ABI that end in a stream synchronise, their arguments packed beforehand
(median, minimum and maximum of --steps after --warmup): upload_pairs (the sources H2D + the gather of every segment), run,
set_pairs (the gather alone, the sources stay resident) and set_pairs + run; upload_segments = swmi_batch_upload of the same segment bytes cut on the host (H2D + sw_encode_kernel:
what the gather replaces, timed as one batch whatever its pairs would be).  --baseline prints instead per_read_upload_run: the
whole list as one upload + run per read, which needs nothing of this feature and so runs on a library without it (SWMI_LIB
selects another build; --lib-note labels the lines).  The two modes print a checksum of the scores, which must agree.
--prep-only runs only the uploads: under a kernel trace it shows sw_gather_kernel beside sw_encode_kernel on the same bytes."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sparksmithwaterman_amd as sw            # noqa: E402
from sparksmithwaterman_amd import _capi       # noqa: E402
from sparksmithwaterman_amd.aligner import cut_segments, normalise_pairs      # noqa: E402


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _mutate(rng, s):
    """a copy of s with 3 % substitutions and a few single-base indels"""
    out = []
    for c in s:
        x = rng.random()
        if x < 0.001:
            continue
        if x < 0.002:
            out.append(rng.choice("ACGT"))
        out.append(rng.choice("ACGT") if rng.random() < 0.03 else c)
    return "".join(out)


def shape(name, rng, ref):
    """(options, scores, reads, pairs, pairs of a second list of the same lengths for set_pairs)"""
    if name == "extend4096":
        opts = dict(gap_open=-6, align_mode=2, extend=1)
        reads, pairs, moved = [], [], []
        for q in range(512):
            at = rng.randrange(1000, len(ref) - 1000)
            reads.append(_mutate(rng, ref[at:at + 150])[:150].ljust(150, "A"))
            rev = bool(q & 1)
            for d in range(-3, 5):
                start = at + 150 - 190 + d if rev else at + d       # a left extension's window ends where the read does
                pairs.append((0, q, start, 190, 0, 150, rev))
                moved.append((0, q, start + 1, 190, 0, 150, rev))
        return opts, (5, -3, -2), reads, pairs, moved
    if name == "long64":
        opts = dict(gap_open=-6, align_mode=2, long_reads=1, band=500)
        reads, pairs, moved = [], [], []
        for q in range(64):
            at = rng.randrange(1000, len(ref) - 12000)
            reads.append(_mutate(rng, ref[at:at + 10000])[:10000].ljust(10000, "A"))
            pairs.append((0, q, at, 10000, 0, 10000, False))
            moved.append((0, q, at + 1, 10000, 0, 10000, False))
        return opts, (5, -3, -2), reads, pairs, moved
    raise SystemExit("unknown shape %s" % name)


def timed(fn, steps, warmup):
    ms = []
    for k in range(warmup + steps):
        t0 = time.perf_counter()
        own = fn()                                   # (a function that frees what it made times its call itself)
        if k >= warmup:
            ms.append(own if isinstance(own, float) else (time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _spec_array(specs):
    arr = (_capi.PairSpec * max(len(specs), 1))()
    for k, (r, q, rs, rl, qs, ql, rev) in enumerate(specs):
        arr[k] = _capi.PairSpec(r, q, rs, rl, qs, ql, _capi.SPEC_REVERSE if rev else 0, 0)
    return arr


def measure(name, ref, args):
    """every timed call is a call of the C ABI through ctypes with its arguments packed beforehand: the library, not the packing"""
    rng = random.Random(2026)
    opts, sc, reads, pairs, moved = shape(name, rng, ref)
    specs = normalise_pairs(pairs)
    refs_b, reads_b = [ref.encode()], [r.encode() for r in reads]
    ctx = sw.Context(0)
    lib, C = _capi.load(), ctypes
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        p = sw.make_params(sc)
        n = len(specs)
        out = {"shape": name, "lib": args.lib_note, "pairs": n, "source_bytes": len(ref) + sum(len(r) for r in reads),
               "segment_bytes": sum(s[3] + s[5] for s in specs)}
        segs = [cut_segments(refs_b, reads_b, s) for s in specs]
        scores = (C.c_int32 * n)()
        if args.baseline:
            # the list as a library without pair lists takes it: per read, its windows cut (and reversed) on the host, one batch
            by_read = {}
            for k, s in enumerate(specs):
                by_read.setdefault((s[1], s[6]), []).append(k)
            packed = [(ks, _capi.pack([segs[k][0] for k in ks]), _capi.pack([segs[ks[0]][1]])) for ks in by_read.values()]
            got = [0] * n

            def per_read():
                for ks, (rb, ro), (qb, qo) in packed:
                    h = C.c_void_p()
                    _capi.check(lib.swmi_batch_upload(ctx._h, rb, ro, len(ks), qb, qo, 1, C.byref(h)))
                    _capi.check(lib.swmi_batch_run(ctx._h, h, C.byref(p)))
                    _capi.check(lib.swmi_batch_pair_results(h, scores, None, len(ks)))
                    for x, k in enumerate(ks):
                        got[k] = scores[x]
                    lib.swmi_batch_free(ctx._h, h)
            out["per_read_upload_run_ms"] = timed(per_read, args.steps, args.warmup)
            out["batches"] = len(packed)
            out["score_sum"] = sum(got)
            return out
        (rb, ro), (qb, qo) = _capi.pack(refs_b), _capi.pack(reads_b)
        (sb, so), (tb, to) = _capi.pack([s[0] for s in segs]), _capi.pack([s[1] for s in segs])
        first = _spec_array(specs)
        lists = [_spec_array(normalise_pairs(moved)), first]
        h = C.c_void_p()

        def upload_pairs():
            if h.value:
                lib.swmi_batch_free(ctx._h, h)
            t0 = time.perf_counter()
            _capi.check(lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 1, qb, qo, len(reads), first, n, C.byref(h)))
            return (time.perf_counter() - t0) * 1e3

        def set_pairs():
            _capi.check(lib.swmi_batch_set_pairs(ctx._h, h, lists[0], n))
            lists.reverse()

        def upload_segments():
            x = C.c_void_p()
            t0 = time.perf_counter()
            _capi.check(lib.swmi_batch_upload(ctx._h, sb, so, n, tb, to, n, C.byref(x)))
            ms = (time.perf_counter() - t0) * 1e3
            lib.swmi_batch_free(ctx._h, x)
            return ms

        def run():
            _capi.check(lib.swmi_batch_run(ctx._h, h, C.byref(p)))
        out["upload_pairs_ms"] = timed(upload_pairs, args.steps, args.warmup)
        out["set_pairs_ms"] = timed(set_pairs, args.steps, args.warmup)
        out["upload_segments_ms"] = timed(upload_segments, args.steps, args.warmup)
        if not args.prep_only:
            _capi.check(lib.swmi_batch_set_pairs(ctx._h, h, first, n))          # (the list the baseline aligns)
            out["run_ms"] = timed(run, args.steps, args.warmup)
            _capi.check(lib.swmi_batch_pair_results(h, scores, None, n))
            out["score_sum"] = sum(scores)
            out["set_pairs_run_ms"] = timed(lambda: (set_pairs(), run()), args.steps, args.warmup)
        lib.swmi_batch_free(ctx._h, h)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="extend4096,long64")
    ap.add_argument("--baseline", action="store_true", help="one upload + run per read over host-cut strings (any library)")
    ap.add_argument("--prep-only", action="store_true", help="uploads only (for a kernel trace)")
    ap.add_argument("--lib-note", default="")
    args = ap.parse_args()
    if args.baseline:
        # a library from before this feature lacks its three symbols: bind what it exports (the baseline calls none of them)
        lib = ctypes.CDLL(_capi.LIB_PATH)
        _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(lib, s[0])]
    ref = _rand(random.Random(2025), 1000000)
    for name in args.shapes.split(","):
        print(json.dumps(measure(name, ref, args)), flush=True)


if __name__ == "__main__":
    main()
