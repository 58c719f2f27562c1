#!/usr/bin/env python3
"""The minus strand (SWMI_SPEC_READ_REVCOMP): what the gather costs when it also reverse-complements the reads, and
whether the forward path -- a list of plus pairs only -- moved against a library from before the flag.  One JSON line per shape
and strand.

  short4096     4,096 pairs: 512 reads of 150 bases x 8 overlapping windows of 190 columns, cut from one 1 Mbp reference; extend,
                gap_open = -6.  8,192 short segments per list, 4,096 of them read segments.
  long64        64 pairs of 10 kbp reads against 10 kbp windows of the same reference: long_reads, global, band 500

--strand plus: the reads are uploaded as they lie on the reference and every pair is (.., False): no segment is transformed,
nothing is copied.  --strand minus: the SAME reads uploaded reverse-complemented and every pair carries "-": the kernel turns
them back, so the two lists align the same bases and their score checksums must agree.  A plus list sets no new flag bit and
calls no new symbol: with SWMI_LIB it runs on the parent commit's library through this binding (--lib-note labels the lines).

Per line, host wall times in ms around calls of the C ABI that end in a stream synchronise, their arguments packed beforehand
(median, minimum and maximum of --steps after --warmup): set_pairs (validation, layout, four small H2D copies, one memset and
the two gather launches; the sources stay resident -- the call the gather dominates), upload_pairs (the sources H2D as well)
and run.  --prep-only runs set_pairs alone: under `rocprofv3 --kernel-trace` every sw_gather_kernel launch of the process is
then one strand of one shape, the reference side and the read side alternating.  --trace DIR reads such a trace back and prints
the launches' durations in microseconds (no GPU needed)."""
import argparse
import csv
import ctypes
import glob
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

COMP = bytes.maketrans(b"ACGT", b"TGCA")       # (stated here: a plus run must not need this build's package additions)


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
    """(options, scores, reads as they lie on the reference, pairs as (ref, read, ref_start, ref_len, read_start, read_len),
    a second list of the same lengths for set_pairs to alternate with)"""
    if name == "short4096":
        opts = dict(gap_open=-6, align_mode=2, extend=1)
        reads, pairs, moved = [], [], []
        for q in range(512):
            at = rng.randrange(1000, len(ref) - 1000)
            reads.append(_mutate(rng, ref[at:at + 150])[:150].ljust(150, "A"))
            for d in range(-3, 5):
                pairs.append((0, q, at + d, 190, 0, 150))
                moved.append((0, q, at + d + 1, 190, 0, 150))
        return opts, (5, -3, -2), reads, pairs, moved
    if name == "long64":
        opts = dict(gap_open=-6, align_mode=2, long_reads=1, band=500)
        reads, pairs, moved = [], [], []
        for q in range(64):
            at = rng.randrange(1000, len(ref) - 12000)
            reads.append(_mutate(rng, ref[at:at + 10000])[:10000].ljust(10000, "A"))
            pairs.append((0, q, at, 10000, 0, 10000))
            moved.append((0, q, at + 1, 10000, 0, 10000))
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


def _spec_array(pairs, flags):
    arr = (_capi.PairSpec * max(len(pairs), 1))()
    for k, (r, q, rs, rl, qs, ql) in enumerate(pairs):
        arr[k] = _capi.PairSpec(r, q, rs, rl, qs, ql, flags, 0)
    return arr


def measure(name, strand, ref, args):
    """every timed call is a call of the C ABI through ctypes with its arguments packed beforehand: the library, not the packing"""
    rng = random.Random(2026)
    opts, sc, reads, pairs, moved = shape(name, rng, ref)
    minus = strand == "minus"
    flags = 4 if minus else 0                        # SWMI_SPEC_READ_REVCOMP
    reads_b = [r.encode().translate(COMP)[::-1] if minus else r.encode() for r in reads]
    ctx = sw.Context(0)
    lib, C = _capi.load(), ctypes
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        p = sw.make_params(sc)
        n = len(pairs)
        out = {"shape": name, "strand": strand, "lib": args.lib_note, "pairs": n, "source_bytes": len(ref) + sum(len(r) for r in reads),
               "transformed_bytes": sum(s[5] for s in pairs) if minus else 0}
        (rb, ro), (qb, qo) = _capi.pack([ref.encode()]), _capi.pack(reads_b)
        first = _spec_array(pairs, flags)
        lists = [_spec_array(moved, flags), first]
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

        def run():
            _capi.check(lib.swmi_batch_run(ctx._h, h, C.byref(p)))
        if args.prep_only:
            upload_pairs()
        else:
            out["upload_pairs_ms"] = timed(upload_pairs, args.steps, args.warmup)
        out["set_pairs_ms"] = timed(set_pairs, args.steps, args.warmup)
        if not args.prep_only:
            _capi.check(lib.swmi_batch_set_pairs(ctx._h, h, first, n))
            out["run_ms"] = timed(run, args.run_steps, args.warmup)
            scores = (C.c_int32 * n)()
            _capi.check(lib.swmi_batch_pair_results(h, scores, None, n))
            out["score_sum"] = sum(scores)
        lib.swmi_batch_free(ctx._h, h)
        return out
    finally:
        ctx.close()


def read_trace(path):
    """the sw_gather_kernel launches of a `rocprofv3 --kernel-trace --output-format csv` directory, in start order: the even ones
    are the reference side of a list, the odd ones its read side"""
    rows = []
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                if row.get("Kernel_Name", "").startswith("sw_gather_kernel"):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    us = [(e - s) / 1e3 for s, e in rows]
    out = {"trace": path, "launches": len(us)}
    for side, part in (("ref_side_us", us[0::2]), ("read_side_us", us[1::2]), ("both_sides_us", [a + b for a, b in zip(us[0::2], us[1::2])])):
        if part:
            out[side] = {"median": round(statistics.median(part), 2), "min": round(min(part), 2), "max": round(max(part), 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200, help="timed set_pairs / upload_pairs calls")
    ap.add_argument("--run-steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="short4096,long64")
    ap.add_argument("--strand", default="plus,minus")
    ap.add_argument("--prep-only", action="store_true", help="set_pairs only (for a kernel trace)")
    ap.add_argument("--lib-note", default="")
    ap.add_argument("--trace", default=None, help="summarise the sw_gather_kernel launches of a rocprofv3 kernel trace directory")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(read_trace(args.trace)), flush=True)
        return
    ref = _rand(random.Random(2025), 1000000)
    for name in args.shapes.split(","):
        for strand in args.strand.split(","):
            print(json.dumps(measure(name, strand, ref, args)), flush=True)


if __name__ == "__main__":
    main()
