#!/usr/bin/env python3
"""Option "cigar" (SwmiCigar in swmi_emit.h, the emit site of aff_traceback in swmi_affine.hip) against the two other payloads of
the same affine run: traceback time, result bytes written and the host's time to read every alignment, one JSON line per run.

  shapes     long   64 x (10,000 x 10,000), extend (align_mode global), band 500, scores (2, -4, -2), gap_open -4
             short  4,096 x (150 x 400) = 64 references x 64 reads, local, scores (5, -4, -3), gap_open -5
  payloads   strings  device_strings = 1: both aligned strings behind every record
             ops      device_strings = 0: the 2-bit ops, 16 per dword
             cigar    cigar = 2: {n_cigar, nm, entries}

Per line: `steps` runs with option "profiling" = 1 after `warmup`; the median, minimum and maximum of the traceback time and of
the sweep time; result_bytes = 32 per record (the record table) + 4 per payload dword, computed from the results by the payload's
format; host_read_ms = the median over the steps of what the host needs after a run before it has every alignment in hand --
swmi_batch_materialise_all for strings and ops (index, and for ops the strings built from them), for cigar the record index
plus swmi_pair_cigar of every alignment through ctypes (expand_ms: what swmi_batch_materialise_all costs on top when the caller
wants the strings as well).  The cigar lines carry the ratio of their traceback median to the ops line's.  On a library without
the option the cigar lines are left out (SWMI_LIB selects another build; --lib-note labels the lines)."""
import argparse
import ctypes as C
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


def _load_any_build():
    """binds what the library at SWMI_LIB exports: a build from before the option lacks swmi_pair_cigar, and is measured all the same"""
    lib = C.CDLL(_capi.LIB_PATH)
    _capi.SYMBOLS[:] = [s for s in _capi.SYMBOLS if hasattr(lib, s[0])]
    return any(s[0] == "swmi_pair_cigar" for s in _capi.SYMBOLS)


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
    rng = random.Random(2027)
    base = _rand(rng, 10000)
    long_ = dict(refs=[_mutate(rng, base, 10000) for _ in range(8)], reads=[_mutate(rng, base, 10000) for _ in range(8)],
                 scores=(2, -4, -2, -4), options=dict(long_reads=1, align_mode=sw.ALIGN_GLOBAL, extend=1, band=500))
    refs = [_rand(rng, 400) for _ in range(64)]
    reads = [_mutate(rng, refs[k][rng.randrange(0, 250):][:150], 150) for k in range(64)]
    short = dict(refs=refs, reads=reads, scores=(5, -4, -3, -5), options={})
    return {"long": long_, "short": short}


def _spread(xs):
    return [round(statistics.median(xs), 4), round(min(xs), 4), round(max(xs), 4)]


def measure(shape, case, payload, steps, warmup, note):
    ctx = sw.Context(0)
    try:
        ctx.set_option("gap_open", case["scores"][3])
        for name, v in case["options"].items():
            ctx.set_option(name, v)
        ctx.set_option("device_strings", 1 if payload == "strings" else 0)
        if payload == "cigar":
            ctx.set_option("cigar", 2)
        ctx.set_option("profiling", 1)
        b = ctx.upload(case["refs"], case["reads"])
        p = sw.make_params(case["scores"][:3])
        n_pairs = len(case["refs"]) * len(case["reads"])
        lib = ctx._lib
        for _ in range(warmup):
            b.run(p)
            b.materialise_all()
        fill, tb, read, expand = [], [], [], []
        sc, na = None, None
        for _ in range(steps):
            b.run(p)
            t = b.timing()
            fill.append(t.fill_ms)
            tb.append(t.traceback_ms)
            if payload == "cigar":
                sc, na = b.pair_results()
                cg, n, nm = C.POINTER(C.c_uint32)(), C.c_uint32(), C.c_uint32()
                t0 = time.perf_counter()
                for pair in range(n_pairs):
                    for k in range(int(na[pair])):
                        lib.swmi_pair_cigar(b._h, pair, k, None, None, None, C.byref(cg), C.byref(n), C.byref(nm))
                read.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                b.materialise_all()
                expand.append((time.perf_counter() - t0) * 1e3)
            else:
                t0 = time.perf_counter()
                b.materialise_all()
                read.append((time.perf_counter() - t0) * 1e3)
        sc, na = b.pair_results()
        n_aln, words = 0, 0
        for pair in range(n_pairs):
            if b.n_alignments(pair)[1] & sw.PAIR_DEGENERATE:
                continue
            for k in range(int(na[pair])):
                n_aln += 1
                if payload == "cigar":
                    words += 2 + len(b.cigar(pair, k)[3])
                else:
                    n_ops = len(b.alignment(pair, k)[1][0])
                    words += 2 * (n_ops // 4 + 1) if payload == "strings" else (n_ops + 15) // 16
        out = {"shape": shape, "payload": payload, "lib": note, "pairs": n_pairs, "mode": b.pipeline_mode(), "steps": steps,
               "traceback_ms": _spread(tb), "sweep_ms": _spread(fill), "host_read_ms": _spread(read),
               "records": n_aln, "payload_dwords": words, "result_bytes": 32 * n_aln + 4 * words,
               "score_sum": int(sc.astype("int64").sum())}
        if expand:
            out["expand_ms"] = _spread(expand)
        b.free()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib-note", default="")
    ap.add_argument("--shapes", default="long,short")
    args = ap.parse_args()
    has_cigar = _load_any_build()
    cases = shapes()
    for shape in args.shapes.split(","):
        ops = None
        for payload in ("strings", "ops", "cigar"):
            if payload == "cigar" and not has_cigar:
                continue
            out = measure(shape, cases[shape], payload, args.steps, args.warmup, args.lib_note)
            if payload == "ops":
                ops = out
            if payload == "cigar":
                out["traceback_ratio_to_ops"] = round(out["traceback_ms"][0] / ops["traceback_ms"][0], 3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
