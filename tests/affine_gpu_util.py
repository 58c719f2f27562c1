"""What the GPU tests of the affine path share (test_affine_gpu, test_matrix_gpu, test_ends_gpu, test_long_reads_gpu, test_band_gpu,
test_extend_gpu, test_affine_grid_gpu) -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix), no fixtures: every file keeps its own `ctx`.  Inputs (rand, mutate), one launch with
its run options (run), the expected values of a batch from tests/gotoh_reference.py (expect), the comparison of a batch with them
(check_pair, check), and the C99 program that drives the JNI shim (run_shim)."""
import os
import subprocess

import numpy as np

import sparksmithwaterman_amd as sw

import affine_grid_cases as gc
import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = object()                             # run(matrix=KEEP): leave the context's score matrix as it is
NO_ALIGNMENT = (0, ("", ""))                # what a cell of a degenerate pair yields


def rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, subs=0.04, indels=0.004, alphabet="ACGT"):
    """a copy of s with substitutions and a few one-base insertions and deletions"""
    return gc.mutate(rng, s, alphabet, subs, indels)


def run(ctx, refs, reads, sc, tie=0, mode=None, w=None, extend=None, matrix=KEEP, mode3=True, **options):
    """one batch run under sc = (match, mismatch, gap, gap_open).  align_mode, band, extend and any further option are set where
    given and left as the context has them where None; matrix: (alphabet, rows) sets it, None clears it.  mode3: the run must have
    taken the affine kernels."""
    ctx.set_option("gap_open", sc[3])
    for name, value in [("align_mode", mode), ("band", w), ("extend", extend)] + list(options.items()):
        if value is not None:
            ctx.set_option(name, value)
    if matrix is None:
        ctx.clear_score_matrix()
    elif matrix is not KEEP:
        ctx.set_score_matrix(*matrix)
    b = ctx.upload(refs, reads).run(sw.make_params(sc[:3], None, tie))
    if mode3:
        assert b.pipeline_mode() == 3
    return b


def expect(refs, reads, sc, mode=0, w=0, extend=False, tie=0, matrix=None, cells=False):
    """{(r, q): what the numpy restatement returns for reference r and read q}"""
    return {(r, q): gr.align_numpy(refs[r], reads[q], sc, mode, w, extend, tie, matrix, cells=cells)
            for r in range(len(refs)) for q in range(len(reads))}


def check_pair(b, pair, want, mode=0, what=None):
    """one pair in full: score, number of alignments, flags, every alignment's begin and both strings, and its maximum cell where
    want = (score, alignments, cells).  mode: the run's align_mode -- only a local pair may be degenerate, and is iff it scores 0
    with both sides non-empty; its alignments are not materialised (one per cell), the last one is looked at."""
    es, ea = want[:2]
    assert b.score(pair) == es, (what, b.score(pair), es)
    n, flags = b.n_alignments(pair)
    assert n == len(ea), (what, n, len(ea))
    if mode != sw.ALIGN_LOCAL:
        assert flags == 0, (what, flags)
    elif flags & sw.PAIR_DEGENERATE:
        assert flags == sw.PAIR_DEGENERATE and es == 0, (what, flags, es)
        assert n == 0 or b.alignment(pair, n - 1) == NO_ALIGNMENT, what
        return
    else:
        assert flags == 0 and (es > 0 or n == 0), (what, flags, es, n)
    assert b.alignments(pair) == ea, what
    if len(want) > 2:
        assert b.alignments(pair, with_cell=True) == [a + (c,) for a, c in zip(ea, want[2])], what


def check(b, refs, reads, exp, mode=0, alignments=True, map_ref=True):
    """every pair of the batch against exp[(r, q)] = (score, alignments[, cells]) as check_pair does (alignments=False: scores
    only), then the MapRef view: totals as Java ints, the degenerate count, the match sites stably sorted by begin"""
    for r in range(len(refs)):
        for q in range(len(reads)):
            pair = r * len(reads) + q
            what = (r, q, len(refs[r]), len(reads[q]))
            if alignments:
                check_pair(b, pair, exp[(r, q)], mode, what)
            else:
                assert b.score(pair) == exp[(r, q)][0], what
    if not map_ref:
        return
    packed = b.ref_sites_packed() if alignments else None
    for r in range(len(refs)):
        row = [exp[(r, q)] for q in range(len(reads))]
        total = int(np.int32(sum(e[0] for e in row)))
        assert b.ref_total(r) == total, r
        if alignments:
            sites = sorted([a for e in row for a in e[1] if a != NO_ALIGNMENT], key=lambda t: t[0])
            ndeg = sum(len(e[1]) for e in row if mode == sw.ALIGN_LOCAL and e[0] == 0)
            assert packed[r] == (total, ndeg, sites), r
            if ndeg < 5000:
                assert b.ref_match_sites(r) == [NO_ALIGNMENT] * ndeg + sites, r


def run_shim(tmp_path, name, text=None):
    """compiles tests/c/<name>.c -- or `text`, written out under that name -- with bindings/jni/swmi_shim.c as strict C99 against
    the library, runs the program and returns what it printed"""
    src = os.path.join(ROOT, "tests", "c", name + ".c")
    if text is not None:
        src = tmp_path / (name + ".c")
        src.write_text(text)
    exe = tmp_path / name
    lib = os.path.join(ROOT, "sparksmithwaterman_amd", "lib")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bindings", "jni"),
                           str(src), os.path.join(ROOT, "bindings", "jni", "swmi_shim.c"),
                           "-L", lib, "-lswmi", "-Wl,-rpath," + lib, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout
