"""Seed extension on the GPU (option "extend" on a global run: the sw_affine_sweep_*extend* kernels of swmi_affine.hip and the
global tracebacks) against tests/gotoh_reference.py: every score, every alignment with its begin, both
strings and its maximum cell, the flags and the MapRef view.  set_option("extend", ...) is what fails without the feature.

The eight extend sweeps and the tests that run them (the table of tests/test_affine_grid_gpu.py, continued):

  sweep kernel (sw_affine_sweep_...)    rows per lane     run by
  extend_kernel                         1 .. 4            test_extend_grid_shapes[False-*], test_extend_grid_walks[False-*], test_extend_kats
  extend_wide_kernel                    5 .. 16           test_extend_grid_shapes[False-*], test_extend_grid_walks[False-*]
  long_extend_kernel                    strips of 16      test_extend_long_reads, test_extend_mixed_launch[False]
  extend_matrix_kernel                  1 .. 4            test_extend_grid_shapes[True-*], test_extend_grid_walks[True-*]
  extend_matrix_wide_kernel             5 .. 16           test_extend_grid_shapes[True-*], test_extend_grid_walks[True-*]
  long_extend_matrix_kernel             strips of 16      test_extend_mixed_launch[True], test_extend_long_read_with_a_matrix_strict_ties
  band_extend_kernel                    strips of 16      test_extend_band_maximum_on_a_window_edge, test_extend_band_geometry
  band_extend_matrix_kernel             strips of 16      test_extend_band_shapes_and_matrix, test_extend_mixed_launch[True]

The walks are those of sw_affine_traceback_global_kernel, _long_global_kernel and _band_global_kernel, started at cells other than
(m, n): test_extend_grid_walks, test_extend_long_reads, test_extend_band_maximum_on_a_window_edge."""
import json
import os
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
SC = (5, -3, -2, -6)
GLOBAL = sw.ALIGN_GLOBAL


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# every run of this module is a global run with long reads on, and every expected value an extend result with its cells
def _run(ctx, refs, reads, sc, tie=0, w=0, matrix=None, extend=1, **options):
    return u.run(ctx, refs, reads, sc, tie, GLOBAL, w, extend, matrix, long_reads=1, **options)


def _extend(ref, read, sc, w=0, tie=0, matrix=None, cells=True, align=gr.align_numpy):
    return align(ref, read, sc, GLOBAL, w, True, tie, matrix, cells=cells)


def _expect(refs, reads, sc, w=0, tie=0, matrix=None):
    return u.expect(refs, reads, sc, GLOBAL, w, True, tie, matrix, cells=True)


def _planted(rng, m, n, i):
    """a pair whose one maximum cell is (i, i): a common head of i bases, then a read of A's against a reference of C's"""
    head = u.rand(rng, i)
    return head + "C" * (n - i), head + "A" * (m - i)


# 1 -- the known answers
def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "extend_kat.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("tie", [0, 1])
def test_extend_kats(ctx, tie):
    for k in _kats():
        sc = tuple(k["scores"])
        want = _extend(k["ref"], k["read"], sc, k["w"], tie)       # (strip 1024: none of these reads is banded)
        if k["strip"] == 1024:
            e = k["strict" if tie else "serial"]
            assert want == (e["score"], [(b, tuple(s)) for b, s in e["alignments"]], [tuple(c) for c in e["cells"]]), k["name"]
        b = _run(ctx, [k["ref"]], [k["read"]], sc, tie, k["w"])
        u.check_pair(b, 0, want, GLOBAL, k["name"])
        b.free()


# 2 -- every rows-per-lane class: 48 read lengths against the long reference, the first of every class against the 37-base one
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("matrix", [False, True])
def test_extend_grid_shapes(ctx, matrix, tie):
    refs, reads = gc.shape_grid(matrix)
    assert sorted({gc.rows_per_lane(len(q)) for q in reads}) == list(gc.RS)
    sc = gc.SHAPE_SCORES[matrix]
    mat = gc.score_matrix() if matrix else None
    b = _run(ctx, refs, reads, sc, tie, 0, mat)
    for q in range(len(reads)):
        u.check_pair(b, q, _extend(refs[0], reads[q], sc, 0, tie, mat), GLOBAL, (0, q))
    for q in gc.FIRST_OF_CLASS:
        u.check_pair(b, len(reads) + q, _extend(refs[1], reads[q], sc, 0, tie, mat), GLOBAL, (1, q))
    b.free()


# 3 -- the maximum in hard places
def test_extend_maximum_in_hard_places(ctx):
    rng = random.Random(9960)
    cases = [("cell (1, 1)", _planted(rng, 40, 50, 1), (1, 1))]
    for R in (1, 3, 5, 16):
        for m in (64 * R - 63, 64 * R):                           # row m: slot -64 mod R of the last lane that owns rows, and slot R - 1 of lane 63
            cases.append(("row m = %d" % m, _planted(rng, m, m + 21, m), (m, m)))
    for n, m in ((37, 300), (61, 64), (203, 1000)):               # column n, no multiple of 8; fewer columns than lanes
        cases.append(("column n = %d" % n, _planted(rng, m, n, n), (n, n)))
    # the last step of the last block: lane lact - 1 at column n with (n + lact - 1) % 8 == 0; three columns are deleted on the way
    head = u.rand(rng, 100)
    ref = head[:50] + "TTT" + head[50:]
    cases.append(("last step", (ref, head), (100, 103)))
    assert gc.rows_per_lane(100) == 2 and (103 + 50 - 1) % 8 == 0
    sc = (5, -3, -1, -1)
    for tie in (0, 1):
        want = [_extend(ref, read, sc, 0, tie) for _, (ref, read), _ in cases]
        for (name, _, cell), e in zip(cases, want):
            assert e[2] == [cell], (name, e[2])
        b = _run(ctx, [c[1][0] for c in cases], [c[1][1] for c in cases], sc, tie)
        for x, (name, _, _) in enumerate(cases):
            u.check_pair(b, x * len(cases) + x, want[x], GLOBAL, name)
        b.free()


# 4 -- pad rows must not compete: with mismatch = +1 a pad row, which mismatches every base, out-scores row m
@pytest.mark.parametrize("matrix", [False, True])
def test_extend_pad_rows_do_not_compete(ctx, matrix):
    rng = random.Random(9961)
    draw = gc.MATRIX_DRAW if matrix else "ACGT"
    refs = [u.rand(rng, 150, draw), u.rand(rng, 37, draw)]
    reads = [u.rand(rng, 65, draw), u.rand(rng, 200, draw)]
    assert [gc.rows_per_lane(len(q)) * 64 - len(q) for q in reads] == [63, 56]
    sc = (2, 1, -1, -3)
    mat = gc.score_matrix() if matrix else None
    for tie in (0, 1):
        exp = _expect(refs, reads, sc, 0, tie, mat)
        if not matrix:
            assert all(c[0] == 65 for c in exp[(0, 0)][2])         # every base adds to the score: the best cells are in row m,
                                                                  # where the reference is long enough, and a pad row would beat them
        b = _run(ctx, refs, reads, sc, tie, 0, mat)
        u.check(b, refs, reads, exp, GLOBAL)
        b.free()


# 5 -- the walk grid: long gap runs and tile changes, started from cells that are not (m, n)
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("matrix", [False, True])
def test_extend_grid_walks(ctx, matrix, tie):
    rng = random.Random(9962)
    draw = gc.MATRIX_DRAW if matrix else "ACGT"
    grid = gc.walk_grid(matrix)
    refs = [ref + u.rand(rng, 9, draw) for _, ref, _ in grid]         # a tail the extension leaves unaligned
    reads = [read for _, _, read in grid]
    assert [gc.rows_per_lane(len(read)) for read in reads] == list(gc.RS)
    mat = gc.score_matrix() if matrix else None
    exp = [_extend(ref, read, gc.WALK_SCORES, 0, tie, mat) for ref, read in zip(refs, reads)]
    assert all((len(read), len(ref)) not in e[2] for e, ref, read in zip(exp, refs, reads))
    assert all(gc.longest_run(e[1][0][1][0]) >= 8 and gc.longest_run(e[1][0][1][1]) >= 8 for e in exp)
    for device_strings in (1, 0):
        b = _run(ctx, refs, reads, gc.WALK_SCORES, tie, 0, mat, device_strings=device_strings)
        for x, e in enumerate(exp):
            u.check_pair(b, x * len(reads) + x, e, GLOBAL, x + 1)
        b.free()


# 6 -- ties
@pytest.mark.parametrize("tie", [0, 1])
def test_extend_more_ties_than_cell_cap(ctx, tie):
    """match = 0 on a periodic reference: every cell (k, k) of the read's diagonal ties at 0"""
    refs = ["ACGT" * 50, "AC" * 40]
    reads = ["ACGT" * 10, "ACAC"]
    sc = (0, -3, -1, -3)
    exp = _expect(refs, reads, sc, 0, tie)
    assert exp[(0, 0)][0] == 0 and exp[(0, 0)][2] == [(k, k) for k in range(1, 41)]
    b = _run(ctx, refs, reads, sc, tie, cell_cap=8)
    assert b.timing().rerun_pairs > 0
    u.check(b, refs, reads, exp, GLOBAL)                                   # the list is complete and in order
    b.free()


@pytest.mark.parametrize("tie", [0, 1])
def test_extend_random_pairs_with_many_ties(ctx, tie):
    """small alphabets: many tied maxima, which the two tie modes list in different orders; empty sides score 0"""
    rng = random.Random(9963 + tie)
    differ = 0
    for sc, alpha in (((1, -1, -1, 0), "AC"), ((3, 1, 0, -2), "A"), ((0, -2, -2, 0), "ACGTacgtN\xe9"), ((2, -1, -1, -1), "AC")):
        refs = [u.rand(rng, rng.randint(1, 90), alpha) for _ in range(6)] + ["", "AC" * 150, "CACC"]
        reads = [u.rand(rng, rng.randint(1, 70), alpha) for _ in range(6)] + ["", "CA", "ACA"]
        exp = _expect(refs, reads, sc, 0, tie)
        differ += sum(sorted(e[2]) != e[2] for e in exp.values()) if tie else 0      # (a strict order that is not the row-major one)
        assert exp[(6, 0)] == (0, [], []) and exp[(0, 6)] == (0, [], [])
        b = _run(ctx, refs, reads, sc, tie)
        u.check(b, refs, reads, exp, GLOBAL)
        b.free()
    assert differ >= 5 or not tie


# 7 -- negative and zero scores
def test_extend_negative_and_zero_scores(ctx):
    refs = ["G" * 70, "GGGG", "T"]
    reads = ["C" * 65, "CC", "C" * 300]
    for sc, best in (((2, -3, -1, -3), -3), ((2, 0, -1, -3), 0)):
        exp = _expect(refs, reads, sc)
        assert all(v[0] == best for v in exp.values())
        b = _run(ctx, refs, reads, sc)
        u.check(b, refs, reads, exp, GLOBAL)
        for pair in range(9):
            assert not b.n_alignments(pair)[1] & sw.PAIR_DEGENERATE
        b.free()


# 8 -- long reads
@pytest.mark.parametrize("m,n,i", [(1025, 1030, 500), (2048, 2040, 1024), (2049, 2049, 1025), (2049, 2061, 2049)])
def test_extend_long_reads(ctx, m, n, i):
    """maxima planted in strip 0, on rows 1024 and 1025 and in the last strip"""
    rng = random.Random(9964 + m + i)
    ref, read = _planted(rng, m, n, i)
    for tie in (0, 1):
        want = _extend(ref, read, SC, 0, tie)
        assert want[2] == [(i, i)] and want[0] == 5 * i
        b = _run(ctx, [ref], [read], SC, tie)
        u.check_pair(b, 0, want, GLOBAL, (m, n, i, tie))
        b.free()


@pytest.mark.parametrize("matrix", [False, True])
def test_extend_mixed_launch(ctx, matrix):
    """narrow, wide and strip pairs in one launch, without and with a band"""
    refs, reads = gc.mixed_launch(matrix)
    sc = gc.SHAPE_SCORES[matrix]
    mat = gc.score_matrix() if matrix else None
    exp = _expect(refs, reads, sc, 0, 0, mat)
    b = _run(ctx, refs, reads, sc, 0, 0, mat)
    u.check(b, refs, reads, exp, GLOBAL)
    b.free()
    w = gc.MIXED_BAND
    expb = _expect(refs, reads, sc, w, 0, mat)
    assert expb != exp and all(expb[(r, q)] == exp[(r, q)] for r in range(2) for q in range(2))      # the band applies to the long read
    b = _run(ctx, refs, reads, sc, 0, w, mat)
    u.check(b, refs, reads, expb, GLOBAL)
    b.free()


def test_extend_long_read_with_a_matrix_strict_ties(ctx):
    """sw_affine_sweep_long_extend_matrix_kernel in the strict tie order (test_extend_mixed_launch[True] runs the serial one):
    the smallest pair of two strips"""
    rng = random.Random(9967)
    mat, sc = gc.score_matrix(), gc.SHAPE_SCORES[True]
    ref = u.rand(rng, 1060, gc.MATRIX_DRAW)
    read = gc.mutate(rng, ref, gc.MATRIX_DRAW, 0.04, 0.004)[:1025]
    read += u.rand(rng, 1025 - len(read), gc.MATRIX_DRAW)
    want = _extend(ref, read, sc, 0, 1, mat)
    assert want[0] > 0 and want[2][0][0] > 1024                   # (the maximum is in the second strip)
    b = _run(ctx, [ref], [read], sc, 1, 0, mat)
    u.check_pair(b, 0, want, GLOBAL, 1025)
    b.free()


# 9 -- band
@pytest.mark.parametrize("w", [16, 64])
def test_extend_band_maximum_on_a_window_edge(ctx, w):
    rng = random.Random(9965 + w)
    m = 2049
    win = gr.windows(m, 2049, w)
    # first in-band column of strip 1: w read bases are inserted on the way, the maximum is cell (1025, 1025 - w)
    head = u.rand(rng, 1025)
    first = (head[:500] + head[500 + w:] + "C" * (2049 - 1025 + w), head + "A" * 1024)
    assert win[1][0] == 1025 - w
    # last in-band column of strip 0: w reference columns are deleted on the way, the maximum is cell (1024, 1024 + w)
    head = u.rand(rng, 1024)
    last = (head[:500] + u.rand(rng, w, "T") + head[500:] + "C" * (2049 - 1024 - w), head + "A" * 1025)
    assert win[0][1] == 1024 + w
    for (ref, read), cell in ((first, (1025, 1025 - w)), (last, (1024, 1024 + w))):
        assert (len(read), len(ref)) == (m, 2049)
        for tie in (0, 1):
            want = _extend(ref, read, SC, w, tie)
            assert want[2] == [cell], (want[2], cell)
            b = _run(ctx, [ref], [read], SC, tie, w)
            u.check_pair(b, 0, want, GLOBAL, (w, cell, tie))
            b.free()


def test_extend_band_shapes_and_matrix(ctx):
    """random mutated pairs inside the band, window origins off the 8-step grid, plain and with a matrix"""
    rng = random.Random(9966)
    for w, m, matrix, tie in ((7, 1025, False, 0), (9, 2049, True, 1), (300, 2048, False, 1)):
        draw = gc.MATRIX_DRAW if matrix else "ACGT"
        base = u.rand(rng, m + w + 40, draw)
        read = gc.mutate(rng, base, draw, 0.04, 0.004)[:m]
        read += u.rand(rng, m - len(read), draw)
        refs = [base[:m - w], base]
        reads = [read, gc.mutate(rng, base[200:500], draw)]       # (the short read of the batch is swept in full)
        mat = gc.score_matrix() if matrix else None
        sc = gc.SHAPE_SCORES[matrix]
        exp = _expect(refs, reads, sc, w, tie, mat)
        b = _run(ctx, refs, reads, sc, tie, w, mat)
        u.check(b, refs, reads, exp, GLOBAL)
        b.free()


def _refused(b, params):
    with pytest.raises(_capi.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED


def test_extend_band_geometry(ctx):
    rng = random.Random(9967)
    base = u.rand(rng, 2100)
    p = sw.make_params(SC[:3])
    # a read of 1025 bases has two strips: global mode takes a reference of up to 2048 + 16 bases; the end cell of an extend run
    # is free, so it takes a longer one
    ref, read = base, gc.mutate(rng, base, "ACGT", 0.03, 0.003)[:1025]
    assert len(ref) > 2048 + 16 and len(read) == 1025
    b = _run(ctx, [ref], [read], SC, 0, 16)
    u.check_pair(b, 0, _extend(ref, read, SC, 16, 0), GLOBAL)
    ctx.set_option("extend", 0)                                   # today's behaviour: (m, n) outside the band
    _refused(b, p)
    b.free()
    # the empty window is refused as ever: a read of 2049 bases has three strips, the last one's window starts at 2048 + 1 - 8
    ctx.set_option("extend", 1)
    ctx.set_option("band", 8)
    b = ctx.upload([base[:2041]], [base[:2049]]).run(p)
    u.check_pair(b, 0, _extend(base[:2041], base[:2049], SC, 8, 0), GLOBAL)
    b.free()
    b = ctx.upload([base[:2040]], [base[:2049]])
    _refused(b, p)
    b.free()


# 10 -- the options that apply to mode-3 runs give the same results
_VARIANTS = {}


def _variants():
    if not _VARIANTS:
        rng = random.Random(9968)
        refs = ["ACGTTGCA" * 40, u.rand(rng, 900), "GATTACA" * 30 + u.rand(rng, 200), u.rand(rng, 64), u.rand(rng, 2500)]
        reads = ["ACGTTGCAAC", u.rand(rng, 150), "GATTACAGATTACA", u.rand(rng, 300), refs[4][1000:1400]]
        _VARIANTS.update(refs=refs, reads=reads, exp=_expect(refs, reads, (2, -3, -1, -2)))
    return _VARIANTS["refs"], _VARIANTS["reads"], _VARIANTS["exp"]


@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("zero_copy", 0), ("cell_cap", 1),
                                 ("max_workspace_bytes", 1 << 20)])
def test_extend_options(ctx, opt):
    refs, reads, exp = _variants()
    b = _run(ctx, refs, reads, (2, -3, -1, -2), 0, 0, None, 1, **dict([opt]))
    if opt[0] == "scores_only":
        for (r, q), want in exp.items():
            assert b.score(r * len(reads) + q) == want[0]
        assert [b.ref_total(r) for r in range(len(refs))] == [sum(exp[(r, q)][0] for q in range(len(reads))) for r in range(len(refs))]
    else:
        u.check(b, refs, reads, exp, GLOBAL)
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    b.free()


# 11 -- option semantics
def test_extend_invalid_values_leave_the_context(ctx):
    k = _kats()[0]
    sc = tuple(k["scores"])
    want = _extend(k["ref"], k["read"], sc, 0, 0)
    assert want[:2] != gr.align_numpy(k["ref"], k["read"], sc, GLOBAL)
    for start in (1, 0):
        b = _run(ctx, [k["ref"]], [k["read"]], sc, extend=start)
        for bad in (2, -1, 1 << 40):
            with pytest.raises(_capi.SwmiError) as e:
                ctx.set_option("extend", bad)
            assert e.value.code == ERR_INVALID
        b.run(sw.make_params(sc[:3]))                             # the next run is still what it was
        if start:
            u.check_pair(b, 0, want, GLOBAL)
        else:
            assert (b.score(0), b.alignments(0)) == gr.align_numpy(k["ref"], k["read"], sc, GLOBAL)
        b.free()


@pytest.mark.parametrize("mode", [sw.ALIGN_LOCAL, sw.ALIGN_FIT])
def test_extend_needs_global(ctx, mode):
    rng = random.Random(9969)
    ref, read = u.rand(rng, 200), u.rand(rng, 80)
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("align_mode", mode)
    ctx.set_option("extend", 1)
    b = ctx.upload([ref], [read])
    p = sw.make_params(SC[:3])
    _refused(b, p)
    ctx.set_option("extend", 0)                                   # the batch is still usable
    b.run(p)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, SC, mode)
    ctx.set_option("gap_open", 0)                                 # the linear pipeline refuses it too
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)
    ctx.set_option("extend", 1)
    _refused(b, p)
    b.free()


def test_extend_travels_with_the_run(ctx):
    rng = random.Random(9970)
    base = u.rand(rng, 700)
    refs = [base[:600] + u.rand(rng, 60), gc.mutate(rng, base), u.rand(rng, 300)] + [gc.mutate(rng, base) for _ in range(5)]
    reads = [gc.mutate(rng, base[:400]), base[:90] + u.rand(rng, 40)]
    exp = _expect(refs, reads, SC)
    glob = {k: gr.align_numpy(refs[k[0]], reads[k[1]], SC, GLOBAL) for k in exp}
    assert all(exp[k][:2] != glob[k] for k in exp)
    p = sw.make_params(SC[:3])
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("align_mode", GLOBAL)
    for value in (1, 0):
        ctx.set_option("extend", value)
        ctx.set_option("debug_async_delay_us", 50000)
        b = ctx.upload(refs, reads).run_async(p)
        ctx.set_option("extend", 1 - value)                       # does not reach the run in flight
        b.wait()
        ctx.set_option("debug_async_delay_us", 0)
        for (r, q) in exp:
            pair = r * len(reads) + q
            assert (b.score(pair), b.alignments(pair)) == (exp[(r, q)][:2] if value else glob[(r, q)]), (value, r, q)
        b.free()
    ctx.set_option("extend", 1)
    st = ctx.stream(reads, p, slots=2, chunk_bytes=1 << 11)
    ctx.set_option("extend", 0)                                   # (the slots copied it at the open)
    st.push(refs[:5]).push(refs[5:]).finish()
    assert [int(t) for t in st.totals()] == [sum(exp[(r, q)][0] for q in range(len(reads))) for r in range(len(refs))]
    n_chunks = 0
    for first, c in st.chunks():
        n_chunks += 1
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            for q in range(len(reads)):
                u.check_pair(c, r * len(reads) + q, exp[(first + r, q)], GLOBAL, (first + r, q))
    assert n_chunks >= 2
    st.close()


def test_extend_0_is_global(ctx):
    """nothing moved: with extend = 0 a global run equals the reference's plain global mode, before and after an extend run of the
    batch"""
    refs, reads, exp = _variants()
    sc = (2, -3, -1, -2)
    b = _run(ctx, refs, reads, sc, extend=0)
    p = sw.make_params(sc[:3])
    glob = {(r, q): gr.align_numpy(refs[r], reads[q], sc, GLOBAL) for r in range(len(refs)) for q in range(len(reads))}
    for value in (0, 1, 0):
        ctx.set_option("extend", value)
        b.run(p)
        if value:
            u.check(b, refs, reads, exp, GLOBAL)
            continue
        for r in range(len(refs)):
            for q in range(len(reads)):
                pair = r * len(reads) + q
                assert (b.score(pair), b.alignments(pair)) == glob[(r, q)], (r, q)
                assert b.alignments(pair, with_cell=True)[0][2] == (len(reads[q]), len(refs[r]))
    b.free()


def test_extend_mirror(ctx):
    k = _kats()[8]                                                # (the two tie modes order its cells differently)
    sc = k["scores"]
    for cls, tie in ((sw.SmithWaterman.OptAlignments, 0), (sw.DistributedSW.OptAlignments, 1)):
        got = cls(ctx, align_mode=GLOBAL, extend=True).call([k["ref"], k["read"]], sc)
        assert got == _extend(k["ref"], k["read"], sc, 0, tie, cells=False)
        assert ctx.options["extend"] == 0 and ctx.options["align_mode"] == sw.ALIGN_LOCAL
    reads = [k["read"], "ACGT"]
    total, (ref, sites) = sw.Distribution.MapRef(ctx, align_mode=GLOBAL, extend=True).call(((">r", k["ref"]), reads, (sc, ["a", "i", "d", "-"])))
    exp = [_extend(k["ref"], q, sc, cells=False) for q in reads]
    assert total == sum(e[0] for e in exp) and sites == [a for e in exp for a in e[1]]


# 12 -- global mode's arithmetic bounds hold in extend mode, each pinned from both sides against the scalar restatement
def test_extend_bound_int32(ctx):
    """3 * |gap_open| + (64 * ceil(m / 64) + n) * |gap| <= 2^31 -- the last n inside, the first outside"""
    rng = random.Random(9971)
    e, o, m = -(1 << 20), 0, 64
    n_ok = (1 << 31) // -e - 64
    assert (64 + n_ok) * -e <= 1 << 31 < (64 + n_ok + 1) * -e
    read = u.rand(rng, m, "AC")
    ref = read[:40] + u.rand(rng, n_ok + 1 - 40, "AC")
    sc = (1 << 20, -3, e, o)
    b = _run(ctx, [ref[:n_ok]], [read], sc)
    u.check_pair(b, 0, _extend(ref[:n_ok], read, sc, align=gr.align_scalar), GLOBAL)
    b.free()
    b = ctx.upload([ref], [read])
    _refused(b, sw.make_params(sc[:3]))
    b.free()


def test_extend_bounds_banded(ctx):
    """under a band: 3 * |gap_open| + (1024 * ceil(m / 1024) + n) * |gap| <= 2^30 and M * S <= 2^29, with M = 2048"""
    rng = random.Random(9972)
    S = 1 << 18
    read = u.rand(rng, 1025, "AC")
    ref = read[:900] + u.rand(rng, 1149, "AC")
    assert len(ref) == 2049
    sc = (5, -3, -S, 0)                                           # (2048 + 2048) * 2^18 = 2^30, and M * S = 2^29
    b = _run(ctx, [ref[:2048]], [read], sc, 0, 8)
    u.check_pair(b, 0, _extend(ref[:2048], read, sc, 8, align=gr.align_scalar), GLOBAL)
    _refused(b, sw.make_params((S + 1, -3, -S)))                  # M * S one step past 2^29
    b.free()
    b = ctx.upload([ref], [read])                                 # one more column
    _refused(b, sw.make_params(sc[:3]))
    b.free()
    ctx.set_option("band", 0)                                     # unbanded the bounds are 2^31 and 2^30: the same pair runs
    b = ctx.upload([ref], [read]).run(sw.make_params(sc[:3]))
    u.check_pair(b, 0, _extend(ref, read, sc), GLOBAL)
    b.free()


# 13 -- the JNI shim's entry point from plain C99 (tests/c/shim_extend.c)
def test_c99_shim_sets_extend(tmp_path):
    out = u.run_shim(tmp_path, "shim_extend")
    k = _kats()[0]
    assert (k["ref"], k["read"], k["scores"]) == ("ACGTTGCA", "ACGTAC", [2, -3, -1, -3])
    g = gr.align_numpy(k["ref"], k["read"], k["scores"], GLOBAL)
    assert out.splitlines() == ["8 1 1:ACGT/ACGT mode 3", "%d 1 1:%s/%s mode 3" % (g[0], g[1][0][1][0], g[1][0][1][1]),
                                       "refused %d" % ERR_UNSUPPORTED]
