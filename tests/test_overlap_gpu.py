"""Overlap (ends-free) alignment on the GPU (option "overlap" on a fit run: the sw_affine_sweep_*overlap* kernels and the two
overlap tracebacks of swmi_affine.hip) against tests/overlap_reference.py: every score, every alignment with
its begin, both strings and its maximum cell, the flags and the MapRef view.  set_option("overlap", ...) is what fails without the
feature.

  sweep kernel (sw_affine_sweep_...)    rows per lane     run by
  overlap_kernel                        1 .. 4            test_rows_per_lane, test_planted_overlaps, test_census, test_walk_grid,
                                                          test_random_pairs_with_many_ties, test_options
  overlap_wide_kernel                   5 .. 16           test_rows_per_lane, test_planted_overlaps, test_census, test_walk_grid,
                                                          test_bounds, test_options
  overlap_matrix_kernel                 1 .. 4            test_matrix, test_census, test_walk_grid
  overlap_matrix_wide_kernel            5 .. 16           test_matrix, test_census, test_walk_grid
  long_overlap_kernel                   strips of 16      test_long_reads, test_census, test_long_reads_seams,
                                                          test_long_reads_more_ties_than_cell_cap, test_bounds
  long_overlap_matrix_kernel            strips of 16      test_matrix, test_census
The walks: sw_affine_traceback_overlap_kernel with every short read (gap runs: test_walk_grid; alignments that start with a gap:
test_random_pairs_with_many_ties), sw_affine_traceback_long_overlap_kernel with every long one (a run across row 1024, two seams,
column 0 at a seam: test_long_reads_seams; 709 walks of one pair: test_long_reads_more_ties_than_cell_cap).  The inputs of the tests
named here for the first time come from tests/overlap_cases.py, which states what each is built for."""
import ctypes as C
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import affine_census as census
import affine_gpu_util as u
import affine_grid_cases as gc
import cigar_reference as cr
import gotoh_reference as gr
import overlap_cases as oc
import overlap_reference as ov

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
FIT = sw.ALIGN_FIT
SC = (5, -3, -2, -6)
OVERLAP = 4                                 # AffRun.mode of an overlap run


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _run(ctx, refs, reads, sc, tie=0, matrix=None, overlap=1, **options):
    return u.run(ctx, refs, reads, sc, tie, FIT, 0, 0, matrix, long_reads=1, overlap=overlap, **options)


def _want(ref, read, sc, tie=0, matrix=None):
    return ov.align_numpy(ref, read, sc, FIT, 0, False, tie, matrix, cells=True)


def _expect(refs, reads, sc, tie=0, matrix=None):
    return {(r, q): _want(refs[r], reads[q], sc, tie, matrix) for r in range(len(refs)) for q in range(len(reads))}


def _check_diagonal(b, cases, want, n_reads):
    for x, e in enumerate(want):
        u.check_pair(b, x * n_reads + x, e, FIT, cases[x][0])


# 1 -- every rows-per-lane class
_GRID = {}


def _grid():
    """reads of 64 (R - 1) + 1, 64 R - 1 and 64 R bases for R = 1 .. 16 -- among them m = 1 -- each a mutated stretch of one base
    sequence; references of 1, 37 and 203 bases (no multiple of 8; shorter and longer than the reads) cut from it, and one longer
    than every read for the reads of 64 R bases"""
    if not _GRID:
        rng = random.Random(8801)
        base = u.rand(rng, 1400)
        lengths = [m for R in gc.RS for m in (64 * (R - 1) + 1, 64 * R - 1, 64 * R)]
        assert sorted({gc.rows_per_lane(m) for m in lengths}) == list(gc.RS) and lengths[0] == 1
        reads = []
        for x, m in enumerate(lengths):
            at = (37 * x) % 150
            read = gc.mutate(rng, base[at:at + m + 8], "ACGT", 0.05, 0.01)[:m]
            reads.append(read + u.rand(rng, m - len(read)))
        refs = [base[100:101], base[60:97], base[20:223]]
        assert [len(r) for r in refs] == [1, 37, 203] and all(len(r) % 8 for r in refs)
        _GRID.update(refs=refs, reads=reads, long_ref=base[300:1337], last=[q for q in reads if len(q) % 64 == 0])
        assert len(_GRID["long_ref"]) == 1037 and len(_GRID["last"]) == 16
    return _GRID


@pytest.mark.parametrize("tie", [0, 1])
def test_rows_per_lane(ctx, tie):
    g = _grid()
    exp = _expect(g["refs"], g["reads"], SC, tie)
    b = _run(ctx, g["refs"], g["reads"], SC, tie)
    u.check(b, g["refs"], g["reads"], exp, FIT)
    b.free()


@pytest.mark.parametrize("tie", [0, 1])
def test_rows_per_lane_reference_longer_than_the_read(ctx, tie):
    g = _grid()
    exp = _expect([g["long_ref"]], g["last"], SC, tie)
    b = _run(ctx, [g["long_ref"]], g["last"], SC, tie)
    u.check(b, [g["long_ref"]], g["last"], exp, FIT)
    b.free()


# 2 -- planted overlaps: the shared stretch X is drawn from "CG", the read's own bases are A's and the reference's T's, so that the one
# best overlap and its coordinates are known by construction
def _suffix_prefix(rng, m, n, L):
    """the read's suffix equals the reference's prefix: cell (m, L), span (m - L + 1, m, 1, L)"""
    X = u.rand(rng, L, "CG")
    return X + "T" * (n - L), "A" * (m - L) + X, (m, L), (m - L + 1, m, 1, L)


def _prefix_suffix(rng, m, n, L):
    """the reference's suffix equals the read's prefix: cell (L, n), span (1, L, n - L + 1, n)"""
    X = u.rand(rng, L, "CG")
    return "T" * (n - L) + X, X + "A" * (m - L), (L, n), (1, L, n - L + 1, n)


def _read_contained(rng, m, n, at):
    """the read is contained in the reference from column at + 1 on: cell (m, at + m), span (1, m, at + 1, at + m)"""
    X = u.rand(rng, m, "CG")
    return "T" * at + X + "T" * (n - at - m), X, (m, at + m), (1, m, at + 1, at + m)


def _ref_contained(rng, m, n, at):
    """the reference is contained in the read from row at + 1 on: cell (at + n, n), span (at + 1, at + n, 1, n)"""
    X = u.rand(rng, n, "CG")
    return X, "A" * at + X + "A" * (m - at - n), (at + n, n), (at + 1, at + n, 1, n)


def _planted_cases():
    rng = random.Random(8802)
    cases = []
    # row m (kinds 1 and 3): its lane and slot follow from m -- lane (m - 1) // R, slot (m - 1) % R.  R = 1: a middle lane and the
    # last, the one slot being first and last; R = 2: lane 32, slot 0; lane 63, slot 1; R = 5: lane 59, slot 4; R = 16: lane 63,
    # slot 15.  (Row m lies in the first lane only for m <= R, which is m = 1: test_rows_per_lane has that read.)
    for m in (20, 64, 65, 128, 300, 1024):
        L = min(m - 3, 40)
        cases.append(("suffix-prefix m=%d" % m, _suffix_prefix(rng, m, 90, L)))
        cases.append(("read contained m=%d" % m, _read_contained(rng, m, m + 57, 30)))
    # column n (kinds 2 and 4) with R = 16: the end row is free -- row 16: the first lane, its last slot; 17: lane 1, slot 0; 513:
    # lane 32, slot 0; 528: lane 32, slot 15; 1009: lane 63, slot 0; 1024: lane 63, slot 15.  And R = 3: row 190, lane 63, slot 0
    for row in (16, 17, 513, 528, 1009):
        cases.append(("prefix-suffix row=%d" % row, _prefix_suffix(rng, 1024, 1101, row)))
    for row in (16, 513, 1009, 1024):
        cases.append(("ref contained row=%d" % row, _ref_contained(rng, 1024, 12, row - 12)))
    cases.append(("prefix-suffix R=3", _prefix_suffix(rng, 192, 45, 40)))
    cases.append(("ref contained R=3", _ref_contained(rng, 192, 23, 190 - 23)))
    return cases


@pytest.mark.parametrize("tie", [0, 1])
def test_planted_overlaps(ctx, tie):
    cases = _planted_cases()
    refs, reads = [c[1][0] for c in cases], [c[1][1] for c in cases]
    want = [_want(ref, read, SC, tie) for ref, read in zip(refs, reads)]
    for (name, (_, _, cell, span)), e in zip(cases, want):
        assert e[2] == [cell] and ov.span(cell, e[1][0]) == span, (name, e[2], cell)
    b = _run(ctx, refs, reads, SC, tie)
    _check_diagonal(b, cases, want, len(reads))
    for x, (name, (_, _, cell, span)) in enumerate(cases):
        assert b.span(x * len(reads) + x, 0) == span, name
    b.free()
    ctx.set_option("cigar", 2)                                    # Batch.span from the CIGAR
    b = ctx.upload(refs[:4], reads[:4]).run(sw.make_params(SC[:3], None, tie))
    for x in range(4):
        assert b.span(x * 4 + x, 0) == cases[x][1][3], cases[x][0]
    b.free()


# 3 -- ties on row m and on column n at once
@pytest.mark.parametrize("tie", [0, 1])
def test_more_ties_than_cell_cap(ctx, tie):
    """match = 0 on periodic sequences: every overlap without a mismatch scores 0 -- the cells (m, j) and (i, n) with even i, j"""
    refs, reads = ["AC" * 40, "ACGT" * 12], ["AC" * 30, "ACGT" * 5]
    sc = (0, -3, -1, -3)
    exp = _expect(refs, reads, sc, tie)
    score, alns, cells = exp[(0, 0)]
    assert score == 0 and cells.count((60, 80)) == 1 and len(cells) == len(set(cells)) == 69
    assert sum(c[0] == 60 for c in cells) == 40 and sum(c[1] == 80 for c in cells) == 30
    assert all(len(e[2]) > 8 for e in (exp[(0, 0)], exp[(1, 1)]))                 # more than cell_cap: the exact-size re-run is taken
    b = _run(ctx, refs, reads, sc, tie, cell_cap=8)
    assert b.timing().rerun_pairs >= 2
    u.check(b, refs, reads, exp, FIT)
    b.free()


def test_a_non_competing_cell_at_the_maximum_is_not_listed(ctx):
    """H(2, 2) = 2 is the score, which competing cells reach in the last column only"""
    for tie in (0, 1):
        want = _want("ACGAC", "ACT", (1, -3, -1, 0), tie)
        assert want[0] == 2 and want[2] == [(2, 5)]
        b = _run(ctx, ["ACGAC"], ["ACT"], (1, -3, -1, 0), tie)
        u.check_pair(b, 0, want, FIT)
        b.free()


# 3a -- direction ties, tied maximum cells and alignments that start with a gap: small alphabets, scores down to 0
@pytest.mark.parametrize("tie", [0, 1])
def test_random_pairs_with_many_ties(ctx, tie):
    """the six sets of overlap_cases.tie_sets, 64 pairs each, with cell_cap = 8.  Sets 3 and 5 hold the alignments that start with a
    gap: there the chains meet E(i,0) := o and F(0,j) := o.  Each set has at least 10 pairs with more than 8 tied cells over the two
    tie modes together (tests/test_overlap_cpu.py); a run has one tie mode, so what it is held to is the restatement's count of such
    pairs in that mode -- 17, 60, 6, 25, 6, 15 in either -- which sums to the 10 and more per set over this test's two cases."""
    failed = []                                                   # every set is run: the message names all that differ
    for k, (sc, refs, reads) in enumerate(oc.tie_sets(), 1):
        exp = {(r, q): oc.want(refs[r], reads[q], sc, tie) for r in range(len(refs)) for q in range(len(reads))}
        over = sum(len(e[2]) > oc.TIE_CELL_CAP for e in exp.values())
        b = _run(ctx, refs, reads, sc, tie, cell_cap=oc.TIE_CELL_CAP)
        print("set %d tie %d: rerun_pairs %d, pairs over cell_cap %d" % (k, tie, b.timing().rerun_pairs, over))
        try:
            u.check(b, refs, reads, exp, FIT)
            assert b.timing().rerun_pairs >= over >= 5
        except AssertionError as e:
            failed.append(("set %d" % k, sc, str(e)[:200]))
        b.free()
    assert not failed, failed


# 3b -- gap runs: the walk grid with all four ends free, and as it stands (the corner cell)
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("matrix", [False, True])
def test_walk_grid(ctx, matrix, tie):
    """an inserted run that crosses lanes and a deleted run longer than one traceback tile (R >= 6) in every rows-per-lane class, in
    an alignment that ends on row m left of column n and reaches column 0 below row 1 (the cut pairs) or ends at (m, n) (the uncut
    ones); Batch.span, then the same walks under cigar = 2"""
    mat = oc.matrix_of(matrix)
    for grid in (oc.walk_pairs(matrix), gc.walk_grid(matrix)):
        refs, reads = [ref for _, ref, _ in grid], [read for _, _, read in grid]
        assert [gc.rows_per_lane(len(read)) for read in reads] == list(gc.RS)
        want = [oc.want(ref, read, gc.WALK_SCORES, tie, mat) for ref, read in zip(refs, reads)]
        b = _run(ctx, refs, reads, gc.WALK_SCORES, tie, mat)
        _check_diagonal(b, grid, want, len(reads))
        for x, (_, alns, cells) in enumerate(want):
            for k, (aln, cell) in enumerate(zip(alns, cells)):
                assert b.span(x * len(reads) + x, k) == ov.span(cell, aln), (grid[x][0], k)
        b.free()
        b = _run(ctx, refs, reads, gc.WALK_SCORES, tie, mat, cigar=2)
        for x, (score, alns, cells) in enumerate(want):
            pair = x * len(reads) + x
            got = b.cigars(pair)
            assert b.score(pair) == score and len(got) == len(alns) >= 1, grid[x][0]
            for k, ((begin, (ra, qa)), cell) in enumerate(zip(alns, cells)):
                ent, nm = cr.cigar(ra, qa, 2)
                assert got[k] == (begin, cell[0], cell[1], ent, nm), (grid[x][0], k)
                assert b.span(pair, k) == ov.span(cell, alns[k]), (grid[x][0], k)
        b.free()
        ctx.set_option("cigar", 0)


# 4 -- no overlap worth having
def test_no_overlap(ctx):
    refs, reads = ["G" * 70, "G"], ["C" * 65, "C"]
    sc = (2, -3, -1, -3)
    exp = _expect(refs, reads, sc)
    assert all(e[0] == -3 for e in exp.values()) and sorted(exp[(0, 0)][2]) == [(1, 70), (65, 1)]
    b = _run(ctx, refs, reads, sc)
    u.check(b, refs, reads, exp, FIT)
    for pair in range(4):
        assert b.n_alignments(pair)[1] == 0
    b.free()
    # a mismatch dearer than a gap: the one alignment of a pair of one base each inserts the read's base (serial ties) or deletes
    # the reference's (strict), and `begin` is the end column
    sc = (2, -9, -1, -1)
    assert _want("G", "C", sc, 0) == (-2, [(1, ("_", "C"))], [(1, 1)]) and _want("G", "C", sc, 1) == (-2, [(1, ("G", "_"))], [(1, 1)])
    for tie in (0, 1):
        b = _run(ctx, ["G", ""], ["C", ""], sc, tie)
        u.check(b, ["G", ""], ["C", ""], _expect(["G", ""], ["C", ""], sc, tie), FIT)
        assert b.span(0, 0) == ((1, 1, 1, 1) if tie == 0 else (2, 1, 1, 1))
        assert (b.score(1), b.n_alignments(1)) == (0, (0, 0)) and (b.score(3), b.n_alignments(3)) == (0, (0, 0))      # an empty side
        b.free()


# 5 -- a score matrix; 7 -- the census: every new kernel in both tie orders
def _census_case(matrix, m):
    rng = random.Random(8805 + m + int(matrix))
    draw = gc.MATRIX_DRAW if matrix else "ACGT"
    base = u.rand(rng, m + 400, draw)
    read = gc.mutate(rng, base[200:200 + m + 10], draw, 0.04, 0.005)[:m]
    read += u.rand(rng, m - len(read), draw)
    # the reference ends inside the read, and starts inside it
    return [base[:200 + m // 2], base[200 + m // 3:]], [read]


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("matrix", [False, True])
def test_census(ctx, matrix, tie):
    mat = gc.score_matrix() if matrix else None
    sc = gc.SHAPE_SCORES[matrix]
    for m, shape, long_reads in ((100, 0, 0), (300, 1, 0), (1100, 2, 1)):
        run = census.AffRun(gap_open=sc[3], mode=OVERLAP, mat=census.dummy_matrix() if matrix else None, nn=len(mat[0]) + 1 if matrix else 0)
        assert census.names(run, long_reads, shape) == (
            "sw_affine_sweep_%soverlap%s%s_kernel" % ("long_" if long_reads else "", "_matrix" if matrix else "", "_wide" if shape == 1 else ""),
            "sw_affine_traceback_%soverlap_kernel" % ("long_" if long_reads else ""))
        refs, reads = _census_case(matrix, m)
        assert (len(reads[0]) > 1024) == bool(long_reads) and (long_reads or (gc.rows_per_lane(m) > 4) == (shape == 1))
        exp = _expect(refs, reads, sc, tie, mat)
        assert exp[(0, 0)][0] > m and exp[(1, 0)][0] > m
        assert all(c[1] == len(refs[0]) for c in exp[(0, 0)][2]) and all(c[0] == m for c in exp[(1, 0)][2])     # a column-n and a row-m end
        b = _run(ctx, refs, reads, sc, tie, mat)
        u.check(b, refs, reads, exp, FIT)
        b.free()
    if matrix:
        # the matrix is not symmetric: rows are the read's bases
        swapped = (mat[0], [list(col) for col in zip(*mat[1])])
        assert _want(refs[0], reads[0], sc, tie, swapped)[0] != exp[(0, 0)][0]


# 6 -- long reads
def _long_cases():
    rng = random.Random(8806)
    X = u.rand(rng, 1500, "CG")
    return {
        # row m is the one row of the last strip; the walk crosses the seam below row 1024
        "m=1025": ([X[:400] + "T" * 300], ["A" * 625 + X[:400]], [[(1025, 400)]], [(626, 1025, 1, 400)]),
        # column n: a maximum in strip 0 and one in strip 1 whose walk crosses the seam
        "m=2048": (["T" * 1600 + X], [X[900:] + "A" * 1448, X + "A" * 548], [[(600, 3100)], [(1500, 3100)]], [(1, 600, 2501, 3100), (1, 1500, 1601, 3100)]),
        # row m = 2049, alone in the third strip
        "m=2049": ([X[:300] + "T" * 200], ["A" * 1749 + X[:300]], [[(2049, 300)]], [(1750, 2049, 1, 300)]),
        # the reference inside the read: the walk ends at column 0 in strip 1, a head of 1100 read bases hangs over
        "m=3000": ([X[:300]], ["A" * 1100 + X[:300] + "A" * 1600], [[(1400, 300)]], [(1101, 1400, 1, 300)]),
    }


@pytest.mark.parametrize("case", ["m=1025", "m=2048", "m=2049", "m=3000"])
def test_long_reads_planted(ctx, case):
    refs, reads, cells, spans = _long_cases()[case]
    assert len(refs) == 1 and all(len(q) == int(case[2:]) for q in reads)
    for tie in (0, 1):
        exp = _expect(refs, reads, SC, tie)
        assert [exp[(0, q)][2] for q in range(len(reads))] == cells
        b = _run(ctx, refs, reads, SC, tie)
        u.check(b, refs, reads, exp, FIT)
        assert [b.span(q, 0) for q in range(len(reads))] == spans
        b.free()


@pytest.mark.parametrize("tie", [0, 1])
def test_long_reads_mutated_dovetail(ctx, tie):
    """about 3,000 bases against 3,100: the reference's tail continues into the read, with substitutions and indels"""
    rng = random.Random(8807)
    base = u.rand(rng, 5200)
    ref = base[:3100]
    read = gc.mutate(rng, base[2100:5200], "ACGT", 0.04, 0.004)[:2990]
    want = _want(ref, read, SC, tie)
    assert want[0] > 3000 and all(c[1] == 3100 and 900 < c[0] < 1100 for c in want[2])
    b = _run(ctx, [ref], [read], SC, tie)
    u.check_pair(b, 0, want, FIT, tie)
    b.free()


# 6a -- the seams: column 0 at rows 1025 and 2049, a gap run across row 1024, a walk across two seams
@pytest.mark.parametrize("tie", [0, 1])
def test_long_reads_seams(ctx, tie):
    """lane 0's diagonal for the first row of strip sx is H(1024 sx, 0) = 0 (fit has o + 1024 sx e there): only an alignment whose
    first row is 1024 sx + 1, at column 1, reads it"""
    failed = []                                                   # every case is run: the message names all that differ
    for name, ref, read, sc, span in oc.seam_cases():
        want = oc.want(ref, read, sc, tie)
        assert len(read) > 1024 and len(want[2]) == 1, name
        b = _run(ctx, [ref], [read], sc, tie)
        try:
            u.check_pair(b, 0, want, FIT, name)
            assert b.span(0, 0) == ov.span(want[2][0], want[1][0]) and span in (None, b.span(0, 0)), name
        except AssertionError as e:
            failed.append(str(e)[:200])
        b.free()
    assert not failed, failed


# 6b -- tied maxima on column n of both strips and on row m, more than cell_cap: the exact-size re-run of the strip sweep
@pytest.mark.parametrize("tie", [0, 1])
def test_long_reads_more_ties_than_cell_cap(ctx, tie):
    ref, read = oc.long_tie_case()
    want = oc.want(ref, read, oc.LONG_TIE_SCORES, tie)
    assert len(want[2]) == 709
    b = _run(ctx, [ref], [read], oc.LONG_TIE_SCORES, tie, cell_cap=8)
    assert b.timing().rerun_pairs == 1 and b.n_alignments(0)[0] == 709
    u.check(b, [ref], [read], {(0, 0): want}, FIT)
    b.free()


# 6c -- the arithmetic bounds: |score| = 2^20 with no floor, and M * S <= 2^30 under long_reads from both sides
def test_bounds(ctx):
    for name, ref, read, sc in oc.bound_cases():
        for tie in (0, 1):
            want = oc.want(ref, read, sc, tie)
            if len(read) > 1024:                                  # 2048 rows * 2^20: the restatement's 2^30 is out of the library's reach
                ctx.set_option("gap_open", sc[3])
                b = ctx.upload([ref], [read])
                _refused(b, sw.make_params(sc[:3], None, tie), "2^30")
                assert b.timing().fill_launches == 0
                b.free()
                continue
            b = _run(ctx, [ref], [read], sc, tie)
            u.check_pair(b, 0, want, FIT, (name, tie))
            b.free()
    cases = oc.long_bound_cases()
    refs, reads = [c[1] for c in cases], [c[2] for c in cases]
    S = oc.LONG_S_OK
    sc = (S, -S, -S, -S)
    want = [oc.want(ref, read, sc) for ref, read in zip(refs, reads)]
    assert want[0][0] == 2049 * S
    b = _run(ctx, refs, reads, sc)
    _check_diagonal(b, cases, want, len(reads))
    b.free()
    S = oc.LONG_S_REFUSED
    ctx.set_option("gap_open", -S)
    b = ctx.upload(refs, reads)
    _refused(b, sw.make_params((S, -S, -S)), "2^30")
    assert b.timing().fill_launches == 0                          # nothing was launched
    ctx.set_option("gap_open", -oc.LONG_S_OK)
    b.run(sw.make_params(sc[:3]))                                 # the batch is still usable
    _check_diagonal(b, cases, want, len(reads))
    b.free()


# 8 -- the options that combine
_VARIANTS = {}


def _variants():
    if not _VARIANTS:
        rng = random.Random(8808)
        base = u.rand(rng, 1600)
        refs = [base[:700], base[400:1100], "ACGTTGCA" * 20, base[300:1500]]
        reads = [gc.mutate(rng, base[500:900]), base[1000:1100] + u.rand(rng, 50), "GCAACGTT" * 6, gc.mutate(rng, base[200:1300])[:1050]]
        _VARIANTS.update(refs=refs, reads=reads, exp=_expect(refs, reads, (2, -3, -1, -2)))
    return _VARIANTS["refs"], _VARIANTS["reads"], _VARIANTS["exp"]


@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("zero_copy", 0), ("cigar", 1), ("cigar", 2),
                                 ("arena_words_per_pair", 1), ("cell_cap", 1), ("max_workspace_bytes", 1 << 20)])
def test_options(ctx, opt):
    refs, reads, exp = _variants()
    if opt[0] == "max_workspace_bytes":                           # (the 1050 x 1200 field alone is over 1 MiB: that run is refused)
        reads = reads[:3]
        exp = {k: v for k, v in exp.items() if k[1] < 3}
    b = _run(ctx, refs, reads, (2, -3, -1, -2), **dict([opt]))
    if opt[0] == "cell_cap":
        assert any(len(want[2]) > 1 for want in exp.values()) and b.timing().rerun_pairs >= 1
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    for (r, q), want in exp.items():
        pair = r * len(reads) + q
        assert b.score(pair) == want[0], (r, q)
        if opt[0] == "cigar":
            got = b.cigars(pair)
            assert len(got) == len(want[1]) >= 1
            for x, ((begin, (ra, qa)), cell) in enumerate(zip(want[1], want[2])):
                ent, nm = cr.cigar(ra, qa, opt[1])
                assert got[x] == (begin, cell[0], cell[1], ent, nm), (r, q, x)
                assert b.span(pair, x) == ov.span(cell, want[1][x])
        elif opt[0] != "scores_only":
            u.check_pair(b, pair, want, FIT, (r, q))
    if opt[0] == "scores_only":
        assert [b.ref_total(r) for r in range(len(refs))] == [sum(exp[(r, q)][0] for q in range(len(reads))) for r in range(len(refs))]
    b.free()


def test_pair_lists_and_set_pairs(ctx):
    """a plus pair, a minus pair (overlaps between reads of opposite strands) and a reversed pair, then another list on the batch"""
    rng = random.Random(8809)
    a = u.rand(rng, 500)
    other = sw.revcomp(a[300:] + u.rand(rng, 260))                 # the continuation of `a`, read from the other strand
    refs, reads = [a], [a[350:] + u.rand(rng, 200), other]
    specs = [(0, 0), (0, 1, 0, None, 0, None, False, "-"), (0, 0, 100, 400, 0, 300, True), (0, 1, 50, 450, 100, 360, True, "-")]
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("align_mode", FIT)
    ctx.set_option("overlap", 1)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    try:
        assert b.pipeline_mode() == 3

        def check_all():
            for k in range(b.n_pairs()):
                ref, read = b.segments(k)
                u.check_pair(b, k, _want(ref, read, SC), FIT, (k, b.spec(k)))
        check_all()
        assert b.strand(1) == "-" and b.score(1) == 5 * 200 and b.span(1, 0) == (1, 200, 301, 500)      # the dovetail across strands
        assert b.score(0) == 5 * 150 and b.span(0, 0) == (1, 150, 351, 500)
        b.set_pairs([(0, 1, 100, 400, 0, 300, False, "-"), (0, 0, 0, 420, 0, None)]).run(sw.make_params(SC[:3]))
        assert b.n_pairs() == 2
        check_all()
    finally:
        b.free()


def test_stream_and_two_batches_in_flight(ctx):
    refs, reads, exp = _variants()
    refs, reads = refs[:3], reads[:3]
    sc = (2, -3, -1, -2)
    p = sw.make_params(sc[:3])
    fit = {k: gr.align_numpy(refs[k[0]], reads[k[1]], sc, FIT) for k in exp if k[0] < 3 and k[1] < 3}
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("align_mode", FIT)
    ctx.set_option("long_reads", 1)
    # the option travels with the run: what is set behind the call does not reach the run in flight
    for value in (1, 0):
        ctx.set_option("overlap", value)
        ctx.set_option("debug_async_delay_us", 50000)
        b = ctx.upload(refs, reads).run_async(p)
        ctx.set_option("overlap", 1 - value)
        b2 = ctx.upload(refs, reads).run(p)                        # a second batch meanwhile, under the other value
        b.wait()
        ctx.set_option("debug_async_delay_us", 0)
        for (r, q) in fit:
            pair = r * len(reads) + q
            assert (b.score(pair), b.alignments(pair)) == (exp[(r, q)][:2] if value else fit[(r, q)]), (value, r, q)
            assert (b2.score(pair), b2.alignments(pair)) == (fit[(r, q)] if value else exp[(r, q)][:2]), (value, r, q)
        b.free()
        b2.free()
    ctx.set_option("overlap", 1)
    st = ctx.stream(reads, p, slots=2, chunk_bytes=1 << 10)
    ctx.set_option("overlap", 0)                                  # (the slots copied it at the open)
    st.push(refs[:2]).push(refs[2:]).finish()
    assert [int(t) for t in st.totals()] == [sum(exp[(r, q)][0] for q in range(len(reads))) for r in range(len(refs))]
    n_chunks = 0
    for first, c in st.chunks():
        n_chunks += 1
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            for q in range(len(reads)):
                u.check_pair(c, r * len(reads) + q, exp[(first + r, q)], FIT, (first + r, q))
    assert n_chunks >= 2
    st.close()


# 9 -- overlap = 0 is fit
def test_overlap_0_is_fit(ctx):
    """the plan and the prep caches key on the option: fit before and after an overlap run of the same batch"""
    refs, reads, exp = _variants()
    sc = (2, -3, -1, -2)
    fit = {k: gr.align_numpy(refs[k[0]], reads[k[1]], sc, FIT, cells=True) for k in exp}
    assert sum(fit[k] != exp[k] for k in exp) >= 8                # (a read the reference contains is the same under both)
    b = _run(ctx, refs, reads, sc, overlap=0)
    p = sw.make_params(sc[:3])
    for value in (0, 1, 0):
        ctx.set_option("overlap", value)
        b.run(p)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, exp if value else fit, FIT)
    b.free()
    # gap_open = 0: the run takes the affine kernels all the same
    sc0 = (2, -3, -2, 0)
    b = _run(ctx, refs[:2], reads[:2], sc0)
    u.check(b, refs[:2], reads[:2], _expect(refs[:2], reads[:2], sc0), FIT)
    b.free()


# 10 -- refusals
def _refused(b, params, *words):
    with pytest.raises(_capi.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED
    assert all(w in str(e.value) for w in words), str(e.value)


def test_invalid_values_leave_the_context(ctx):
    sc = (1, -3, -1, 0)
    want = _want("ACGAC", "ACT", sc)
    fit = gr.align_numpy("ACGAC", "ACT", sc, FIT)
    assert want[:2] != fit
    for start in (1, 0):
        b = _run(ctx, ["ACGAC"], ["ACT"], sc, overlap=start)
        for bad in (2, -1, 1 << 40):
            with pytest.raises(_capi.SwmiError) as e:
                ctx.set_option("overlap", bad)
            assert e.value.code == ERR_INVALID
        b.run(sw.make_params(sc[:3]))                             # the next run is still what it was
        assert (b.score(0), b.alignments(0)) == (want[:2] if start else fit)
        b.free()
    with pytest.raises(_capi.SwmiError) as e:
        ctx.set_option("align_mode", 3)                           # no fourth align_mode: overlap is an option of fit
    assert e.value.code == ERR_INVALID


@pytest.mark.parametrize("option", [("align_mode", sw.ALIGN_LOCAL), ("align_mode", sw.ALIGN_GLOBAL), ("band", 64), ("extend", 1), ("xdrop", 50),
                                    ("band_adapt", 1), ("gap_open2", -12), ("subopt", 5), ("hits", 3), ("end_bonus", 7)])
def test_refused_combinations(ctx, option):
    rng = random.Random(8810)
    ref, read = u.rand(rng, 200), u.rand(rng, 80)
    p = sw.make_params(SC[:3])
    for gap_open in (SC[3], 0):                                   # (0: the linear pipeline refuses it too)
        ctx.set_option("gap_open", gap_open)
        ctx.set_option("align_mode", FIT)
        ctx.set_option("long_reads", 1)
        ctx.set_option("overlap", 1)
        ctx.set_option(*option)
        b = ctx.upload([ref], [read])
        _refused(b, p, "overlap = 1", "%s" % option[0], "%d" % option[1])
        assert b.timing().fill_launches == 0                      # nothing was launched
        ctx.set_option(option[0], FIT if option[0] == "align_mode" else 0)      # the batch is still usable
        b.run(p)
        u.check_pair(b, 0, _want(ref, read, (SC[0], SC[1], SC[2], gap_open)), FIT)
        b.free()
