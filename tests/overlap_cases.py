"""Inputs of the overlap (option "overlap") tests that go beyond planted exact copies, shared by
tests/test_overlap_cpu.py and tests/test_overlap_gpu.py -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Everything is deterministic (fixed seeds).  What a recipe is built for is asserted on
tests/overlap_reference.py alone, by the function of the same name with `check_` in front; tests/test_overlap_cpu.py calls every
one of them, and none of them sees what a GPU returned.  want() keeps the restatement's result of a pair, so that the tests of one
process sweep a pair once.

  walk_pairs      the walk grid of tests/affine_grid_cases.py cut so that all four ends are free: gap runs longer than a lane's
                  rows and than one traceback tile, in an alignment that ends on row m left of column n and starts at column 0
  tie_sets        small alphabets, scores down to 0 and mismatches dearer than a gap: direction ties, many tied maximum cells,
                  alignments that start with a gap (the E(i,0) := o and F(0,j) := o stand-ins)
  seam_cases      reads of more than 1024 bases: a first aligned row 1025 and 2049 at column 1 (the diagonal H(1024 sx, 0) of a
                  strip's first row), a gap run across row 1024, a walk across two seams
  long_tie_case   tied maxima on column n of strip 0, column n of strip 1 and row m at once, more than any cell_cap of the tests
  bound_cases     |score| = 2^20 on a read of 1024 bases, and the M * S <= 2^30 rule of long reads from both sides"""
import random

import affine_grid_cases as gc
import gotoh_reference as gr
import limit_cases as lc
import overlap_reference as ov

GAP = gr.GAP_CHAR
SC = (5, -3, -2, -6)                            # the scores of tests/test_overlap_gpu.py
CUT_REF_HEAD, CUT_READ_TAIL = 7, 9

_WANT = {}


def want(ref, read, sc, tie=0, matrix=None):
    """overlap_reference.align_numpy(..., cells=True), computed once per pair, scores, tie mode and matrix"""
    key = (ref, read, tuple(sc), tie, None if matrix is None else (matrix[0], tuple(map(tuple, matrix[1]))))
    if key not in _WANT:
        _WANT[key] = ov.align_numpy(ref, read, sc, ov.FIT, 0, False, tie, matrix, cells=True)
    return _WANT[key]


def starts_with_a_gap(alignment):
    return alignment[1][0][:1] == GAP or alignment[1][1][:1] == GAP


def gap_rows(alignment, cell):
    """the runs of inserted read bases of an alignment that ends at `cell`, as (first row, last row)"""
    ra, qa = alignment[1]
    i = cell[0] - sum(c != GAP for c in qa)
    runs, start = [], None
    for r, q in zip(ra, qa):
        if q != GAP:
            i += 1
        if r == GAP and start is None:
            start = i
        if r != GAP and start is not None:
            runs.append((start, i - (q != GAP)))
            start = None
    if start is not None:
        runs.append((start, i))
    return runs


# ---- 1 -- gap runs ---------------------------------------------------------------------------------------------------
def matrix_of(matrix):
    return gc.score_matrix() if matrix else None


def walk_pairs(matrix=False):
    """[(R, ref, read)]: the walk grid's 16 pairs, the reference without its first 7 bases and the read without its last 9"""
    return [(R, ref[CUT_REF_HEAD:], read[:-CUT_READ_TAIL]) for R, ref, read in gc.walk_grid(matrix)]


def check_walk_pairs(matrix, tie):
    differ = 0
    for (R, ref, read), (_, whole_ref, whole_read) in zip(walk_pairs(matrix), gc.walk_grid(matrix)):
        m, ins, dele = gc.walk_plan(R)
        assert len(read) == m - CUT_READ_TAIL and gc.rows_per_lane(len(read)) == R
        score, alns, cells = want(ref, read, gc.WALK_SCORES, tie, matrix_of(matrix))
        differ += (score, alns) != gr.align_numpy(ref, read, gc.WALK_SCORES, gr.FIT, tie_mode=tie, matrix=matrix_of(matrix))
        assert len(alns) >= 1
        for aln, cell in zip(alns, cells):
            assert gc.longest_run(aln[1][0], GAP) >= ins and gc.longest_run(aln[1][1], GAP) >= dele, (R, tie)
            assert cell[0] == len(read) and cell[1] < len(ref), (R, tie)                            # on row m, left of the corner
            first, _, begin, _ = ov.span(cell, aln)
            assert begin == 1 and first > 1, (R, tie)
        # the uncut pair: the corner cell, with both runs
        score, alns, cells = want(whole_ref, whole_read, gc.WALK_SCORES, tie, matrix_of(matrix))
        assert cells == [(m, len(whole_ref))], (R, tie)
        assert gc.longest_run(alns[0][1][0], GAP) >= ins and gc.longest_run(alns[0][1][1], GAP) >= dele, (R, tie)
    return differ


# ---- 2 -- tie-heavy random pairs -------------------------------------------------------------------------------------------
TIE_SETS = (((1, -1, -1, 0), "AC"), ((3, 1, 0, -2), "A"), ((0, -2, -2, 0), "ACGTacgtN\xe9"), ((2, -1, -1, -1), "AC"),
            ((2, -9, -1, -1), "ACGT"), ((2, -9, -1, 0), "AC"))
TIE_CELL_CAP = 8
_TIES = []


def tie_sets():
    """[(scores, refs, reads)], 8 x 8 pairs each"""
    if not _TIES:
        rng = random.Random(8811)
        for sc, alpha in TIE_SETS:
            refs = [gc.rand_seq(rng, rng.randint(1, 90), alpha) for _ in range(6)] + ["AC" * 75, "CACC"]
            reads = [gc.rand_seq(rng, rng.randint(1, 130), alpha) for _ in range(6)] + ["CA" * 40, "A"]
            _TIES.append((sc, refs, reads))
    return _TIES


def tie_counts():
    """per set, over both tie modes: (pairs with more than TIE_CELL_CAP tied cells, alignments that start with a gap, the largest
    score)"""
    out = []
    for sc, refs, reads in tie_sets():
        got = [want(ref, read, sc, tie) for tie in (0, 1) for ref in refs for read in reads]
        out.append((sum(len(g[2]) > TIE_CELL_CAP for g in got), sum(starts_with_a_gap(a) for g in got for a in g[1]), max(g[0] for g in got)))
    return out


def check_tie_sets():
    counts = tie_counts()
    assert all(c[0] >= 10 for c in counts), counts
    assert counts[2][1] >= 20 and counts[4][1] >= 20, counts      # sets 3 and 5
    assert counts[2][2] <= 0, counts
    return counts


# ---- 3, 4 -- long reads: seams -------------------------------------------------------------------------------------------
_SEAMS = []


def seam_cases():
    """[(name, ref, read, scores, span)]: span is (read_first, end_i, begin, end_j) of the one alignment"""
    if not _SEAMS:
        rng = random.Random(8813)
        X = gc.rand_seq(rng, 300, "CG")
        _SEAMS.append(("column 0 at row 1025", X, "A" * 1024 + X + "A" * 40, SC, (1025, 1324, 1, 300)))
        _SEAMS.append(("column 0 at row 2049", X, "A" * 2048 + X + "A" * 40, SC, (2049, 2348, 1, 300)))
        rng = random.Random(8814)
        X = gc.rand_seq(rng, 1400)
        read = gc.rand_seq(rng, 30) + X[:980] + gc.rand_seq(rng, 40) + X[980:]
        ref = X[:700] + gc.rand_seq(rng, 30) + X[700:] + gc.rand_seq(rng, 50)
        assert len(read) == 1470 and len(ref) == 1480
        _SEAMS.append(("a run across the seam", ref, read, gc.WALK_SCORES, (31, 1470, 1, 1430)))
        rng = random.Random(8812)
        ref = gc.rand_seq(rng, 2400)
        read = gc.mutate(rng, ref[150:2280], "ACGT", 0.04, 0.004)[:2100]
        assert len(read) == 2100
        _SEAMS.append(("two seams", ref, read, SC, None))
    return _SEAMS


def check_seam_cases(tie):
    for name, ref, read, sc, span in seam_cases():
        score, alns, cells = want(ref, read, sc, tie)
        assert len(cells) == 1, (name, cells)
        if span is not None:
            assert ov.span(cells[0], alns[0]) == span and cells[0] == (span[1], span[3]), (name, cells)
        if name.startswith("column 0"):
            assert score == 300 * sc[0] and alns[0][1][0] == alns[0][1][1] == ref
        elif name == "a run across the seam":
            assert cells[0][0] == len(read)
            runs = gap_rows(alns[0], cells[0])
            assert any(b - a + 1 == 40 and a <= 1024 and b >= 1025 for a, b in runs), runs
            assert gc.longest_run(alns[0][1][1], GAP) == 30
        else:
            assert cells[0][0] == 2100 == len(read) and len(alns[0][1][0]) > 2048
            assert ov.span(cells[0], alns[0])[0] == 1             # the walk starts in strip 0 and ends in strip 2


# ---- 4 -- long reads: tied maxima in both strips and on row m --------------------------------------------------------
LONG_TIE_SCORES = (0, -3, -1, -3)


def long_tie_case():
    """(ref, read): n = 300, m = 1120"""
    return "AC" * 150, "AC" * 560


def check_long_tie_case(tie):
    ref, read = long_tie_case()
    score, alns, cells = want(ref, read, LONG_TIE_SCORES, tie)
    assert score == 0 and len(cells) == len(set(cells)) == 709
    assert sum(c[1] == 300 and c[0] <= 1024 for c in cells) == 512
    assert sum(c[1] == 300 and 1024 < c[0] < 1120 for c in cells) == 47
    assert sum(c[0] == 1120 for c in cells) == 150


# ---- 5 -- arithmetic bounds ----------------------------------------------------------------------------------------
L = lc.L
LONG_S_OK, LONG_S_REFUSED = 349525, 349526                           # 3072 rows: 3072 * 349525 <= 2^30 < 3072 * 349526
assert 3072 * LONG_S_OK <= 1 << 30 < 3072 * LONG_S_REFUSED
_BOUNDS = {}


def _bound_read():
    if not _BOUNDS:
        rng = random.Random(8815)
        read = gc.rand_seq(rng, 1024, "AC")
        _BOUNDS.update(read=read, ref=gc.rand_seq(rng, 50, "AC") + read[400:], long_read=gc.rand_seq(rng, 2049, "AC"),
                       sides=(gc.rand_seq(rng, 60, "AC"), gc.rand_seq(rng, 70, "AC")))
    return _BOUNDS


def bound_cases():
    """[(name, ref, read, scores)] with every score at its bound.  The pair "2^30, two strips" has a read of 1029 bases: the
    restatement scores it, the library refuses it (2048 rows * 2^20 > 2^30), so "2^30" is the same run of 1024 matches with the
    read of 1024 bases itself, which the library takes: H reaches 2^30 there, at cell (1024, 1029)."""
    b = _bound_read()
    cases = [("bound %s" % lc.score_id(sc), b["ref"], b["read"], sc) for sc in lc.AFFINE_BOUND_SCORES]
    sc = (L, -L, -L, -L)
    cases.append(("2^30, two strips", b["read"] + "C" * 10, "G" * 5 + b["read"], sc))
    cases.append(("2^30", "G" * 5 + b["read"] + "C" * 10, b["read"], sc))
    cases.append(("-2^20", "G" * 700, "C" * 1024, sc))
    return cases


def long_bound_cases():
    """[(name, ref, read)] under (S, -S, -S, -S): reads of 2049 bases, 3072 swept rows"""
    b = _bound_read()
    return [("read inside", b["sides"][0] + b["long_read"] + b["sides"][1], b["long_read"]), ("no match", "G" * 400, "C" * 2049)]


def check_bound_cases():
    tied = []
    for name, ref, read, sc in bound_cases():
        for tie in (0, 1):
            score, alns, cells = want(ref, read, sc, tie)
            assert -(1 << 31) <= score < (1 << 31), name
            tied.append(len(cells))
            if name.startswith("2^30"):
                assert score == 1 << 30 and cells == ([(1029, 1024)] if len(read) == 1029 else [(1024, 1029)])
            if name == "-2^20":
                assert score == -L and len(cells) == 2
    assert max(tied[:8]) > 64, tied
    sc = (LONG_S_OK, -LONG_S_OK, -LONG_S_OK, -LONG_S_OK)
    (_, ref, read), (_, ref2, read2) = long_bound_cases()
    assert want(ref, read, sc)[0] == 2049 * LONG_S_OK < 1 << 30
    assert want(ref2, read2, sc)[0] == -LONG_S_OK
