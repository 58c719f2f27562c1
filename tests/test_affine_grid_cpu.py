"""Host-side checks of the rows-per-lane grid (tests/affine_grid_cases.py) that need no GPU: the expected values of
tests/test_affine_grid_gpu.py do not rest on one restatement, the cases are what they are built for, and the GPU module's
parametrisation reaches every (rows per lane, mode, matrix, tie order) body of the sweeps."""
import itertools

import pytest

import affine_grid_cases as gc
import gotoh_reference as gr

GAP = gr.GAP_CHAR
_NUMPY = {}


def _numpy(matrix, R, mode, tie):
    """the numpy restatement's result for the walk-grid pair of class R (computed once)"""
    key = (matrix, R, mode, tie)
    if key not in _NUMPY:
        _, ref, read = gc.walk_grid(matrix)[R - 1]
        _NUMPY[key] = gr.align_numpy(ref, read, gc.WALK_SCORES, mode, tie_mode=tie, matrix=gc.score_matrix() if matrix else None)
    return _NUMPY[key]


def _scalar(ref, read, sc, mode, tie, matrix=None):
    """the plain-loop restatement"""
    return gr.align_scalar(ref, read, sc, mode, tie_mode=tie, matrix=matrix)


def _walk_ties(R, mode):
    """both tie orders up to R = 8; above, where the plain loop takes seconds per pair, the tie order alternates with R and the
    mode, so that every mode meets both orders four times among R = 9 .. 16 and every R meets both"""
    return (0, 1) if R <= 8 else ((R + mode) % 2,)


def test_grid_lengths():
    assert [gc.rows_per_lane(m) for m in (0, 1, 64, 65, 1024, 1025)] == [1, 1, 1, 2, 16, 17]
    for R in gc.RS:
        lengths = [m for m in gc.GRID_LENGTHS if gc.rows_per_lane(m) == R]
        assert len(lengths) == 3 and lengths[0] == 64 * R - 63 and lengths[2] == 64 * R
        assert gc.row_slot(lengths[2], R) == R - 1
        if R >= 3:
            assert 0 < gc.row_slot(lengths[1], R) < R - 1
        assert gc.row_slot(gc.walk_plan(R)[0], R) == 0            # (the walk grid's row m: slot 0 in every class)
    for matrix in (False, True):
        refs, reads = gc.shape_grid(matrix)
        assert tuple(len(q) for q in reads) == gc.GRID_LENGTHS and [len(r) for r in refs] == [150, 37]
        draw = set(gc.MATRIX_DRAW if matrix else gc.PLAIN_ALPHABET)
        assert set("".join(refs + reads)) == draw
        assert [gc.rows_per_lane(len(read)) for _, _, read in gc.walk_grid(matrix)] == list(gc.RS)
    alphabet, rows = gc.score_matrix()
    assert alphabet == "ACGTN" and "X" not in alphabet
    assert any(rows[a][b] != rows[b][a] for a in range(5) for b in range(5))
    assert any(rows[a][b] > 0 for a in range(5) for b in range(5) if a != b)


# 1 -- the restatements agree
@pytest.mark.parametrize("R", gc.RS)
def test_walk_grid_scalar_and_numpy_agree(R):
    _, ref, read = gc.walk_grid(False)[R - 1]
    for mode in (0, 1, 2):
        for tie in _walk_ties(R, mode):
            assert _numpy(False, R, mode, tie) == _scalar(ref, read, gc.WALK_SCORES, mode, tie), (R, mode, tie)


def test_walk_grid_tie_orders_cover_every_mode_and_class():
    for mode in (0, 1, 2):
        assert sorted(t for R in range(9, 17) for t in _walk_ties(R, mode)) == [0] * 4 + [1] * 4
    for R in gc.RS:
        assert {t for mode in (0, 1, 2) for t in _walk_ties(R, mode)} == {0, 1}


@pytest.mark.parametrize("matrix", [False, True])
def test_shape_grid_sample_scalar_and_numpy_agree(matrix):
    """the first-of-class reads against the 37-base reference: every class in every mode; plain scores under both tie orders,
    with the matrix the tie order alternates with the class and the mode"""
    refs, reads = gc.shape_grid(matrix)
    mat = gc.score_matrix() if matrix else None
    sc = gc.SHAPE_SCORES[matrix]
    for q in gc.FIRST_OF_CLASS:
        for mode in (0, 1, 2):
            for tie in (((q // 3 + mode) % 2,) if matrix else (0, 1)):
                want = _scalar(refs[1], reads[q], sc, mode, tie, mat)
                assert gr.align_numpy(refs[1], reads[q], sc, mode, tie_mode=tie, matrix=mat) == want, (len(reads[q]), mode, tie)
                if mode == 2:
                    assert len(want[1]) == 1                      # global mode ends in the one cell (m, n)


# 2 -- the cases are what they are built for
@pytest.mark.parametrize("matrix", [False, True])
def test_walk_grid_holds_the_planted_runs(matrix):
    """fit and global: an insertion run and a deletion run of at least the planted lengths; local: at least 80 % of the read
    (plain scores under both tie orders, with the matrix under the serial one)"""
    for R in gc.RS:
        m, ins, dele = gc.walk_plan(R)
        _, ref, read = gc.walk_grid(matrix)[R - 1]
        assert len(read) == m and len(ref) == m - ins + dele <= m + 100
        for tie in ((0,) if matrix else (0, 1)):
            for mode in (1, 2):
                score, al = _numpy(matrix, R, mode, tie)
                for begin, (ra, qa) in al:
                    assert qa.replace(GAP, "") == read
                    assert gc.longest_run(ra, GAP) >= ins, (R, mode, tie)            # the reference side gaps: inserted read bases
                    assert gc.longest_run(qa, GAP) >= dele, (R, mode, tie)           # the read side gaps: deleted columns
            score, al = _numpy(matrix, R, 0, tie)
            assert score > 0 and al
            if R >= 3:
                for begin, (ra, qa) in al:
                    assert len(qa.replace(GAP, "")) * 5 >= 4 * m, (R, tie)
                    assert gc.longest_run(ra, GAP) >= ins and gc.longest_run(qa, GAP) >= dele, (R, tie)


def test_walk_grid_runs_cross_lanes_and_tiles():
    for R in gc.RS:
        m, ins, dele = gc.walk_plan(R)
        assert gc.rows_per_lane(m) == R and ins > R                          # the insertion run leaves its lane at least once
        if R >= 3:
            assert ins == 40 and ins > 16
        if R >= 6:
            blocks = gc.TILE_WORDS // (64 * R)                   # NB of the traceback: blocks of 8 steps in one tile
            assert dele == 8 * blocks + 8 > 8 * blocks
        elif R >= 3:
            assert dele == 24
    assert [gc.TILE_WORDS // (64 * R) for R in (7, 15)] == [9, 4]            # (the inexact divisions the issue names)


# 3 -- ties
@pytest.mark.parametrize("matrix", [False, True])
def test_shape_grid_has_tied_alignments(matrix):
    """local and fit: a pair of the shape grid with more than one alignment (global mode has the one cell (m, n): see above)"""
    refs, reads = gc.shape_grid(matrix)
    mat = gc.score_matrix() if matrix else None
    sc = gc.SHAPE_SCORES[matrix]
    for mode in (0, 1):
        for tie in (0, 1):
            assert any(len(gr.align_numpy(refs[0], reads[q], sc, mode, tie_mode=tie, matrix=mat)[1]) > 1 for q in range(len(reads))), (mode, tie)


# 4 -- the mixed launches
@pytest.mark.parametrize("matrix", [False, True])
def test_mixed_launch_cases(matrix):
    refs, reads = gc.mixed_launch(matrix)
    mat = gc.score_matrix() if matrix else None
    sc = gc.SHAPE_SCORES[matrix]
    assert [gc.rows_per_lane(len(q)) for q in reads[:2]] == [4, 5] and len(reads[2]) == 1025
    assert sorted(map(sorted, gc.MIXED_SUBSETS)) == sorted([[0, 2], [1, 2], [0, 1, 2], [2], [0, 1]])
    for mode in (1, 2):
        for r in range(2):
            assert not gr.refused(1025, len(refs[r]), gc.MIXED_BAND, mode)
        # the band bites: the banded result of the long read differs from the unbanded one
        assert gr.align_numpy(refs[0], reads[2], sc, mode, gc.MIXED_BAND, matrix=mat) != gr.align_numpy(refs[0], reads[2], sc, mode, matrix=mat)


# 5 -- coverage: every (R, mode, matrix, tie) body is reached by the GPU module's parametrisation (nothing is launched)
def _parametrize(fn):
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    assert len(marks) == 1
    return marks[0].args


def test_gpu_module_reaches_every_body():
    import test_affine_grid_gpu as tg
    want = set(itertools.product(gc.RS, (0, 1, 2), (False, True), (0, 1)))
    assert len(want) == 192
    for fn, grid in ((tg.test_grid_shapes, lambda matrix: [len(q) for q in gc.shape_grid(matrix)[1]]),
                     (tg.test_grid_walks, lambda matrix: [len(read) for _, _, read in gc.walk_grid(matrix)])):
        names, cases = _parametrize(fn)
        assert names == "mode,matrix,tie" and len(cases) == len(set(cases)) == 12
        got = {(gc.rows_per_lane(m), mode, matrix, tie) for mode, matrix, tie in cases for m in grid(matrix)}
        assert got == want
    names, cases = _parametrize(tg.test_mixed_launch_fit_global)
    assert names == "mode,matrix" and sorted(cases) == sorted(itertools.product((1, 2), (False, True)))
    assert any(m.name == "gpu" for m in (tg.pytestmark if isinstance(tg.pytestmark, list) else [tg.pytestmark]))
