"""Host-side checks of the rows-per-lane grid (tests/affine_grid_cases.py) and of the kernel census (tests/affine_census.py) that
need no GPU: the expected values of tests/test_affine_grid_gpu.py do not rest on one restatement, the cases are what they are
built for, the GPU module's parametrisation reaches every (rows per lane, mode, matrix, tie order) body of the sweeps and every
(rows per lane, matrix, tie order) body of the subopt, hits and end_bonus sweeps, and the census is the two kernel lists of
swmi_affine.hip, each kernel with inputs that select it."""
import itertools

import pytest

import affine_census as ac
import affine_grid_cases as gc
import end_bonus_reference as er
import gotoh_reference as gr
import hits_reference as hr
import subopt_reference as sr

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
    # the option grids: 3 x 16 x 2 x 2 = 192 bodies of the subopt, hits and end_bonus sweeps
    want = set(itertools.product(("subopt", "hits", "endb"), gc.RS, (False, True), (0, 1)))
    assert len(want) == 192
    got = set()
    for what, fn in (("subopt", tg.test_grid_subopt), ("hits", tg.test_grid_hits)):
        names, cases = _parametrize(fn)
        assert names == "matrix,tie" and len(cases) == len(set(cases)) == 4
        got |= {(what, gc.rows_per_lane(len(q)), matrix, tie) for matrix, tie in cases for q in gc.shape_grid(matrix)[1]}
    names, cases = _parametrize(tg.test_grid_end_bonus)
    assert names == "R,matrix,tie" and len(cases) == len(set(cases)) == 64
    for R, matrix, tie in cases:
        classes = {gc.rows_per_lane(len(q)) for q in gc.endb_grid(R, matrix)[1]}
        assert classes == {R}
        got.add(("endb", R, matrix, tie))
    assert got == want
    names, cases = _parametrize(tg.test_band_subopt_hits_matrix)
    assert names == "tie" and sorted(cases) == [0, 1]
    # the census times both tie orders
    names, cases = _parametrize(tg.test_census)
    assert names == "kernel,tie" and len(cases) == len(set(cases)) == 144
    assert sorted(cases) == sorted((e.sweep, tie) for e in ac.census() for tie in (0, 1))
    names, cases = _parametrize(tg.test_mixed_launch_fit_global)
    assert names == "mode,matrix" and sorted(cases) == sorted(itertools.product((1, 2), (False, True)))
    assert any(m.name == "gpu" for m in (tg.pytestmark if isinstance(tg.pytestmark, list) else [tg.pytestmark]))


# 6 -- the option grids are what they are built for
_OPTION_GRID = {}


def _option_grid(matrix):
    """{(r, q): (subopt, hits)} of the shape grid under the options of test_grid_subopt and test_grid_hits"""
    if matrix not in _OPTION_GRID:
        refs, reads = gc.shape_grid(matrix)
        sc, mat = gc.SHAPE_SCORES[matrix], gc.score_matrix() if matrix else None
        _OPTION_GRID[matrix] = {(r, q): (sr.subopt_numpy(refs[r], reads[q], sc, gc.GRID_SUBOPT, 0, mat),
                                         hr.hits_numpy(refs[r], reads[q], sc, gc.GRID_SUBOPT, gc.GRID_HITS, 0, mat))
                                for r in range(len(refs)) for q in range(len(reads))}
    return _OPTION_GRID[matrix]


@pytest.mark.parametrize("matrix", [False, True])
def test_option_grid_has_a_runner_up_and_hits_in_every_class(matrix):
    """every class R has a pair with score2 > 0, one with two hits or more whose rows differ, and for R >= 3 a hit whose row lies in
    a slot strictly between 0 and R - 1: the rows the sweeps' row carry gets wrong where it is wrong"""
    reads = gc.shape_grid(matrix)[1]
    grid = _option_grid(matrix)
    for R in gc.RS:
        mine = [v for (r, q), v in grid.items() if gc.rows_per_lane(len(reads[q])) == R]
        assert len(mine) == 6
        assert any(sub[1] > 0 for sub, _ in mine), R
        assert any(len({h[1] for h in hits}) >= 2 for _, hits in mine), R
        if R >= 3:
            assert any(0 < gc.row_slot(h[1], R) < R - 1 for _, hits in mine for h in hits), R
    assert sum(sub[1] > 0 for sub, _ in grid.values()) >= 90 and sum(len(hits) >= 2 for _, hits in grid.values()) >= 90
    assert len({h[1] for _, hits in grid.values() for h in hits}) > 250
    for sub, hits in grid.values():                               # entry 1 is the runner-up
        assert (hits[1][0], hits[1][2]) == sub[1:] if len(hits) >= 2 else sub[1:] == (0, 0)


@pytest.mark.parametrize("matrix", [False, True])
def test_option_grid_sample_scalar_and_numpy_agree(matrix):
    """the first-of-class reads against the 37-base reference, the tie order alternating with the class"""
    refs, reads = gc.shape_grid(matrix)
    sc, mat = gc.SHAPE_SCORES[matrix], gc.score_matrix() if matrix else None
    grid = _option_grid(matrix)
    for q in gc.FIRST_OF_CLASS:
        tie = (q // 3) % 2
        assert sr.subopt_scalar(refs[1], reads[q], sc, gc.GRID_SUBOPT, 0, tie, mat) == grid[(1, q)][0], len(reads[q])
        assert hr.hits_scalar(refs[1], reads[q], sc, gc.GRID_SUBOPT, gc.GRID_HITS, 0, tie, mat) == grid[(1, q)][1], len(reads[q])


_ENDB_TOOK = {}


def _endb_took(R, matrix):
    """{bonus: [taken to the end, per pair]} of the end_bonus grid of class R"""
    if (R, matrix) not in _ENDB_TOOK:
        refs, reads = gc.endb_grid(R, matrix)
        sc, mat = gc.SHAPE_SCORES[matrix], gc.score_matrix() if matrix else None
        _ENDB_TOOK[(R, matrix)] = {b: [er.align(ref, read, sc, b, 0, 0, mat)[3] for ref in refs for read in reads] for b in gc.ENDB_BONUSES}
    return _ENDB_TOOK[(R, matrix)]


@pytest.mark.parametrize("matrix", [False, True])
@pytest.mark.parametrize("R", gc.RS)
def test_endb_grid_shows_both_outcomes(R, matrix):
    """over a class's 9 pairs and the two bonuses the restatement alone shows a pair taken to the end and one that is not, with
    bonuses far from the largest ones (which take every pair)"""
    refs, reads = gc.endb_grid(R, matrix)
    first, mid, last = gc.GRID_LENGTHS[3 * (R - 1):3 * R]
    assert [len(q) for q in reads] == [first, mid, last] and all(reads[2].startswith(q) for q in reads)
    assert len(refs) == 3 and len(refs[0]) <= first + 5 and mid < len(refs[1]) < last + 7 and len(refs[2]) > last
    assert set("".join(refs + reads)) <= set(gc.MATRIX_DRAW if matrix else gc.PLAIN_ALPHABET)
    assert len(gc.ENDB_BONUSES) == 2 and 0 < min(gc.ENDB_BONUSES) and max(gc.ENDB_BONUSES) < (1 << 30) - 2
    took = _endb_took(R, matrix)
    seen = [t for b in gc.ENDB_BONUSES for t in took[b]]
    assert len(seen) == 18 and True in seen and False in seen, (R, matrix, seen)
    if R >= 3:                                                    # (the middle read's row m lies in a middle slot)
        assert 0 < gc.row_slot(mid, R) < R - 1


def test_endb_grid_bonus_decides_somewhere():
    """the two bonuses differ in what they take: in 10 classes or more of either grid a pair is taken under one and not the other"""
    for matrix in (False, True):
        assert sum(_endb_took(R, matrix)[gc.ENDB_BONUSES[0]] != _endb_took(R, matrix)[gc.ENDB_BONUSES[1]] for R in gc.RS) >= 10, matrix


@pytest.mark.parametrize("R", (3, 7, 12))
def test_endb_grid_sample_scalar_and_numpy_agree(R):
    """the shortest read of three classes against the three references, with the matrix, both bonuses, the tie order alternating"""
    refs, reads = gc.endb_grid(R, True)
    for x, ref in enumerate(refs):
        for b in gc.ENDB_BONUSES:
            args = (ref, reads[0], gc.SHAPE_SCORES[True], b, 0, (R + x) % 2, gc.score_matrix())
            assert er.align(*args) == er.align_scalar(*args), (R, x, b)


def test_band_matrix_case():
    """a read of two strips with 76 rows in the second; under the band 8 hits with rows on both sides of row 1024, and a runner-up"""
    ref, read = gc.band_matrix_case()
    sc, mat, w = gc.SHAPE_SCORES[True], gc.score_matrix(), gc.BAND_MATRIX_W
    assert len(read) == 1100 and len(read) - 1024 == 76 and set(ref + read) == set(gc.MATRIX_DRAW)
    assert not gr.refused(len(read), len(ref), w, gr.LOCAL) and len(gr.windows(len(read), len(ref), w)) == 2
    hits = hr.hits_numpy(ref, read, sc, gc.BAND_MATRIX_SUBOPT, gc.BAND_MATRIX_HITS, w, mat)
    assert len(hits) == 8 and min(h[1] for h in hits) < 1024 < max(h[1] for h in hits)
    sub = sr.subopt_numpy(ref, read, sc, gc.BAND_MATRIX_SUBOPT, w, mat)
    assert sub[1] > 0 and (hits[1][0], hits[1][2]) == sub[1:] and hits[0][0] == sub[0]


# 7 -- the census (tests/affine_census.py): it is the two kernel lists, and every entry's inputs select its kernel
def test_census_is_the_kernel_lists():
    """the sweeps the launchers give over the option product are exactly the rows of AFF_SWEEPS, each once, and the tracebacks they
    imply exactly the rows of AFF_TRACEBACKS: a kernel added to a list with no admitted run, or a run whose kernel is not listed,
    fails here by name"""
    from test_affine_kernel_table_cpu import _listed
    listed_sweeps, listed_tracebacks = _listed("AFF_SWEEPS"), _listed("AFF_TRACEBACKS")
    entries = ac.census()
    sweeps = [e.sweep for e in entries]
    assert len(sweeps) == len(set(sweeps)) and len(listed_sweeps) == len(set(listed_sweeps)) and len(listed_tracebacks) == len(set(listed_tracebacks))
    assert not set(listed_sweeps) - set(sweeps), ("listed, but no run of the census gets it", sorted(set(listed_sweeps) - set(sweeps)))
    assert not set(sweeps) - set(listed_sweeps), ("a run gets it, but it is not listed", sorted(set(sweeps) - set(listed_sweeps)))
    tracebacks = {e.traceback for e in entries}
    assert not set(listed_tracebacks) - tracebacks, ("listed, but no entry of the census implies it", sorted(set(listed_tracebacks) - tracebacks))
    assert not tracebacks - set(listed_tracebacks), ("an entry implies it, but it is not listed", sorted(tracebacks - set(listed_tracebacks)))
    assert len(entries) == len(listed_sweeps) == 72 and len(tracebacks) == len(listed_tracebacks) == 13
    for e in entries:                                             # the entry is what the launchers say of its own point
        assert ac.names(ac.point_affrun(e.point), e.point["long_reads"], e.shape) == (e.sweep, e.traceback), e.sweep
        assert e.shape == 2 if e.point["long_reads"] else e.shape in (0, 1), e.sweep


@pytest.mark.parametrize("kernel", [e.sweep for e in ac.census()])
def test_census_inputs_select_the_kernel_and_make_its_rule_matter(kernel):
    """the kernel names of the options and read lengths that inputs() actually produces are the entry's -- what keeps test_census
    honest about which kernel it ran -- and the inputs have the properties their options need (affine_census.properties)"""
    entry = next(e for e in ac.census() if e.sweep == kernel)
    inp = ac.inputs(entry)
    assert len(ac.pairs(inp)) == 2
    long_reads, shape = ac.launch_of(inp)
    got = ac.names(ac.options_to_affrun(ac.run_options(inp), inp.matrix), long_reads, shape)
    assert got == (entry.sweep, entry.traceback), ("the inputs of %s launch" % kernel, got)
    assert (long_reads, shape) == (entry.point["long_reads"], entry.shape), kernel
    assert [gc.rows_per_lane(len(q)) for q in inp.reads if len(q) <= 1024] in ([], [(2, 5, 17)[shape]] * len(inp.reads)), kernel
    ac.properties(entry)


# one narrow, one wide and one long entry per restatement, where it has them (xdrop and band_adapt are the long shape's); the long
# ones with one of their two pairs, the plain loops taking seconds there
CENSUS_SAMPLE = [("sw_affine_sweep_fit_kernel", 0, None), ("sw_affine_sweep_global_matrix_wide_kernel", 1, None), ("sw_affine_sweep_band_kernel", 1, 0),
                 ("sw_affine_sweep_subopt_kernel", 1, None), ("sw_affine_sweep_hits_matrix_wide_kernel", 0, None), ("sw_affine_sweep_band_hits_matrix_kernel", 1, 0),
                 ("sw_affine_sweep_endb_kernel", 0, None), ("sw_affine_sweep_endb_matrix_wide_kernel", 1, None), ("sw_affine_sweep_band_endb_kernel", 1, 0),
                 ("sw_affine_sweep2_extend_kernel", 1, None), ("sw_affine_sweep2_global_wide_kernel", 0, None), ("sw_affine_sweep2_band_extend_kernel", 0, 1),
                 ("sw_affine_sweep_long_xdrop_kernel", 0, 0), ("sw_affine_sweep_band_xdrop_matrix_kernel", 1, 1),
                 ("sw_affine_sweep_band_adapt_matrix_kernel", 0, 0), ("sw_affine_sweep_band_adapt_xdrop_kernel", 1, 1)]


@pytest.mark.parametrize("kernel,tie,only", CENSUS_SAMPLE)
def test_census_sample_scalar_and_numpy_agree(kernel, tie, only):
    entry = next(e for e in ac.census() if e.sweep == kernel)
    fast, plain = ac.expected(entry, tie), ac.expected_scalar(entry, tie, only)
    assert len(fast) == len(plain) == 2
    for f, s in zip(fast, plain):
        if s is not None:
            assert s and {k: f[k] for k in s} == s, kernel
