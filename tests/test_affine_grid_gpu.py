"""The affine kernels (swmi_affine.hip) against the restatements of the contract: every rows-per-lane class of every narrow and wide
sweep, and every kernel of the two lists AFF_SWEEPS and AFF_TRACEBACKS.

What the module guarantees, and tests/test_affine_grid_cpu.py enforces without a GPU:
  * every (R, mode, matrix, tie order) body of the local, fit and global sweeps is run by test_grid_shapes and test_grid_walks, and
    every (R, matrix, tie order) body of the subopt, hits and end_bonus sweeps by test_grid_subopt, test_grid_hits and
    test_grid_end_bonus -- 192 + 192 bodies (test_gpu_module_reaches_every_body); option "extend" has its grid in
    tests/test_extend_gpu.py and the two-piece sweeps theirs in tests/test_twopiece_gpu.py::test_rows_per_lane_classes;
  * every listed kernel is launched by test_census, in both tie orders, on inputs that make its own rule matter, and everything
    the run returns is compared: tests/affine_census.py derives the list from the launchers' own selection, so a kernel added to
    a list without an admitted run and an input recipe fails test_census_is_the_kernel_lists, which names it.

Each narrow and wide sweep kernel holds one body per (R, tie order).  All comparisons are exact: score, flags, number and order of
the alignments, every begin, both strings and the maximum cell, the MapRef view, and each option's own values."""
import pytest

import sparksmithwaterman_amd as sw

import affine_census as ac
import affine_gpu_util as u
import affine_grid_cases as gc
import end_bonus_reference as er
import gotoh_reference as gr
import hits_reference as hr
import subopt_reference as sr

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -5                         # swmi_status (include/swmi.h)

MODES = (0, 1, 2)                            # local, fit, global
MATRIX = (False, True)
TIES = (0, 1)
# (mode, matrix, tie) of test_grid_shapes and test_grid_walks; every case runs all 16 classes of gc.RS
GRID_PARAMS = [(mode, matrix, tie) for mode in MODES for matrix in MATRIX for tie in TIES]
MIXED_PARAMS = [(mode, matrix) for mode in (1, 2) for matrix in MATRIX]
OPTION_PARAMS = [(matrix, tie) for matrix in MATRIX for tie in TIES]                   # test_grid_subopt, test_grid_hits
ENDB_PARAMS = [(R, matrix, tie) for R in gc.RS for matrix in MATRIX for tie in TIES]   # test_grid_end_bonus
CENSUS_PARAMS = [(e.sweep, tie) for e in ac.census() for tie in TIES]                  # test_census


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _matrix(matrix):
    return gc.score_matrix() if matrix else None


def _results(b, n_pairs):
    """what the batch holds for every pair: (score, (count, flags), alignments or None where the pair is degenerate)"""
    out = []
    for pair in range(n_pairs):
        n, flags = b.n_alignments(pair)
        out.append((b.score(pair), (n, flags), None if flags & sw.PAIR_DEGENERATE else b.alignments(pair)))
    return out


# 1 -- the shape grid: three read lengths of every class against a reference of about 150 bases and one of 37.  The issue pairs
# the short reference with the 16 first-of-class reads only; all 48 cost about a second more of reference time, so one batch of
# 2 x 48 pairs is launched and all of it is checked.
@pytest.mark.parametrize("mode,matrix,tie", GRID_PARAMS)
def test_grid_shapes(ctx, mode, matrix, tie):
    refs, reads = gc.shape_grid(matrix)
    assert sorted({gc.rows_per_lane(len(q)) for q in reads}) == list(gc.RS)
    sc = gc.SHAPE_SCORES[matrix]
    exp = u.expect(refs, reads, sc, mode, tie=tie, matrix=_matrix(matrix))
    b = u.run(ctx, refs, reads, sc, tie, mode, matrix=_matrix(matrix))
    u.check(b, refs, reads, exp, mode)
    b.free()


# 2 -- the walk grid: a long alignment per class, with an insertion run that crosses lanes and a deletion run longer than one
# traceback tile.  The 16 pairs in one batch: a batch is the cross product of its references and reads, so the batch holds 256
# pairs and all of them are swept and walked, but the restatement (half a second for the longest pair) is computed for the 16
# matching ones only and those are checked in full, with the MapRef sites of their references that stem from them.
@pytest.mark.parametrize("mode,matrix,tie", GRID_PARAMS)
def test_grid_walks(ctx, mode, matrix, tie):
    grid = gc.walk_grid(matrix)
    assert [gc.rows_per_lane(len(read)) for _, _, read in grid] == list(gc.RS)
    refs = [ref for _, ref, _ in grid]
    reads = [read for _, _, read in grid]
    exp = [gr.align_numpy(ref, read, gc.WALK_SCORES, mode, tie_mode=tie, matrix=_matrix(matrix)) for _, ref, read in grid]
    first = None
    for device_strings in (1, 0):                                 # (the second run reuses the expected values)
        b = u.run(ctx, refs, reads, gc.WALK_SCORES, tie, mode, matrix=_matrix(matrix), device_strings=device_strings)
        for x, (es, ea) in enumerate(exp):
            pair = x * len(reads) + x
            assert b.score(pair) == es, (x + 1, b.score(pair), es)
            assert b.n_alignments(pair) == (len(ea), 0), x + 1
            assert b.alignments(pair) == ea, x + 1
            sites = b.ref_match_sites(x)
            assert sites == sorted(sites, key=lambda t: t[0]) and all(a in sites for a in ea), x + 1
        got = _results(b, len(refs) * len(reads))
        if first is None:
            first = got
        assert got == first                                       # every one of the 256 pairs: both string paths agree
        b.free()


# 3 -- narrow (R = 4), wide (R = 5) and strip pairs in one launch of the end-to-end modes: the launcher's choice of kernels by
# the launch's smallest and largest R, and the plan's partition of the long pairs to the back.  [1-True] is the first coverage of
# sw_affine_sweep_long_fit_matrix_kernel: no other test runs it.
@pytest.mark.parametrize("mode,matrix", MIXED_PARAMS)
def test_mixed_launch_fit_global(ctx, mode, matrix):
    refs, reads = gc.mixed_launch(matrix)
    sc = gc.SHAPE_SCORES[matrix]
    mat = _matrix(matrix)
    exp = u.expect(refs, reads, sc, mode, matrix=mat)
    seen = {}
    for subset in gc.MIXED_SUBSETS:
        sub = [reads[q] for q in subset]
        b = u.run(ctx, refs, sub, sc, 0, mode, w=0, matrix=_matrix(matrix), long_reads=1)
        u.check(b, refs, sub, {(r, x): exp[(r, q)] for r in range(len(refs)) for x, q in enumerate(subset)}, mode)
        got = _results(b, len(refs) * len(sub))
        for r in range(len(refs)):
            for x, q in enumerate(subset):                        # a pair's result is the same in every sub-batch it occurs in
                assert seen.setdefault((r, q), got[r * len(sub) + x]) == got[r * len(sub) + x], (subset, r, q)
        b.free()
    assert len(seen) == len(exp)
    # the three-read batch inside a band: the band applies to the read of more than 1024 bases only
    w = gc.MIXED_BAND
    for r in range(len(refs)):
        assert not gr.refused(len(reads[2]), len(refs[r]), w, mode)
        exp[(r, 2)] = gr.align_numpy(refs[r], reads[2], sc, mode, w, matrix=mat)
    b = u.run(ctx, refs, reads, sc, 0, mode, w=w, matrix=_matrix(matrix), long_reads=1)
    u.check(b, refs, reads, exp, mode)
    b.free()


# 4 -- the option grids.  subopt and hits run the shape grid in one launch of 96 pairs: every class of the SUBOPT and HITS sweeps,
# with the alignments checked as test_grid_shapes checks them -- each of those sweeps is an instantiation of its own that writes
# its own direction field and cell list.  The expected values are kept: the alignments per (matrix, tie order), the option's
# values per matrix (the tie order changes no H).
_KEPT = {}


def _kept(key, make):
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def _grid_expected(matrix, tie):
    refs, reads = gc.shape_grid(matrix)
    sc, mat = gc.SHAPE_SCORES[matrix], _matrix(matrix)
    pairs = [(r, q) for r in range(len(refs)) for q in range(len(reads))]
    exp = _kept(("align", matrix, tie), lambda: u.expect(refs, reads, sc, 0, tie=tie, matrix=mat))
    sub = _kept(("subopt", matrix), lambda: {(r, q): sr.subopt_numpy(refs[r], reads[q], sc, gc.GRID_SUBOPT, 0, mat) for r, q in pairs})
    return refs, reads, sc, exp, sub


def _check_subopts(b, n_reads, sub):
    s2, e2 = b.subopts()
    assert len(s2) == len(e2) == len(sub)
    for (r, q), want in sub.items():
        pair = r * n_reads + q
        got = (b.score(pair),) + b.subopt(pair)
        assert got == want, (r, q, got, want)
        assert (int(s2[pair]), int(e2[pair])) == want[1:], (r, q)


def _check_hits(b, n_reads, hits):
    cnt, sc, ei, ej = b.hits_all()
    assert len(cnt) == len(hits)
    for (r, q), want in hits.items():
        pair = r * n_reads + q
        assert b.hits(pair) == want, (r, q, b.hits(pair), want)
        assert int(cnt[pair]) == len(want), (r, q)
        assert [(int(sc[pair, x]), int(ei[pair, x]), int(ej[pair, x])) for x in range(len(want))] == want, (r, q)


@pytest.mark.parametrize("matrix,tie", OPTION_PARAMS)
def test_grid_subopt(ctx, matrix, tie):
    refs, reads, sc, exp, sub = _grid_expected(matrix, tie)
    b = u.run(ctx, refs, reads, sc, tie, 0, matrix=_matrix(matrix), subopt=gc.GRID_SUBOPT)
    u.check(b, refs, reads, exp, 0)
    _check_subopts(b, len(reads), sub)
    b.free()


@pytest.mark.parametrize("matrix,tie", OPTION_PARAMS)
def test_grid_hits(ctx, matrix, tie):
    refs, reads, sc, exp, sub = _grid_expected(matrix, tie)
    mat = _matrix(matrix)
    hits = _kept(("hits", matrix), lambda: {(r, q): hr.hits_numpy(refs[r], reads[q], sc, gc.GRID_SUBOPT, gc.GRID_HITS, 0, mat)
                                            for r in range(len(refs)) for q in range(len(reads))})
    b = u.run(ctx, refs, reads, sc, tie, 0, matrix=mat, subopt=gc.GRID_SUBOPT, hits=gc.GRID_HITS)
    u.check(b, refs, reads, exp, 0)
    _check_subopts(b, len(reads), sub)
    _check_hits(b, len(reads), hits)
    b.free()


def _check_end_bonus(b, refs, reads, exp, what):
    """every pair against end_bonus_reference.align: score, the three values through both accessors, the count with PAIR_TO_END,
    every alignment with its cell"""
    ends = b.end_scores()
    assert all(len(a) == len(refs) * len(reads) for a in ends)
    for r in range(len(refs)):
        for q in range(len(reads)):
            pair = r * len(reads) + q
            score, alns, cells, took, want_ends = exp[(r, q)]
            where = (what, r, q, len(refs[r]), len(reads[q]))
            assert b.score(pair) == score, (where, b.score(pair), score)
            assert b.end_score(pair) == want_ends, (where, b.end_score(pair), want_ends)
            assert tuple(int(a[pair]) for a in ends) == want_ends, where
            assert b.n_alignments(pair) == (len(alns), sw.PAIR_TO_END if took else 0), (where, b.n_alignments(pair), len(alns), took)
            assert b.alignments(pair, with_cell=True) == [a + (c,) for a, c in zip(alns, cells)], where


# the end_bonus grid: the three reads of class R against references that end before, between and behind their ends, under two
# bonuses (the restatement sweeps a pair once for both)
@pytest.mark.parametrize("R,matrix,tie", ENDB_PARAMS)
def test_grid_end_bonus(ctx, R, matrix, tie):
    refs, reads = gc.endb_grid(R, matrix)
    assert [gc.rows_per_lane(len(q)) for q in reads] == [R] * 3
    sc, mat = gc.SHAPE_SCORES[matrix], _matrix(matrix)
    for bonus in gc.ENDB_BONUSES:
        exp = {(r, q): er.align(refs[r], reads[q], sc, bonus, 0, tie, mat) for r in range(len(refs)) for q in range(len(reads))}
        b = u.run(ctx, refs, reads, sc, tie, sw.ALIGN_GLOBAL, 0, 1, matrix=mat, end_bonus=bonus)
        _check_end_bonus(b, refs, reads, exp, (R, matrix, tie, bonus))
        b.free()


# the banded matrix runs of subopt and hits: sw_affine_sweep_band_subopt_matrix_kernel and sw_affine_sweep_band_hits_matrix_kernel,
# which no other test of the per-feature modules launches
@pytest.mark.parametrize("tie", TIES)
def test_band_subopt_hits_matrix(ctx, tie):
    ref, read = gc.band_matrix_case()
    sc, mat = gc.SHAPE_SCORES[True], gc.score_matrix()
    w, width, k = gc.BAND_MATRIX_W, gc.BAND_MATRIX_SUBOPT, gc.BAND_MATRIX_HITS
    exp = {(0, 0): gr.align_numpy(ref, read, sc, 0, w, False, tie, mat, cells=True)}
    sub = _kept("band subopt", lambda: {(0, 0): sr.subopt_numpy(ref, read, sc, width, w, mat)})
    hits = _kept("band hits", lambda: {(0, 0): hr.hits_numpy(ref, read, sc, width, k, w, mat)})
    for n_hits in (0, k):
        b = u.run(ctx, [ref], [read], sc, tie, 0, w, matrix=mat, long_reads=1, subopt=width, hits=n_hits)
        u.check(b, [ref], [read], exp, 0)
        _check_subopts(b, 1, sub)
        if n_hits:
            _check_hits(b, 1, hits)
        assert [b.band_window(0, s) for s in range(2)] == gr.windows(len(read), len(ref), w)
        b.free()


# 5 -- the census: every kernel of AFF_SWEEPS is launched on two pairs that make its own rule matter, and with it the traceback it
# implies -- all of AFF_TRACEBACKS.  tests/test_affine_grid_cpu.py checks that the census is the two lists and that the options and
# read lengths of ac.inputs() select the kernel the case is named after
@pytest.mark.parametrize("kernel,tie", CENSUS_PARAMS, ids=["%s-%d" % p for p in CENSUS_PARAMS])
def test_census(ctx, kernel, tie):
    entry = next(e for e in ac.census() if e.sweep == kernel)
    inp = ac.inputs(entry)
    exp = ac.expected(entry, tie)
    b = u.run(ctx, inp.refs, inp.reads, inp.scores, tie, inp.mode, inp.band, inp.extend, inp.matrix, **inp.options)
    assert b.pipeline_mode() == 3
    for pair, ((ref, read), e) in enumerate(zip(ac.pairs(inp), exp)):
        what = (kernel, tie, pair)
        score, alns, cells = e["align"]
        assert b.score(pair) == score, (what, b.score(pair), score)
        assert b.n_alignments(pair) == (len(alns), sw.PAIR_TO_END if e.get("taken") else 0), (what, b.n_alignments(pair), len(alns))
        assert b.alignments(pair, with_cell=True) == [a + (c,) for a, c in zip(alns, cells)], what
        assert b.rows_swept(pair) == e["rows_swept"], (what, b.rows_swept(pair), e["rows_swept"])
        assert [b.band_window(pair, s) for s in range(len(e["windows"]))] == [tuple(x) for x in e["windows"]], what
        if "subopt" in e:
            assert (b.score(pair),) + b.subopt(pair) == e["subopt"], (what, b.subopt(pair), e["subopt"])
        if "hits" in e:
            assert b.hits(pair) == e["hits"], (what, b.hits(pair), e["hits"])
        if "ends" in e:
            assert b.end_score(pair) == e["ends"], (what, b.end_score(pair), e["ends"])
    b.free()


# 6 -- the JNI shim's entry points from plain C99 (tests/c/shim_long.c)
def _lcg(n, x):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def test_c99_shim_sets_long_reads_and_band(tmp_path):
    out = u.run_shim(tmp_path, "shim_long")
    read = _lcg(1025, 20260)
    ref = _lcg(300, 4242) + read
    sc = (5, -3, -2, -6)

    def line(res):
        s, al = res
        sites = sorted(al, key=lambda t: t[0])
        return " ".join([str(s), str(len(sites))] + ["%d:%s/%s" % (a[0], a[1][0], a[1][1]) for a in sites] + ["mode", "3"])

    full = gr.align_numpy(ref, read, sc)
    banded = gr.align_numpy(ref, read, sc, 0, 16)
    assert full[0] == 5 * 1025 and 0 < banded[0] < full[0]        # the band cuts the read's diagonal
    refused = "refused %d" % ERR_UNSUPPORTED
    assert out.splitlines() == [refused, line(full), line(banded), refused]
