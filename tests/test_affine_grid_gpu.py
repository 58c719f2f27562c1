"""Every rows-per-lane class of the affine kernels in every mode (swmi_affine.hip), against the restatements of the contract.

The 40 sweep kernels and 10 traceback kernels, and the tests that run them (G: this module; a new kernel goes into this table).
Between them the tests named on a row of the extend, xdrop and band_adapt kernels run both tie orders; a test that runs the
strict order is marked `strict:` where the others on the row run the serial one only:

  sweep kernel (sw_affine_sweep_...)    rows per lane     run by
  kernel                                1 .. 4            G test_grid_shapes[0-False-*], test_grid_walks[0-False-*]; test_affine_gpu.py
  wide_kernel                           5 .. 16           G test_grid_shapes[0-False-*], test_grid_walks[0-False-*]; test_affine_gpu.py
  long_kernel                           strips of 16      test_long_reads_gpu.py::test_long_reads_strip_counts_and_skew
  matrix_kernel                         1 .. 4            G test_grid_shapes[0-True-*], test_grid_walks[0-True-*]; test_matrix_gpu.py
  matrix_wide_kernel                    5 .. 16           G test_grid_shapes[0-True-*], test_grid_walks[0-True-*]; test_matrix_gpu.py
  long_matrix_kernel                    strips of 16      test_long_reads_gpu.py::test_long_reads_blosum62[0]
  fit_kernel                            1 .. 4            G test_grid_shapes[1-False-*], test_grid_walks[1-False-*]; test_ends_gpu.py
  fit_wide_kernel                       5 .. 16           G test_grid_shapes[1-False-*], test_grid_walks[1-False-*]; test_ends_gpu.py
  long_fit_kernel                       strips of 16      G test_mixed_launch_fit_global[1-False]; test_long_reads_gpu.py::test_long_reads_fit_and_global
  fit_matrix_kernel                     1 .. 4            G test_grid_shapes[1-True-*], test_grid_walks[1-True-*]
  fit_matrix_wide_kernel                5 .. 16           G test_grid_shapes[1-True-*], test_grid_walks[1-True-*]
  long_fit_matrix_kernel                strips of 16      G test_mixed_launch_fit_global[1-True] (no other test)
  global_kernel                         1 .. 4            G test_grid_shapes[2-False-*], test_grid_walks[2-False-*]; test_ends_gpu.py
  global_wide_kernel                    5 .. 16           G test_grid_shapes[2-False-*], test_grid_walks[2-False-*]; test_ends_gpu.py
  long_global_kernel                    strips of 16      G test_mixed_launch_fit_global[2-False]; test_long_reads_gpu.py::test_long_reads_fit_and_global
  global_matrix_kernel                  1 .. 4            G test_grid_shapes[2-True-*], test_grid_walks[2-True-*]
  global_matrix_wide_kernel             5 .. 16           G test_grid_shapes[2-True-*], test_grid_walks[2-True-*]
  long_global_matrix_kernel             strips of 16      G test_mixed_launch_fit_global[2-True]; test_long_reads_gpu.py::test_long_reads_blosum62[2]
  band_kernel                           strips of 16      test_band_gpu.py::test_band_shapes; G test_c99_shim_sets_long_reads_and_band
  band_matrix_kernel                    strips of 16      test_band_gpu.py::test_band_blosum62[0]
  band_fit_kernel                       strips of 16      G test_mixed_launch_fit_global[1-False]; test_band_gpu.py::test_band_shapes
  band_fit_matrix_kernel                strips of 16      G test_mixed_launch_fit_global[1-True]; test_band_gpu.py::test_band_64_symbol_matrix
  band_global_kernel                    strips of 16      G test_mixed_launch_fit_global[2-False]; test_band_gpu.py::test_band_shapes
  band_global_matrix_kernel             strips of 16      G test_mixed_launch_fit_global[2-True]; test_band_gpu.py::test_band_blosum62[2]
  (option "extend" on a global run: test_extend_gpu.py, E)
  extend_kernel                         1 .. 4            E test_extend_grid_shapes[False-*], test_extend_grid_walks[False-*], test_extend_kats
  extend_wide_kernel                    5 .. 16           E test_extend_grid_shapes[False-*], test_extend_grid_walks[False-*]
  long_extend_kernel                    strips of 16      E test_extend_mixed_launch[False]; strict: test_extend_long_reads
  extend_matrix_kernel                  1 .. 4            E test_extend_grid_shapes[True-*], test_extend_grid_walks[True-*]
  extend_matrix_wide_kernel             5 .. 16           E test_extend_grid_shapes[True-*], test_extend_grid_walks[True-*]
  long_extend_matrix_kernel             strips of 16      E test_extend_mixed_launch[True]; strict: test_extend_long_read_with_a_matrix_strict_ties
  band_extend_kernel                    strips of 16      E test_extend_band_geometry; strict: test_extend_band_maximum_on_a_window_edge, test_extend_band_shapes_and_matrix
  band_extend_matrix_kernel             strips of 16      E test_extend_mixed_launch[True]; strict: test_extend_band_shapes_and_matrix
  (option "xdrop" on an extend run: test_xdrop_gpu.py, X)
  long_xdrop_kernel                     strips of 16      X test_xdrop_hand_derivable[0], test_xdrop_strip_edges; strict: test_xdrop_random_tails[1-0]
  long_xdrop_matrix_kernel              strips of 16      X test_xdrop_mixed_launch[True-0]; strict: test_xdrop_matrix_strict_ties[0]
  band_xdrop_kernel                     strips of 16      X test_xdrop_hand_derivable[64 / 16]; strict: test_xdrop_random_tails[1-64 / 16]
  band_xdrop_matrix_kernel              strips of 16      X test_xdrop_mixed_launch[True-64]; strict: test_xdrop_matrix_strict_ties[64]
  (option "band_adapt" on a banded extend run: test_adapt_gpu.py, A)
  band_adapt_kernel                     strips of 16      A test_adapt_tie_rule; strict: test_adapt_drift[*-1], test_adapt_centre_stands_still[1], test_adapt_ties_and_the_rerun[1]
  band_adapt_matrix_kernel              strips of 16      A test_adapt_mixed_launch[True]; strict: test_adapt_matrix_strict_ties
  band_adapt_xdrop_kernel               strips of 16      A test_adapt_xdrop_planted_head; strict: test_adapt_xdrop_diverging_tail
  band_adapt_xdrop_matrix_kernel        strips of 16      A test_adapt_mixed_launch_xdrop[True]; strict: test_adapt_matrix_strict_ties

  traceback kernel (sw_affine_traceback_...)              run by
  kernel                                                  G test_grid_walks[0-*] (walks of several tiles); test_affine_gpu.py
  fit_kernel                                              G test_grid_walks[1-*], test_grid_shapes[1-*]; test_ends_gpu.py
  global_kernel                                           G test_grid_walks[2-*], test_grid_shapes[2-*]; test_ends_gpu.py
  long_kernel                                             test_long_reads_gpu.py::test_long_reads_across_the_seam
  long_fit_kernel                                         G test_mixed_launch_fit_global[1-*]; test_long_reads_gpu.py::test_long_reads_fit_and_global
  long_global_kernel                                      G test_mixed_launch_fit_global[2-*]; test_long_reads_gpu.py::test_long_reads_fit_and_global
  band_kernel                                             test_band_gpu.py::test_band_edges[0]; G test_c99_shim_sets_long_reads_and_band
  band_fit_kernel                                         G test_mixed_launch_fit_global[1-*]; test_band_gpu.py::test_band_edges[1]
  band_global_kernel                                      G test_mixed_launch_fit_global[2-*]; test_band_gpu.py::test_band_edges[2]
  band_adapt_global_kernel                                A every test of test_adapt_gpu.py but the scores_only case
  (an extend run is walked by global_kernel, long_global_kernel and band_global_kernel, started at cells other than (m, n):
  E test_extend_grid_walks, test_extend_long_reads, test_extend_band_maximum_on_a_window_edge)

Each narrow and wide sweep kernel holds one body per (R, tie order): 16 x 3 modes x 2 (plain / matrix) x 2 tie orders = 192
bodies.  GRID_PARAMS below times the 16 classes of affine_grid_cases.RS is that grid; tests/test_affine_grid_cpu.py checks it.
All comparisons are exact: score, flags, number and order of the alignments, every begin and both strings, and the MapRef view."""
import pytest

import sparksmithwaterman_amd as sw

import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -5                         # swmi_status (include/swmi.h)

MODES = (0, 1, 2)                            # local, fit, global
MATRIX = (False, True)
TIES = (0, 1)
# (mode, matrix, tie) of test_grid_shapes and test_grid_walks; every case runs all 16 classes of gc.RS
GRID_PARAMS = [(mode, matrix, tie) for mode in MODES for matrix in MATRIX for tie in TIES]
MIXED_PARAMS = [(mode, matrix) for mode in (1, 2) for matrix in MATRIX]


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


# 4 -- the JNI shim's entry points from plain C99 (tests/c/shim_long.c)
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
