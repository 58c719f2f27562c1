"""Gap-heavy alignments at the column-chunk halo and at the path-length bound (tests/gap_path_cases.py), on the GPU.

Two pieces of host arithmetic decide whether the linear pipelines are correct, and every other alignment in the suite is a
near copy of its read, which comes near neither:
  a  the halo of a column chunk (swmi_plan.h: path_span, col_chunk).  A chunk's wavefront -- or its strip pipeline -- starts
     from zero at column col0 + 1; were the halo too short, the window maxima and checkpoints it owns would be too low.  The
     ratchets here span 0.94 .. 0.99 of path_span and end in the first window a chunk owns, in the chunk's first and last
     step: a sweep begun past the path's first column, at the next window edge, loses score on every one of them
     (tests/test_gap_paths_cpu.py; for most placements that edge is several windows to the right of the chunk's own).
  b  the longest possible traceback (path_bound), which sizes the LDS staging of every walk.  The ratchets here walk 0.94 ..
     0.99 of it, deletions and insertions, in every pipeline, and in the affine kernels.
Every pair against the oracle the way test_gpu_parity.py does it: score, tied cells, every begin, both strings and the MapRef
view.  The chunk counts are asserted against the restated plan, so that a plan that drifts away from the restatement fails
here instead of quietly blunting the inputs."""
import pytest

import sparksmithwaterman_amd as sw

import affine_gpu_util as u
import gap_path_cases as gp
from test_gpu_parity import check_batch

pytestmark = pytest.mark.gpu


# ---- a: the halo ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1], ids=["fused-traceback", "split-traceback"])
def halo_ctx(request):
    """mode 1 with the sweep kernels on every pair, traced back by one workgroup per pair or split per window / alignment"""
    c = sw.Context(0)
    c.set_option("mode", 1)
    c.set_option("zero_copy", 1)
    c.set_option("tb_split", request.param)
    c.set_option("resident", 0)
    c.set_option("tfused", 0)
    yield c
    c.close()


def _run_halo(ctx, case, batches, col_chunks, ties, reverse_strips=0):
    """the references of a halo case in launches refs[lo:hi], under option col_chunks: the run took mode 1 and cut every pair
    into the chunks of the restated plan (none for col_chunks = 1); then every pair in full"""
    m, sc = case
    c = gp.halo_case(m, sc)
    want = 0 if col_chunks == 1 else len(c.chunks)
    assert col_chunks == 1 or tuple(gp.plan_chunks(m, c.n, sc, 4, col_chunks)) == c.chunks
    ctx.set_option("col_chunks", col_chunks)
    ctx.set_option("debug_reverse_strips", reverse_strips)
    try:
        for lo, hi in batches:
            refs = list(c.refs[lo:hi])
            b = ctx.upload(refs, [c.read]).run(sw.make_params(sc))
            try:
                assert b.pipeline_mode() == 1
                assert b.timing().col_chunks == want * len(refs), (lo, hi, col_chunks)
            finally:
                b.free()
            for tie in ties:
                check_batch(ctx, refs, [c.read], sc, tie=tie)
    finally:
        ctx.set_option("col_chunks", 0)
        ctx.set_option("debug_reverse_strips", 0)


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("case", gp.HALO_SINGLE, ids=gp.halo_id)
def test_halo_of_a_chunk_wavefront(halo_ctx, case, tie):
    """sw_sweep_winmax_cols_kernel: reads of one strip, the chunk count automatic (at most 4 pairs per launch) and forced"""
    for col_chunks in (0, gp.FORCED_CHUNKS):
        _run_halo(halo_ctx, case, gp.HALO_BATCHES, col_chunks, (tie,))


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("case", gp.HALO_MULTI, ids=gp.halo_id)
def test_halo_of_a_chunked_strip_pipeline(halo_ctx, case, tie):
    """sw_sweep_winmax_strips_kernel: reads of two and three strips, chunk bodies a quarter of the halo; one case also with the
    strips of every chunk listed in reverse"""
    _run_halo(halo_ctx, case, gp.HALO_BATCHES, gp.FORCED_CHUNKS, (tie,))
    if case == gp.HALO_MULTI[-1]:
        _run_halo(halo_ctx, case, gp.HALO_BATCHES, gp.FORCED_CHUNKS, (tie,), reverse_strips=1)


@pytest.mark.parametrize("case", gp.HALO_SINGLE + gp.HALO_MULTI, ids=gp.halo_id)
def test_halo_cases_swept_whole(halo_ctx, case):
    """the same pairs with no chunks at all: tells a fault of the chunks from a fault of the sweep"""
    _run_halo(halo_ctx, case, ((0, 5),), 1, (0, 1))


# ---- b: the path bound ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(1, 1, 0, 0, 0), (2, 1, 0, 0, 0), (0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (-1, 1, -1, -1, -1), (1, 1, 1, 0, 0),
                                        (1, 0, 1, 0, 0), (1, 1, 0, 1, 0), (1, 0, -1, 1, 0), (1, 1, 0, 0, 1), (1, 0, -1, -1, 1),
                                        (-1, 1, -1, -1, -1, 0)],
                ids=["mode1-winmax", "mode2-events", "mode0-field", "mode1-d2h-copy", "automatic", "mode1-split-traceback",
                     "mode1-split-d2h-copy", "mode1-resident", "mode1-resident-d2h-copy", "mode1-tfused", "mode1-tfused-d2h-copy",
                     "automatic-host-strings"])
def ctx(request):
    """every kernel pipeline, as the fixture of test_gpu_parity.py builds them: (mode, zero_copy, tb_split, resident, tfused
    [, device_strings])"""
    c = sw.Context(0)
    for name, value in zip(("mode", "zero_copy", "tb_split", "resident", "tfused"), request.param):
        c.set_option(name, value)
    c.set_option("device_strings", request.param[5] if len(request.param) > 5 else 1)
    c.test_mode, c.test_resident, c.test_tfused = request.param[0], request.param[3], request.param[4]
    yield c
    c.close()


@pytest.mark.parametrize("name", gp.BOUND_NAMES)
def test_walks_as_long_as_the_path_bound(ctx, name):
    """one near-bound pair per launch, so that it alone dimensions the staging: LDS ops of the traceback kernels, the resident
    kernel's per-lane ops, the transposed kernel's stage words.  "shapes-2x2" is one launch of four pairs of two reference and
    two read lengths, the near-bound one among them: mixed shapes, nothing more -- a run schedules its pairs longest first, so
    the planner meets that pair first (test_planner_memo_of_the_last_bound is the test of its memo)"""
    c = gp.bound_case(name)
    refs, reads = list(c.refs), list(c.reads)
    b = ctx.upload(refs, reads).run(sw.make_params(c.scores))
    try:
        if ctx.test_mode == 1:
            assert b.pipeline_mode() == 1
            if ctx.test_resident == 1 and name in gp.RESIDENT_NAMES:
                assert b.timing().resident_pairs > 0
            if ctx.test_tfused == 1 and name == "del-256x2000":
                assert b.timing().tfused_pairs > 0
    finally:
        b.free()
    for tie in (0, 1):
        check_batch(ctx, refs, reads, c.scores, tie=tie)


def test_planner_memo_of_the_last_bound(ctx):
    """plan_chunk keeps the bound of the last pair's lengths.  A run schedules its pairs longest first, so in one launch the
    largest bound comes first and a stale memo could not lower max_path; under a workspace cap the second launch of this batch
    begins in the middle of one reference's reads and goes on into a reference of the same length: (24000, 24), bound 192, then
    the near-bound pair (24000, 128), bound 1024 (tests/test_gap_paths_cpu.py::test_memo_case_reaches_the_memo).  The number of
    launches is asserted against the restated schedule, so that a schedule that drifts away fails here."""
    c = gp.memo_case()
    refs, reads = list(c.refs), list(c.reads)
    b = ctx.upload(refs, reads).run(sw.make_params(c.scores))
    mode = b.pipeline_mode()
    b.free()
    assert mode in (0, 1, 2)
    cut = gp.launches([len(x) for x in refs], [len(x) for x in reads], mode, gp.memo_cap(mode))
    assert cut[1] == [(0, 2), c.near]
    ctx.set_option("max_workspace_bytes", gp.memo_cap(mode))
    try:
        b = ctx.upload(refs, reads).run(sw.make_params(c.scores))
        try:
            assert b.pipeline_mode() == mode and b.timing().fill_launches == len(cut)
        finally:
            b.free()
        for tie in (0, 1):
            check_batch(ctx, refs, reads, c.scores, tie=tie)
    finally:
        ctx.set_option("max_workspace_bytes", 32 << 30)


@pytest.mark.parametrize("tie", [0, 1])
def test_affine_walk_as_long_as_the_path_bound(tie):
    """the affine kernels' ops_words: a deletion ratchet under gap_open -1, runs of 7k - 2 bases"""
    ref, read, moves = gp.affine_case()
    exp = u.expect([ref], [read], gp.AFFINE_SCORES, tie=tie, cells=True)
    assert len(exp[(0, 0)][1][0][1][0]) == moves
    c = sw.Context(0)
    try:
        for device_strings in (1, 0):
            b = u.run(c, [ref], [read], gp.AFFINE_SCORES, tie, device_strings=device_strings)
            try:
                u.check(b, [ref], [read], exp)
            finally:
                b.free()
    finally:
        c.close()
