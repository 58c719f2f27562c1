"""The steady part of the mode-1 sweep (sweep_fast, swmi_sweep.hip): one generated statement per checkpoint window
(SweepWindowAsm, tools/gen_step.py) between a head and a tail that run block by block.  The shapes are the smallest at
which that loop can go wrong: zero, one and two steady windows with the reference ending on, before and after a window
edge; every rows-per-lane class with full and partial lane counts; the maximum on either side of a window edge, in the
first window and in the tail; column chunks that start behind a halo.  Every pair against the oracle the way
test_gpu_parity.py does it: score, tied cells, both strings of every alignment and the MapRef view, in both tie orders.
"""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import synth

from test_gpu_parity import check_batch, _planted

pytestmark = pytest.mark.gpu

NS = (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)
MS = (1, 63, 64, 65, 128, 129, 150, 192, 193, 256)
STEP_W = 32                       # anti-diagonal steps per checkpoint window


@pytest.fixture(scope="module", params=[0, 1], ids=["fused-traceback", "split-traceback"])
def ctx(request):
    """mode 1 with the sweep kernels on every pair (no resident pairs, no transposed ones), traced back by one workgroup
    per pair or split per window / alignment"""
    c = sw.Context(0)
    c.set_option("mode", 1)
    c.set_option("zero_copy", 1)
    c.set_option("tb_split", request.param)
    c.set_option("resident", 0)
    c.set_option("tfused", 0)
    c.split = request.param
    yield c
    c.close()


def _boundary_seqs():
    rng = random.Random(3211)
    base = "".join(rng.choice("ACGT") for _ in range(256))
    reads = [base[:m] for m in MS]
    refs = []
    for n in NS:                                  # random, with a piece of the reads' common prefix somewhere inside
        ref = [rng.choice("ACGT") for _ in range(n)]
        piece = base[:rng.randint(8, min(n, 40))]
        at = rng.randint(0, n - len(piece))
        ref[at:at + len(piece)] = piece
        refs.append("".join(ref))
    return refs, reads


@pytest.mark.parametrize("tie", [0, 1])
def test_window_boundaries(ctx, tie):
    refs, reads = _boundary_seqs()
    assert [len(x) for x in refs] == list(NS) and [len(x) for x in reads] == list(MS)
    if ctx.split:                                 # 8 pairs per launch
        for r in range(0, len(refs), 4):
            for q in range(0, len(reads), 2):
                check_batch(ctx, refs[r:r + 4], reads[q:q + 2], tie=tie)
    else:                                         # 70 pairs per launch
        check_batch(ctx, refs[:7], reads, tie=tie)
        check_batch(ctx, refs[5:], reads, tie=tie)


def _max_step(s, p, rows_per_lane):
    """0-based step of the sweep at which the last cell of a copy of the read's first p bases, planted at 0-based column
    s, is computed: lane l works on column t - l + 1 at step t"""
    return s + p + (p - 1) // rows_per_lane - 1


@pytest.mark.parametrize("tie", [0, 1])
def test_where_the_maximum_sits(ctx, tie):
    rng = random.Random(3212)
    read = "".join(rng.choice("ACG") for _ in range(150))        # 3 rows per lane; 700 columns: 21 steady windows
    n = 700
    cases = [(150, [121]), (150, [122]), (10, [0]), (150, [550]), (150, [100, 300]), (150, [])]
    assert _max_step(121, 150, 3) % STEP_W == STEP_W - 1 and _max_step(121, 150, 3) < n // STEP_W * STEP_W    # last step of a steady window
    assert _max_step(122, 150, 3) % STEP_W == 0                                                              # first step of the next
    assert _max_step(0, 10, 3) < STEP_W                                                                      # the first window
    assert _max_step(550, 150, 3) >= n // STEP_W * STEP_W                                                    # the tail blocks
    assert _max_step(100, 150, 3) // STEP_W != _max_step(300, 150, 3) // STEP_W                              # tied, two steady windows
    refs = [_planted(rng, read[:p], n, starts) for p, starts in cases]
    if ctx.split:
        check_batch(ctx, refs, [read], tie=tie)
    else:
        check_batch(ctx, (refs * 12)[:70], [read], tie=tie)


def _chunk_edges(m, n, n_pairs, scores=(5, -3, -4)):
    """first windows of the column chunks the plan cuts an m x n pair into (swmi_plan.h: path_span, take_cols)"""
    span = m + scores[0] * m // -scores[2] + 1
    n_ck = ((n + 63 + 15) // 16 + 1) // 2
    chunks = min(max(1, 1024 // n_pairs), n // max(span + 64, 256), n_ck)
    wpc = (n_ck + chunks - 1) // chunks
    return list(range(wpc, n_ck, wpc))


@pytest.mark.parametrize("m,n,n_pairs", [(150, 4100, 4), (64, 8200, 2)])
def test_column_chunks_start_behind_a_halo(ctx, m, n, n_pairs):
    rng = random.Random(3213 + m)
    read = "".join(rng.choice("ACG") for _ in range(m))
    rows_per_lane = (m + 63) // 64
    edges = _chunk_edges(m, n, n_pairs)
    assert len(edges) >= 2
    refs = []
    for k in range(n_pairs):
        e1, e2 = edges[k % len(edges)], edges[(k + 1) % len(edges)]
        straddle = e1 * STEP_W - m // 2                         # a copy across the first column a chunk owns
        inside = e2 * STEP_W + 5 - (m + (m - 1) // rows_per_lane - 1)   # ... and one whose last cell is in the chunk's first window
        assert _max_step(inside, m, rows_per_lane) // STEP_W == e2 and inside > straddle + m
        refs.append(_planted(rng, read, n, [straddle, inside]))
    b = ctx.upload(refs, [read]).run()
    try:
        assert b.pipeline_mode() == 1 and b.timing().col_chunks >= 2 * n_pairs
    finally:
        b.free()
    for tie in (0, 1):
        check_batch(ctx, refs, [read], tie=tie)


def test_headline_shape(ctx):
    refs, reads = synth.config_1k(n_refs=64)
    assert len(refs) == 64 and len(refs[0]) == 2000 and len(reads) == 1 and len(reads[0]) == 150
    for tie in (0, 1):
        check_batch(ctx, refs, reads, tie=tie)
