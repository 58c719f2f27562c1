"""The pick kernels on the GPU (sw_subopt_kernel and sw_hits_kernel of swmi_subopt.hip, DESIGN.md sections 8n and 8p): the cases of
tests/pick_cases.py, every value exact against tests/subopt_reference.py and tests/hits_reference.py.

tests/test_subopt_gpu.py and tests/test_hits_gpu.py place their cases where the sweeps can write the row of column maxima wrongly;
here the row is simple -- a comb of planted copies of one 8-base read -- and what is placed is the pass over it: a maximum column,
its runner-up or an earlier hit on either side of every 64-column step edge and of the 256-column edge of the unrolled loop, the
next maximum column in each of the lookahead's four in-flight loads, a quad skipped, the row exhausted, every row-end length class
with the guarded fourth load, a maximum column every 16 columns, sixteen entries with all fifteen readlane tests live, mask widths
around 64 and at 2^30, workgroups with one, two and three pairs, a degenerate and an empty pair inside a workgroup, several
launches, the exact-size re-run, and a banded row that ends between two steps.  tests/test_pick_cpu.py shows without a GPU that
these cases take every branch of the pass and that each of fourteen one-line errors in it would change a value compared here.

Every family runs as one batch per (w, K): many references against one read, first under "subopt" alone (sw_subopt_kernel), then
under "hits" = K (sw_hits_kernel).  Each run is compared through the helpers of tests/pick_gpu_util.py: score, subopt(pair) and
subopts() with subopt_numpy; hits(pair) and hits_all() with hits_numpy, entry 1 with subopt(pair), entry 0's cell with the pair's
alignment end cells.  The expected values are computed once per pair and mask width and shared by all runs.

The cost is the restatement, not the GPU.  Measured where the module was written, both restatements of every pair, once: slide 77
pairs 1.6 s, row ends 47 pairs 0.7 s, lookahead 36 pairs 1.7 s, dense 8 pairs 0.25 s, rounds 6 pairs 0.1 s, wide masks 21 pairs
0.4 s, the mixed batch 112 pairs 1.2 s (the cut batches reuse slide's), band 2 pairs with and without the band 1.75 s (0.44 s per
restatement of 1,100 x 2,300 cells: no reference was shortened) -- 7.7 s for 253 distinct pairs.  On an MI355X the module's 17
tests take 5 s, the slowest (lookahead) 1.0 s."""
import pytest

import sparksmithwaterman_amd as sw

import hits_reference as hr
import pick_cases as pc
import subopt_reference as sr
from pick_gpu_util import subopt_check, subopt_run_and_check, hits_run_and_check

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


_exp = {}


def expected(c):
    """((score, score2, end2), the K = 16 list) of a case, once: the lists of a smaller K are its prefixes"""
    key = (c.ref, c.read, c.w, c.band, c.sc)
    if key not in _exp:
        _exp[key] = (sr.subopt_numpy(c.ref, c.read, c.sc, c.w, c.band), hr.hits_numpy(c.ref, c.read, c.sc, c.w, hr.K_MAX, c.band))
    return _exp[key]


def batches(cases):
    """the cases grouped into batches of many references against one read: [(read, w, k, band, sc, cases)]"""
    out = {}
    for c in cases:
        out.setdefault((c.read, c.w, c.k, c.band, c.sc), []).append(c)
    return [key + (group,) for key, group in out.items()]


def run_grid(ctx, refs, reads, w, k, band, sc, tie=0, **options):
    """one grid under "subopt" alone, then under "hits" = k; returns the two runs' timings"""
    grid = {(r, q): expected(pc.Case("", ref, read, w, k, band, sc)) for r, ref in enumerate(refs) for q, read in enumerate(reads)}
    sub = {key: v[0] for key, v in grid.items()}
    hit = {key: v[1][:k] for key, v in grid.items()}
    b, _ = subopt_run_and_check(ctx, refs, reads, sc, w, band, tie=tie, exp=sub, hits=0, **options)
    t_sub = b.timing()
    b.free()
    b, _ = hits_run_and_check(ctx, refs, reads, sc, w, k, band, tie=tie, exp=hit, **options)
    subopt_check(b, refs, reads, sub, ("hits", w, k, band, tie))
    t_hit = b.timing()
    b.free()
    return t_sub, t_hit


def run_cases(ctx, cases, tie=0, **options):
    return [run_grid(ctx, [c.ref for c in group], [read], w, k, band, sc, tie, **options) for read, w, k, band, sc, group in batches(cases)]


# ---- the comb families ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("w", [1, 2])
def test_slide(ctx, w, tie):
    """one copy moved across every step edge of 321 columns: the runner-up in the step before and in the step behind its maximum column"""
    run_cases(ctx, pc.slide(w), tie)


def test_row_ends(ctx):
    """8 .. 513 columns: the maximum column, then end2, in the row's last column; both loops' every length class"""
    run_cases(ctx, pc.row_ends())


def test_lookahead(ctx):
    """700 and 1,100 columns, the second maximum column one to nine steps behind the first"""
    cases = pc.lookahead()
    assert all(expected(c)[0][1:] == want for c in cases for name, want in pc.LOOK_CHECKED.items() if c.name == name)
    run_cases(ctx, cases)


@pytest.mark.parametrize("tie", [0, 1])
def test_dense(ctx, tie):
    """a maximum column every 16 columns; with cell_cap 1 every such pair is re-run with an exact-size list"""
    run_cases(ctx, pc.dense(), tie)
    if tie == 0:
        for t_sub, t_hit in run_cases(ctx, pc.dense(), cell_cap=1):
            assert t_sub.rerun_pairs > 0 and t_hit.rerun_pairs > 0


@pytest.mark.parametrize("tie", [0, 1])
def test_rounds(ctx, tie):
    """sixteen entries, one per step; K = 1, 2, 3, 16; an earlier entry across a step edge from the candidate"""
    cases = pc.rounds()
    assert len(expected(cases[0])[1]) == 16
    run_cases(ctx, cases, tie)


def test_wide_masks(ctx):
    run_cases(ctx, pc.wide())


# ---- the launch layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,r", [(2, 1), (3, 2), (1, 3)])
def test_partly_filled_workgroup(ctx, q, r):
    """4 q + r pairs: the last workgroup of four wavefronts holds r"""
    cases = pc.layout_cut(q, r)
    assert len(cases) == 4 * q + r
    run_cases(ctx, cases)


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_mixed_batch_in_one_and_in_several_launches(ctx, zero_copy):
    """slide, dense and rounds references against the comb's read and A x 8 -- unequal answers side by side, a degenerate pair and
    an empty reference's two pairs inside workgroups -- in one launch, then under the smallest max_workspace_bytes in several"""
    refs, reads, w, k = pc.layout_mixed()
    assert expected(pc.case("", refs[2], w, k, reads[1])) == ((0, 0, 0), []) and refs[4] == ""
    ctx.set_option("zero_copy", zero_copy)
    for t in run_grid(ctx, refs, reads, w, k, 0, pc.SC):
        assert t.fill_launches == 1
    ctx.set_option("max_workspace_bytes", 1 << 20)
    for t in run_grid(ctx, refs, reads, w, k, 0, pc.SC):
        assert t.fill_launches > 1


# ---- the band --------------------------------------------------------------------------------------------------------------------------
def test_band(ctx):
    """a read of 1,100 bases under band 50: the row ends at column 2098, inside a step.  The best alignment ends there; the stronger
    copy right of it does not count -- and wins with the band off"""
    ctx.set_option("long_reads", 1)
    cases = pc.band()
    free = [c._replace(band=0) for c in cases]
    for c, f in zip(cases, free):
        (s, _, _), (fs, _, _) = expected(c)[0], expected(f)[0]
        assert pc.cols_of(c) == 2098 and expected(c)[1][0][2] == 2098 and fs >= 300 > s and expected(f)[1][0][2] > 2098
    run_cases(ctx, cases)
    run_cases(ctx, free)
