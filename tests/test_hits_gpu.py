"""Option "hits" on the GPU (the HITS sweeps of swmi_affine.hip, sw_hits_kernel of swmi_subopt.hip): every
pair's list of (score, end_i, end_j) against tests/hits_reference.py, exactly.  set_option("hits", ...) is what fails without the
feature.

On every pair of every test: entry 1 is Batch.subopt(pair), and entry 0's cell is one of the pair's alignment end cells wherever
the run has alignments.  The cases are chosen where the row carry can go wrong -- every rows-per-lane class with the storing lane
below and at 63, the strip seam, the band's windows, a maximum held by several rows of one lane, of two lanes, of two strips -- and
where the rounds can: equal secondaries, the strict mask around an earlier hit, a list shorter than K, K = 1; then the host
machinery around the per-pair array.  Where the rounds of sw_hits_kernel over a row can go wrong -- step edges, the lookahead, row
ends, sixteen entries, an earlier entry across a step edge -- is tests/test_pick_gpu.py's; the check helpers are shared with it
(tests/pick_gpu_util.py)."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M

import affine_gpu_util as u
import hits_reference as hr
from pick_gpu_util import weaken, planted, hits_expect as expect, hits_check_pair as check_pair, hits_check as check, hits_run_and_check as run_and_check

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -5, -6       # swmi_status (include/swmi.h)
LOCAL, FIT, GLOBAL = sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL
SC = (5, -4, -3, -5)
LOG = (2, -3, -4, -6)          # keeps random sequence in the logarithmic phase: long random flanks stay weak
AUTO = sw.SUBOPT_AUTO
PERIOD = "ACGTTGCAAGCT"


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# ---- the row carry in every sweep ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", range(1, 17))
def test_rows_per_lane_and_storing_lane(ctx, R):
    """reads of 64 R rows (the last row in lane 63) and 64 R - 37 (in a lane below): the narrow kernel (R <= 4) and the wide one.  The
    references hold two pieces of the read from different rows, so the hits' rows differ"""
    rng = random.Random(9400 + R)
    base = u.rand(rng, 1100)
    reads = [base[30:30 + 64 * R], base[30:30 + 64 * R - 37]]
    m = len(reads[1])
    refs = [u.mutate(rng, base[20:20 + n], 0.06, 0.02)[:n] for n in (101, 137)]
    refs.append(base[30:30 + min(m, 50)] + u.rand(rng, 41) + base[30 + m - min(m, 70):30 + m] + u.rand(rng, 9))
    exp = expect(refs, reads, SC, 10, 4)
    assert any(len(v) >= 2 for v in exp.values()) and len({h[1] for v in exp.values() for h in v}) >= 3
    for tie in (0, 1):
        b, _ = run_and_check(ctx, refs, reads, SC, 10, 4, tie=tie, exp=exp)
        b.free()


def diagonal_case(rng, m, n):
    """a random pair with pieces of the read planted on the diagonal, of decreasing similarity, at least one in every strip and one
    across the seam"""
    read = u.rand(rng, m)
    ref = list(u.rand(rng, n))
    for a, z, load in ((40, 160, 4), (400, 560, 2), (940, min(m, 1100), 0), (1200, 1330, 6), (1700, 1800, 3)):
        if z <= min(m, n):
            ref[a:z] = weaken(read[a:z], load)
    return "".join(ref), read


@pytest.mark.parametrize("m", [1025, 1500, 2048])
@pytest.mark.parametrize("band", [0, 32])
def test_long_reads_and_band(ctx, m, band):
    rng = random.Random(9420 + m + band)
    ref, read = diagonal_case(rng, m, m + 30)
    ctx.set_option("long_reads", 1)
    exp = expect([ref], [read], LOG, 60, 16, band)
    assert len(exp[(0, 0)]) >= 3 and max(h[1] for h in exp[(0, 0)]) > 1024 > min(h[1] for h in exp[(0, 0)])
    for tie in ((0, 1) if m == 1500 else (0,)):
        b, _ = run_and_check(ctx, [ref], [read], LOG, 60, 16, band=band, tie=tie, exp=exp)
        b.free()


# ---- row ties: the smaller row -------------------------------------------------------------------------------------------------
def test_row_ties(ctx):
    """`GAG` against C x k + AA + C...: column 2's maximum is held by rows k + 1 and k + 2 -- two slots of one lane (m = 128: R = 2, k =
    0 and 2), the last slot of a lane and the first of the next (k = 1), rows 1024 and 1025 on either side of the strip seam (k =
    1023); and A x m against `A`: every row, row 1 wins.  Short and long reads in one launch"""
    def two(k, m):
        return "C" * k + "AA" + "C" * (m - k - 2)
    reads = [two(0, 128), two(2, 128), two(1, 128), two(1023, 1040), two(63, 200), "A", "A" * 64, "A" * 200, "A" * 1500]
    refs = ["GAG", "A"]
    ctx.set_option("long_reads", 1)
    exp = expect(refs, reads, SC, 1, 4)
    assert [exp[(0, q)] for q in range(5)] == [[(5, k + 1, 2)] for k in (0, 2, 1, 1023, 63)]
    assert [exp[(1, q)] for q in range(5, 9)] == [[(5, 1, 1)]] * 4
    for tie in (0, 1):
        b, _ = run_and_check(ctx, refs, reads, SC, 1, 4, tie=tie, exp=exp)
        b.free()


# ---- the rounds ----------------------------------------------------------------------------------------------------------------
def test_three_copies_in_order_and_every_k(ctx):
    rng = random.Random(9430)
    read = u.rand(rng, 40)
    ref, ends = planted(rng, read, (25, 37, 41, 25), (3, 0, 6))
    full = expect([ref], [read], SC, 30, 16)[(0, 0)]
    assert [(v, i, j) for v, i, j in full[:3]] == [(200, 40, ends[1]), (200 - 3 * 9, 40, ends[0]), (200 - 6 * 9, 40, ends[2])]
    for k in (1, 2, 3, 16):
        b, exp = run_and_check(ctx, [ref], [read], SC, 30, k)
        assert exp[(0, 0)] == full[:k]
        if k == 1:          # entry 1 is not listed, but it is computed: subopt is what it is without the option
            assert b.subopt(0) == (full[1][0], full[1][2])
        b.free()


def test_equal_secondaries_and_fewer_than_k(ctx):
    rng = random.Random(9431)
    read = u.rand(rng, 30)
    ref, ends = planted(rng, read, (20, 45, 45, 20), (2, 0, 2))
    b, exp = run_and_check(ctx, [ref, PERIOD[:9]], [read], SC, 20, 16)
    assert exp[(0, 0)][:3] == [(150, 30, ends[1]), (132, 30, ends[0]), (132, 30, ends[2])] and len(exp[(0, 0)]) < 16
    b.free()


def test_the_mask_around_an_earlier_hit_is_strict(ctx):
    """three copies; the third ends d columns behind the second: under w = d - 1 it is listed, under w = d it is not"""
    rng = random.Random(9432)
    read = u.rand(rng, 40)
    ref, ends = planted(rng, read, (25, 60, 17, 25), (0, 2, 5))
    d = ends[2] - ends[1]
    near, exp_near = run_and_check(ctx, [ref], [read], SC, d - 1, 8)
    far, exp_far = run_and_check(ctx, [ref], [read], SC, d, 8)
    assert [h[2] for h in exp_near[(0, 0)][:3]] == ends and ends[2] not in [h[2] for h in exp_far[(0, 0)]]
    assert exp_far[(0, 0)][1][2] == ends[1] and all(abs(h[2] - ends[1]) > d for h in exp_far[(0, 0)][2:])
    near.free()
    far.free()


@pytest.mark.parametrize("m,w", [(20, 15), (100, 50)])
def test_auto(ctx, m, w):
    rng = random.Random(9440 + m)
    read = u.rand(rng, m)
    ref, ends = planted(rng, read, (10, w - 3, w - 3, 10), (0, 2, 4))
    b, exp = run_and_check(ctx, [ref], [read], SC, AUTO, 16)
    assert exp == expect([ref], [read], SC, w, 16) and [h[2] for h in exp[(0, 0)][:3]] == ends
    b.free()


def test_degenerate_and_empty_pairs(ctx):
    refs, reads = ["CCCC", "", "ACGTACGT"], ["AAAA", "", "ACGT"]
    b, exp = run_and_check(ctx, refs, reads, SC, 1, 16)
    assert exp[(0, 0)] == exp[(1, 2)] == exp[(2, 1)] == [] and exp[(2, 2)][0] == (20, 4, 4)
    assert b.n_alignments(0)[1] == sw.PAIR_DEGENERATE
    b.free()


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def standard():
    rng = random.Random(9450)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300] + base[40:120] for _ in range(6)]
    reads = [u.mutate(rng, base[20:], 0.05, 0.02)[:290 - 23 * k] for k in range(6)]
    return refs, reads


_std = {}


def standard_expected():
    if not _std:
        refs, reads = standard()
        _std["v"] = (refs, reads, expect(refs, reads, SC, 25, 5))
    return _std["v"]


def everything(b, n_pairs, cigar):
    return [(b.score(p), b.n_alignments(p), b.alignments(p, with_cell=True), b.cigars(p) if cigar else None, b.subopt(p))
            for p in range(n_pairs)]


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_zero_copy_scores_only_chunks_and_cigar(ctx, zero_copy):
    refs, reads, exp = standard_expected()
    assert any(len(v) >= 3 for v in exp.values())
    ctx.set_option("zero_copy", zero_copy)
    off = u.run(ctx, refs, reads, SC, 0, LOCAL, subopt=25, hits=0, cigar=2)
    want = everything(off, 36, True)
    for call in (lambda: off.hits(0), off.hits_all, off.hit_specs):
        with pytest.raises(_capi.SwmiError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED and "hits" in str(e.value)
    off.free()
    b, _ = run_and_check(ctx, refs, reads, SC, 25, 5, exp=exp, cigar=2)
    assert b.timing().fill_launches == 1 and everything(b, 36, True) == want        # every other result is unchanged
    b.free()
    b, _ = run_and_check(ctx, refs, reads, SC, 25, 5, exp=exp, scores_only=1, cigar=0)
    with pytest.raises(_capi.SwmiError):
        b.alignment(0, 0)
    b.free()
    ctx.set_option("scores_only", 0)
    ctx.set_option("max_workspace_bytes", 1 << 20)
    b, _ = run_and_check(ctx, refs, reads, SC, 25, 5, exp=exp)
    assert b.timing().fill_launches > 1
    b.free()


def test_mixed_short_and_long_launches_and_a_score_matrix(ctx):
    rng = random.Random(9451)
    amino = "ARNDCQEGHILKMFPSTWYV"
    short = u.rand(rng, 70, amino)
    long_ = u.rand(rng, 1100, amino)
    refs = [u.rand(rng, 30, amino) + short + u.rand(rng, 50, amino) + u.mutate(rng, short, 0.2, 0.0, amino) + u.rand(rng, 20, amino),
            long_[300:700] + u.rand(rng, 100, amino) + u.mutate(rng, long_[800:1000], 0.15, 0.0, amino)]
    ctx.set_option("long_reads", 1)
    b, exp = run_and_check(ctx, refs, [short, long_], (1, -1, -1, -11), 30, 6, matrix=M.BLOSUM62)
    assert len(exp[(0, 0)]) >= 2 and len(exp[(1, 1)]) >= 2
    b.free()


def test_independent_of_the_cell_list(ctx):
    """a periodic reference: a maximum column per period.  With cell_cap 1 the pair is re-run with an exact-size list"""
    refs, reads = [PERIOD * 20 + "GG" + PERIOD[:9]], [PERIOD, PERIOD + PERIOD[:5]]
    exp = expect(refs, reads, SC, 3, 16)
    assert len(exp[(0, 0)]) >= 2
    small, _ = run_and_check(ctx, refs, reads, SC, 3, 16, exp=exp, cell_cap=1)
    assert small.timing().rerun_pairs > 0
    large, _ = run_and_check(ctx, refs, reads, SC, 3, 16, exp=exp, cell_cap=4096)
    assert large.timing().rerun_pairs == 0
    small.free()
    large.free()


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_arena_retry(ctx, zero_copy):
    """two alignments of 1,500 columns do not fit the smallest record arena: the traceback is repeated with a larger one"""
    rng = random.Random(9452)
    read = u.rand(rng, 1500)
    refs = [u.mutate(rng, read, 0.03, 0.002) + read[200:330], u.mutate(rng, read, 0.03, 0.002)[:1480]]
    ctx.set_option("long_reads", 1)
    ctx.set_option("zero_copy", zero_copy)
    ctx.set_option("arena_words_per_pair", 1)
    b, exp = run_and_check(ctx, refs, [read], LOG, 100, 4)
    assert len(exp[(0, 0)]) >= 2
    b.free()


def test_async_run_keeps_the_value_it_was_asked_with(ctx):
    rng = random.Random(9453)
    read = u.rand(rng, 40)
    ref, ends = planted(rng, read, (25, 37, 41, 25), (3, 0, 6))
    p = sw.make_params(SC[:3])
    for name, v in dict(gap_open=SC[3], subopt=30, hits=3, debug_async_delay_us=20000).items():
        ctx.set_option(name, v)
    b = ctx.upload([ref], [read]).run_async(p)
    ctx.set_option("hits", 2)                                 # does not reach the run in flight
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    check(b, [ref], [read], expect([ref], [read], SC, 30, 3), 3)
    assert len(b.hits(0)) == 3
    b.run(p)                                                  # ... but the next one
    check(b, [ref], [read], expect([ref], [read], SC, 30, 2), 2)
    b.free()


@pytest.mark.parametrize("keep", [1, 0])
def test_stream_of_two_chunks(ctx, keep):
    refs, reads, exp = standard_expected()
    reads = reads[:2]
    for name, v in dict(gap_open=SC[3], subopt=25, hits=5, stream_keep_records=keep).items():
        ctx.set_option(name, v)
    st = ctx.stream(reads, sw.make_params(SC[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("hits", 0)                                 # (the stream keeps the value it was opened with)
    st.push(refs[:3]).push(refs[3:]).finish()
    chunks = st.chunks()
    assert [first for first, _ in chunks] == [0, 3]
    for first, c in chunks:
        part = refs[first:first + 3]
        assert c.pipeline_mode() == 3
        check(c, part, reads, {(r, q): exp[(first + r, q)] for r in range(3) for q in range(2)}, 5, cells=bool(keep))
    st.close()


def test_pair_list_with_a_reversed_segment(ctx):
    rng = random.Random(9454)
    read = u.rand(rng, 80)
    src, ends = planted(rng, read, (100, 70, 90, 60), (0, 4, 7))
    refs, reads = [src], [u.rand(rng, 10) + read + u.rand(rng, 10)]
    specs = [(0, 0, 40, 300, 10, 80), (0, 0, 120, 350, 10, 80), (0, 0, 40, 420, 5, 90, True), (0, 0)]
    for name, v in dict(gap_open=SC[3], align_mode=LOCAL, subopt=30, hits=4).items():
        ctx.set_option(name, v)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    assert b.pipeline_mode() == 3
    for k in range(len(specs)):
        ref, rd = b.segments(k)
        want = hr.hits_numpy(ref, rd, SC, 30, 4)
        check_pair(b, k, want, 4, k)
        assert len(want) >= 2
    # the cells are the segments': the source bytes they name hold the last base of the copy the hit ends on
    _, i, j = b.hits(0)[0]
    assert b.to_source(0, i, j) == (10 + i - 1, 40 + j - 1) and 40 + j in ends and i == 80
    _, i, j = b.hits(2)[0]
    assert b.to_source(2, i, j) == (5 + 90 - i, 40 + 420 - j)
    # the reverse extensions of an unreversed pair are offset by its starts; a reversed pair has none
    assert b.hit_specs(0)[0] == (0, 0, 40, b.hits(0)[0][2], 10, 80, 1)
    with pytest.raises(ValueError):
        b.hit_specs(2)
    b.free()


# ---- the reverse extension on the device ---------------------------------------------------------------------------------------
def test_reverse_extension_on_the_device(ctx):
    """hit_specs() into upload_pairs on the same sources, then an extend run: every pair's score is its hit's score"""
    refs, reads, exp = standard_expected()
    b, _ = run_and_check(ctx, refs, reads, SC, 25, 5, exp=exp)
    specs = b.hit_specs()
    want = [h[0] for r in range(len(refs)) for q in range(len(reads)) for h in exp[(r, q)]]
    assert len(specs) == len(want) > 36 and specs[0][2:] == (0, exp[(0, 0)][0][2], 0, exp[(0, 0)][0][1], 1)
    b.free()
    for name, v in dict(align_mode=GLOBAL, extend=1, subopt=0, hits=0).items():
        ctx.set_option(name, v)
    pb = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    assert [pb.score(k) for k in range(len(specs))] == want
    pb.free()
    # ... and from a pair list with unreversed specs
    for name, v in dict(align_mode=LOCAL, extend=0, subopt=25, hits=3).items():
        ctx.set_option(name, v)
    lst = [(0, 1, 30, 300, 20, 200), (3, 0, 10, None, 0, None)]
    b = ctx.upload_pairs(refs, reads, lst).run(sw.make_params(SC[:3]))
    specs = b.hit_specs()
    want = [h[0] for k in range(2) for h in b.hits(k)]
    assert len(want) >= 3
    b.free()
    for name, v in dict(align_mode=GLOBAL, extend=1, subopt=0, hits=0).items():
        ctx.set_option(name, v)
    pb = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    assert [pb.score(k) for k in range(len(specs))] == want
    pb.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rng = random.Random(9455)
    read = u.rand(rng, 40)
    ref, _ = planted(rng, read, (25, 37, 41, 25), (3, 0, 6))
    exp = expect([ref], [read], SC, 30, 3)
    # values outside 0 .. 16 leave the context as it was
    ctx.set_option("hits", 3)
    for bad in (17, -1):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("hits", bad)
        assert e.value.code == ERR_INVALID and "hits" in str(e.value)
    b = u.run(ctx, [ref], [read], SC, 0, LOCAL, subopt=30)
    check(b, [ref], [read], exp, 3)
    # a pair out of range; an array too small
    with pytest.raises(_capi.SwmiError) as e:
        b.hits(1)
    assert e.value.code == ERR_RANGE
    with pytest.raises(_capi.SwmiError) as e:
        b.hits_all(2)
    assert e.value.code == ERR_RANGE
    import ctypes as C
    n, arr = C.c_uint32(), (_capi.Hit * 2)()
    assert b._lib.swmi_pair_hits(b._h, 0, arr, 2, C.byref(n)) == ERR_RANGE and n.value == 3
    assert b._lib.swmi_pair_hits(b._h, 0, None, 0, C.byref(n)) == 0 and n.value == 3
    assert b.hits_all(3)[1].shape == (1, 3)
    # without subopt, and in fit, global and extend runs: refused before anything is launched, the message names an option
    p = sw.make_params(SC[:3])
    ctx.set_option("subopt", 0)
    with pytest.raises(_capi.SwmiError) as e:
        b.run(p)
    assert e.value.code == ERR_UNSUPPORTED and "hits" in str(e.value)
    ctx.set_option("subopt", 30)
    for mode in (FIT, GLOBAL):
        ctx.set_option("align_mode", mode)
        for extend in ((0, 1) if mode == GLOBAL else (0,)):
            ctx.set_option("extend", extend)
            with pytest.raises(_capi.SwmiError) as e:
                b.run(p)
            assert e.value.code == ERR_UNSUPPORTED
    ctx.set_option("extend", 0)
    ctx.set_option("align_mode", LOCAL)
    # a run with hits = 0: the accessors are refused, subopt's are not
    ctx.set_option("hits", 0)
    b.run(p)
    for call in (lambda: b.hits(0), b.hits_all):
        with pytest.raises(_capi.SwmiError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED and "hits" in str(e.value)
    assert b.score(0) == exp[(0, 0)][0][0] and b.subopt(0) == (exp[(0, 0)][1][0], exp[(0, 0)][1][2])
    b.free()
