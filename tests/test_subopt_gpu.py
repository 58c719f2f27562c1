"""Option "subopt" on the GPU (the SUBOPT sweeps of swmi_affine.hip, sw_subopt_kernel of swmi_subopt.hip):
every pair's score, score2 and end2 against tests/subopt_reference.py, exactly.  set_option("subopt", ...) is what fails without
the feature.

The cases are chosen where the column maxima can go wrong: every rows-per-lane class with the storing lane below and at 63, the
8-column blocks' edges, the mask's strict '>' on either side, tied maxima, the seam between two strips with the runner-up on either
side of it, the band's windows (a column left of a later window, a copy outside the band, the columns right of the last window),
and the host machinery around the per-pair array: zero-copy or not, several launches, the exact-size re-run, async, streams, pair
lists.  Where the pass of sw_subopt_kernel over a row can go wrong -- step edges, the lookahead, row ends, dense maxima, partly filled
workgroups -- is tests/test_pick_gpu.py's; the check helpers are shared with it (tests/pick_gpu_util.py)."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M

import affine_gpu_util as u
import subopt_reference as sr
from pick_gpu_util import weaken, planted, subopt_expect as expect, subopt_check as check, subopt_run_and_check as run_and_check

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -5, -6       # swmi_status (include/swmi.h)
LOCAL, FIT, GLOBAL = sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL
SC = (5, -4, -3, -5)
AUTO = sw.SUBOPT_AUTO
PERIOD = "ACGTTGCAAGCT"


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# ---- the sweep: rows per lane, the storing lane, block edges -----------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 100, 256, 257, 1024])
def test_rows_per_lane_and_storing_lane(ctx, m):
    """R = 1, 2, 4, 5, 16; the lane that owns the last row is below 63 (m = 1, 63, 65, 100, 257) and 63 (64, 256, 1024): the narrow and
    the wide kernel"""
    rng = random.Random(9200 + m)
    base = u.rand(rng, 1100)
    reads = [base[30:30 + m]]
    refs = [u.mutate(rng, base[20:20 + n], 0.06, 0.02)[:n] for n in (90, 137, 200)] + [base[30:30 + min(m, 60)] + u.rand(rng, 40) + base[30:30 + min(m, 90)]]
    for w in (AUTO, 3):
        b, exp = run_and_check(ctx, refs, reads, SC, w)
        b.free()
    assert any(v[1] > 0 for v in exp.values()) or m == 1


def test_block_edges(ctx):
    rng = random.Random(9210)
    read = u.rand(rng, 10)
    refs = [(read[3:] + read + read[:6] + u.rand(rng, 60))[:n] for n in (1, 7, 8, 9, 64, 65)]
    b, exp = run_and_check(ctx, refs, [read], SC, 1)
    b.free()
    assert exp[(5, 0)][1] > 0


# ---- the mask and ties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loads", [(0, 3), (3, 0)])
def test_mask_is_strict(ctx, loads):
    """the read planted twice d columns apart, the weaker copy right or left: under w = d - 1 it counts, under w = d it does not"""
    rng = random.Random(9220)
    read = u.rand(rng, 40)
    ref, ends = planted(rng, read, (25, 37, 25), loads)
    d = ends[1] - ends[0]
    weak = ends[0] if loads[0] else ends[1]
    near, exp_near = run_and_check(ctx, [ref], [read], SC, d - 1)
    far, exp_far = run_and_check(ctx, [ref], [read], SC, d)
    assert exp_near[(0, 0)][2] == weak and exp_far[(0, 0)][2] != weak and exp_far[(0, 0)][1] < exp_near[(0, 0)][1]
    near.free()
    far.free()


def test_ties(ctx):
    rng = random.Random(9230)
    read = u.rand(rng, 30)
    # two exact copies and a weaker third: two maximum columns, both masked
    ref, ends = planted(rng, read, (20, 45, 45, 20), (0, 0, 2))
    b, exp = run_and_check(ctx, [ref], [read], SC, 20)
    assert exp[(0, 0)] == (150, 150 - 2 * 9, ends[2]) and b.n_alignments(0)[0] == 2
    b.free()
    # two equally weak copies around the exact one: the smaller column
    ref, ends = planted(rng, read, (20, 45, 45, 20), (2, 0, 2))
    b, exp = run_and_check(ctx, [ref], [read], SC, 20)
    assert exp[(0, 0)] == (150, 132, ends[0])
    b.free()


def test_independent_of_the_cell_list(ctx):
    """a periodic reference: a maximum column per period.  With cell_cap 1 the pair is re-run with an exact-size list; the values are
    those of a large cap"""
    refs, reads = [PERIOD * 20 + "GG" + PERIOD[:9]], [PERIOD, PERIOD + PERIOD[:5]]
    exp = expect(refs, reads, SC, 3)
    assert exp[(0, 0)][1] > 0
    small, _ = run_and_check(ctx, refs, reads, SC, 3, exp=exp, cell_cap=1)
    assert small.timing().rerun_pairs > 0
    large, _ = run_and_check(ctx, refs, reads, SC, 3, exp=exp, cell_cap=4096)
    assert large.timing().rerun_pairs == 0
    assert [small.subopt(p) for p in range(2)] == [large.subopt(p) for p in range(2)]
    assert [small.alignments(p) for p in range(2)] == [large.alignments(p) for p in range(2)]
    small.free()
    large.free()


def test_degenerate_and_empty_pairs(ctx):
    refs, reads = ["CCCC", "", "ACGTACGT"], ["AAAA", "", "ACGT"]
    b, exp = run_and_check(ctx, refs, reads, SC, 1)
    assert exp[(0, 0)] == exp[(1, 2)] == exp[(2, 1)] == (0, 0, 0) and exp[(2, 2)][0] == 20
    assert b.n_alignments(0)[1] == sw.PAIR_DEGENERATE
    b.free()


@pytest.mark.parametrize("m,w", [(20, 15), (100, 50)])
def test_auto(ctx, m, w):
    rng = random.Random(9240 + m)
    read = u.rand(rng, m)
    ref, ends = planted(rng, read, (10, w - 3, 10, 10), (0, 2, 3))     # the second copy ends m + w - 3 behind the first: w + 17 or more
    assert sr.mask_width(AUTO, m) == w
    b, exp = run_and_check(ctx, [ref], [read], SC, AUTO)
    assert exp == expect([ref], [read], SC, w) and exp[(0, 0)][2] == ends[1]
    b.free()


# ---- long reads and the band ---------------------------------------------------------------------------------------------------
# A strong alignment leaves high column maxima on its own columns and a slowly decaying tail to its right, so a planted runner-up
# decides only when it lies LEFT of the best alignment and w is wider than that one: the cases below put the best alignment last
# and give w explicitly.  LOG keeps random sequence in the logarithmic phase (under SC gapped random alignments grow linearly).
LOG = (2, -3, -4, -6)


def near(got, want, slack=6):
    """a planted copy's score and end column, give or take the chance matches around it"""
    return want[0] <= got[0] <= want[0] + slack and want[1] <= got[1] <= want[1] + slack


def seam_case(rng, tail, cross):
    """a read of two strips, P (1024 rows) + Q (`tail` rows).  The best alignment takes the last 300 rows of P and the first `cross` of Q,
    so it crosses the seam; `up` is a weaker copy of rows 101 .. 300 (strip 0 alone: its column maxima must survive strip 1), `down` one
    of Q's rows 601 .. 800 (strip 1 alone)"""
    P, Q = u.rand(rng, 1024), u.rand(rng, tail)
    return P + Q, P[724:] + Q[:cross], weaken(P[100:300], 8), weaken(Q[600:800], 4) if tail >= 800 else ""


def test_long_reads_across_the_seam(ctx):
    rng = random.Random(9250)
    ctx.set_option("long_reads", 1)
    # m = 1025: strip 1 has one row.  The copy ends at column 200, the best alignment spans 800 .. 1100
    read, main, up, _ = seam_case(rng, 1, 1)
    ref = up + u.rand(rng, 599) + main
    assert len(read) == 1025 and len(ref) == 1100
    b, exp = run_and_check(ctx, [ref], [read], LOG, 315)
    assert exp[(0, 0)][0] >= 602 and near(exp[(0, 0)][1:], (360, 200))
    b.free()
    # m = 2049: the runner-up in strip 0's rows only, in strip 1's rows only, and both (the stronger one wins); 861 .. 1260 is the best
    read, main, up, down = seam_case(rng, 1025, 100)
    refs = [up + u.rand(rng, 660) + main,
            u.rand(rng, 220) + down + u.rand(rng, 440) + main,
            up + u.rand(rng, 20) + down + u.rand(rng, 440) + main]
    assert len(read) == 2049 and [len(r) for r in refs] == [1260] * 3
    b, exp = run_and_check(ctx, refs, [read], LOG, 410)
    assert near(exp[(0, 0)][1:], (360, 200)) and near(exp[(1, 0)][1:], (380, 420)) and near(exp[(2, 0)][1:], (380, 420))
    b.free()
    b, _ = run_and_check(ctx, refs, [read], LOG, AUTO, tie=1)
    b.free()


def band_case(rng, m, n, rows):
    """a random pair with four planted pieces: the best alignment, read rows `rows` on the diagonal; a weaker copy of rows 151 .. 270 at
    columns 401 .. 520 -- inside strip 0's window under band 64, left of strip 1's (961 ..); a strong copy of rows 101 .. 400 at columns
    1301 .. 1600 -- outside strip 0's window (.. 1088), so not a cell; a copy of rows 1041 .. 1090 at columns 2201 .. 2250, right of
    strip 1's window (.. 2112)"""
    read = u.rand(rng, m)
    ref = list(u.rand(rng, n))
    ref[rows[0]:rows[1]] = read[rows[0]:rows[1]]
    ref[400:520] = weaken(read[150:270], 3)
    ref[1300:1600] = read[100:400]
    ref[2200:2250] = read[1040:1090]
    return "".join(ref), read


@pytest.mark.parametrize("m,rows", [(2100, (1700, 2090)), (1100, (900, 1100))])
def test_band(ctx, m, rows):
    """band 64 against n = 2300; the best alignment crosses the last seam.  m = 1100: the last window ends at column 2112 and the
    columns right of it read 0.  Under w = 400 the runner-up is the copy that only strip 0 sees -- a column left of every later
    window -- and the copy outside the band, which wins without the band, does not count"""
    rng = random.Random(9260 + m)
    ref, read = band_case(rng, m, 2300, rows)
    ctx.set_option("long_reads", 1)
    exp = expect([ref], [read], LOG, 400, 64)
    free = expect([ref], [read], LOG, 400, 0)
    assert exp[(0, 0)][0] >= 2 * (rows[1] - rows[0]) and near(exp[(0, 0)][1:], (225, 520), 15) and free[(0, 0)][1] >= 400 > exp[(0, 0)][1]
    b, _ = run_and_check(ctx, [ref], [read], LOG, 400, band=64, exp=exp)
    assert b.band_window(0, 1) == (961, 2112)
    b.free()
    # ... and with nothing masked but the end's neighbourhood
    b, _ = run_and_check(ctx, [ref], [read], LOG, 5, band=64)
    b.free()


# ---- scoring variants ------------------------------------------------------------------------------------------------------------
def test_score_matrix(ctx):
    rng = random.Random(9270)
    amino = "ARNDCQEGHILKMFPSTWYV"
    short = u.rand(rng, 70, amino)
    long_ = u.rand(rng, 1100, amino)
    refs = [u.rand(rng, 30, amino) + short + u.rand(rng, 50, amino) + u.mutate(rng, short, 0.2, 0.0, amino) + u.rand(rng, 20, amino),
            long_[300:700] + u.rand(rng, 100, amino) + u.mutate(rng, long_[800:1000], 0.15, 0.0, amino)]
    sc = (1, -1, -1, -11)
    ctx.set_option("long_reads", 1)
    b, exp = run_and_check(ctx, refs, [short, long_], sc, 30, matrix=M.BLOSUM62)
    assert exp[(0, 0)][1] > 0 and exp[(1, 1)][1] > 0
    b.free()


def test_strict_tie_mode(ctx):
    rng = random.Random(9271)
    read = u.rand(rng, 150)
    refs = [planted(rng, read, (30, 60, 30), (0, 6))[0], PERIOD * 12]
    reads = [read, PERIOD * 2]
    exp = expect(refs, reads, SC, 10)
    b, _ = run_and_check(ctx, refs, reads, SC, 10, tie=1, exp=exp)
    b.free()


def test_gap_open_0_gives_the_linear_scores(ctx):
    rng = random.Random(9272)
    base = u.rand(rng, 500)
    refs = [u.mutate(rng, base, 0.05, 0.02) for _ in range(3)] + [PERIOD * 6]
    reads = [base[50:200], u.mutate(rng, base[200:360], 0.08, 0.03), PERIOD]
    sc = sw.DEFAULT_SCORES + (0,)
    lin = u.run(ctx, refs, reads, sc, 0, LOCAL, mode3=False, subopt=0)
    assert lin.pipeline_mode() in (1, 2)
    want = [(lin.score(p), lin.alignments(p, with_cell=True)) for p in range(12)]
    lin.free()
    b, _ = run_and_check(ctx, refs, reads, sc, AUTO)
    assert b.pipeline_mode() == 3
    assert [(b.score(p), b.alignments(p, with_cell=True)) for p in range(12)] == want
    b.free()


# ---- the rest of the run is unchanged --------------------------------------------------------------------------------------------
def everything(b, n_pairs, cigar):
    out = []
    for p in range(n_pairs):
        out.append((b.score(p), b.n_alignments(p), b.alignments(p, with_cell=True), b.cigars(p) if cigar else None))
    return out


def test_every_other_result_is_unchanged(ctx):
    rng = random.Random(9280)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300] for _ in range(3)] + [PERIOD * 8, "CCCC"]
    reads = [u.mutate(rng, base[20:], 0.05, 0.02)[:150], PERIOD, "AAAA"]
    for cigar in (0, 2):
        off = u.run(ctx, refs, reads, SC, 0, LOCAL, subopt=0, cigar=cigar)
        want = everything(off, 15, cigar)
        with pytest.raises(_capi.SwmiError) as e:
            off.subopt(0)
        assert e.value.code == ERR_UNSUPPORTED and "subopt" in str(e.value)
        off.free()
        b, _ = run_and_check(ctx, refs, reads, SC, 5, cigar=cigar)
        assert everything(b, 15, cigar) == want
        b.free()


def test_scores_only(ctx):
    rng = random.Random(9281)
    read = u.rand(rng, 60)
    refs = [planted(rng, read, (20, 30, 20), (0, 3))[0], planted(rng, read, (5, 50, 5), (4, 1))[0]]
    b, exp = run_and_check(ctx, refs, [read], SC, 10, scores_only=1)
    with pytest.raises(_capi.SwmiError):
        b.alignment(0, 0)
    assert all(v[1] > 0 for v in exp.values())
    b.free()


# ---- run paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_copy", [0, 1])
def test_zero_copy_and_several_launches(ctx, zero_copy):
    rng = random.Random(9290)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300] + base[40:120] for _ in range(8)]
    reads = [u.mutate(rng, base[20:], 0.05, 0.02)[:290 - 17 * k] for k in range(8)]
    exp = expect(refs, reads, SC, AUTO)
    ctx.set_option("zero_copy", zero_copy)
    b, _ = run_and_check(ctx, refs, reads, SC, AUTO, exp=exp)
    assert b.timing().fill_launches == 1
    b.free()
    b, _ = run_and_check(ctx, refs, reads, SC, AUTO, exp=exp, scores_only=1)
    b.free()
    ctx.set_option("scores_only", 0)
    ctx.set_option("max_workspace_bytes", 1 << 20)
    b, _ = run_and_check(ctx, refs, reads, SC, AUTO, exp=exp)
    assert b.timing().fill_launches > 1
    b.free()


def test_async_run_keeps_the_value_it_was_asked_with(ctx):
    rng = random.Random(9291)
    read = u.rand(rng, 40)
    ref, ends = planted(rng, read, (25, 37, 25), (0, 3))
    d = ends[1] - ends[0]
    p = sw.make_params(SC[:3])
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("subopt", d - 1)
    ctx.set_option("debug_async_delay_us", 20000)
    b = ctx.upload([ref], [read]).run_async(p)
    ctx.set_option("subopt", d)                               # does not reach the run in flight
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    check(b, [ref], [read], expect([ref], [read], SC, d - 1))
    assert b.subopt(0)[1] == ends[1]
    b.run(p)                                                  # ... but the next one
    check(b, [ref], [read], expect([ref], [read], SC, d))
    assert b.subopt(0)[1] != ends[1]
    b.free()


@pytest.mark.parametrize("keep", [1, 0])
def test_stream_of_two_chunks(ctx, keep):
    rng = random.Random(9292)
    base = u.rand(rng, 300)
    refs = [u.mutate(rng, base, 0.05, 0.02) + base[100:160] for _ in range(6)]
    reads = [base[30:180], u.mutate(rng, base[100:260], 0.05, 0.02)]
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("subopt", 12)
    ctx.set_option("stream_keep_records", keep)
    st = ctx.stream(reads, sw.make_params(SC[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("subopt", 0)                               # (the stream keeps the value it was opened with)
    st.push(refs[:3]).push(refs[3:]).finish()
    chunks = st.chunks()
    assert [first for first, _ in chunks] == [0, 3]
    for first, c in chunks:
        part = refs[first:first + 3]
        assert c.pipeline_mode() == 3
        check(c, part, reads, expect(part, reads, SC, 12))
    st.close()


def test_pair_list_overlapping_windows_and_reversed(ctx):
    rng = random.Random(9293)
    read = u.rand(rng, 80)
    src, ends = planted(rng, read, (100, 70, 90, 60), (0, 4, 7))
    refs, reads = [src], [u.rand(rng, 10) + read + u.rand(rng, 10)]
    specs = [(0, 0, 40, 300, 10, 80), (0, 0, 120, 350, 10, 80), (0, 0, 40, 420, 5, 90, True), (0, 0)]
    for name, v in dict(gap_open=SC[3], align_mode=LOCAL, subopt=30).items():
        ctx.set_option(name, v)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    assert b.pipeline_mode() == 3
    s2, e2 = b.subopts()
    for k in range(len(specs)):
        ref, rd = b.segments(k)
        want = sr.subopt_numpy(ref, rd, SC, 30)
        assert (b.score(k),) + b.subopt(k) == want, k
        assert (int(s2[k]), int(e2[k])) == want[1:]
        assert want[1] > 0
    # end2 is the segment's column: the source byte it names holds the last base of the copy it ends on
    j = b.subopt(0)[1]
    assert b.to_source(0, 1, j)[1] == 40 + j - 1 and 40 + j in ends
    j = b.subopt(2)[1]
    assert b.to_source(2, 1, j)[1] == 40 + 420 - j
    b.free()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rng = random.Random(9294)
    read = u.rand(rng, 40)
    ref, _ = planted(rng, read, (25, 37, 25), (0, 3))
    exp = expect([ref], [read], SC, 7)
    # values outside -1 .. 2^30 leave the context as it was
    ctx.set_option("subopt", 7)
    for bad in (-2, (1 << 30) + 1):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("subopt", bad)
        assert e.value.code == ERR_INVALID and "subopt" in str(e.value)
    ctx.set_option("subopt", 1 << 30)
    ctx.set_option("subopt", 7)
    b = u.run(ctx, [ref], [read], SC, 0, LOCAL)
    check(b, [ref], [read], exp)
    # a pair out of range
    with pytest.raises(_capi.SwmiError) as e:
        b.subopt(1)
    assert e.value.code == ERR_RANGE
    # fit and global: refused before anything is launched, the message names the option
    p = sw.make_params(SC[:3])
    for mode in (FIT, GLOBAL):
        ctx.set_option("align_mode", mode)
        for extend in ((0, 1) if mode == GLOBAL else (0,)):
            ctx.set_option("extend", extend)
            with pytest.raises(_capi.SwmiError) as e:
                b.run(p)
            assert e.value.code == ERR_UNSUPPORTED and "subopt" in str(e.value)
    ctx.set_option("extend", 0)
    ctx.set_option("align_mode", LOCAL)
    # a run with subopt = 0: the accessors are refused
    ctx.set_option("subopt", 0)
    b.run(p)
    for call in (lambda: b.subopt(0), b.subopts):
        with pytest.raises(_capi.SwmiError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED and "subopt" in str(e.value)
    assert b.score(0) == exp[(0, 0)][0]
    b.free()
