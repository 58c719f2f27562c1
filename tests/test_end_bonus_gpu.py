"""Option "end_bonus" on the GPU (the ENDB sweeps of swmi_affine.hip): every pair's score, flags, alignments,
max_score, end_score and end_col against tests/end_bonus_reference.py, exactly.  set_option("end_bonus", ...) and the two accessors
are what fail without the feature.

The cases are chosen where the tracker of read row m can go wrong: every rows-per-lane class with the owner lane below and at 63,
the first and the last slot of a strip's lanes, the 8-column blocks' edges, the strict choice on either side of the bonus, the
smallest column on a tie, the band's last window -- and the host machinery around the per-pair array: zero-copy or not, several
launches, the exact-size re-run, the arena retry, async, streams, pair lists."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M

import affine_gpu_util as u
import cigar_reference as cr
import end_bonus_reference as er

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -5, -6       # swmi_status (include/swmi.h)
LOCAL, FIT, GLOBAL = sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL
SC = (5, -4, -3, -5)
TIE = (5, -3, -3, -5)
ALL = 1 << 30                                               # the largest bonus: every pair is taken to the end
# N scores 0 against everything: a read base that neither gains nor loses, so two cells of the diagonal tie
NMAT = ("ACGTN", [[0 if "N" in (a, c) else (5 if a == c else -4) for c in "ACGTN"] for a in "ACGTN"])


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def expect(refs, reads, sc, b, w=0, tie=0, matrix=None):
    return {(r, q): er.align(refs[r], reads[q], sc, b, w, tie, matrix) for r in range(len(refs)) for q in range(len(reads))}


def check_pair(b, pair, want, what=None, alignments=True, ends=None, flags=True):
    """alignments=False: the records are not strings (option "cigar") or not kept; flags=False: nor are the counts (scores_only)"""
    score, alns, cells, took, want_ends = want
    assert b.score(pair) == score, (what, b.score(pair), score)
    assert b.end_score(pair) == want_ends, (what, b.end_score(pair), want_ends)
    if ends is not None:
        assert tuple(int(a[pair]) for a in ends) == want_ends, (what, pair)
    if alignments:
        assert b.n_alignments(pair) == (len(alns), sw.PAIR_TO_END if took else 0), (what, b.n_alignments(pair), len(alns), took)
        assert b.alignments(pair, with_cell=True) == [a + (c,) for a, c in zip(alns, cells)], what
    elif flags:
        assert b.n_alignments(pair) == (len(alns), sw.PAIR_TO_END if took else 0), what


def check(b, refs, reads, exp, what=None, alignments=True, flags=True):
    """every pair: score, flags, alignments with their cells, and the three values through both accessors"""
    ends = b.end_scores()
    assert all(len(a) == len(refs) * len(reads) for a in ends)
    for r in range(len(refs)):
        for q in range(len(reads)):
            check_pair(b, r * len(reads) + q, exp[(r, q)], (what, r, q, len(refs[r]), len(reads[q])), alignments, ends, flags)


def run_and_check(ctx, refs, reads, sc, bonus, band=None, matrix=None, tie=0, exp=None, alignments=True, **options):
    exp = exp or expect(refs, reads, sc, bonus, band or 0, tie, matrix)
    b = u.run(ctx, refs, reads, sc, tie, GLOBAL, band, 1, matrix=matrix, end_bonus=bonus, **options)
    check(b, refs, reads, exp, (bonus, band, tie), alignments and not options.get("scores_only"), not options.get("scores_only"))
    return b, exp


def took(exp):
    return [v[3] for v in exp.values()]


# ---- which lane owns row m ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 100, 256, 257, 1024])
def test_owner_lane_short_reads(ctx, m):
    """R = 1, 2, 4, 5, 16; the lane that owns row m is below 63 (m = 1, 63, 65, 100, 257) and 63 (64, 256, 1024): the narrow and the wide
    kernel.  The references end before, at and behind the read's end; a bonus that takes none or few, one in between, and every pair"""
    rng = random.Random(9300 + m)
    base = u.rand(rng, 1100)
    read = base[30:30 + m]
    refs = [u.mutate(rng, base[30:30 + n], 0.06, 0.01)[:n] for n in (m + 40, m + 3, max(1, m - 7), 8)] + [read + "G", read]
    seen = []
    for bonus in (1, 9, ALL):
        b, exp = run_and_check(ctx, refs, [read], SC, bonus)
        seen += took(exp)
        b.free()
    assert True in seen and (False in seen or m == 1)


@pytest.mark.parametrize("band", [0, 32])
@pytest.mark.parametrize("m", [1025, 1500, 2048])
def test_owner_lane_strips(ctx, m, band):
    """row m lies in the last strip alone: slot 0 of lane 0 (m = 1025), a lane in between (1500), slot 15 of lane 63 (2048).  Under
    band 32 the row's cells are the last window's"""
    rng = random.Random(9310 + m)
    read = u.rand(rng, m)
    refs = [u.mutate(rng, read, 0.03, 0.002)[:m - 4] + u.rand(rng, 30), u.mutate(rng, read, 0.05, 0.0)[:m - 1]]
    ctx.set_option("long_reads", 1)
    seen = []
    for bonus in (1, 60, ALL):
        b, exp = run_and_check(ctx, refs, [read], SC, bonus, band=band)
        seen += took(exp)
        if band:
            lo, hi = b.band_window(0, (m - 1) // 1024)
            assert all(lo <= v[4][2] <= hi for v in exp.values())
        b.free()
    assert True in seen and False in seen


def test_block_edges(ctx):
    rng = random.Random(9320)
    read = u.rand(rng, 10)
    refs = [(read[:9] + u.rand(rng, 60))[:n] for n in (1, 7, 8, 9, 64, 65)]
    for bonus in (1, ALL):
        b, exp = run_and_check(ctx, refs, [read], SC, bonus)
        b.free()
    assert [exp[(r, 0)][4][2] for r in range(4)] == [1, 7, 8, 9]          # end_col = n


# ---- the choice --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [100, 1500])
def test_choice_is_strict(ctx, m):
    """the read is a prefix of the reference with its last base substituted: the best cell is (m - 1, m - 1) and row m is 4 worse, at
    column m.  Bonus 4 leaves the pair alone, bonus 5 takes it to the end"""
    rng = random.Random(9330 + m)
    ref = u.rand(rng, m + 40)
    read = ref[:m - 1] + next(c for c in "ACGT" if c not in ref[m - 1:m + 2])
    ctx.set_option("long_reads", 1)
    at, exp4 = run_and_check(ctx, [ref], [read], SC, 4)
    over, exp5 = run_and_check(ctx, [ref], [read], SC, 5)
    assert exp4[(0, 0)][4] == exp5[(0, 0)][4] == (5 * (m - 1), 5 * (m - 1) - 4, m)
    assert exp4[(0, 0)][2] == [(m - 1, m - 1)] and not exp4[(0, 0)][3]
    assert exp5[(0, 0)][2] == [(m, m)] and exp5[(0, 0)][3]
    assert at.score(0) == 5 * (m - 1) and over.score(0) == 5 * (m - 1) - 4
    at.free()
    over.free()


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("m", [20, 1030])
def test_end_col_is_the_smallest_column_on_a_tie(ctx, m, tie):
    """P + "T" against P + "GT" + tail: row m ties at columns m and m + 1"""
    rng = random.Random(9340 + m)
    P = u.rand(rng, m - 1)
    read, ref = P + "T", P + "GT" + u.rand(rng, 12)
    ctx.set_option("long_reads", 1)
    b, exp = run_and_check(ctx, [ref], [read], TIE, 4, tie=tie)
    H = er.xr._matrices_numpy(ref, read, TIE, 0, tie, None, 1024)[1]
    assert int(H[m][m]) == int(H[m][m + 1]) == 5 * (m - 1) - 3 == int(H[m][1:].max())
    assert exp[(0, 0)][3] and exp[(0, 0)][4] == (5 * (m - 1), 5 * (m - 1) - 3, m)
    b.free()


# ---- the to-end pair itself, and the pair that is not taken ------------------------------------------------------------------
def everything(b, n_pairs, cigar):
    out = []
    for p in range(n_pairs):
        out.append((b.score(p), b.n_alignments(p), b.cigars(p) if cigar else b.alignments(p, with_cell=True)))
    return out


@pytest.mark.parametrize("m,band", [(150, 0), (1500, 0), (1500, 32)])
def test_to_end_alignment_and_cigar(ctx, m, band):
    """the walk from (m, end_col) in the short, the long and the banded walk: strings, begin / end_i / end_j, and under option "cigar"
    the CIGAR and nm of those strings"""
    rng = random.Random(9350 + m + band)
    read = u.rand(rng, m)
    refs = [u.mutate(rng, read, 0.04, 0.004)[:m - 2] + u.rand(rng, 25), u.mutate(rng, read[:m - 20], 0.03, 0.002) + u.rand(rng, 40)]
    ctx.set_option("long_reads", 1)
    b, exp = run_and_check(ctx, refs, [read], SC, ALL, band=band)
    assert all(took(exp))
    for p in range(2):
        (begin, (ra, qa)), (ei, ej) = exp[(p, 0)][1][0], exp[(p, 0)][2][0]
        assert (begin, ei, ej) == (1, m, exp[(p, 0)][4][2]) and b.n_alignments(p) == (1, sw.PAIR_TO_END)
    b.free()
    for cigar in (1, 2):
        b, _ = run_and_check(ctx, refs, [read], SC, ALL, band=band, exp=exp, alignments=False, cigar=cigar)
        for p in range(2):
            (begin, (ra, qa)), (ei, ej) = exp[(p, 0)][1][0], exp[(p, 0)][2][0]
            ent, nm = cr.cigar(ra, qa, cigar)
            assert b.cigars(p) == [(begin, ei, ej, ent, nm)], (p, cigar)
        b.free()
    ctx.set_option("cigar", 0)


@pytest.mark.parametrize("cigar", [0, 2])
def test_a_pair_that_is_not_taken_is_the_run_without_the_option(ctx, cigar):
    rng = random.Random(9360)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300] for _ in range(3)] + ["CCCC"]
    reads = [u.mutate(rng, base, 0.05, 0.02)[:150] + u.rand(rng, 30), base[:90] + u.rand(rng, 25), "AAAA"]
    exp = expect(refs, reads, SC, 1)
    assert took(exp).count(False) >= 9
    off = u.run(ctx, refs, reads, SC, 0, GLOBAL, None, 1, end_bonus=0, cigar=cigar)
    want = everything(off, 12, cigar)
    with pytest.raises(_capi.SwmiError) as e:
        off.end_score(0)
    assert e.value.code == ERR_UNSUPPORTED and "end_bonus" in str(e.value)
    off.free()
    b, _ = run_and_check(ctx, refs, reads, SC, 1, exp=exp, alignments=not cigar, cigar=cigar)
    got = everything(b, 12, cigar)
    for k, v in enumerate(exp.values()):
        if not v[3]:
            assert got[k] == want[k], k
    b.free()
    ctx.set_option("cigar", 0)


def test_empty_sides(ctx):
    refs, reads = ["ACGTACGT", ""], ["ACGT", ""]
    b, exp = run_and_check(ctx, refs, reads, SC, 3)
    assert exp[(0, 1)] == exp[(1, 0)] == exp[(1, 1)] == er.EMPTY and exp[(0, 0)][3]
    assert [b.end_score(p) for p in (1, 2, 3)] == [(0, 0, 0)] * 3 and b.n_alignments(1) == (0, 0)
    b.free()


# ---- mixed launches ----------------------------------------------------------------------------------------------------------
def test_taken_and_not_taken_short_and_long_in_one_launch(ctx):
    rng = random.Random(9370)
    long_ = u.rand(rng, 1100)
    short = long_[:150]
    reads = [short, long_, long_[:64]]
    refs = [u.mutate(rng, long_, 0.03, 0.002) + u.rand(rng, 20),           # reaches every read's end
            long_[:1000] + u.rand(rng, 150),                               # the long read's tail does not match
            short[:120] + u.rand(rng, 60)]                                 # ends long before the long read does
    ctx.set_option("long_reads", 1)
    b, exp = run_and_check(ctx, refs, reads, SC, 5)
    assert b.timing().fill_launches == 1
    # (random tails still align a little under SC: the long read's end lies 9 below its best score on reference 1, far below on 2)
    assert exp[(0, 1)][3] and not exp[(1, 1)][3] and not exp[(2, 1)][3] and exp[(0, 0)][3] and exp[(1, 0)][3]
    b.free()


# ---- the exact-size re-run ---------------------------------------------------------------------------------------------------
def test_exact_size_rerun_applies_to_a_pair_that_is_not_taken_only(ctx):
    """Q + "N" against Q + "G": under NMAT cells (q, q) and (q + 1, q + 1) tie at the maximum, and the read's tail loses 8.  With
    cell_cap 1 the list overflows: the pair is re-run when it is not taken, and is not when it is (its one cell replaces the list)"""
    rng = random.Random(9380)
    Q = u.rand(rng, 30)
    read, ref = Q + "NTT", Q + "GCC" + "C" * 10
    exp1, expall = expect([ref], [read], SC, 1, matrix=NMAT), expect([ref], [read], SC, ALL, matrix=NMAT)
    assert exp1[(0, 0)][2] == [(30, 30), (31, 31)] and not exp1[(0, 0)][3] and expall[(0, 0)][3]
    b, _ = run_and_check(ctx, [ref], [read], SC, 1, matrix=NMAT, exp=exp1, cell_cap=1)
    assert b.timing().rerun_pairs == 1
    b.free()
    b, _ = run_and_check(ctx, [ref], [read], SC, ALL, matrix=NMAT, exp=expall, cell_cap=1)
    assert b.timing().rerun_pairs == 0
    b.free()
    b, _ = run_and_check(ctx, [ref], [read], SC, 1, matrix=NMAT, exp=exp1, cell_cap=64)
    assert b.timing().rerun_pairs == 0
    b.free()


# ---- options -----------------------------------------------------------------------------------------------------------------
def test_score_matrix(ctx):
    rng = random.Random(9390)
    amino = "ARNDCQEGHILKMFPSTWYV"
    short, long_ = u.rand(rng, 70, amino), u.rand(rng, 1100, amino)
    refs = [u.mutate(rng, short, 0.1, 0.0, amino)[:66] + u.rand(rng, 30, amino), u.mutate(rng, long_, 0.1, 0.002, amino) + u.rand(rng, 10, amino)]
    sc = (1, -1, -1, -11)
    mat = (M.BLOSUM62.alphabet, M.BLOSUM62.scores)
    ctx.set_option("long_reads", 1)
    seen = []
    for bonus in (2, ALL):
        b, exp = run_and_check(ctx, refs, [short, long_], sc, bonus, matrix=mat)
        seen += took(exp)
        b.free()
    b, exp = run_and_check(ctx, refs[1:], [short, long_], sc, 30, band=48, matrix=mat)      # (the long reference: no window is empty)
    b.free()
    assert True in seen and False in seen


def test_strict_tie_mode(ctx):
    rng = random.Random(9391)
    long_ = u.rand(rng, 1100)
    reads = [long_[:150], long_]
    refs = [u.mutate(rng, long_, 0.04, 0.004)[:1090] + u.rand(rng, 30), long_[:140] + u.rand(rng, 40)]
    ctx.set_option("long_reads", 1)
    for bonus in (12, ALL):
        b, exp = run_and_check(ctx, refs, reads, SC, bonus, tie=1)
        b.free()
    assert all(took(exp))


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_zero_copy_scores_only_and_several_launches(ctx, zero_copy):
    rng = random.Random(9392)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300 - 11 * k] for k in range(8)]
    reads = [u.mutate(rng, base, 0.05, 0.02)[:290 - 17 * k] for k in range(8)]
    exp = expect(refs, reads, SC, 25)
    t = took(exp)
    assert True in t and False in t
    ctx.set_option("zero_copy", zero_copy)
    b, _ = run_and_check(ctx, refs, reads, SC, 25, exp=exp)
    assert b.timing().fill_launches == 1
    b.free()
    b, _ = run_and_check(ctx, refs, reads, SC, 25, exp=exp, scores_only=1)
    with pytest.raises(_capi.SwmiError):
        b.alignment(0, 0)
    b.free()
    ctx.set_option("scores_only", 0)
    ctx.set_option("max_workspace_bytes", 1 << 20)
    b, _ = run_and_check(ctx, refs, reads, SC, 25, exp=exp)
    assert b.timing().fill_launches > 1
    b.free()


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_arena_retry_keeps_the_array(ctx, zero_copy):
    """two alignments of 1,500 columns do not fit the smallest record arena: the traceback is repeated with a larger one, and the sweep
    is not -- the array it left comes back with the pair outputs"""
    rng = random.Random(9393)
    read = u.rand(rng, 1500)
    refs = [u.mutate(rng, read, 0.03, 0.002) + u.rand(rng, 20), u.mutate(rng, read, 0.03, 0.002)[:1480]]
    ctx.set_option("long_reads", 1)
    ctx.set_option("zero_copy", zero_copy)
    ctx.set_option("arena_words_per_pair", 1)
    b, exp = run_and_check(ctx, refs, [read], SC, ALL)
    assert all(took(exp))
    b.free()


def test_async_run_keeps_the_value_it_was_asked_with(ctx):
    rng = random.Random(9394)
    m = 60
    ref = u.rand(rng, m + 30)
    read = ref[:m - 1] + next(c for c in "ACGT" if c not in ref[m - 1:m + 2])
    p = sw.make_params(SC[:3])
    for name, v in dict(gap_open=SC[3], align_mode=GLOBAL, extend=1, end_bonus=5, debug_async_delay_us=20000).items():
        ctx.set_option(name, v)
    b = ctx.upload([ref], [read]).run_async(p)
    ctx.set_option("end_bonus", 4)                            # does not reach the run in flight
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    check(b, [ref], [read], expect([ref], [read], SC, 5))
    assert b.n_alignments(0) == (1, sw.PAIR_TO_END)
    b.run(p)                                                  # ... but the next one
    check(b, [ref], [read], expect([ref], [read], SC, 4))
    assert b.n_alignments(0) == (1, 0)
    b.free()


@pytest.mark.parametrize("keep", [1, 0])
def test_stream_of_two_chunks(ctx, keep):
    rng = random.Random(9395)
    base = u.rand(rng, 300)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:200 + 15 * k] for k in range(6)]
    reads = [base[:180], u.mutate(rng, base[:260], 0.05, 0.02)]
    for name, v in dict(gap_open=SC[3], align_mode=GLOBAL, extend=1, end_bonus=15, stream_keep_records=keep).items():
        ctx.set_option(name, v)
    st = ctx.stream(reads, sw.make_params(SC[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("end_bonus", 0)                            # (the stream keeps the value it was opened with)
    st.push(refs[:3]).push(refs[3:]).finish()
    chunks = st.chunks()
    assert [first for first, _ in chunks] == [0, 3]
    seen = []
    for first, c in chunks:
        part = refs[first:first + 3]
        assert c.pipeline_mode() == 3
        exp = expect(part, reads, SC, 15)
        seen += took(exp)
        check(c, part, reads, exp, alignments=bool(keep))
    assert True in seen and False in seen
    st.close()


def test_pair_list_with_a_reversed_segment(ctx):
    rng = random.Random(9396)
    read = u.rand(rng, 80)
    src = u.rand(rng, 100) + u.mutate(rng, read, 0.04, 0.0) + u.rand(rng, 60)
    refs, reads = [src], [u.rand(rng, 10) + read + u.rand(rng, 10)]
    # (reference source, read source, reference start, length, read start, length[, reversed]): forward from the copy's start, reversed
    # from its end (left extension), a window that starts too early, whole sources
    specs = [(0, 0, 100, 120, 10, 80), (0, 0, 60, 120, 10, 80, True), (0, 0, 90, 130, 10, 80), (0, 0)]
    for name, v in dict(gap_open=SC[3], align_mode=GLOBAL, extend=1, end_bonus=30).items():
        ctx.set_option(name, v)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    assert b.pipeline_mode() == 3
    ends = b.end_scores()
    flags = []
    for k in range(len(specs)):
        ref, rd = b.segments(k)
        want = er.align(ref, rd, SC, 30)
        check_pair(b, k, want, k, True, ends)
        flags.append(want[3])
    assert flags[0] and flags[1]
    # end_col is the segment's column: in the reversed segment it counts from the segment's last source byte
    j = b.end_score(0)[2]
    assert b.to_source(0, 80, j)[1] == 100 + j - 1
    j = b.end_score(1)[2]
    assert b.to_source(1, 80, j)[1] == 60 + 120 - j
    b.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    rng = random.Random(9397)
    long_ = u.rand(rng, 1100)
    ref, read = u.mutate(rng, long_, 0.03, 0.002), long_[:70]
    exp = expect([ref[:90]], [read], SC, 7)
    # values outside 0 .. 2^30 leave the context as it was
    ctx.set_option("end_bonus", 7)
    for bad in (-1, (1 << 30) + 1):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("end_bonus", bad)
        assert e.value.code == ERR_INVALID and "end_bonus" in str(e.value)
    ctx.set_option("end_bonus", 1 << 30)
    ctx.set_option("end_bonus", 7)
    b = u.run(ctx, [ref[:90]], [read], SC, 0, GLOBAL, None, 1)
    check(b, [ref[:90]], [read], exp)
    # a pair out of range
    with pytest.raises(_capi.SwmiError) as e:
        b.end_score(1)
    assert e.value.code == ERR_RANGE
    p = sw.make_params(SC[:3])

    def refused(batch):
        with pytest.raises(_capi.SwmiError) as e:
            batch.run(p)
        assert e.value.code == ERR_UNSUPPORTED and "end_bonus" in str(e.value)
    # runs that are not extend runs: local, fit, global without extend, and the linear pipeline
    ctx.set_option("extend", 0)
    for mode in (LOCAL, FIT, GLOBAL):
        ctx.set_option("align_mode", mode)
        refused(b)
    ctx.set_option("align_mode", LOCAL)
    ctx.set_option("gap_open", 0)
    refused(b)
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("align_mode", GLOBAL)
    ctx.set_option("extend", 1)
    # xdrop, band_adapt, gap_open2
    ctx.set_option("long_reads", 1)
    lb = ctx.upload([ref], [long_])
    ctx.set_option("xdrop", 100)
    refused(lb)
    refused(b)
    ctx.set_option("xdrop", 0)
    ctx.set_option("band", 64)
    ctx.set_option("band_adapt", 1)
    refused(lb)
    ctx.set_option("band_adapt", 0)
    ctx.set_option("band", 0)
    ctx.set_option("gap2", -1)
    ctx.set_option("gap_open2", -20)
    refused(b)
    ctx.set_option("gap_open2", 0)
    lb.run(p)                                                 # ... and with none of them it runs
    check(lb, [ref], [long_], expect([ref], [long_], SC, 7))
    lb.free()
    # a run with end_bonus = 0: the accessors are refused
    ctx.set_option("end_bonus", 0)
    b.run(p)
    for call in (lambda: b.end_score(0), b.end_scores):
        with pytest.raises(_capi.SwmiError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED and "end_bonus" in str(e.value)
    assert b.score(0) == exp[(0, 0)][4][0] and b.n_alignments(0)[1] == 0
    b.free()
