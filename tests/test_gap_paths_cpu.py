"""The inputs of tests/test_gap_paths_gpu.py are as sharp as they claim (tests/gap_path_cases.py) -- proven on the CPU.

A halo case is worth running only if the pair's optimum really is the ratchet (it begins at the planted column), spans nearly
path_span columns, begins within the slack cap of the column its chunk starts at, and loses score to a sweep that
starts at the first window edge past the path's first column.  A bound case is worth running only if the optimum has nearly path_bound moves.  The
thresholds (0.93 of the bound, a slack of at most 0.06 * span + 96 columns) are conditions on the inputs, met by the oracle
alone; every figure is printed (pytest -s).

The second sweep starts slack // 32 + 1 windows further right, where slack is the distance from the chunk's first column to the
path's: up to 7 windows.  Only the placements with a slack below 32 columns (a of m99 and m255 at (5, -3, -4), a of m255 and m256
at (4, -6, -5)) would notice a halo that is ONE window short; the others notice one that is short by their slack.

Figures of the cases as committed: halo cases spanned / path_span 0.937 .. 0.994, slack 21 .. 203 columns for the placements
a, b, ca, cb (up to 1018 for d, which sits inside its chunk by design); bound cases moves / path_bound 0.942 .. 0.988."""
import random

import pytest

from oracle import sw_oracle as orc

import gap_path_cases as gp
import gotoh_reference as gr

HALO = gp.HALO_SINGLE + gp.HALO_MULTI


@pytest.fixture(scope="module")
def optimum():
    """{(m, scores, label): (score, alignments)} of the halo cases, computed once"""
    memo = {}

    def get(m, scores, x):
        key = (m, scores, x)
        if key not in memo:
            c = gp.halo_case(m, scores)
            memo[key] = orc.opt_alignments((c.refs[x], c.read), scores)
        return memo[key]
    return get


def test_ratchet_parameters():
    """the k of every score set, the runs of the plain formula d = (match * k - 1) // |gap|, and a score set with |gap| > match > 1"""
    assert gp.RATCHET == {(5, -3, -4): (9, 9, 6), (7, -8, -1): (3, 8, 1), (4, -6, -5): (4, 4, 1)}
    assert all(sc[1] < 0 for sc in gp.HALO_SCORES) and any(-sc[2] > sc[0] > 1 for sc in gp.HALO_SCORES)
    body, read, gaps = gp.ratchet(random.Random(1), 256, (7, -8, -1), 8, "del")
    assert len(read) == 256 and gaps == 31 * 55 and len(body) == 256 + gaps == 1961 and "T" not in read
    assert body.replace("T", "") == read
    ref, read, gaps = gp.ratchet(random.Random(1), 32, (7, -8, -1), 1, "ins", tight=1)
    assert len(ref) == 32 and gaps == 6 + 29 * 7 + 6 and read.replace("T", "") == ref
    assert gp.planted("ACG", 10, 7) == "TTTTACGTTT"


def test_restated_plan_by_hand():
    """the restatement against values worked out by hand from swmi_plan.h"""
    assert gp.path_span(150, (5, -3, -4)) == 150 + 187 + 1 and gp.path_span(256, (7, -8, -1)) == 2049
    assert gp.path_bound(2000, 256, (7, -8, -1)) == 2048 and gp.path_bound(32, 256, (7, -8, -1)) == 256
    assert gp.path_bound(40, 330, (7, -8, -1)) == 320 and gp.path_bound(10, 10, (5, -3, -4), align_mode=1) == 20
    assert gp.ck_windows(1) == 2 and gp.ck_windows(4100) == 131
    # 150 x 4100, 4 pairs, automatic: min(256, 4100 // 402, 131) = 10 chunks of 14 windows
    chunks = gp.plan_chunks(150, 4100, (5, -3, -4), 4, 0)
    assert [c[0] for c in chunks] == list(range(0, 131, 14)) and chunks[-1][1] == 131
    assert chunks[1] == (14, 28, 32) and chunks[2] == (28, 42, (28 * 32 - 65 - 338) // 32 * 32)
    assert gp.plan_chunks(150, 4100, (5, -3, -4), 4, 1) == [] and gp.plan_chunks(150, 4100, (5, -3, -4), 600, 0) == []
    assert gp.plan_chunks(150, 700, (5, -3, -4), 4, 7) == []                   # 700 // 402 < 2
    # 520 x 2600 (three strips): automatic budget 256 // 3, bodies of (1171 + 64) // 4 columns
    assert len(gp.plan_chunks(520, 2600, (5, -3, -4), 4, 0)) == len(gp._chunk_list(2600 // 308, 2600, 1171))
    assert gp.end_lane(99) == 49 and gp.end_lane(256) == 63 and gp.end_lane(300) == 10 and gp.end_lane(520) == 1


@pytest.mark.parametrize("case", HALO, ids=gp.halo_id)
def test_halo_case_layout(case):
    """at least three chunks behind a halo, the same plan whether the chunk count is forced or automatic (4 pairs or 1 per
    launch), every placement where it claims to be"""
    m, sc = case
    c = gp.halo_case(m, sc)
    assert sum(1 for ch in c.chunks if ch[2] > 0) >= 3
    for n_pairs in (4, 1):
        assert tuple(gp.plan_chunks(m, c.n, sc, n_pairs, 0)) == c.chunks
    assert gp.plan_chunks(m, c.n, sc, 4, 1) == []
    first = gp._first_behind_a_halo(c.chunks)
    by = {p.label: p for p in c.places}
    assert by["a"].chunk == by["b"].chunk == first
    assert by["ca"].chunk == by["cb"].chunk == len(c.chunks) - 1 and c.chunks[-1][1] == gp.ck_windows(c.n)
    for lo, hi in (("a", "b"), ("ca", "cb")):
        g_lo = c.chunks[by[lo].chunk][0]
        assert gp.end_step(m, by[lo].end_col) == g_lo * gp.STEP_W                  # first step of the first owned window
        assert gp.end_step(m, by[hi].end_col) == g_lo * gp.STEP_W + gp.STEP_W - 1    # ... and its last
    d = by["d"]
    begins_in = max(x for x, ch in enumerate(c.chunks) if ch[0] * gp.STEP_W < d.end_col - c.body_cols + 1)
    assert d.chunk > first and begins_in < d.chunk                                  # the walk crosses a chunk edge
    assert all(len(r) == c.n for r in c.refs) and len(c.read) == m


@pytest.mark.parametrize("case", HALO, ids=gp.halo_id)
def test_halo_case_is_sharp(case, optimum):
    m, sc = case
    c = gp.halo_case(m, sc)
    span = gp.path_span(m, sc)
    for x, (p, ref) in enumerate(zip(c.places, c.refs)):
        es, ea = optimum(m, sc, x)
        first_col, cols, moves = gp.path_columns(ea[0])
        col0 = c.chunks[p.chunk][2]
        slack = first_col - 1 - col0
        print("halo %s %s: n %d, spanned %d / path_span %d = %.3f, moves %d / path_bound %d = %.3f, col0 %d, slack %d (cap %.1f)"
              % (gp.halo_id(case), p.label, c.n, cols, span, cols / span, moves, gp.path_bound(c.n, m, sc),
                 moves / gp.path_bound(c.n, m, sc), col0, slack, 0.06 * span + 96))
        assert first_col == p.end_col - c.body_cols + 1 and cols == c.body_cols and moves == m + c.gaps, p.label
        assert cols >= 0.93 * span, p.label
        assert col0 > 0 and slack >= 0, p.label
        if p.label != "d":
            assert slack <= 0.06 * span + 96, p.label
        else:                          # d sits further inside its chunk by design: its walk crosses the edge behind it
            assert first_col <= c.chunks[p.chunk][0] * gp.STEP_W, p.label
        assert gp.cut_sweep_max(ref, c.read, sc, col0) == es, p.label
        assert gp.cut_sweep_max(ref, c.read, sc, col0 + gp.STEP_W * (slack // gp.STEP_W + 1)) < es, p.label


def test_cut_sweep_is_the_oracle_sweep():
    """cut_sweep_max from column 1 is the pair's score, on random pairs too"""
    rng = random.Random(77)
    for sc in gp.HALO_SCORES + ((2, -1, -3),):
        for _ in range(4):
            ref = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 300)))
            read = "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 80)))
            assert gp.cut_sweep_max(ref, read, sc, 0) == orc.opt_alignments((ref, read), sc)[0]


@pytest.mark.parametrize("name", gp.BOUND_NAMES)
def test_bound_case_is_near_the_bound(name):
    c = gp.bound_case(name)
    r, q = c.near
    n, m = len(c.refs[r]), len(c.reads[q])
    bound = gp.path_bound(n, m, c.scores)
    assert bound == max(gp.path_bound(len(ref), len(read), c.scores) for ref in c.refs for read in c.reads)
    es, ea = orc.opt_alignments((c.refs[r], c.reads[q]), c.scores)
    _, cols, moves = gp.path_columns(ea[0])
    print("bound %s: %d x %d, moves %d / path_bound %d = %.3f" % (name, m, n, moves, bound, moves / bound))
    assert 0.93 * bound <= moves <= bound
    assert max(len(a[1][0]) for a in ea) <= bound


def test_bound_case_shapes():
    assert tuple(c.name for c in gp.bound_cases()) == gp.BOUND_NAMES
    sizes = {c.name: (len(c.refs[c.near[0]]), len(c.reads[c.near[1]])) for c in gp.bound_cases()}
    assert sizes["del-256x2000"] == (2000, 256) and sizes["ins-32x256"] == (32, 256) and sizes["ins-40x330-seam"] == (40, 330)
    for name in gp.RESIDENT_NAMES:
        n, m = sizes[name]
        assert gp.res_size_fits(m, n, gp.bound_case(name).scores), name
    n, m = sizes["del-90x740-resident"]
    assert gp.res_need_words(m, n, (7, -8, -1)) * 4 > 36 * 1024                    # ... and fills its 40 KB
    # the seam of the two strips of the 330-base read runs through an insertion run, whose rows also cross lanes (4 rows each)
    read = gp.bound_case("ins-40x330-seam").reads[0]
    used = read.rstrip("T")                                                        # (up to the last segment)
    lo = hi = 255                                                                  # 0-based index of row 256
    while read[lo - 1] == "T":
        lo -= 1
    while read[hi + 1] == "T":
        hi += 1
    assert read[255] == "T" and read[256] == "T" and lo > gp.INS_SEAM_FRONT and hi + 1 < len(used) and hi - lo + 1 >= 6
    mixed = gp.bound_case("shapes-2x2")
    assert len({len(x) for x in mixed.refs}) == 2 and len({len(x) for x in mixed.reads}) == 2 and mixed.near == (1, 1)
    # ... which the planner meets first: the schedule is longest first
    assert gp.schedule([len(x) for x in mixed.refs], [len(x) for x in mixed.reads])[0] == mixed.near


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_memo_case_reaches_the_memo(mode):
    """under memo_cap the planner meets, in one launch, a pair of a small bound and then the near-bound pair of the same
    reference length: a memo that is not refreshed when only the read length changes, or never, plans too short a path there.
    (One keyed on the read length alone cannot be caught through the API: references come in descending length, so under one
    read length the bound never grows within a launch.)"""
    c = gp.memo_case()
    ref_lens, read_lens = [len(x) for x in c.refs], [len(x) for x in c.reads]
    assert ref_lens == [gp.MEMO_N, gp.MEMO_N, 40] and read_lens == [128, 64, 24]
    cap = gp.memo_cap(mode)
    assert cap >= 1 << 20                                                          # the option's minimum
    cut = gp.launches(ref_lens, read_lens, mode, cap)
    assert cut[0] == [(0, 0), (0, 1)] and cut[1] == [(0, 2), c.near] and sum(len(x) for x in cut) == 9
    bound = gp.path_bound(gp.MEMO_N, 128, c.scores)
    assert gp.planned_max_path(cut[1], ref_lens, read_lens, c.scores) == bound == 1024
    assert gp.planned_max_path(cut[1], ref_lens, read_lens, c.scores, "n") == gp.path_bound(gp.MEMO_N, 24, c.scores) == 192
    assert gp.planned_max_path(cut[1], ref_lens, read_lens, c.scores, "") == 192
    for x in cut:                                                                  # the read length alone: never too short
        assert gp.planned_max_path(x, ref_lens, read_lens, c.scores, "m") >= gp.planned_max_path(x, ref_lens, read_lens, c.scores)
    es, ea = orc.opt_alignments((c.refs[c.near[0]], c.reads[c.near[1]]), c.scores)
    moves = len(ea[0][1][0])
    print("bound memo (mode %d): cap %d bytes, launches %s, moves %d / path_bound %d = %.3f"
          % (mode, cap, [len(x) for x in cut], moves, bound, moves / bound))
    assert len(ea) == 1 and 0.93 * bound <= moves <= bound
    for r, ref in enumerate(c.refs):                                               # no pair is degenerate
        for read in c.reads:
            assert orc.opt_alignments((ref, read), c.scores)[0] > 0


def test_affine_case_is_near_the_bound():
    ref, read, want_moves = gp.affine_case()
    es, ea = gr.align_numpy(ref, read, gp.AFFINE_SCORES)
    bound = gp.path_bound(len(ref), len(read), gp.AFFINE_SCORES[:3])
    moves = len(ea[0][1][0])
    print("bound affine: %d x %d, moves %d / path_bound %d = %.3f" % (len(read), len(ref), moves, bound, moves / bound))
    assert moves == want_moves and 0.93 * bound <= moves <= bound
