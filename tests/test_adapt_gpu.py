"""The adaptive band of seed extension on the GPU (option "band_adapt": the sw_affine_sweep_band_adapt[_xdrop][_matrix]_kernel sweeps
and sw_affine_traceback_band_adapt_global_kernel of swmi_affine.hip) against tests/adapt_reference.py: every
score, every alignment with its begin, both strings and its maximum cell, the flags, and swmi_pair_band_window of every strip
swept.  set_option("band_adapt", ...) and Batch.band_window are what fail without the feature.

Every case is built by a function of its own that needs no GPU and asserts, on the reference, the property that makes it a test
(the drift the static band loses, the tie on the seam row, the window that stands still, ...), so a changed generator cannot turn
it vacuous; the results are kept, so the cases of a parametrised test share them.  Every pair has 3 strips or fewer.

  kernel (sw_affine_...)                       run by
  sweep_band_adapt_kernel                      test_adapt_drift, test_adapt_tie_rule, test_adapt_centre_stands_still, ...
  sweep_band_adapt_matrix_kernel               test_adapt_mixed_launch[True], test_adapt_matrix_strict_ties
  sweep_band_adapt_xdrop_kernel                test_adapt_xdrop_*, test_adapt_mixed_launch_xdrop[False]
  sweep_band_adapt_xdrop_matrix_kernel         test_adapt_mixed_launch_xdrop[True], test_adapt_matrix_strict_ties
  traceback_band_adapt_global_kernel           every test but the scores_only case"""
import functools
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import adapt_reference as ar
import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -5, -6       # swmi_status (include/swmi.h)
SC = (5, -3, -2, -6)                                       # the drift cases
SC2 = (2, -4, -2, -4)                                      # the hand-derivable cases: unrelated stretches lose score
GLOBAL = sw.ALIGN_GLOBAL


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# every run of this module is a banded extend run with long reads on
def _run(ctx, refs, reads, w, tie=0, X=0, matrix=None, sc=SC, adapt=1, **options):
    return u.run(ctx, refs, reads, sc, tie, GLOBAL, w, 1, matrix, long_reads=1, xdrop=X, band_adapt=adapt, **options)


def _check_windows(b, pair, wins, m, what=None):
    """band_window of every strip swept is the reference's, and the strips behind them are out of range"""
    assert [b.band_window(pair, s) for s in range(len(wins))] == [tuple(x) for x in wins], (what, wins)
    for s in (len(wins), (m + 1023) // 1024):
        with pytest.raises(_capi.SwmiError) as e:
            b.band_window(pair, s)
        assert e.value.code == ERR_RANGE, what


def _check_pair(b, pair, want, m, what=None):
    """want = (score, alignments, cells, windows[, rows_swept]) of adapt_reference.align"""
    u.check_pair(b, pair, want[:3], GLOBAL, what)
    _check_windows(b, pair, want[3], m, what)
    assert b.rows_swept(pair) == (want[4] if len(want) > 4 else m), what


def _drift_pair(rng, m, every=1000, first=500, extra=40, tail=300):
    """a read of m bases, and the read with `extra` random bases inserted after read bases first, first + every, ... and a random
    tail: the alignment drifts `extra` columns to the right per `every` rows"""
    read = u.rand(rng, m)
    ref, at = "", 0
    for cut in list(range(first, m, every)) + [m]:
        ref += read[at:cut] + (u.rand(rng, extra) if cut < m else "")
        at = cut
    return ref + u.rand(rng, tail), read


# 1 -- drift: 40 extra reference bases per 1000 read bases.  The static band of half-width 48 or 64 loses the alignment (the drift
# adds up to 120), the adaptive one keeps it (40 inside a strip); at 16 neither holds it.  The test that cannot pass by running
# the static band
@functools.lru_cache(maxsize=None)
def _drift_case():
    ref, read = _drift_pair(random.Random(9950), 3000)
    assert (len(read), len(ref)) == (3000, 3420)
    free = gr.align_numpy(ref, read, SC, GLOBAL, 0, True, cells=True)
    assert free[2] == [(3000, 3120)]
    want = {}
    for w in (16, 48, 64):
        static = gr.align_numpy(ref, read, SC, GLOBAL, w, True, cells=True)
        for tie in (0, 1):
            want[(w, tie)] = ar.align(ref, read, SC, w, 0, tie)
        assert want[(w, 0)][3] == want[(w, 1)][3] and want[(w, 0)][3] != gr.windows(3000, 3420, w)
        if w == 16:
            assert want[(w, 0)][:3] != free
        else:
            assert want[(w, 0)][:3] == free and static[0] < free[0], (w, static[0], free[0])
    return ref, read, want


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("w", [16, 48, 64])
def test_adapt_drift(ctx, w, tie):
    ref, read, want = _drift_case()
    b = _run(ctx, [ref], [read], w, tie)
    _check_pair(b, 0, want[(w, tie)], len(read), (w, tie))
    b.free()


# 2 -- the tie rule of p(s), hand-derivable: 1023 common bases, then the read's A against the reference's CA.  On row 1024 the
# maximum 2 * 1023 - 4 is tied at column 1024 (A / C mismatch) and column 1025 (C deleted, A matched) and nowhere else: p(0) is
# the smaller column
@functools.lru_cache(maxsize=None)
def _tie_case(w=32):
    rng = random.Random(9951)
    P, rest = u.rand(rng, 1023), u.rand(rng, 400)
    read = P + "A" + rest
    ref = P + "CA" + rest + u.rand(rng, 100)
    res, H = ar._sweep(True, ref, read[:1024], SC2, [ar.window(0, len(ref), w)], w, 0, None, 1024)
    lo, hi = ar.window(0, len(ref), w)
    top = int(H[1024, lo:hi + 1].max())
    assert top == 2 * 1023 - 4 and [j for j in range(lo, hi + 1) if H[1024, j] == top] == [1024, 1025]
    want = ar.align(ref, read, SC2, w)
    assert len(ref) < 1025 + 1024 + w and want[3][1] == (1024 + 1 - w, len(ref))
    return ref, read, w, want


def test_adapt_tie_rule(ctx):
    ref, read, w, want = _tie_case()
    b = _run(ctx, [ref], [read], w, sc=SC2)
    assert b.band_window(0, 1) == (1024 + 1 - w, len(ref))           # not 1025 + 1 - w
    _check_pair(b, 0, want, len(read))
    b.free()


# 3 -- the centre stands still: rows 1025 .. 2048 of the read have nothing to do with the reference, the best of row 2048 lies at
# or left of the best of row 1024, and strip 2 starts where strip 1 did -- left of it, the seam row holds nothing strip 1 wrote
@functools.lru_cache(maxsize=None)
def _still_case(w=48):
    rng = random.Random(9952)
    head = u.rand(rng, 1024)
    read = head + "A" * 1024 + u.rand(rng, 200)
    ref = head[:400] + u.rand(rng, 30) + head[400:] + "C" * 1400
    want = {tie: ar.align(ref, read, SC2, w, 0, tie) for tie in (0, 1)}
    wins = want[0][3]
    assert len(wins) == 3 and wins[2][0] == wins[1][0] > 1, wins
    return ref, read, w, want


@pytest.mark.parametrize("tie", [0, 1])
def test_adapt_centre_stands_still(ctx, tie):
    ref, read, w, want = _still_case()
    b = _run(ctx, [ref], [read], w, tie, sc=SC2)
    _check_pair(b, 0, want[tie], len(read), tie)
    b.free()


# 4 -- strip edges: reads of 2048, 2049, 1025 and 1024 bases in one launch (the last one is computed in full); and a reference
# far shorter than the read, which the static band refuses
@functools.lru_cache(maxsize=None)
def _edges_case(w=64):
    ref, base = _drift_pair(random.Random(9953), 2049, every=700, first=350, extra=30, tail=100)
    reads = [base[:2048], base, base[:1025], base[:1024]]
    want = [ar.align(ref, q, SC, w) for q in reads]
    assert [len(e[3]) for e in want] == [2, 3, 2, 1] and want[3][3] == [(1, len(ref))]
    assert want[3][:3] == gr.align_numpy(ref, reads[3], SC, GLOBAL, 0, True, cells=True)
    assert want[1][3][1] != gr.windows(2049, len(ref), w)[1]                                  # the windows did move
    return ref, reads, w, want


def test_adapt_strip_edges(ctx):
    ref, reads, w, want = _edges_case()
    b = _run(ctx, [ref], reads, w)
    for q, e in enumerate(want):
        _check_pair(b, q, e, len(reads[q]), len(reads[q]))
    b.free()


@functools.lru_cache(maxsize=None)
def _short_ref_case(w=64):
    rng = random.Random(9954)
    read = u.rand(rng, 3000)
    ref = u.mutate(rng, read[:1500])[:1500]
    ref += u.rand(rng, 1500 - len(ref))
    assert len(ref) == 1500 and gr.refused(3000, 1500, w, GLOBAL, True)
    want = ar.align(ref, read, SC, w)
    assert len(want[3]) == 3 and want[3][2][1] == 1500 and all(lo <= hi for lo, hi in want[3])
    return ref, read, w, want


def test_adapt_short_reference(ctx):
    ref, read, w, want = _short_ref_case()
    b = ctx.upload([ref], [read])
    for name, value in (("gap_open", SC[3]), ("align_mode", GLOBAL), ("extend", 1), ("long_reads", 1), ("band", w), ("band_adapt", 0)):
        ctx.set_option(name, value)
    with pytest.raises(_capi.SwmiError) as e:                     # the static band: strip 2 has an empty window
        b.run(sw.make_params(SC[:3]))
    assert e.value.code == ERR_UNSUPPORTED
    ctx.set_option("band_adapt", 1)
    b.run(sw.make_params(SC[:3]))
    assert b.band_window(0, 2)[1] == 1500
    _check_pair(b, 0, want, 3000)
    b.free()


# 5 -- a mixed launch: short reads, long reads with different drifts and one with none, several pairs per workgroup, plain and
# with the 4 x 4 matrix of affine_grid_cases.score_matrix()
@functools.lru_cache(maxsize=None)
def _mixed_case(matrix, w=64):
    rng = random.Random(9955 + int(matrix))
    mat = gc.score_matrix() if matrix else None
    ref, base = _drift_pair(rng, 2500, every=700, first=350, extra=30, tail=150)
    still = ref[:2300]                                                            # no drift: the static windows
    reads = [base, still, base[:1400], u.mutate(rng, base[:300]), base[:1024], u.mutate(rng, ref[:2100]), base[:90]]
    want = [ar.align(ref, q, SC, w, 0, 0, mat) for q in reads]
    assert want[1][3] == gr.windows(2300, len(ref), w) and want[0][3] != gr.windows(2500, len(ref), w)
    assert [len(e[3]) for e in want] == [3, 3, 2, 1, 1, 3, 1]
    return ref, reads, w, mat, want


@pytest.mark.parametrize("matrix", [False, True])
def test_adapt_mixed_launch(ctx, matrix):
    ref, reads, w, mat, want = _mixed_case(matrix)
    b = _run(ctx, [ref], reads, w, 0, 0, mat)
    for q, e in enumerate(want):
        _check_pair(b, q, e, len(reads[q]), (matrix, q))
    total = int(sum(e[0] for e in want))
    assert b.ref_total(0) == total
    assert b.ref_sites_packed()[0] == (total, 0, sorted([a for e in want for a in e[1]], key=lambda t: t[0]))
    b.free()


# 6 -- with xdrop: the stop test runs on the adaptive windows, on the same pass, and comes first
def _four(d0, d1):
    assert 1 <= d0 < d1, (d0, d1)
    return (d0 - 1, d0, d1 - 1, d1)


@functools.lru_cache(maxsize=None)
def _planted_case(w=64):
    """test_xdrop_gpu's planted head: a common head of 700, then A's against C's -- the one maximum cell is (700, 700)"""
    rng = random.Random(9956)
    h = u.rand(rng, 700)
    ref, read = h + "C" * 2400, h + "A" * 2300
    _, _, drops = ar.trace(ref, read, SC2, w)
    d = [best - seam for best, seam in drops]
    assert len(d) == 2
    cases = []
    for X, rows in zip(_four(d[0], d[1]), (1024, 2048, 2048, 3000)):
        want = ar.align(ref, read, SC2, w, X)
        assert want[4] == rows and len(want[3]) == (rows + 1023) // 1024 and want[2] == [(700, 700)]
        cases.append((X, want))
    return ref, read, w, cases


def test_adapt_xdrop_planted_head(ctx):
    ref, read, w, cases = _planted_case()
    for X, want in cases:
        b = _run(ctx, [ref], [read], w, 0, X, sc=SC2)
        _check_pair(b, 0, want, len(read), X)
        b.free()


@functools.lru_cache(maxsize=None)
def _diverging_case(w=64):
    """the drift of test 1 for 1600 rows, then a read that has nothing to do with the reference"""
    rng = random.Random(9957)
    ref, base = _drift_pair(rng, 1600, every=700, first=350, extra=30, tail=1500)
    read = base + "A" * 1400
    ref = ref[:1800] + "C" * 1400
    _, _, drops = ar.trace(ref, read, SC2, w)
    d = [best - seam for best, seam in drops]
    assert len(d) == 2 and d[0] <= 0 < d[1], d                   # strip 0 ends on the alignment, strip 1 far below it
    cases = []
    for tie in (0, 1):
        for X, rows in ((d[1] - 1, 2048), (d[1], 3000)):
            want = ar.align(ref, read, SC2, w, X, tie)
            assert want[4] == rows and len(want[3]) == (rows + 1023) // 1024
            assert want[3][1] != gr.windows(3000, len(ref), w)[1]
            cases.append((tie, X, want))
    return ref, read, w, cases


def test_adapt_xdrop_diverging_tail(ctx):
    ref, read, w, cases = _diverging_case()
    for tie, X, want in cases:
        b = _run(ctx, [ref], [read], w, tie, X, sc=SC2)
        _check_pair(b, 0, want, len(read), (tie, X))
        b.free()


@pytest.mark.parametrize("matrix", [False, True])
def test_adapt_mixed_launch_xdrop(ctx, matrix):
    """the mixed launch under a threshold nothing exceeds: the xdrop sweeps give the adaptive result, rows_swept = m"""
    ref, reads, w, mat, want = _mixed_case(matrix)
    drops = [ar.trace(ref, q, SC, w, 0, 0, mat)[2] for q in reads]
    X = max([b_ - s_ for dr in drops for b_, s_ in dr] + [0]) + 1
    b = _run(ctx, [ref], reads, w, 0, X, mat)
    for q, e in enumerate(want):
        _check_pair(b, q, e + (len(reads[q]),), len(reads[q]), (matrix, q))
    b.free()


def test_adapt_matrix_strict_ties(ctx):
    """sw_affine_sweep_band_adapt_matrix_kernel and _band_adapt_xdrop_matrix_kernel in the strict tie order (the mixed launches
    run the serial one): a drifting read of two strips, without a threshold and under one nothing exceeds"""
    rng = random.Random(9959)
    w, mat = 64, gc.score_matrix()
    ref, read = _drift_pair(rng, 1400, every=700, first=350, extra=30, tail=150)
    want = ar.align(ref, read, SC, w, 0, 1, mat)
    assert len(want[3]) == 2
    drops = ar.trace(ref, read, SC, w, 0, 1, mat)[2]
    for X in (0, max([b_ - s_ for b_, s_ in drops] + [0]) + 1):
        b = _run(ctx, [ref], [read], w, 1, X, mat)
        _check_pair(b, 0, want + (len(read),), len(read), X)
        b.free()


# 7 -- cell_cap = 1 on a pair with two tied maximum cells: the exact-size re-run places the same windows
@functools.lru_cache(maxsize=None)
def _ties_case(w=64):
    rng = random.Random(9958)
    head = u.rand(rng, 700)
    ref, read = head + "GTT" + "C" * 2400, head + "TTT" + "A" * 1346
    want = {tie: ar.align(ref, read, SC2, w, 0, tie) for tie in (0, 1)}
    assert want[0][2] == [(700, 700), (703, 703)] and len(want[0][3]) == 3
    return ref, read, w, want


@pytest.mark.parametrize("tie", [0, 1])
def test_adapt_ties_and_the_rerun(ctx, tie):
    ref, read, w, want = _ties_case()
    b = _run(ctx, [ref], [read], w, tie, sc=SC2, cell_cap=1)
    assert b.timing().rerun_pairs == 1
    _check_pair(b, 0, want[tie], len(read), tie)
    b.free()


# 8 -- the options of an affine run
@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("zero_copy", 0)])
def test_adapt_options(ctx, opt):
    ref, reads, w, want = _edges_case()
    refs = [ref, ref[:1200]]
    reads = [reads[1], reads[2][:800]]
    exp = {(0, 0): want[1]}
    for r, q in ((0, 1), (1, 0), (1, 1)):
        exp[(r, q)] = ar.align(refs[r], reads[q], SC, w)
    b = _run(ctx, refs, reads, w, **dict([opt]))
    for (r, q), e in exp.items():
        pair = r * 2 + q
        if opt[0] != "scores_only":
            _check_pair(b, pair, e, len(reads[q]), (opt, r, q))
            continue
        assert b.score(pair) == e[0]
        _check_windows(b, pair, e[3], len(reads[q]), (opt, r, q))
        for call in (lambda: b.n_alignments(pair), lambda: b.alignment(pair, 0)):
            with pytest.raises(_capi.SwmiError) as err:
                call()
            assert err.value.code == ERR_INVALID
    b.free()


# 9 -- option semantics
def _refused(b, params):
    with pytest.raises(_capi.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED


def test_adapt_invalid_values_leave_the_context(ctx):
    ref, reads, w, want = _edges_case()
    static = gr.align_numpy(ref, reads[2], SC, GLOBAL, w, True, cells=True) + (gr.windows(1025, len(ref), w),)
    for start, e in ((1, want[2]), (0, static)):
        b = _run(ctx, [ref], [reads[2]], w, adapt=start)
        for bad in (-1, 2, 1 << 40):
            with pytest.raises(_capi.SwmiError) as err:
                ctx.set_option("band_adapt", bad)
            assert err.value.code == ERR_INVALID
        b.run(sw.make_params(SC[:3]))                             # the next run is still what it was
        _check_pair(b, 0, e, 1025, start)
        b.free()


@pytest.mark.parametrize("mode,extend,w", [(sw.ALIGN_GLOBAL, 1, 0), (sw.ALIGN_GLOBAL, 0, 64), (sw.ALIGN_FIT, 0, 64), (sw.ALIGN_LOCAL, 0, 64)])
def test_adapt_needs_a_banded_extend_run(ctx, mode, extend, w):
    rng = random.Random(9959)
    ref, read = u.rand(rng, 200), u.rand(rng, 80)
    for name, value in (("gap_open", SC[3]), ("align_mode", mode), ("extend", extend), ("band", w), ("long_reads", 1), ("band_adapt", 1)):
        ctx.set_option(name, value)
    b = ctx.upload([ref], [read])
    p = sw.make_params(SC[:3])
    _refused(b, p)
    with pytest.raises(_capi.SwmiError):                          # nothing was launched: the batch has no results
        b.band_window(0, 0)
    ctx.set_option("band_adapt", 0)                               # the batch is still usable
    b.run(p)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, SC, mode, 0, bool(extend))
    assert b.band_window(0, 0) == (1, 200)
    ctx.set_option("gap_open", 0)                                 # the linear pipeline refuses it too
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)
    ctx.set_option("extend", 0)
    ctx.set_option("band", 0)
    ctx.set_option("band_adapt", 1)
    _refused(b, p)
    ctx.set_option("band_adapt", 0)
    b.run(p)
    assert b.pipeline_mode() != 3 and b.band_window(0, 0) == (1, 200)
    with pytest.raises(_capi.SwmiError) as e:
        b.band_window(0, 1)
    assert e.value.code == ERR_RANGE
    b.free()


def test_adapt_0_is_the_static_band(ctx):
    """nothing moved: with band_adapt = 0 the run is gotoh_reference's banded extend run, before and after an adaptive run"""
    ref, reads, w, want = _edges_case()
    reads = [reads[1], reads[2], reads[3][:300]]
    exp = u.expect([ref], reads, SC, GLOBAL, w, True, cells=True)
    assert exp[(0, 0)][:3] != want[1][:3]                                        # the two bands differ on this pair
    b = _run(ctx, [ref], reads, w, adapt=0)
    p = sw.make_params(SC[:3])
    for adapt in (0, 1, 0):
        ctx.set_option("band_adapt", adapt)
        b.run(p)
        if adapt:
            _check_pair(b, 0, want[1], 2049)
            _check_pair(b, 1, want[2], 1025)
            continue
        u.check(b, [ref], reads, exp, GLOBAL)
        for q, read in enumerate(reads):
            wins = gr.windows(len(read), len(ref), w)
            assert [b.band_window(q, s) for s in range(len(wins))] == wins
    b.free()


def test_adapt_travels_with_the_run(ctx):
    ref, reads, w, want = _edges_case()
    refs, reads = [ref, ref[:1300]], [reads[2], reads[2][:400]]
    exp = {1: {(r, q): ar.align(refs[r], reads[q], SC, w) for r in range(2) for q in range(2)},
           0: {(r, q): gr.align_numpy(refs[r], reads[q], SC, GLOBAL, w, True, cells=True) + (gr.windows(len(reads[q]), len(refs[r]), w),)
               for r in range(2) for q in range(2)}}
    assert exp[1][(0, 0)][3] != exp[0][(0, 0)][3]
    p = sw.make_params(SC[:3])
    for name, value in (("gap_open", SC[3]), ("align_mode", GLOBAL), ("extend", 1), ("long_reads", 1), ("band", w)):
        ctx.set_option(name, value)
    for adapt in (1, 0):
        ctx.set_option("band_adapt", adapt)
        ctx.set_option("debug_async_delay_us", 50000)
        b = ctx.upload(refs, reads).run_async(p)
        ctx.set_option("band_adapt", 1 - adapt)                   # does not reach the run in flight
        b.wait()
        ctx.set_option("debug_async_delay_us", 0)
        for (r, q), e in exp[adapt].items():
            _check_pair(b, r * 2 + q, e, len(reads[q]), (adapt, r, q))
        b.free()
    ctx.set_option("band_adapt", 1)
    st = ctx.stream(reads, p, slots=2, chunk_bytes=1 << 10)
    ctx.set_option("band_adapt", 0)                               # (the slots copied it at the open)
    st.push(refs[:1]).push(refs[1:]).finish()
    n_chunks = 0
    for first, c in st.chunks():
        n_chunks += 1
        for r in range(c.n_refs):
            for q in range(2):
                _check_pair(c, r * 2 + q, exp[1][(first + r, q)], len(reads[q]), (first + r, q))
    assert n_chunks >= 2
    st.close()


def test_adapt_mirror(ctx):
    ref, reads, w, want = _edges_case()
    read = reads[2]
    for cls, tie in ((sw.SmithWaterman.OptAlignments, 0), (sw.DistributedSW.OptAlignments, 1)):
        got = cls(ctx, align_mode=GLOBAL, long_reads=True, band=w, extend=True, band_adapt=True).call([ref, read], SC)
        assert got == ar.align(ref, read, SC, w, 0, tie)[:2]
        assert ctx.options["band_adapt"] == 0 and ctx.options["band"] == 0 and ctx.options["extend"] == 0
    two = [read, "ACGT"]
    f = sw.Distribution.MapRef(ctx, align_mode=GLOBAL, long_reads=True, band=w, extend=True, band_adapt=True)
    total, (_, sites) = f.call(((">r", ref), two, (SC, ["a", "i", "d", "-"])))
    exp = [ar.align(ref, q, SC, w) for q in two]
    assert total == sum(e[0] for e in exp) and sites == [a for e in exp for a in e[1]]
    with pytest.raises(ValueError):
        sw.SmithWaterman.OptAlignments(ctx, band_adapt=1).call([ref, read], SC)


# the JNI shim's entry point from plain C99 (tests/c/shim_adapt.c)
def _lcg(x, n):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def test_c99_shim_sets_band_adapt(tmp_path):
    out = u.run_shim(tmp_path, "shim_adapt")
    ref = _lcg(1, 1300)
    read = ref[:300] + _lcg(2, 40) + ref[300:700] + _lcg(3, 40) + ref[700:1220]
    assert (len(ref), len(read)) == (1300, 1300)
    w = 48
    adaptive = ar.align(ref, read, SC2, w)
    static = gr.align_numpy(ref, read, SC2, GLOBAL, w, True, cells=True) + (gr.windows(1300, 1300, w),)
    assert adaptive[0] > static[0] and adaptive[3][1] != static[3][1]
    lines = []
    for e in (adaptive, static):
        lines.append("%d %d" % (e[0], len(e[1])) + "".join(" %d:%d" % (beg, len(ra)) for beg, (ra, _) in e[1]) +
                     " windows %d-%d %d-%d mode 3" % (e[3][0] + e[3][1]))
    assert out.splitlines() == lines + ["range %d" % ERR_RANGE, "refused %d" % ERR_UNSUPPORTED]


# 10 -- the bound's edge: (2 NS + 1) |o| + (1024 NS + n) |e| <= 2^30 with M * S = 2^29
def _bound_pairs():
    """a read of 1025 bases (NS = 2, M = 2048) under |gap| = |gap_open| = 2^18 = S: 5 + 2048 + n <= 4096, so n = 2043 is the last
    reference the run takes"""
    L = 1 << 18
    sc = (L, -L, -L, -L)
    rng = random.Random(9960)
    read = u.rand(rng, 1025, "AC")
    ref = read[:500] + u.rand(rng, 20, "AC") + read[500:] + u.rand(rng, 2044 - 1045, "AC")
    assert len(ref) == 2044
    assert ar.bound_ok(1025, 2043, sc) and not ar.bound_ok(1025, 2044, sc) and 2048 * L == 1 << 29
    return sc, read, ref[:2043], ref


def test_adapt_refusal_at_the_bounds_edge(ctx):
    sc, read, inside, outside = _bound_pairs()
    w = 64
    want = ar.align(inside, read, sc, w)
    b = _run(ctx, [inside], [read], w, sc=sc)
    _check_pair(b, 0, want, 1025)
    b.free()
    b = ctx.upload([outside], [read])
    _refused(b, sw.make_params(sc[:3]))
    with pytest.raises(_capi.SwmiError):                          # nothing was launched
        b.score(0)
    ctx.set_option("band_adapt", 0)                               # the static band's own bound (3 |o|) takes it
    b.run(sw.make_params(sc[:3]))
    assert b.score(0) == gr.align_numpy(outside, read, sc, GLOBAL, w, True)[0]
    b.free()
