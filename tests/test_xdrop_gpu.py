"""The drop-off rule of seed extension on the GPU (option "xdrop": the sw_affine_sweep_{long,band}_xdrop[_matrix]_kernel sweeps of
swmi_affine.hip) against tests/xdrop_reference.py: every score, every alignment with its begin, both
strings and its maximum cell, the flags, and swmi_pair_rows_swept.  set_option("xdrop", ...) and Batch.rows_swept are what
fail without the feature.

Scores are (2, -4, -2, -4): under the repository's usual (5, -3, -2, -6) unrelated random DNA keeps gaining score in global mode
and nothing ever drops.  Every case computes its differences best(s) - seam(s) with xdrop_reference.drops and asserts
1 <= d0 < d1 (and what else it relies on) before it uses them, so a changed generator cannot turn a case vacuous.  Every pair
has 3 strips or fewer.

  sweep kernel (sw_affine_sweep_...)    run by
  long_xdrop_kernel                     test_xdrop_hand_derivable[0], test_xdrop_random_tails[*-0], test_xdrop_strip_edges, ...
  long_xdrop_matrix_kernel              test_xdrop_mixed_launch[True-0], test_xdrop_matrix_strict_ties[0]
  band_xdrop_kernel                     test_xdrop_hand_derivable[64 / 16], test_xdrop_random_tails[*-64 / 16], test_xdrop_mixed_launch[False-64]
  band_xdrop_matrix_kernel              test_xdrop_mixed_launch[True-64], test_xdrop_matrix_strict_ties[64]

The comparison's width has no test: best(s) - seam(s) <= |gap_open| + 1024 (s + 1) |gap| < 2^31 within the bounds a run is
held to (DESIGN.md 8h has the proof), so no input reaches a difference that an int32 comparison would get wrong."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr
import xdrop_reference as xr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
SC = (2, -4, -2, -4)
GLOBAL = sw.ALIGN_GLOBAL
D0, D1 = 652, 2700                          # the hand-derivable case: |o| + 324 |e| and |o| + 1348 |e|


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# every run of this module is an extend run with long reads on
def _run(ctx, refs, reads, X, tie=0, w=0, matrix=None, sc=SC, **options):
    return u.run(ctx, refs, reads, sc, tie, GLOBAL, w, 1, matrix, long_reads=1, xdrop=X, **options)


def _check_pair(b, pair, want, what=None):
    """want = (score, alignments, cells, rows_swept) of xdrop_reference.align"""
    u.check_pair(b, pair, want[:3], GLOBAL, what)
    assert b.rows_swept(pair) == want[3], (what, b.rows_swept(pair), want[3])


def _differences(ref, read, w=0, matrix=None, tie=0):
    """best(s) - seam(s) for s = 0 .. NS - 2 (tie: of the xr.align calls that follow, which then share the sweep)"""
    return [best - seam for best, seam in xr.drops(ref, read, SC, w, matrix, tie_mode=tie)]


def _four(d0, d1, later=()):
    """the four thresholds around two differences, after the conditions that make them mean what the tests say"""
    assert 1 <= d0 < d1 and all(d1 - 1 > d for d in later), (d0, d1, later)
    return (d0 - 1, d0, d1 - 1, d1)


def _planted(rng, head, m, n):
    """a common head, then a read of A's against a reference of C's: the one maximum cell is (head, head)"""
    h = u.rand(rng, head)
    return h + "C" * (n - head), h + "A" * (m - head)


# 1 -- the hand-derivable case: from the one maximum cell (700, 700), score 1400, the best way down to row 1024 is one insertion
# of 324 read bases and to row 2048 one of 1348; a mismatch costs as much as a gap base plus the open
@pytest.mark.parametrize("w", [0, 64, 16])
def test_xdrop_hand_derivable(ctx, w):
    rng = random.Random(9700)
    ref, read = _planted(rng, 700, 3000, 3100)
    d = _differences(ref, read, w)
    assert d[0] == D0 and (w or d == [D0, D1])
    for X, rows in zip(_four(d[0], d[1]), (1024, 2048, 2048, 3000)):
        want = xr.align(ref, read, SC, X, w)
        assert want[3] == rows and (w or want[:3] == (1400, [(1, (ref[:700], read[:700]))], [(700, 700)]))
        b = _run(ctx, [ref], [read], X, 0, w)
        _check_pair(b, 0, want, (w, X))
        b.free()


# 2 -- random tails (7: and the strict tie mode)
def _random_tails(seed=9701):
    rng = random.Random(seed)
    head = u.rand(rng, 700)
    return head + u.rand(rng, 2400), u.mutate(rng, head) + u.rand(rng, 2300)


@pytest.mark.parametrize("w", [0, 64, 16])
@pytest.mark.parametrize("tie", [0, 1])
def test_xdrop_random_tails(ctx, tie, w):
    ref, read = _random_tails()
    d = _differences(ref, read, w, None, tie)
    assert len(d) == 2
    for X, rows in zip(_four(d[0], d[1]), (1024, 2048, 2048, len(read))):
        want = xr.align(ref, read, SC, X, w, tie)
        assert want[3] == rows
        b = _run(ctx, [ref], [read], X, tie, w)
        _check_pair(b, 0, want, (tie, w, X))
        b.free()


# 3 -- a later, better stretch is not found: the test that cannot pass by computing everything
def test_xdrop_later_better_stretch_is_not_found(ctx):
    rng = random.Random(9702)
    head, tail = u.rand(rng, 700), u.rand(rng, 900)
    ref, read = head + u.rand(rng, 1400) + tail, head + u.rand(rng, 1400) + tail
    assert len(ref) == len(read) == 3000
    full = gr.align_numpy(ref, read, SC, GLOBAL, 0, True, cells=True)
    assert full[0] > 1400 and all(i > 2048 for i, _ in full[2])                    # extend ends in strip 2
    d = _differences(ref, read)
    want = xr.align(ref, read, SC, d[0] - 1)
    assert d[0] >= 2 and want[0] == 1400 and want[2] == [(700, 700)] and want[3] == 1024
    b = _run(ctx, [ref], [read], d[0] - 1)
    _check_pair(b, 0, want)
    b.run(sw.make_params(SC[:3]))                                                 # the same batch again: nothing is left over
    _check_pair(b, 0, want)
    ctx.set_option("xdrop", max(d))                                               # and with an X no strip exceeds: extend
    b.run(sw.make_params(SC[:3]))
    _check_pair(b, 0, full + (3000,))
    b.free()


# 4 -- strip edges: m = 2048 has one test point and a stop skips a full strip; in m = 2049 a stop behind strip 1, in m = 1025 a
# stop behind strip 0 skips a strip with one real row; a read of 1024 bases in the same launch is computed in full
def test_xdrop_strip_edges(ctx):
    rng = random.Random(9704)
    head = u.rand(rng, 700)
    ref = head + "C" * 1400
    reads = [head + "A" * (m - 700) for m in (2048, 2049, 1025, 1024)]
    cases = ((D0 - 1, (1024, 1024, 1024, 1024)), (D0, (2048, 2048, 1025, 1024)), (D1 - 1, (2048, 2048, 1025, 1024)),
             (D1, (2048, 2049, 1025, 1024)))
    want = {}
    for q, read in enumerate(reads):                              # (read by read: the reference keeps one sweep)
        assert _differences(ref, read) == [[D0], [D0, D1], [D0], []][q]
        for X, _ in cases:
            want[(X, q)] = xr.align(ref, read, SC, X)
    assert want[(D0 - 1, 3)][:3] == gr.align_numpy(ref, reads[3], SC, GLOBAL, 0, True, cells=True)
    for X, rows in cases:
        assert tuple(want[(X, q)][3] for q in range(4)) == rows
        b = _run(ctx, [ref], reads, X)
        for q in range(4):
            _check_pair(b, q, want[(X, q)], (X, len(reads[q])))
        b.free()


# 5 -- a mixed launch: short reads, long reads that stop behind strip 0, behind strip 1 and not at all in one batch -- several
# pairs per workgroup with different exits -- plain and with the 4 x 4 matrix of test_extend_mixed_launch, banded and not
def _mixed(matrix):
    rng = random.Random(9705 + int(matrix))
    qt = "T" if matrix else "A"             # the read's tail against a reference tail of C's: a negative entry of the matrix (A / C is not)
    base = u.rand(rng, 2200)
    ref = base[:1800] + "C" * 400
    reads = [base[:700] + qt * 800, base[:1700] + qt * 400, u.mutate(rng, base[:1500]), base[:500] + qt * 1000,
             u.mutate(rng, base[:100]), base[:300], base[:1024]]
    return ref, reads


@pytest.mark.parametrize("w", [0, 64])
@pytest.mark.parametrize("matrix", [False, True])
def test_xdrop_mixed_launch(ctx, matrix, w):
    ref, reads = _mixed(matrix)
    mat = gc.score_matrix() if matrix else None
    assert mat is None or gr.cell_score("C", "T", SC, mat) < 0
    d = [_differences(ref, q, w, mat) for q in reads]
    X = min(d[0][0], d[3][0]) - 1                                                 # stops both behind strip 0 ...
    assert (matrix or d[0][0] == D0) and 0 <= d[1][0] <= X < d[1][1] and max(d[2]) <= X and d[4:] == [[], [], []], d
    want = [xr.align(ref, q, SC, X, w, 0, mat) for q in reads]
    assert [e[3] for e in want] == [1024, 2048, len(reads[2]), 1024, len(reads[4]), 300, 1024]
    b = _run(ctx, [ref], reads, X, 0, w, mat)
    for q, e in enumerate(want):
        _check_pair(b, q, e, (matrix, w, q))
    total = int(sum(e[0] for e in want))
    assert b.ref_total(0) == total
    assert b.ref_sites_packed()[0] == (total, 0, sorted([a for e in want for a in e[1]], key=lambda t: t[0]))
    assert b.timing().cells == sum(len(q) * len(ref) for q in reads)              # nominal: a stopped pair counts in full
    b.free()


@pytest.mark.parametrize("w", [0, 64])
def test_xdrop_matrix_strict_ties(ctx, w):
    """sw_affine_sweep_long_xdrop_matrix_kernel and _band_xdrop_matrix_kernel in the strict tie order (test_xdrop_mixed_launch
    runs the serial one): the mixed launch's first read alone, on either side of its one difference"""
    ref, reads = _mixed(True)
    mat, read = gc.score_matrix(), reads[0]
    d = _differences(ref, read, w, mat, 1)
    assert len(d) == 1 and d[0] >= 1
    for X, rows in ((d[0] - 1, 1024), (d[0], len(read))):
        want = xr.align(ref, read, SC, X, w, 1, mat)
        assert want[3] == rows
        b = _run(ctx, [ref], [read], X, 1, w, mat)
        _check_pair(b, 0, want, (w, X))
        b.free()


# 6 -- ties and the exact-size re-run (7: and the strict tie mode)
@pytest.mark.parametrize("tie", [0, 1])
def test_xdrop_ties_and_the_rerun(ctx, tie):
    rng = random.Random(9703)
    head = u.rand(rng, 700)
    ref, read = head + "GTT" + "C" * 2400, head + "TTT" + "A" * 1346
    d = _differences(ref, read, 0, None, tie)
    X = _four(d[0], d[1])[0]
    want = xr.align(ref, read, SC, X, 0, tie)
    assert want[0] == 1400 and want[2] == [(700, 700), (703, 703)] and want[3] == 1024
    b = _run(ctx, [ref], [read], X, tie, cell_cap=1)
    assert b.timing().rerun_pairs == 1                                            # the re-run stops behind the same strip
    _check_pair(b, 0, want, tie)
    b.free()


# 8 -- the options of an affine run on a stopped pair
@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("zero_copy", 0)])
def test_xdrop_options(ctx, opt):
    rng = random.Random(9706)
    ref, read = _planted(rng, 700, 2049, 2100)
    refs, reads = [ref, ref[:900]], [read, read[:800]]
    want = {(r, q): xr.align(refs[r], reads[q], SC, D0 - 1) for r in range(2) for q in range(2)}
    assert [want[k][3] for k in sorted(want)] == [1024, 800, 1024, 800]
    b = _run(ctx, refs, reads, D0 - 1, **dict([opt]))
    for (r, q), e in want.items():
        pair = r * 2 + q
        if opt[0] != "scores_only":
            _check_pair(b, pair, e, (opt, r, q))
            continue
        assert (b.score(pair), b.rows_swept(pair)) == (e[0], e[3])
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


def test_xdrop_invalid_values_leave_the_context(ctx):
    rng = random.Random(9707)
    ref, read = _planted(rng, 700, 1025, 1100)
    stopped, full = xr.align(ref, read, SC, D0 - 1), xr.align(ref, read, SC, 0)
    assert (stopped[3], full[3]) == (1024, 1025)
    for start, want in ((D0 - 1, stopped), (0, full)):
        b = _run(ctx, [ref], [read], start)
        for bad in (-1, 1 << 31, 1 << 40):
            with pytest.raises(_capi.SwmiError) as e:
                ctx.set_option("xdrop", bad)
            assert e.value.code == ERR_INVALID
        b.run(sw.make_params(SC[:3]))                             # the next run is still what it was
        _check_pair(b, 0, want, start)
        b.free()
    ctx.set_option("xdrop", (1 << 31) - 1)                        # the largest threshold
    b = ctx.upload([ref], [read]).run(sw.make_params(SC[:3]))
    _check_pair(b, 0, full)
    b.free()


@pytest.mark.parametrize("mode,extend", [(sw.ALIGN_GLOBAL, 0), (sw.ALIGN_FIT, 0), (sw.ALIGN_LOCAL, 0), (sw.ALIGN_FIT, 1)])
def test_xdrop_needs_an_extend_run(ctx, mode, extend):
    rng = random.Random(9708)
    ref, read = u.rand(rng, 200), u.rand(rng, 80)
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("align_mode", mode)
    ctx.set_option("extend", extend)
    ctx.set_option("xdrop", 5)
    b = ctx.upload([ref], [read])
    p = sw.make_params(SC[:3])
    _refused(b, p)
    with pytest.raises(_capi.SwmiError):                          # nothing was launched: the batch has no results
        b.rows_swept(0)
    ctx.set_option("xdrop", 0)                                    # the batch is still usable
    ctx.set_option("extend", 0)
    b.run(p)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, SC, mode)
    assert b.rows_swept(0) == 80                                  # the read's length in every mode
    ctx.set_option("gap_open", 0)                                 # the linear pipeline refuses it too
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)
    ctx.set_option("xdrop", 5)
    _refused(b, p)
    ctx.set_option("xdrop", 0)
    b.run(p)
    assert b.pipeline_mode() != 3 and b.rows_swept(0) == 80
    b.free()


def test_xdrop_0_is_extend(ctx):
    """nothing moved: with xdrop = 0 the run is the extend run, before and after an xdrop run of the batch"""
    ref, reads = _mixed(False)
    reads = [reads[0], reads[2], reads[5]]
    exp = u.expect([ref], reads, SC, GLOBAL, 0, True, cells=True)
    b = _run(ctx, [ref], reads, 0)
    p = sw.make_params(SC[:3])
    for X in (0, D0 - 1, 0):
        ctx.set_option("xdrop", X)
        b.run(p)
        if X:
            assert [b.rows_swept(q) for q in range(3)] == [1024, len(reads[1]), 300]
            continue
        u.check(b, [ref], reads, exp, GLOBAL)
        assert [b.rows_swept(q) for q in range(len(reads))] == [len(q) for q in reads]
    b.free()


def test_xdrop_travels_with_the_run(ctx):
    rng = random.Random(9709)
    ref, read = _planted(rng, 700, 1025, 1100)
    refs, reads = [ref, ref[:1000] + u.rand(rng, 60)], [read, read[:400]]
    want = {X: {(r, q): xr.align(refs[r], reads[q], SC, X) for r in range(2) for q in range(2)} for X in (D0 - 1, 0)}
    assert [want[X][(r, 0)][3] for X in (D0 - 1, 0) for r in range(2)] == [1024, 1024, 1025, 1025]
    p = sw.make_params(SC[:3])
    for name, value in (("gap_open", SC[3]), ("align_mode", GLOBAL), ("extend", 1), ("long_reads", 1)):
        ctx.set_option(name, value)
    for X in (D0 - 1, 0):
        ctx.set_option("xdrop", X)
        ctx.set_option("debug_async_delay_us", 50000)
        b = ctx.upload(refs, reads).run_async(p)
        ctx.set_option("xdrop", D0 - 1 - X)                       # does not reach the run in flight
        b.wait()
        ctx.set_option("debug_async_delay_us", 0)
        for (r, q), e in want[X].items():
            _check_pair(b, r * 2 + q, e, (X, r, q))
        b.free()
    ctx.set_option("xdrop", D0 - 1)
    st = ctx.stream(reads, p, slots=2, chunk_bytes=1 << 10)
    ctx.set_option("xdrop", 0)                                    # (the slots copied it at the open)
    st.push(refs[:1]).push(refs[1:]).finish()
    n_chunks = 0
    for first, c in st.chunks():
        n_chunks += 1
        for r in range(c.n_refs):
            for q in range(2):
                _check_pair(c, r * 2 + q, want[D0 - 1][(first + r, q)], (first + r, q))
    assert n_chunks >= 2
    st.close()


def test_xdrop_mirror(ctx):
    rng = random.Random(9710)
    ref, read = _planted(rng, 700, 1025, 1100)
    for cls, tie in ((sw.SmithWaterman.OptAlignments, 0), (sw.DistributedSW.OptAlignments, 1)):
        for X in (D0 - 1, D0):
            got = cls(ctx, align_mode=GLOBAL, long_reads=True, extend=True, xdrop=X).call([ref, read], SC)
            assert got == xr.align(ref, read, SC, X, 0, tie)[:2]
            assert ctx.options["xdrop"] == 0 and ctx.options["extend"] == 0
    reads = [read, "ACGT"]
    f = sw.Distribution.MapRef(ctx, align_mode=GLOBAL, long_reads=True, extend=True, xdrop=D0 - 1)
    total, (_, sites) = f.call(((">r", ref), reads, (SC, ["a", "i", "d", "-"])))
    exp = [xr.align(ref, q, SC, D0 - 1) for q in reads]
    assert total == sum(e[0] for e in exp) and sites == [a for e in exp for a in e[1]]
    with pytest.raises(ValueError):
        sw.SmithWaterman.OptAlignments(ctx, xdrop=1.5).call([ref, read], SC)


# the JNI shim's entry point from plain C99 (tests/c/shim_xdrop.c)
def test_c99_shim_sets_xdrop(tmp_path):
    out = u.run_shim(tmp_path, "shim_xdrop")
    ref, read = "ACGTTGCA" * 80 + "C" * 500, "ACGTTGCA" * 80 + "A" * 385
    assert (len(ref), len(read)) == (1140, 1025)
    d = _differences(ref, read)
    assert d == [4 + 2 * 384]                                     # from (640, 640) to row 1024: one insertion of 384 bases
    lines = []
    for X in (d[0] - 1, d[0], 0):
        e = xr.align(ref, read, SC, X)
        lines.append("%d %d" % (e[0], len(e[1])) + "".join(" %d:%d" % (beg, len(ra)) for beg, (ra, _) in e[1]) + " rows %d mode 3" % e[3])
    assert [ln.split()[-3] for ln in lines] == ["1024", "1025", "1025"]
    assert out.splitlines() == lines + ["refused %d" % ERR_UNSUPPORTED]
