"""Two-piece affine gaps on the GPU (options "gap_open2" / "gap2" on global and extend runs: the sw_affine_sweep2_* and
sw_affine_traceback2_* kernels of swmi_affine.hip) against tests/twopiece_reference.py: every score, every
alignment with its begin, both strings and its maximum cell, and the flags.  set_option("gap_open2", ...) is what fails without
the feature.

  kernel                                  run by
  sweep2_{global,extend}[_wide]_kernel    test_rows_per_lane_classes, test_crossover, test_tie_rich, test_limits
  sweep2_long_{global,extend}_kernel      test_seam
  sweep2_band_{global,extend}_kernel      test_band, test_band_differs_from_unbanded
  traceback2_global_kernel                test_rows_per_lane_classes, test_crossover, test_tie_rich
  traceback2_long_global_kernel           test_seam
  traceback2_band_global_kernel           test_band, test_band_differs_from_unbanded"""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import adapt_reference as ar
import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr
import twopiece_reference as tr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
GLOBAL = sw.ALIGN_GLOBAL
SC = (2, -3, -2, -4, -1, -12)               # the pieces tie at k = 8
CROSS = (2, -4, -2, -4, -1, -24)            # ... at k = 20


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _run(ctx, refs, reads, sc, tie=0, w=0, extend=0, **options):
    ctx.set_option("gap_open2", sc[5])                            # (first: what fails without the feature)
    return u.run(ctx, refs, reads, sc, tie, GLOBAL, w, extend, None, long_reads=1, gap2=sc[4], **options)


def _want(ref, read, sc, w=0, extend=0, tie=0, align=tr.align_numpy):
    return align(ref, read, sc, GLOBAL, w, bool(extend), tie, cells=True)


def _expect(refs, reads, sc, w=0, extend=0, tie=0):
    return {(r, q): _want(refs[r], reads[q], sc, w, extend, tie) for r in range(len(refs)) for q in range(len(reads))}


def _check(b, refs, reads, exp):
    for (r, q), want in exp.items():
        u.check_pair(b, r * len(reads) + q, want, GLOBAL, (r, q, len(refs[r]), len(reads[q])))


def _refused(b, params):
    with pytest.raises(_capi.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED
    return str(e.value)


# 1 -- every rows-per-lane class of the narrow and the wide sweep
CLASS_M = (1, 63, 64, 65, 150, 256, 257, 350, 420, 500, 550, 640, 700, 750, 800, 850, 950, 1024)
CLASS_N = (1, 7, 8, 9, 70, 200)
_CLASSES = {}


def _classes():
    if not _CLASSES:
        rng = random.Random(8801)
        base = u.rand(rng, 1100)
        _CLASSES.update(refs=[base[:n] for n in CLASS_N],
                        reads=[(gc.mutate(rng, base[:m + 30], "ACGT", 0.05, 0.02) + u.rand(rng, m))[:m] for m in CLASS_M])
    return _CLASSES["refs"], _CLASSES["reads"]


@pytest.mark.parametrize("n_at", range(len(CLASS_N)))
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("extend", [0, 1])
def test_rows_per_lane_classes(ctx, extend, tie, n_at):
    refs, reads = _classes()
    assert sorted({gc.rows_per_lane(len(q)) for q in reads}) == list(gc.RS)
    refs = refs[n_at:n_at + 1]
    b = _run(ctx, refs, reads, SC, tie, 0, extend)
    _check(b, refs, reads, _expect(refs, reads, SC, 0, extend, tie))
    b.free()


# 2 -- the crossover: gaps of 19, 20 and 21 bases under scores whose pieces tie at 20
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("body", [40, 1000])
def test_crossover(ctx, body, tie):
    """body 40: R = 1, every row crosses a lane; body 1000: R = 16, a run crosses row slots and lanes"""
    rng = random.Random(8802 + body)
    refs, reads = [], []
    for k in (19, 20, 21):
        base, gap = u.rand(rng, body), u.rand(rng, k)
        cut = body // 2 + 3
        refs += [base, (base[:cut] + gap + base[cut:])[:1024]]
        reads += [(base[:cut] + gap + base[cut:])[:1024], base]
    assert {gc.rows_per_lane(len(q)) for q in reads} == ({1} if body == 40 else {16})
    want = [_want(ref, read, CROSS, 0, 0, tie) for ref, read in zip(refs, reads)]
    for x, (score, alns, _) in enumerate(want):
        k = 19 + x // 2
        gapped = alns[0][1][x % 2]                                # the insertion shows in the reference string, the deletion in the read's
        assert "_" * k in gapped and gapped.count("_") >= k, (x, k)
    b = _run(ctx, refs, reads, CROSS, tie)
    for x, e in enumerate(want):
        u.check_pair(b, x * len(reads) + x, e, GLOBAL, x)
    b.free()


# 3 -- the seam: state F2 across it, in the sweep and in the walk
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("extend", [0, 1])
def test_seam(ctx, extend, tie):
    rng = random.Random(8803)
    base = u.rand(rng, 1240)
    read = base[:999] + u.rand(rng, 61) + base[999:1239]          # rows 1000 .. 1060 are inserted
    ref = base[:1239] + (u.rand(rng, 12) if extend else "")
    assert len(read) == 1300
    want = _want(ref, read, CROSS, 0, extend, tie)
    assert "_" * 61 in want[1][0][1][0]
    b = _run(ctx, [ref], [read], CROSS, tie, 0, extend)
    u.check_pair(b, 0, want, GLOBAL, 1300)
    b.free()


@pytest.mark.parametrize("m,n", [(1025, 1000), (2049, 700)])
def test_seam_strips(ctx, m, n):
    """a last strip of one row, and three strips (the long insertion crosses both seams)"""
    rng = random.Random(8804 + m)
    ref = u.rand(rng, n)
    read = (gc.mutate(rng, ref[:n // 2], "ACGT", 0.04, 0.01) + u.rand(rng, m - n) + gc.mutate(rng, ref[n // 2:], "ACGT", 0.04, 0.01) + u.rand(rng, 64))[:m]
    for tie, extend in ((0, 0), (1, 1)):
        want = _want(ref, read, SC, 0, extend, tie)
        b = _run(ctx, [ref], [read], SC, tie, 0, extend)
        u.check_pair(b, 0, want, GLOBAL, (m, n, tie, extend))
        b.free()


# 4 -- band
def _band_pair(rng, m=2100):
    """a 40-column deletion in strip 0 (columns 501 .. 540), and a 40-row insertion over rows 990 .. 1029: it starts in strip 0 and
    ends in strip 1's first rows, so the sweep carries F2 over the banded seam and the walk steps up across it in state F2"""
    base = u.rand(rng, m)
    ref = base[:500] + u.rand(rng, 40) + base[500:989] + base[1029:]
    read = base
    return ref, read


def _insertion_rows(aln, k):
    """first and last read row (1-based) of the run of k inserted rows in an alignment (reference string, read string)"""
    ra, qa = aln
    at = ra.index("_" * k)
    first = len(qa[:at].replace("_", "")) + 1
    return first, first + k - 1


@pytest.mark.parametrize("w", [7, 8, 9, 64])
def test_band(ctx, w):
    rng = random.Random(8805)
    ref, read = _band_pair(rng)
    assert len(read) == 2100 and len(ref) == 2100
    for tie, extend in ((w & 1, 0), (1 - (w & 1), 1)):
        want = _want(ref, read, CROSS, w, extend, tie)
        assert "_" * 40 in want[1][0][1][1]                       # the deletion
        lo, hi = _insertion_rows(want[1][0][1], 40)               # the insertion spans the seam between rows 1024 and 1025
        assert lo <= 1024 < 1025 <= hi and hi - lo == 39, (lo, hi)
        b = _run(ctx, [ref], [read], CROSS, tie, w, extend)
        u.check_pair(b, 0, want, GLOBAL, (w, tie, extend))
        b.free()


def test_band_differs_from_unbanded(ctx):
    """the insertion first: the unbanded path runs 40 columns left of the diagonal into strip 1, outside a band of 7"""
    rng = random.Random(8806)
    base = u.rand(rng, 2100)
    read = base
    ref = base[:500] + base[540:1500] + u.rand(rng, 40) + base[1500:]
    want = _want(ref, read, CROSS, 7)
    assert want[:2] != _want(ref, read, CROSS, 0)[:2]
    b = _run(ctx, [ref], [read], CROSS, 0, 7)
    u.check_pair(b, 0, want, GLOBAL)
    b.free()


def test_band_refusals_unchanged(ctx):
    rng = random.Random(8807)
    base = u.rand(rng, 2100)
    p = sw.make_params(SC[:3])
    # (m, n) outside the band in global mode: a read of 1025 bases takes a reference of up to 2048 + 16
    b = _run(ctx, [base[:2064]], [base[:1025]], SC, 0, 16)
    u.check_pair(b, 0, _want(base[:2064], base[:1025], SC, 16), GLOBAL)
    b.free()
    b = ctx.upload([base[:2065]], [base[:1025]])
    _refused(b, p)
    b.free()
    # an empty window: a read of 2049 bases has three strips, the last one's window starts at 2048 + 1 - 8
    ctx.set_option("band", 8)
    b = ctx.upload([base[:2040]], [base[:2049]])
    _refused(b, p)
    b.free()


# 5 -- tie-rich pairs: the cell lists of an extend run, the exact-size re-run, both string paths
TIES = (2, -2, -2, -2, -1, -8)
_TIE_PAIR = {}


def _tie_pair():
    if not _TIE_PAIR:
        rng = random.Random(8808)
        _TIE_PAIR.update(ref=u.rand(rng, 220, "AC"), read=u.rand(rng, 200, "AC"))
        for tie in (0, 1):
            for extend in (0, 1):
                _TIE_PAIR[(tie, extend)] = _want(_TIE_PAIR["ref"], _TIE_PAIR["read"], TIES, 0, extend, tie)
    return _TIE_PAIR


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("opts", [{}, {"cell_cap": 1}, {"device_strings": 0}, {"device_strings": 0, "cell_cap": 1}, {"zero_copy": 0}])
def test_tie_rich(ctx, opts, tie):
    t = _tie_pair()
    for extend in (1, 0):
        b = _run(ctx, [t["ref"]], [t["read"]], TIES, tie, 0, extend, **opts)
        u.check_pair(b, 0, t[(tie, extend)], GLOBAL, (opts, tie, extend))
        if extend and "cell_cap" in opts and len(t[(tie, extend)][2]) > 1:
            assert b.timing().rerun_pairs > 0
        b.free()


def test_tie_rich_scores_only(ctx):
    t = _tie_pair()
    for extend in (1, 0):
        b = _run(ctx, [t["ref"]], [t["read"]], TIES, 0, 0, extend, scores_only=1)
        assert b.score(0) == t[(0, extend)][0]
        b.free()


# 6 -- (o2, e2) = (o1, e1): the one-piece run, record for record
@pytest.mark.parametrize("tie", [0, 1])
def test_equals_one_piece_run(ctx, tie):
    rng = random.Random(8809)
    base = u.rand(rng, 1400)
    refs = [base[:300], base[:1200], u.rand(rng, 90, "AC")]
    reads = [gc.mutate(rng, base[:280]), gc.mutate(rng, base[:70]), gc.mutate(rng, base[:1100]), u.rand(rng, 80, "AC")]
    sc = (2, -3, -2, -4, -2, -4)
    for extend in (0, 1):
        b2 = _run(ctx, refs, reads, sc, tie, 0, extend)
        got2 = [(b2.score(p), b2.n_alignments(p), b2.alignments(p, with_cell=True)) for p in range(len(refs) * len(reads))]
        b2.free()
        ctx.set_option("gap_open2", 0)
        b1 = u.run(ctx, refs, reads, sc, tie, GLOBAL, 0, extend, None, long_reads=1)
        got1 = [(b1.score(p), b1.n_alignments(p), b1.alignments(p, with_cell=True)) for p in range(len(refs) * len(reads))]
        b1.free()
        assert got2 == got1, extend


# 7 -- the limits
def test_limits(ctx):
    rng = random.Random(8810)
    L = 1 << 20
    ref = u.rand(rng, 64, "AC")
    read = (ref[:30] + u.rand(rng, 1024, "AC"))[:1024]
    sc = (L, -L, -L, -L, -L, -L)
    b = _run(ctx, [ref], [read], sc)
    u.check_pair(b, 0, _want(ref, read, sc, align=tr.align_scalar), GLOBAL)
    p = sw.make_params(sc[:3])
    for name in ("gap_open2", "gap2"):
        ctx.set_option(name, -L - 1)
        _refused(b, p)
        ctx.set_option(name, -L)
    b.run(p)
    b.free()
    # global mode's int32 bound reads |gap_open| and |gap| as the larger of the two pieces': 3 * 1 + (64 + n) * 2^20 <= 2^31 with
    # gap = -1, gap2 = -2^20, gap_open = 0, gap_open2 = -1 -- the last n inside, the first outside
    n_ok = ((1 << 31) - 3) // L - 64
    assert 3 + (64 + n_ok) * L <= 1 << 31 < 3 + (64 + n_ok + 1) * L
    ref = read[:40] + u.rand(rng, n_ok + 1 - 40, "AC")
    sc = (L, -3, -1, 0, -L, -1)
    b = _run(ctx, [ref[:n_ok]], [read[:64]], sc)
    u.check_pair(b, 0, _want(ref[:n_ok], read[:64], sc), GLOBAL)
    b.free()
    b = ctx.upload([ref], [read[:64]])
    _refused(b, sw.make_params(sc[:3]))
    b.free()


# 8 -- option handling
def _small(rng):
    base = u.rand(rng, 260)
    return [base, gc.mutate(rng, base)], [gc.mutate(rng, base[:200]), base[:40] + base[80:150]]


@pytest.mark.parametrize("combo", ["local", "fit", "matrix", "xdrop", "band_adapt"])
def test_refused_combinations(ctx, combo):
    rng = random.Random(8811)
    refs, reads = _small(rng)
    ctx.set_option("gap_open2", SC[5])
    ctx.set_option("gap2", SC[4])
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("long_reads", 1)
    ctx.set_option("align_mode", {"local": sw.ALIGN_LOCAL, "fit": sw.ALIGN_FIT}.get(combo, GLOBAL))
    if combo == "matrix":
        ctx.set_score_matrix(*gc.score_matrix())
    if combo in ("xdrop", "band_adapt"):
        ctx.set_option("extend", 1)
        ctx.set_option("band", 64)
        ctx.set_option("xdrop" if combo == "xdrop" else "band_adapt", 50 if combo == "xdrop" else 1)
    b = ctx.upload(refs, reads)
    p = sw.make_params(SC[:3])
    assert "gap_open2" in _refused(b, p)
    ctx.set_option("gap_open2", 0)                                # the batch is still usable: the run the context now describes
    b.run(p)
    assert b.pipeline_mode() == 3
    b.free()


def test_invalid_values_leave_the_context(ctx):
    rng = random.Random(8812)
    refs, reads = _small(rng)
    exp = _expect(refs, reads, SC)
    b = _run(ctx, refs, reads, SC)
    for name in ("gap_open2", "gap2"):
        for bad in (1, 1 << 40, -(1 << 31) - 1):
            with pytest.raises(_capi.SwmiError) as e:
                ctx.set_option(name, bad)
            assert e.value.code == ERR_INVALID
    b.run(sw.make_params(SC[:3]))
    _check(b, refs, reads, exp)
    b.free()


def test_gap2_alone_changes_nothing(ctx):
    rng = random.Random(8813)
    refs, reads = _small(rng)
    ctx.set_option("gap_open2", 0)
    for mode in (sw.ALIGN_LOCAL, sw.ALIGN_FIT, GLOBAL):
        got = []
        for gap2 in (0, -1):
            b = u.run(ctx, refs, reads, SC[:4], 0, mode, 0, 0, None, gap2=gap2)
            got.append([(b.score(p), b.alignments(p, with_cell=True)) for p in range(4)])
            b.free()
        assert got[0] == got[1]
        assert got[0][0][:1] == gr.align_numpy(refs[0], reads[0], SC[:4], mode)[:1]


def test_values_travel_with_the_run(ctx):
    rng = random.Random(8814)
    refs, reads = _small(rng)
    two = _expect(refs, reads, CROSS)
    other = _expect(refs, reads, CROSS[:4] + (-1, -6))
    assert any(two[k][:2] != other[k][:2] for k in two)
    p = sw.make_params(CROSS[:3])
    for name in ("gap_open", "align_mode", "gap2"):
        ctx.set_option(name, {"gap_open": CROSS[3], "align_mode": GLOBAL, "gap2": CROSS[4]}[name])
    ctx.set_option("gap_open2", CROSS[5])
    ctx.set_option("debug_async_delay_us", 50000)
    b = ctx.upload(refs, reads).run_async(p)
    ctx.set_option("gap_open2", -6)                               # does not reach the run in flight
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    _check(b, refs, reads, two)
    b.run(p)
    _check(b, refs, reads, other)
    b.free()


# 9 -- the doubled field against max_workspace_bytes
def test_doubled_field_and_the_workspace_cap(ctx):
    rng = random.Random(8815)
    ref = u.rand(rng, 1100)
    read = gc.mutate(rng, ref)[:1025] + u.rand(rng, 1025)
    read = read[:1025]
    one = 2 * ((1100 + 70) // 8) * 16 * 64 * 4                    # two strips of a one-piece field, in bytes
    ctx.set_option("max_workspace_bytes", one + one // 2)
    ctx.set_option("gap_open2", 0)
    b = u.run(ctx, [ref], [read], SC[:4], 0, GLOBAL, 0, 0, None, long_reads=1)      # the one-piece field fits
    b.free()
    ctx.set_option("gap_open2", SC[5])
    ctx.set_option("gap2", SC[4])
    b = ctx.upload([ref], [read])
    msg = _refused(b, sw.make_params(SC[:3]))
    assert str(2 * one) in msg
    b.free()
    # shorter pairs are chunked by the doubled field: a read of 640 bases (R = 10) against 1000 columns leaves 133 blocks of 10 * 64
    # dwords, 340,480 bytes -- three fit 1 MiB -- and twice that with two planes: one pair per launch
    base = u.rand(rng, 1000)
    refs = [gc.mutate(rng, base)[:1000] + u.rand(rng, 40) for _ in range(3)]
    refs = [r[:1000] for r in refs]
    reads = [gc.mutate(rng, base[:600]) + u.rand(rng, 60)]
    reads = [reads[0][:640]]
    assert 3 * 340480 <= 1 << 20 < 2 * 2 * 340480
    ctx.set_option("max_workspace_bytes", 1 << 20)
    ctx.set_option("gap_open2", 0)
    b = u.run(ctx, refs, reads, SC[:4], 0, GLOBAL, 0, 0, None, long_reads=1)
    assert b.timing().fill_launches == 1
    b.free()
    b = _run(ctx, refs, reads, SC)
    assert b.timing().fill_launches == 3
    _check(b, refs, reads, _expect(refs, reads, SC))
    b.free()


# 10 -- the schedule key: ONE batch on one context, re-run under options that each give the pair another workspace.  A schedule
# kept from the run before would hand the run a workspace sized for the previous geometry
def test_schedule_follows_the_run_options(ctx):
    rng = random.Random(8816)
    ref = u.rand(rng, 1300)
    read = gc.mutate(rng, ref[:1080]) + u.rand(rng, 40)
    read = read[:1100]
    assert (len(read), len(ref)) == (1100, 1300)                  # two strips
    w, sc = 64, SC[:4]
    plain = u.expect([ref], [read], sc, GLOBAL, 0, False, cells=True)[(0, 0)]
    banded = u.expect([ref], [read], sc, GLOBAL, w, True, cells=True)[(0, 0)]
    assert plain[:2] != banded[:2]
    steps = [({"long_reads": 1}, plain),
             ({"band": w, "extend": 1}, banded),
             ({"band_adapt": 1}, ar.align(ref, read, sc, w)[:3]),
             ({"band_adapt": 0}, banded),
             ({"gap_open2": SC[5], "gap2": SC[4]}, _want(ref, read, SC, w, 1)),
             ({"gap_open2": 0, "band": 0, "extend": 0}, plain)]
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("align_mode", GLOBAL)
    b = ctx.upload([ref], [read])
    p = sw.make_params(sc[:3])
    for at, (options, want) in enumerate(steps):
        for name, value in options.items():
            ctx.set_option(name, value)
        b.run(p)
        assert b.pipeline_mode() == 3
        u.check_pair(b, 0, want, GLOBAL, at)
    b.free()


# 11 -- the JNI shim's entry point from plain C99 (tests/c/shim_twopiece.c)
def test_c99_shim_sets_gap2(tmp_path):
    out = u.run_shim(tmp_path, "shim_twopiece")
    ref, read = "GGCCCAGTCCAGCCCAACTAACGAATAAGTAGAATCCTCGGAAGT", "GGCCCAGTCCAGATCCTCGGAAGT"
    two = tr.align_scalar(ref, read, CROSS)
    one = gr.align_scalar(ref, read, CROSS[:4], GLOBAL)
    assert (two[0], one[0]) == (3, 2) and two[1] == one[1]
    site = "1:%s/%s" % two[1][0][1]
    assert out.splitlines() == ["3 1 %s mode 3" % site, "2 1 %s mode 3" % site, "refused %d" % ERR_UNSUPPORTED]
