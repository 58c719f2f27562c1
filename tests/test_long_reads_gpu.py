"""Reads longer than 1024 bases on the affine kernels (option "long_reads": the strip sweeps and the long traceback of
swmi_affine.hip), against the restatement of tests/gotoh_reference.py.  Every test first sets
long_reads = 1."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M

import affine_gpu_util as u
import gotoh_reference as gr
import long_reads_cases as lc

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)


@pytest.fixture
def ctx():
    c = sw.Context(0)
    c.set_option("long_reads", 1)
    yield c
    c.close()


# 1 -- strip counts and skew: all three kernel families in one batch
_SHAPES = {}


def _shapes():
    if not _SHAPES:
        rng = random.Random(8201)
        refs = [u.rand(rng, n) for n in (1, 40, 63, 300, 700)]
        reads = [u.rand(rng, m) for m in (1025, 1088, 2047, 2048, 2049, 3100, 1, 64, 150, 1024)]
        for k in (0, 2, 4, 5):                                   # (something to find: a stretch of the longest reference on either side of a seam)
            reads[k] = reads[k][:990] + refs[4][100:180] + reads[k][1070:]
        _SHAPES["refs"], _SHAPES["reads"] = refs, reads
    return _SHAPES["refs"], _SHAPES["reads"]


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("o", [-1, -12])
def test_long_reads_strip_counts_and_skew(ctx, o, tie):
    refs, reads = _shapes()
    sc = (5, -3, -2, o)
    key = ("exp", o, tie)
    if key not in _SHAPES:
        _SHAPES[key] = u.expect(refs, reads, sc, tie=tie)
    b = u.run(ctx, refs, reads, sc, tie, 0)
    u.check(b, refs, reads, _SHAPES[key])
    b.free()


# 2 -- across the seam
@pytest.mark.parametrize("tie", [0, 1])
def test_long_reads_across_the_seam(ctx, tie):
    for name, ref, read, sc in lc.seam_cases():
        want = gr.align_numpy(ref, read, sc, tie_mode=tie)
        b = u.run(ctx, [ref], [read], sc, tie, 0)
        assert (b.score(0), b.alignments(0)) == want, name
        u.check(b, [ref], [read], {(0, 0): want})
        b.free()
        rows = sorted(len(a[1][1].replace(gr.GAP_CHAR, "")) for a in want[1])      # (local: read bases each alignment spells)
        if name == "ties_both_strips":
            assert len(want[1]) == 2, name
        if name in ("later_strip_higher", "later_strip_lower"):
            assert len(want[1]) == 1 and rows == [64], name


# 3 -- more tied maxima than the cell list holds: the exact-size re-run
def test_long_reads_cell_list_overflow_rerun(ctx):
    rng = random.Random(8203)
    ref = "ACGTTGCA" * 60
    read = u.rand(rng, 500, "T") + "ACGTTGCAAC" + u.rand(rng, 590, "T")
    assert len(read) == 1100
    sc = (5, -3, -2, -6)
    want = gr.align_numpy(ref, read, sc)
    assert len(want[1]) > 4
    ctx.set_option("cell_cap", 4)
    b = u.run(ctx, [ref], [read], sc, 0, 0)
    assert b.timing().rerun_pairs == 1
    assert b.n_alignments(0)[0] == len(want[1])
    assert (b.score(0), b.alignments(0)) == want
    b.free()


# 4 -- fit and global
@pytest.mark.parametrize("tie", [0, 1])
def test_long_reads_fit_and_global(ctx, tie):
    for name, ref, read, sc, mode in lc.ends_cases():
        want = gr.align_numpy(ref, read, sc, mode, tie_mode=tie)
        b = u.run(ctx, [ref], [read], sc, tie, mode)
        assert (b.score(0), b.alignments(0)) == want, name
        b.free()
        if name == "fit_head_overhang":                          # the j == 0 tail starts at row 1100 and crosses the seam
            assert all(a[1][0].startswith(gr.GAP_CHAR * 1100) for a in want[1]), name


# 5 -- BLOSUM62
@pytest.mark.parametrize("mode", [0, 2])
def test_long_reads_blosum62(ctx, mode):
    rng = random.Random(8205)
    amino = "ARNDCQEGHILKMFPSTWYV"
    ref = u.rand(rng, 400, amino)
    read = list(u.rand(rng, 1500, amino))
    read[950:1150] = ref[100:300]                                 # (a stretch of the reference across the seam)
    read = "".join(read)
    sc = (5, -4, -1, -11)
    ctx.set_score_matrix(M.BLOSUM62)
    b = u.run(ctx, [ref], [read], sc, 0, mode)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, sc, mode, matrix=(M.BLOSUM62.alphabet, M.BLOSUM62.scores))
    b.free()


# 6 -- the bounds from both sides
def test_long_reads_bounds(ctx):
    S = 1 << 19
    sc = (S, -S, -S, -S)
    rng = random.Random(8206)
    read = u.rand(rng, 2049, "AC")
    b = u.run(ctx, [read[:2048]], [read[:2048]], sc, 0, 0)             # M * S = 2^30: runs, and H reaches 2^30
    want = gr.align_numpy(read[:2048], read[:2048], sc)        # (int64 arithmetic)
    assert want[0] == 1 << 30
    assert (b.score(0), b.alignments(0)) == want
    b.free()
    b = ctx.upload([read[:2048]], [read])                         # M = 3072
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params(sc[:3]))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()
    # global: 3 |o| + (M + n) |e| <= 2^31, M = 2048 for a read of 1025
    ctx.set_option("align_mode", 2)
    e_, n = 463419, 2586
    assert (2048 + n) * e_ == (1 << 31) - 2
    ref = u.rand(rng, n, "AC")
    ctx.set_option("gap_open", 0)
    b = ctx.upload([ref], [read[:1025]])                          # 2^31 - 2: runs
    b.run(sw.make_params((5, -3, -e_)))
    assert b.score(0) == gr.align_numpy(ref, read[:1025], (5, -3, -e_, 0), 2)[0]
    ctx.set_option("gap_open", -1)                                # 3 more: 2^31 + 1, one past
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -e_)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()
    # back to 0 on the same context: the 1024 limit again
    ctx.set_option("align_mode", 0)
    ctx.set_option("gap_open", -6)
    ctx.set_option("long_reads", 0)
    b = ctx.upload(["ACGT" * 10], ["A" * 1025])
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    ctx.set_option("long_reads", 1)
    with pytest.raises(_capi.SwmiError) as e:
        ctx.set_option("long_reads", 2)
    assert e.value.code == ERR_INVALID
    b.run(sw.make_params((5, -3, -4)))                            # (still 1)
    assert b.score(0) == 5
    ctx.set_option("long_reads", 0)
    with pytest.raises(_capi.SwmiError) as e:
        ctx.set_option("long_reads", -1)
    assert e.value.code == ERR_INVALID
    with pytest.raises(_capi.SwmiError) as e:                     # (still 0)
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()


def test_long_reads_workspace_cap_is_a_status(ctx):
    """a pair whose field alone is over max_workspace_bytes is refused before a launch"""
    rng = random.Random(8207)
    ctx.set_option("max_workspace_bytes", 1 << 20)
    ctx.set_option("gap_open", -6)
    b = ctx.upload([u.rand(rng, 700)], [u.rand(rng, 3100)])          # 4 strips x 97 blocks x 4 KiB
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -2)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()


# 7 -- plumbing
_PLUMB = {}


def _plumbing():
    if not _PLUMB:
        rng = random.Random(8208)
        refs = [u.rand(rng, 90), "ACGTTGCA" * 12, u.rand(rng, 120)]
        reads = [u.rand(rng, 2049) for _ in range(4)] + [u.rand(rng, 100)]
        reads[1] = reads[1][:1000] + refs[0][10:80] + reads[1][1070:]
        reads[2] = reads[2][:2040] + "ACGTTGCAA"
        sc = (5, -3, -2, -6)
        _PLUMB.update(refs=refs, reads=reads, sc=sc,
                      exp=u.expect(refs, reads, sc))
    return _PLUMB["refs"], _PLUMB["reads"], _PLUMB["sc"], _PLUMB["exp"]


@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("max_workspace_bytes", 1 << 20)])
def test_long_reads_options(ctx, opt):
    refs, reads, sc, exp = _plumbing()
    ctx.set_option(*opt)
    b = u.run(ctx, refs, reads, sc, 0, 0)
    u.check(b, refs, reads, exp, alignments=opt[0] != "scores_only")
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    b.free()


def test_long_reads_async_takes_the_value_at_the_call(ctx):
    refs, reads, sc, exp = _plumbing()
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("debug_async_delay_us", 50000)
    b = ctx.upload(refs, reads).run_async(sw.make_params(sc[:3]))
    ctx.set_option("long_reads", 0)                               # does not reach the run in flight
    b.wait()
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, exp)
    b.free()


def test_long_reads_stream_equals_the_batch(ctx):
    rng = random.Random(8209)
    refs = [u.rand(rng, rng.randint(60, 200)) for _ in range(12)]
    read = u.rand(rng, 1500)
    read = read[:990] + refs[5][20:90] + read[1060:]
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    st = ctx.stream([read], sw.make_params(sc[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("long_reads", 0)                               # (the slots copied it at the open)
    st.push(refs[:7]).push(refs[7:]).finish()
    ctx.set_option("long_reads", 1)
    b = u.run(ctx, refs, [read], sc, 0, 0)
    assert [int(t) for t in st.totals()] == [b.ref_total(r) for r in range(len(refs))]
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            assert c.ref_match_sites(r) == b.ref_match_sites(first + r), first + r
    assert b.ref_match_sites(5) == sorted(gr.align_numpy(refs[5], read, sc)[1], key=lambda t: t[0])
    st.close()
    b.free()
