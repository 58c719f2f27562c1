"""Banded alignment of reads longer than 1024 bases (option "band": the banded strip sweeps and long tracebacks of
swmi_affine.hip) against tests/gotoh_reference.py at strip 1024: score, flags, the order of the cell list,
every alignment's begin and both strings.  Every test sets long_reads = 1 and a band; set_option("band", ...) is what fails
without the feature."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M

import affine_gpu_util as u
import affine_grid_cases as gc
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
SC = (5, -3, -2, -6)


@pytest.fixture
def ctx():
    c = sw.Context(0)
    c.set_option("long_reads", 1)
    yield c
    c.close()


# 1 -- window origins and lengths off the 8-step grid.  Each (w, gap_open) takes the four read lengths.  With wi the index of w,
# ob = (gap_open != 0) and k the index of the length, the case runs mode (2 wi + ob + k) % 3, tie mode ((2 wi + ob) // 3 + k) % 2
# and, for the three multi-strip-or-longer lengths, the reference length number (wi + k) % 3 of (m - w, m, m + w): over the twelve
# cases every length meets every mode four times, both tie modes, and each mode with two of the three reference lengths (six of
# the nine (mode, n) pairs; the crossed ones are left to the 1025-base read, which takes all three reference lengths every time,
# and to the geometry bounds below).  The full cross product would be 72 reference sweeps per case.
_LENGTHS = (1025, 2048, 2049, 3000)


@pytest.mark.parametrize("o", [0, -6])
@pytest.mark.parametrize("w", [1, 7, 8, 9, 64, 300])
def test_band_shapes(ctx, w, o):
    case = [1, 7, 8, 9, 64, 300].index(w) * 2 + (o != 0)
    rng = random.Random(9500 + case)
    sc = (5, -3, -2, o)
    for k, m in enumerate(_LENGTHS):
        mode, tie = (case + k) % 3, (case // 3 + k) % 2
        base = u.rand(rng, m + w + 16)
        read = u.mutate(rng, base)[:m]
        read += u.rand(rng, m - len(read))
        refs = [base[:n] for n in (m - w, m, m + w)]
        if k:
            refs = [refs[(case // 2 + k) % 3]]
        reads = [read, u.mutate(rng, base[200:500])]               # (the short read of the batch is swept in full)
        exp = u.expect(refs, reads, sc, mode, w, tie=tie)
        for r in range(len(refs)):
            assert exp[(r, 1)] == gr.align_numpy(refs[r], reads[1], sc, mode, tie_mode=tie)
        b = u.run(ctx, refs, reads, sc, tie, mode, w)
        u.check(b, refs, reads, exp, mode)
        b.free()


# 2 -- the edges of the staircase; every case is built so that the unbanded result differs
def _edge_cases():
    rng = random.Random(9600)
    w = 20
    out = []
    # upper edge: a stretch on the diagonal j = i + w + 1 over rows 990 .. 1060.  Rows up to 1023 have it inside (column
    # 1024 + w is the last of strip 0), cell (1024, 1025 + w) is outside, and from row 1025 on it is inside again, fed from above
    # by columns past the end of what strip 0 wrote
    read = u.rand(rng, 1300, "AC")
    ref = list(u.rand(rng, 1300 + w, "GT"))
    ref[990 + w: 1061 + w] = read[989:1060]
    out.append(("upper_edge", "".join(ref), read, w))
    # lower edge: a stretch on the diagonal j = i - w - 30 over rows 1000 .. 1100: rows 1025 .. 1054 lie left of strip 1's first
    # column 1025 - w, and the stretch comes back into the band on that column at row 1055
    ref = list(u.rand(rng, 1300, "GT"))
    ref[999 - w - 30: 1100 - w - 30] = read[999:1100]
    out.append(("lower_edge", "".join(ref), read, w))
    # the best unbanded path leaves the band: the whole read lies on the diagonal j = i + 300, which is outside strip 0's window
    # (columns up to 1024 + w) from row 745 to row 1024 and inside again in strip 1
    out.append(("leaves_band", u.rand(rng, 300, "GT") + read, read, w))
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_band_edges(ctx, mode):
    for name, ref, read, w in _edge_cases():
        want0 = gr.align_numpy(ref, read, SC, mode, w)
        assert want0 != gr.align_numpy(ref, read, SC, mode), name
        for tie in (0, 1):
            want = gr.align_numpy(ref, read, SC, mode, w, tie_mode=tie) if tie else want0
            b = u.run(ctx, [ref], [read], SC, tie, mode, w)
            assert (b.score(0), b.alignments(0)) == want, (name, tie)
            b.free()


# 2b -- local mode: an alignment clipped by the staircase begins on an in-band cell whose diagonal predecessor is outside (H = 0)
def _clipped_cases():
    w, out = 20, []
    # left edge: a stretch on the diagonal j = i - d over rows 1025 .. r + 100 that enters strip 1's window on its first column
    # 1025 - w at row r = 1025 - w + d, in the rows of lane 0 (1026 .. 1040); the rows above r are left of the window
    for r in (1026, 1033, 1040):
        d = r - (1025 - w)
        out.append(("left_row_%d" % r, 1024, r + 100, -d, (r, 1025 - w)))
    # upper edge: a stretch on the diagonal j = i + d over rows 1010 .. 1125; in strip 0 it lies right of column 1024 + w, so it
    # begins on row 1025, at column 1025 + d >= (1024 + w) + 16
    for d in (36, 59, 200):
        out.append(("upper_col_%d" % (1025 + d), 1009, 1125, d, (1025, 1025 + d)))
    return w, out


@pytest.mark.parametrize("case", range(6))
def test_band_local_alignment_clipped_by_the_staircase(ctx, case):
    w, cases = _clipped_cases()
    name, r0, r1, d, first = cases[case]
    rng = random.Random((9650, 9651, 9700, 9653, 9654, 9655)[case])      # (seeds under which no chance match of the AC / GT
                                                                          # background joins the stretch: the assert below)
    read = u.rand(rng, 1300, "AC")
    ref = list(u.rand(rng, 1400, "GT"))
    ref[r0 + d:r1 + d] = read[r0:r1]                              # rows r0 + 1 .. r1 on the diagonal j = i + d
    ref = "".join(ref)
    full = gr.align_numpy(ref, read, SC)
    assert full[0] == 5 * (r1 - r0)
    for tie in (0, 1):
        want = gr.align_numpy(ref, read, SC, 0, w, tie_mode=tie)
        # one alignment, the stretch from the first in-band cell on: it begins at that cell's column and is shorter than unbanded
        assert want == (5 * (r1 - first[0] + 1), [(first[1], (ref[first[1] - 1:r1 + d], read[first[0] - 1:r1]))]), name
        assert want[0] < full[0]
        for zc in (1, 0):
            ctx.set_option("zero_copy", zc)
            b = u.run(ctx, [ref], [read], SC, tie, 0, w)
            assert (b.score(0), b.alignments(0)) == want, (name, tie, zc)
            b.free()


# 3 -- tied maxima, the degenerate count, the exact-size re-run
def test_band_ties_in_two_strips(ctx):
    rng = random.Random(9700)
    read = list(u.rand(rng, 2100, "AC"))
    ref = list(u.rand(rng, 2110, "GT"))
    motif = "ACCACAACCCAACACCA"
    for at in (500, 1500):
        read[at:at + len(motif)] = motif
        ref[at + 3:at + 3 + len(motif)] = motif
    read, ref = "".join(read), "".join(ref)
    for tie in (0, 1):
        want = gr.align_numpy(ref, read, SC, 0, 10, tie_mode=tie)
        assert len(want[1]) == 2 and want[0] == 5 * len(motif)
        b = u.run(ctx, [ref], [read], SC, tie, 0, 10)
        assert (b.score(0), b.alignments(0)) == want
        b.free()


def test_band_degenerate_count_is_in_band(ctx):
    ref, read = "C" * 2500, "A" * 2100
    b = u.run(ctx, [ref], [read], SC, 0, 0, 33)
    n, flags = b.n_alignments(0)
    assert b.score(0) == 0 and flags & sw.PAIR_DEGENERATE
    assert n == gr.in_band_cells(2100, 2500, 33) < 2100 * 2500
    b.free()


def test_band_cell_list_overflow_rerun(ctx):
    """fit mode with free gaps: every column of row m from the end of the match on ties, all in the band"""
    rng = random.Random(9701)
    read = u.rand(rng, 1100)
    ref = read + "T" * 40
    sc = (5, -3, 0, 0)
    want = gr.align_numpy(ref, read, sc, 1, 50)
    assert len(want[1]) > 8
    ctx.set_option("cell_cap", 2)
    b = u.run(ctx, [ref], [read], sc, 0, 1, 50)
    assert b.timing().rerun_pairs == 1
    assert (b.score(0), b.alignments(0)) == want
    b.free()


# 4 -- score matrices
@pytest.mark.parametrize("mode", [0, 2])
def test_band_blosum62(ctx, mode):
    rng = random.Random(9800)
    amino = "ARNDCQEGHILKMFPSTWYV"
    ref = u.rand(rng, 1600, amino)
    read = "".join(rng.choice(amino) if rng.random() < 0.2 else c for c in ref[40:1540])
    sc = (5, -4, -1, -11)
    ctx.set_score_matrix(M.BLOSUM62)
    want = gr.align_numpy(ref, read, sc, mode, 200, matrix=(M.BLOSUM62.alphabet, M.BLOSUM62.scores))
    b = u.run(ctx, [ref], [read], sc, 0, mode, 200)
    assert (b.score(0), b.alignments(0)) == want
    b.free()


def test_band_64_symbol_matrix(ctx):
    rng = random.Random(9801)
    alpha = bytes(range(0x21, 0x21 + 64)).decode("latin-1")
    rows = [[rng.randint(-9, 4) for _ in range(64)] for _ in range(64)]
    for k in range(64):
        rows[k][k] = rng.randint(5, 11)
    draw = alpha.replace(gr.GAP_CHAR, "")
    ref = u.rand(rng, 1300, draw)
    read = "".join(rng.choice(draw) if rng.random() < 0.15 else c for c in ref[10:1210])
    sc = (5, -4, -2, -7)
    ctx.set_score_matrix(alpha, rows)
    want = gr.align_numpy(ref, read, sc, 1, 40, tie_mode=1, matrix=(alpha, rows))
    b = u.run(ctx, [ref], [read], sc, 1, 1, 40)
    assert (b.score(0), b.alignments(0)) == want
    b.free()


# 5 -- the bounds from both sides
def _refused(ctx, b, params):
    with pytest.raises(_capi.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED


def test_band_arithmetic_bounds(ctx):
    rng = random.Random(9900)
    read = u.rand(rng, 2048, "AC")
    ref = read[:1000] + u.rand(rng, 1048, "AC")
    S = 1 << 18                                                   # M * S = 2048 * 2^18 = 2^29: runs
    sc = (S, -S, -S, -S)
    want = gr.align_numpy(ref, read, sc, 1, 8)                 # (int64 arithmetic)
    b = u.run(ctx, [ref], [read], sc, 0, 1, 8)
    assert (b.score(0), b.alignments(0)) == want
    _refused(ctx, b, sw.make_params((S + 1, -S, -S)))             # one past
    ctx.set_option("align_mode", 0)                               # local keeps the unbanded bound M * S <= 2^30
    b.run(sw.make_params((2 * S, -S, -S)))
    assert b.score(0) == gr.align_numpy(ref, read, (2 * S, -S, -S, -S), 0, 8)[0]
    b.free()
    # global: 3 |o| + (M + n) |e| <= 2^30 with M = n = 2048, e = -2^18, o = 0: exactly 2^30
    sc = (5, -3, -S, 0)
    want = gr.align_numpy(ref, read, sc, 2, 8)
    b = u.run(ctx, [ref], [read], sc, 0, 2, 8)
    assert (b.score(0), b.alignments(0)) == want
    ctx.set_option("gap_open", -1)                                # 3 more
    _refused(ctx, b, sw.make_params(sc[:3]))
    b.free()


def test_band_geometry_bounds(ctx):
    rng = random.Random(9901)
    base = u.rand(rng, 2100)
    p = sw.make_params(SC[:3])
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("band", 8)
    # a read of 2049 bases has three strips; the last one's window starts at column 2048 + 1 - 8 = 2041
    b = ctx.upload([base[:2041]], [base[:2049]]).run(p)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(base[:2041], base[:2049], SC, 0, 8)
    b.free()
    b = ctx.upload([base[:2040]], [base[:2049]])
    _refused(ctx, b, p)
    b.free()
    # global: a read of 1025 bases has two strips, (m, n) is in the band up to n = 2048 + 8
    ctx.set_option("align_mode", 2)
    ref = base[:1025] + u.rand(rng, 1032)
    b = ctx.upload([ref[:2056]], [base[:1025]]).run(p)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref[:2056], base[:1025], SC, 2, 8)
    b.free()
    b = ctx.upload([ref], [base[:1025]])
    _refused(ctx, b, p)
    b.free()


def test_band_option_values(ctx):
    _, ref, read, w = _edge_cases()[2]
    want = gr.align_numpy(ref, read, SC, 0, w)
    assert want != gr.align_numpy(ref, read, SC)
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("band", w)
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("band", bad)
        assert e.value.code == ERR_INVALID
    b = ctx.upload([ref], [read]).run(sw.make_params(SC[:3]))     # (still w)
    assert (b.score(0), b.alignments(0)) == want
    ctx.set_option("band", 1 << 20)                               # the largest value: a band over everything
    b.run(sw.make_params(SC[:3]))
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, SC)
    b.free()


# 6 -- the workspace: the banded field is what is held against max_workspace_bytes
def test_band_fits_a_workspace_the_full_field_does_not(ctx):
    rng = random.Random(9903)
    ref = u.rand(rng, 3100)
    read = u.mutate(rng, ref)[:3050]
    ctx.set_option("max_workspace_bytes", 4 << 20)                # unbanded: 3 strips x 396 blocks x 4 KiB
    ctx.set_option("gap_open", SC[3])
    b = ctx.upload([ref], [read])
    _refused(ctx, b, sw.make_params(SC[:3]))
    ctx.set_option("band", 60)
    b.run(sw.make_params(SC[:3]))
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, SC, 0, 60)
    b.free()


# 7 -- plumbing
_PLUMB = {}


def _plumbing():
    if not _PLUMB:
        rng = random.Random(9904)
        base = u.rand(rng, 1400)
        refs = [base[:1300], base[40:1400], u.mutate(rng, base)]
        reads = [u.mutate(rng, base)[:1250], base[700:800], u.mutate(rng, base[20:1320])]
        w = 12
        _PLUMB.update(refs=refs, reads=reads, w=w, exp=u.expect(refs, reads, SC, 0, w),
                      full={(r, q): gr.align_numpy(refs[r], reads[q], SC) for r in range(3) for q in range(3)})
        assert _PLUMB["exp"] != _PLUMB["full"]
    return _PLUMB["refs"], _PLUMB["reads"], _PLUMB["w"], _PLUMB["exp"], _PLUMB["full"]


@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("zero_copy", 0)])
def test_band_options(ctx, opt):
    refs, reads, w, exp, _ = _plumbing()
    ctx.set_option(*opt)
    b = u.run(ctx, refs, reads, SC, 0, 0, w)
    if opt[0] == "scores_only":
        for (r, q), (es, _) in exp.items():
            assert b.score(r * len(reads) + q) == es
    else:
        u.check(b, refs, reads, exp)
    b.free()


def test_band_alone_takes_the_affine_kernels(ctx):
    rng = random.Random(9905)
    ref, read = u.rand(rng, 300), u.rand(rng, 100)
    ctx.set_option("band", 5)                                     # gap_open 0, local, no matrix
    b = ctx.upload([ref], [read]).run(sw.make_params((5, -3, -2)))
    assert b.pipeline_mode() == 3
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(ref, read, (5, -3, -2, 0))
    b.free()


def test_band_async_takes_the_value_at_the_call(ctx):
    refs, reads, w, exp, _ = _plumbing()
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("band", w)
    ctx.set_option("debug_async_delay_us", 50000)
    b = ctx.upload(refs, reads).run_async(sw.make_params(SC[:3]))
    ctx.set_option("band", 0)                                     # does not reach the run in flight
    b.wait()
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, exp)
    b.free()


def test_band_0_after_a_banded_run_replans(ctx):
    refs, reads, w, exp, full = _plumbing()
    b = u.run(ctx, refs, reads, SC, 0, 0, w)
    u.check(b, refs, reads, exp)
    ctx.set_option("band", 0)
    b.run(sw.make_params(SC[:3]))
    u.check(b, refs, reads, full)
    ctx.set_option("band", w)
    b.run(sw.make_params(SC[:3]))
    u.check(b, refs, reads, exp)
    b.free()


def test_band_stream_equals_the_batch(ctx):
    refs, reads, w, exp, _ = _plumbing()
    rng = random.Random(9906)
    refs = refs + [u.mutate(rng, refs[0]) for _ in range(5)]
    read = reads[0]
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("band", w)
    st = ctx.stream([read], sw.make_params(SC[:3]), slots=2, chunk_bytes=1 << 12)
    ctx.set_option("band", 0)                                     # (the slots copied it at the open)
    st.push(refs[:5]).push(refs[5:]).finish()
    b = u.run(ctx, refs, [read], SC, 0, 0, w)
    assert [int(t) for t in st.totals()] == [b.ref_total(r) for r in range(len(refs))]
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            assert c.ref_match_sites(r) == b.ref_match_sites(first + r), first + r
    for r in range(3):
        assert b.score(r) == exp[(r, 0)][0]
    st.close()
    b.free()


def test_run_options_travel_together(ctx):
    """The score matrix, align_mode, long_reads and band a run takes are those set when it was asked for, all four together: an
    asynchronous run and a stream's slots hand them over as one value, and a field lost on the way would show here alone.
    Each of the four is changed before the run starts, and each changes the result (long_reads 0 refuses the long read)."""
    refs, reads, w, _, _ = _plumbing()
    reads = reads[:2]                                             # one read of two strips, one short read
    assert 1024 < len(reads[0]) <= 1300 and len(reads[1]) <= 1024
    mat, mode = gc.score_matrix(), 1
    assert not any(gr.refused(len(q), len(r), w, mode) for r in refs for q in reads)
    exp = u.expect(refs, reads, SC, mode, w, matrix=mat)
    assert exp[(1, 1)] != gr.align_numpy(refs[1], reads[1], SC, mode, w)              # no matrix
    assert exp[(1, 0)] != gr.align_numpy(refs[1], reads[0], SC, 0, w, matrix=mat)            # local
    assert exp[(1, 0)] != gr.align_numpy(refs[1], reads[0], SC, mode, 0, matrix=mat)         # no band
    p = sw.make_params(SC[:3])

    def set_all():
        ctx.set_score_matrix(*mat)
        ctx.set_option("align_mode", mode)
        ctx.set_option("long_reads", 1)
        ctx.set_option("band", w)

    def change_all():
        ctx.clear_score_matrix()
        ctx.set_option("align_mode", 0)
        ctx.set_option("long_reads", 0)
        ctx.set_option("band", 0)

    ctx.set_option("gap_open", SC[3])
    set_all()
    ctx.set_option("debug_async_delay_us", 50000)
    b = ctx.upload(refs, reads).run_async(p)
    change_all()                                                  # none of it reaches the run in flight
    b.wait()
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, exp, mode)
    b.free()

    set_all()
    st = ctx.stream(reads, p, slots=2, chunk_bytes=1 << 12)
    change_all()                                                  # (the slots copied all four at the open)
    st.push(refs[:2]).push(refs[2:]).finish()
    set_all()
    b = ctx.upload(refs, reads).run(p)
    u.check(b, refs, reads, exp, mode)
    assert [int(t) for t in st.totals()] == [b.ref_total(r) for r in range(len(refs))]
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            assert c.ref_match_sites(r) == b.ref_match_sites(first + r), first + r
    st.close()
    b.free()
