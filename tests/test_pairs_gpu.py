"""Pair lists on the GPU (swmi_batch_upload_pairs): chosen segments of sources that are uploaded once,
cut, reversed and encoded by sw_gather_kernel.

The contract is one sentence: pair k gives, bit for bit, what the library gives for the two segments cut -- and under
SWMI_SPEC_REVERSE reversed -- by the caller.  So every expected value here comes from the CPU references the other files use
(oracle.sw_oracle.opt_alignments for the linear pipelines; gotoh_reference, xdrop_reference, adapt_reference and
twopiece_reference for the affine kernels), called on PairBatch.segments(), which is plain slicing on the host
(tests/test_pairs_cpu.py).  All comparisons are exact.  Context.upload_pairs is what fails without the feature."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from oracle import sw_oracle as orc

import adapt_reference as ar
import affine_gpu_util as u
import gotoh_reference as gr
import twopiece_reference as tr
import xdrop_reference as xr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
WHOLE = _capi.SPEC_WHOLE
GLOBAL = sw.ALIGN_GLOBAL
TYPES = b"aid-"


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


_ORACLE = {}


def linear_want(ref, read, sc, tie):
    """(score, alignments) of the oracle for one pair, computed once per (segments, scores, tie mode)"""
    key = (ref, read, tuple(sc), tie)
    if key not in _ORACLE:
        _ORACLE[key] = orc.opt_alignments((ref, read), tuple(sc), TYPES, tie)
    return _ORACLE[key]


def check_linear_pair(b, pair, want, what):
    """score, count, flags, every alignment; a degenerate pair (score 0, both sides non-empty) lists one (0, "", "") per cell"""
    es, ea = want
    assert b.score(pair) == es, (what, b.score(pair), es)
    n, flags = b.n_alignments(pair)
    assert n == len(ea), (what, n, len(ea))
    if flags & sw.PAIR_DEGENERATE:
        assert flags == sw.PAIR_DEGENERATE and es == 0 and all(a == u.NO_ALIGNMENT for a in ea), what
        ref, read = b.segments(pair)
        assert b.alignment(pair, 0) == u.NO_ALIGNMENT and b.alignment(pair, n - 1, True) == (0, ("", ""), (len(read), len(ref))), what
        return
    assert flags == 0, (what, flags)
    assert b.alignments(pair) == ea, what


def check_linear(b, sc=(5, -3, -4), tie=0):
    for k in range(b.n_pairs()):
        ref, read = b.segments(k)
        check_linear_pair(b, k, linear_want(ref, read, sc, tie), (k, b.spec(k)))


# ---- 1: the gather grid ---------------------------------------------------------------------------------------------------------
def _grid_sources():
    rng = random.Random(11)
    # lower case, N, K (no fast symbol) and 0xE9 (upper-cased to 0xC9 by the code table): the strings show which bytes came through
    ref = "".join(rng.choice("ACGTacgtNnK\xe9\xc9") for _ in range(300))
    read = "".join(rng.choice("ACGTacgtNK\xe9") for _ in range(200))
    return [u.rand(rng, 40), ref], [u.rand(rng, 30), read]          # the grid runs on the LAST source of each side


def _grid_specs():
    starts, lens = (0, 1, 2, 3, 5, 17), (0, 1, 3, 4, 5, 63, 64, 65, 127)
    specs = []
    for rev in (False, True):
        # every (start, len) on the reference side against a fixed read segment, then on the read side
        for s in starts:
            for ln in lens:
                specs.append((1, 1, s, min(ln, 300 - s), 7, 60, rev))
                specs.append((1, 1, 9, 90, s, min(ln, 200 - s), rev))
        # both sides moving together, at different alignments of the two starts
        for k, s in enumerate(starts):
            specs.append((1, 1, s, 65, starts[-1 - k], 63, rev))
        # segments that end on the last byte of the last source of each side
        specs += [(1, 1, 300 - 66, 66, 200 - 61, 61, rev), (1, 1, 300 - 1, 1, 200 - 3, 3, rev), (1, 1, 233, WHOLE, 150, WHOLE, rev)]
        specs.append((1, 1, 0, WHOLE, 0, WHOLE, rev))
        # the first sources too (their last byte is followed by the next source), the same segment twice, overlapping segments
        specs += [(0, 0, 40 - 17, 17, 30 - 9, 9, rev), (0, 1, 3, WHOLE, 101, 33, rev)]
        specs += [(1, 1, 100, 80, 40, 70, rev), (1, 1, 100, 80, 40, 70, rev), (1, 1, 130, 80, 60, 70, rev), (1, 1, 101, 80, 41, 70, rev)]
    return specs


@pytest.mark.parametrize("device_strings", [1, 0])
def test_gather_grid(ctx, device_strings):
    """every start alignment x every length class of sw_gather_kernel's dword loop, forward and reversed, on both sides"""
    refs, reads = _grid_sources()
    specs = _grid_specs()
    ctx.set_option("device_strings", device_strings)
    b = ctx.upload_pairs(refs, reads, specs)
    try:
        assert b.n_pairs() == len(specs) == _capi.load().swmi_batch_n_pairs(b._h)
        assert b.spec(len(specs) - 1) == specs[-1] and b.spec(0) == specs[0]
        whole = specs.index((1, 1, 0, WHOLE, 0, WHOLE, True))
        assert b.spec(whole) == (1, 1, 0, 300, 0, 200, True)            # WHOLE resolved
        assert b.segments(whole) == (refs[1][::-1], reads[1][::-1])
        for tie in (0, 1):
            b.run(sw.make_params((5, -3, -4), None, tie))
            assert b.pipeline_mode() in (1, 2)
            check_linear(b, tie=tie)
        # the case of the caller's bytes came through: some alignment holds a lower-case base and the 0xE9
        seen = "".join(a[1][0] + a[1][1] for k in range(b.n_pairs()) if not b.n_alignments(k)[1] for a in b.alignments(k))
        assert any(c in seen for c in "acgt") and "\xe9" in seen
    finally:
        b.free()


# ---- 2: every linear pipeline ---------------------------------------------------------------------------------------------------
PIPELINES = [(1, 1, 0, 0, 0), (2, 1, 0, 0, 0), (0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (-1, 1, -1, -1, -1), (1, 1, 1, 0, 0), (1, 0, 1, 0, 0),
             (1, 1, 0, 1, 0), (1, 0, -1, 1, 0), (1, 1, 0, 0, 1), (1, 0, -1, -1, 1), (-1, 1, -1, -1, -1, 0)]
PIPELINE_IDS = ["mode1-winmax", "mode2-events", "mode0-field", "mode1-d2h-copy", "automatic", "mode1-split-traceback",
                "mode1-split-d2h-copy", "mode1-resident", "mode1-resident-d2h-copy", "mode1-tfused", "mode1-tfused-d2h-copy",
                "automatic-host-strings"]


def _pipeline_case():
    """two references (one periodic: its windows have many tied maxima) and six reads, a list of 70 pairs of mixed small
    lengths (between 64 and 256 pairs: the sampled pre-pass of the automatic traceback grain runs through the mapping)"""
    rng = random.Random(5)
    unit = u.rand(rng, 12)
    periodic = unit * 40                                     # 480
    plain = u.rand(rng, 700)
    refs = [plain, periodic]
    reads = [u.mutate(rng, plain[100:250]), u.mutate(rng, plain[400:480]), unit * 3, unit * 2 + u.rand(rng, 5),
             u.mutate(rng, plain[300:620]), u.rand(rng, 33)]
    specs = []
    for k in range(70):
        r, q = (1, rng.choice((2, 3))) if k % 3 == 0 else (0, rng.choice((0, 1, 4, 5)))
        n, m = len(refs[r]), len(reads[q])
        rs, qs = rng.randrange(0, n - 60), rng.randrange(0, max(1, m // 4))
        rl, ql = rng.randrange(40, min(400, n - rs) + 1), rng.randrange(1, m - qs + 1)
        specs.append((r, q, rs, rl, qs, ql, k % 5 == 0))
    return refs, reads, specs


@pytest.fixture(scope="module", params=PIPELINES, ids=PIPELINE_IDS)
def pipe_ctx(request):
    """the option grid of test_gap_paths_gpu.py: (mode, zero_copy, tb_split, resident, tfused[, device_strings])"""
    c = sw.Context(0)
    for name, value in zip(("mode", "zero_copy", "tb_split", "resident", "tfused"), request.param):
        c.set_option(name, value)
    c.set_option("device_strings", request.param[5] if len(request.param) > 5 else 1)
    yield c
    c.close()


def test_every_linear_pipeline(pipe_ctx):
    refs, reads, specs = _pipeline_case()
    b = pipe_ctx.upload_pairs(refs, reads, specs)
    try:
        for tie in (0, 1):
            b.run(sw.make_params((5, -3, -4), None, tie))
            assert b.pipeline_mode() in (0, 1, 2)
            check_linear(b, tie=tie)
        assert max(b.n_alignments(k)[0] for k in range(70) if not b.n_alignments(k)[1]) >= 4        # the tied maxima are there
    finally:
        b.free()


def test_whole_source_list_equals_the_cross_product(pipe_ctx):
    """(r, q) for all r, q: the same pairs in the same order as the cross-product batch of the same sources"""
    refs, reads, _ = _pipeline_case()
    nq = len(reads)
    b = pipe_ctx.upload_pairs(refs, reads, [(r, q) for r in range(len(refs)) for q in range(nq)])
    x = pipe_ctx.upload(refs, reads)
    try:
        p = sw.make_params((5, -3, -4))
        b.run(p)
        x.run(p)
        assert list(b.scores()) == list(x.scores())
        for pair in range(len(refs) * nq):
            assert b.n_alignments(pair) == x.n_alignments(pair), pair
            if not b.n_alignments(pair)[1]:
                assert b.alignments(pair, True) == x.alignments(pair, True), pair
    finally:
        b.free()
        x.free()


# ---- 3: the affine kernels ------------------------------------------------------------------------------------------------------
SC = (5, -3, -2, -6)
MATRIX = ("ACGT", [[4, -2, -1, -2], [-2, 4, -2, -1], [-1, -2, 4, -2], [-2, -1, -2, 4]])


def _small_case():
    rng = random.Random(23)
    ref = u.rand(rng, 900)
    refs = [ref, u.rand(rng, 310)]
    reads = [u.mutate(rng, ref[50:350], 0.05, 0.02), u.mutate(rng, ref[500:700], 0.05, 0.02), u.mutate(rng, refs[1][20:150]), u.rand(rng, 70)]
    specs = []
    for k in range(20):
        r = 0 if k % 4 else 1
        q = (2, 3)[k % 8 == 0] if r else rng.choice((0, 1, 3))
        n, m = len(refs[r]), len(reads[q])
        qs = rng.randrange(0, m // 3)
        ql = rng.randrange(1, m - qs + 1)
        rs = rng.randrange(0, n - 200)
        specs.append((r, q, rs, rng.randrange(1, min(330, n - rs) + 1), qs, ql, k % 3 == 0))
    specs[7] = specs[7][:3] + (0,) + specs[7][4:]               # an empty reference segment
    specs[11] = specs[11][:5] + (0,) + specs[11][6:]            # an empty read segment
    return refs, reads, specs


def _set_affine(ctx, sc, mode, extend=0, matrix=None, **options):
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("align_mode", mode)
    ctx.set_option("extend", extend)
    for name, value in options.items():
        ctx.set_option(name, value)
    if matrix is None:
        ctx.clear_score_matrix()
    else:
        ctx.set_score_matrix(*matrix)


@pytest.mark.parametrize("matrix", [None, MATRIX], ids=["scores", "matrix"])
@pytest.mark.parametrize("mode,extend", [(0, 0), (1, 0), (2, 0), (2, 1)], ids=["local", "fit", "global", "extend"])
def test_affine_modes(ctx, mode, extend, matrix):
    refs, reads, specs = _small_case()
    _set_affine(ctx, SC, mode, extend, matrix)
    b = ctx.upload_pairs(refs, reads, specs)
    try:
        for tie in (0, 1):
            b.run(sw.make_params(SC[:3], None, tie))
            assert b.pipeline_mode() == 3
            for k in range(len(specs)):
                ref, read = b.segments(k)
                want = gr.align_numpy(ref, read, SC, mode, 0, bool(extend), tie, matrix, cells=True)
                u.check_pair(b, k, want, mode, (k, specs[k], tie))
                assert b.rows_swept(k) == len(read) and b.band_window(k, 0) == (1, len(ref))
    finally:
        b.free()


def _long_case():
    """read segments of 1025 and 2100 bases cut from a 2200-base source at an odd start, against windows of a 2400-base
    reference; the read follows the reference with a few indels.  (Every window has at least 1985 columns: a banded run checks
    the last strip of the batch's longest read against its shortest reference.)"""
    rng = random.Random(41)
    ref = u.rand(rng, 2400)
    read = (u.rand(rng, 37) + u.mutate(rng, ref[101:2300], 0.03, 0.002))[:2200].ljust(2200, "A")
    # (read base 37 lies on reference base 101; the reversed pair starts on read base 2162 and reference base 2226)
    specs = [(0, 0, 101, 2000, 37, 1025, False), (0, 0, 101, 2160, 37, 2100, False), (0, 0, 67, 2160, 63, 2100, True)]
    return [ref], [read], specs


LONG_RUNS = {
    "plain-global": dict(mode=GLOBAL),
    "plain-extend": dict(mode=GLOBAL, extend=1),
    "band": dict(mode=GLOBAL, extend=1, band=64),
    "xdrop": dict(mode=GLOBAL, extend=1, xdrop=60),
    "band-adapt": dict(mode=GLOBAL, extend=1, band=64, band_adapt=1),
    "two-piece": dict(mode=GLOBAL, extend=1, two=(2, -4, -2, -4, -1, -24)),
}


@pytest.mark.parametrize("name", list(LONG_RUNS))
def test_long_read_segments(ctx, name):
    o = LONG_RUNS[name]
    refs, reads, specs = _long_case()
    mode, extend, w, X, adapt, two = o["mode"], o.get("extend", 0), o.get("band", 0), o.get("xdrop", 0), o.get("band_adapt", 0), o.get("two")
    sc = two if two else (2, -4, -2, -4)
    _set_affine(ctx, sc, mode, extend, None, long_reads=1, band=w, xdrop=X, band_adapt=adapt, gap_open2=sc[5] if two else 0,
                gap2=sc[4] if two else 0)
    if name == "xdrop":                        # a reference that ends 600 rows before the read does: the sweep stops behind strip 1
        specs = specs + [(0, 0, 101, 1500, 37, 2100, False)]
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(sc[:3]))
    try:
        assert b.pipeline_mode() == 3
        for k in range(len(specs)):
            ref, read = b.segments(k)
            m, n, what = len(read), len(ref), (name, k, specs[k])
            assert m in (1025, 2100)
            if two:
                want = tr.align_numpy(ref, read, sc, GLOBAL, w, bool(extend), 0, cells=True)
            elif adapt:
                want = ar.align(ref, read, sc, w, X, 0)
                assert [b.band_window(k, s) for s in range(len(want[3]))] == [tuple(x) for x in want[3]], what
            elif X:
                want = xr.align(ref, read, sc, X, w, 0)
                assert b.rows_swept(k) == want[3], what
                assert want[3] == (2048 if k == 3 else m), what          # (the case is what it is meant to be)
            else:
                want = gr.align_numpy(ref, read, sc, mode, w, bool(extend), 0, None, cells=True)
            u.check_pair(b, k, want[:3], GLOBAL, what)
            if not X:
                assert b.rows_swept(k) == m, what
            if w and not adapt:
                assert [b.band_window(k, s) for s in range((m + 1023) // 1024)] == [tuple(x) for x in gr.windows(m, n, w)], what
    finally:
        b.free()


def test_seed_extension_as_a_mapper_issues_it(ctx):
    """a 20-base seed in the middle of a 150-base read, at a known place of a 5,000-base reference: the right extension
    forward, the left extension with SWMI_SPEC_REVERSE, both from the resident sources; to_source maps the two end cells back"""
    rng = random.Random(77)
    ref = u.rand(rng, 5000)
    at, seed_q, seed_len = 3127, 62, 20                          # read base 62 lies on reference base 3127 + 62
    read = list(ref[at:at + 150])
    read[10] = "A" if read[10] != "A" else "C"                   # one substitution on either side of the seed
    read[120] = "G" if read[120] != "G" else "T"
    read = "".join(read).lower()                                 # (the strings carry the read's case)
    r0, q0 = at + seed_q, seed_q                                 # the seed's first base, in both sources
    r1, q1 = r0 + seed_len, q0 + seed_len                        # ... and the first base behind it
    specs = [(0, 0, r1, 150, q1, 150 - q1, False),               # right: forward from the seed's end
             (0, 0, r0 - 100, 100, 0, q0, True)]                 # left: the bases before the seed, both reversed
    _set_affine(ctx, SC, GLOBAL, 1)
    b = ctx.upload_pairs([ref], [read], specs).run(sw.make_params(SC[:3]))
    try:
        assert b.segments(0) == (ref[r1:r1 + 150], read[q1:]) and b.segments(1) == (ref[r0 - 100:r0][::-1], read[:q0][::-1])
        for k in (0, 1):
            seg_ref, seg_read = b.segments(k)
            want = gr.align_numpy(seg_ref, seg_read, SC, GLOBAL, 0, True, 0, None, cells=True)
            u.check_pair(b, k, want, GLOBAL, k)
            assert len(want[1]) == 1
        (_, _, (ei, ej)), = b.alignments(0, True)
        assert (ei, ej) == (150 - q1, 150 - q1) and b.to_source(0, ei, ej) == (149, at + 149)          # the read's last base
        (_, _, (ei, ej)), = b.alignments(1, True)
        assert (ei, ej) == (q0, q0) and b.to_source(1, ei, ej) == (0, at)                              # ... and its first
        assert b.to_source(1, 1, 1) == (q0 - 1, r0 - 1) and b.to_source(0, 1, 1) == (q1, r1)
    finally:
        b.free()


# ---- 4: runtime paths -----------------------------------------------------------------------------------------------------------
def test_chunked_under_a_workspace_cap(ctx):
    rng = random.Random(3)
    ref = u.rand(rng, 6000)
    reads = [u.mutate(rng, ref[k * 700:k * 700 + 600]) for k in range(6)]
    specs = [(0, q, q * 700 + d, 2000 - d, 3 * d, 590 - 3 * d, bool(d & 1)) for q in range(6) for d in range(3)]
    ctx.set_option("max_workspace_bytes", 1 << 20)
    b = ctx.upload_pairs([ref], reads, specs).run()
    try:
        assert b.timing().fill_launches >= 3
        check_linear(b)
    finally:
        b.free()


def _tie_heavy():
    rng = random.Random(9)
    unit = u.rand(rng, 9)
    ref, read = u.rand(rng, 50) + unit * 30 + u.rand(rng, 50), unit * 2
    return [ref], [read], [(0, 0, 45 + 3 * k, 200, 0, WHOLE, bool(k & 1)) for k in range(8)] + [(0, 0, 0, 40, 0, 5, False)]


def test_cell_cap_and_the_exact_size_rerun(ctx):
    refs, reads, specs = _tie_heavy()
    ctx.set_option("cell_cap", 1)
    b = ctx.upload_pairs(refs, reads, specs).run()
    try:
        assert b.timing().rerun_pairs > 0
        check_linear(b)
    finally:
        b.free()


def test_async_run_and_the_cached_plan(ctx):
    refs, reads, specs = _tie_heavy()
    b = ctx.upload_pairs(refs, reads, specs)
    try:
        b.run_async().wait()
        check_linear(b)
        b.run()                                                  # the same batch again: the plan is the cached one
        check_linear(b)
        b.run(sw.make_params((5, -3, -4), None, 1))
        check_linear(b, tie=1)
    finally:
        b.free()


def test_set_pairs(ctx):
    refs, reads, specs = _tie_heavy()
    rng = random.Random(13)
    refs, reads = refs + [u.rand(rng, 333)], reads + [u.mutate(rng, refs[0][20:140])]
    b = ctx.upload_pairs(refs, reads, specs).run()
    try:
        check_linear(b)
        # the same lengths at other offsets (the schedule's sizes stay, the segments do not), reversal flipped
        moved = [(r, q, rs + 2, rl, qs, ql, not rev) for r, q, rs, rl, qs, ql, rev in specs]
        assert b.set_pairs(moved).n_pairs() == len(specs)
        with pytest.raises(sw.SwmiError):
            b.score(0)                                           # the old results are gone
        check_linear(b.run())
        # another count, other sources, a list that needs a larger reversed area
        more = [(1, 1, k, 300, 0, WHOLE, True) for k in range(30)] + [(0, 1, 3, 170, 5, 90, False), (1, 0)]
        assert b.set_pairs(more).n_pairs() == 32
        check_linear(b.run())
        assert b.set_pairs([(0, 1, 0, 150, 0, WHOLE)]).n_pairs() == 1
        check_linear(b.run())
        assert b.spec(0) == (0, 1, 0, 150, 0, len(reads[1]), False)
    finally:
        b.free()


def test_an_empty_list(ctx):
    b = ctx.upload_pairs(["ACGT"], ["ACG"], []).run()
    try:
        assert b.n_pairs() == 0 and len(b.scores()) == 0 and b.materialise_all() == (0, 0)
        with pytest.raises(sw.SwmiError):
            b.score(0)
        check_linear(b.set_pairs([(0, 0)]).run())
        assert b.score(0) == 15
        assert b.set_pairs([]).run().n_pairs() == 0
    finally:
        b.free()
    b = ctx.upload_pairs([], [], []).run()
    assert b.n_pairs() == 0
    b.free()


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------
def _spec_array(rows):
    arr = (_capi.PairSpec * len(rows))()
    for k, row in enumerate(rows):
        arr[k] = _capi.PairSpec(*row)
    return arr


BAD = {                          # the third pair of a list of four: (ref, read, ref_start, ref_len, read_start, read_len, flags, reserved)
    "reference index": (2, 0, 0, 4, 0, 4, 0, 0),
    "read index": (0, 1, 0, 4, 0, 4, 0, 0),
    "reference range": (0, 0, 30, 11, 0, 4, 0, 0),
    "reference start": (1, 0, 22, WHOLE, 0, 4, 0, 0),
    "reference range wraps": (0, 0, 0xFFFFFFF0, 0x20, 0, 4, 0, 0),
    "read range": (0, 0, 0, 4, 25, 6, 0, 0),
    "flag bit": (0, 0, 0, 4, 0, 4, 2, 0),
    "reserved": (0, 0, 0, 4, 0, 4, 1, 7),
}


def test_refusals(ctx):
    lib = _capi.load()
    refs, reads = ["ACGTACGTAC" * 4, "TTGACCA" * 3], ["ACGTTGCAAC" * 3]          # 40 and 21 bases; 30
    good = [(0, 0, 2, 30, 1, 25, False), (1, 0, 0, WHOLE, 3, 20, True)]
    b = ctx.upload_pairs(refs, reads, good).run()
    try:
        check_linear(b)
        rb, ro = _capi.pack(refs)
        qb, qo = _capi.pack(reads)
        ok = (0, 0, 0, 4, 0, 4, 0, 0)
        for name, bad in BAD.items():
            arr = _spec_array([ok, ok, bad, ok])
            h = _capi.C.c_void_p()
            assert lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 2, qb, qo, 1, arr, 4, _capi.C.byref(h)) == ERR_INVALID, name
            assert b"pair 2" in lib.swmi_last_error() and not h.value, (name, lib.swmi_last_error())
            assert lib.swmi_batch_set_pairs(ctx._h, b._h, arr, 4) == ERR_INVALID, name
            assert b"pair 2" in lib.swmi_last_error(), (name, lib.swmi_last_error())
        h = _capi.C.c_void_p()
        assert lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 2, qb, qo, 1, None, 3, _capi.C.byref(h)) == ERR_INVALID
        assert b"pair 0" in lib.swmi_last_error()
        assert lib.swmi_batch_set_pairs(ctx._h, b._h, None, 3) == ERR_INVALID and b"pair 0" in lib.swmi_last_error()
        one = _spec_array([ok])
        assert lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 2, qb, qo, 1, one, 1 << 32, _capi.C.byref(h)) == ERR_UNSUPPORTED
        assert lib.swmi_batch_set_pairs(ctx._h, b._h, one, 1 << 32) == ERR_UNSUPPORTED
        # the batch is as it was: the old results are readable, and it still runs its old list
        assert b.n_pairs() == 2 and b.spec(1) == (1, 0, 0, 21, 3, 20, True)
        check_linear(b)
        check_linear(b.run())
        # the MapRef views need the cross product
        for call in (lambda: b.ref_total(0), b.ref_totals, lambda: b.ref_match_sites(0), b.ref_sites_packed):
            with pytest.raises(sw.SwmiError) as e:
                call()
            assert e.value.code == ERR_UNSUPPORTED, str(e.value)
        assert len(b.pair_results()[0]) == 2 and b.materialise_all()[0] == sum(b.n_alignments(k)[0] for k in range(2))
    finally:
        b.free()
    x = ctx.upload(refs, reads)
    try:
        assert lib.swmi_batch_set_pairs(ctx._h, x._h, _spec_array([ok]), 1) == ERR_INVALID
        assert lib.swmi_batch_pair_spec(x._h, 0, _capi.C.byref(_capi.PairSpec())) == ERR_INVALID
        x.run()
        assert x.ref_total(0) == x.score(0)                      # ... and a cross-product batch is what it was
    finally:
        x.free()
