"""End-to-end alignment modes on the GPU (swmi_affine.hip, swmi_set_option "align_mode": 1 fit, 2 global).

Every pair of every launch is checked against the numpy restatement of the contract in tests/gotoh_reference.py: score, number
of alignments, each `beginning` and both strings.  The bounds of swmi.h / DESIGN.md section 8d are pinned from both sides
against the scalar restatement, which computes in unbounded Python ints."""
import json
import os
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as swmatrix

import affine_gpu_util as u
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)
MODES = [sw.ALIGN_FIT, sw.ALIGN_GLOBAL]


def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "ends_kat.json")) as f:
        return json.load(f)["kats"]


def _matrix(name):
    m = getattr(swmatrix, name)
    alpha = m.alphabet if isinstance(m.alphabet, str) else bytes(m.alphabet).decode("latin-1")
    return m, (alpha, [list(map(int, r)) for r in m.scores])


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


# 1 -- the known answers
def test_ends_kats(ctx):
    for k in _kats():
        mat = None
        if k["matrix"]:
            m, mat = _matrix(k["matrix"])
            ctx.set_score_matrix(m)
        else:
            ctx.clear_score_matrix()
        b = u.run(ctx, [k["ref"]], [k["read"]], tuple(k["scores"]), k["tie_mode"], k["align_mode"], mode3=False)
        assert b.pipeline_mode() == 3
        assert b.score(0) == k["score"], k["name"]
        assert b.n_alignments(0) == (len(k["alignments"]), 0), k["name"]
        assert [[x[0], x[1][0], x[1][1]] for x in b.alignments(0)] == k["alignments"], k["name"]
        assert (b.score(0), b.alignments(0)) == gr.align_numpy(k["ref"], k["read"], tuple(k["scores"]), k["align_mode"], tie_mode=k["tie_mode"], matrix=mat)
        b.free()


# 2 -- every R class and both sweep kernels; references shorter and longer than the read, and of several traceback tiles
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tie", [0, 1])
def test_ends_read_lengths(ctx, mode, tie):
    rng = random.Random(300 + 2 * mode + tie)
    big = u.rand(rng, 6000)
    reads = [u.rand(rng, m) for m in (1, 63, 64, 65, 255, 256, 257, 1023)] + [big[2000:2500] + big[2530:3054]]     # (the last: 1024)
    assert [len(r) for r in reads][-1] == 1024
    refs = [u.rand(rng, 40), u.rand(rng, 300), big[1500:3600], big]
    sc = (5, -3, -2, -6) if mode == sw.ALIGN_FIT else (2, -3, -1, -4)
    b = u.run(ctx, refs, reads, sc, tie, mode, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, mode, tie=tie), mode)
    b.free()


# 3 -- a random sweep over small pairs, small alphabets (many tied end cells), gap and gap_open down to 0
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tie", [0, 1])
def test_ends_random_pairs(ctx, mode, tie):
    rng = random.Random(400 + 2 * mode + tie)
    for sc in ((1, -1, -1, 0), (2, -3, -1, -3), (3, 1, 0, -2), (0, -2, -2, 0), (5, -3, 0, 0)):
        alpha = rng.choice(["AC", "A", "ACGTacgtN\xe9"])
        refs = [u.rand(rng, rng.randint(1, 90), alpha) for _ in range(12)] + ["", "AC" * 150]
        reads = [u.rand(rng, rng.randint(1, 70), alpha) for _ in range(10)] + ["", "CA", "ACACAC"]
        b = u.run(ctx, refs, reads, sc, tie, mode, mode3=False)
        u.check(b, refs, reads, u.expect(refs, reads, sc, mode, tie=tie), mode)
        b.free()


# 4 -- more tied end cells than cell_cap: the exact-size re-run
@pytest.mark.parametrize("tie", [0, 1])
def test_ends_cell_cap_rerun(ctx, tie):
    ctx.set_option("cell_cap", 4)
    refs = ["ACGTTGCA" * 40, "AC" * 100, "GATTACA"]
    reads = ["ACGTTGCAAC", "CACA", "ACGTTGCAACGTTGCA"]
    sc = (2, -3, -1, -2)
    b = u.run(ctx, refs, reads, sc, tie, sw.ALIGN_FIT, mode3=False)
    exp = u.expect(refs, reads, sc, sw.ALIGN_FIT, tie=tie)
    u.check(b, refs, reads, exp, sw.ALIGN_FIT)
    assert max(len(v[1]) for v in exp.values()) > 4 and b.timing().rerun_pairs >= 1
    b.free()


# 5 -- with a matrix, with gap_open = 0, with affine = 1
@pytest.mark.parametrize("mode", MODES)
def test_ends_matrix_and_options_that_select_kernels(ctx, mode):
    rng = random.Random(500 + mode)
    m, mat = _matrix("BLOSUM62")
    prot = mat[0][:20]
    refs = [u.rand(rng, 400, prot), u.rand(rng, 90, prot + "z"), u.rand(rng, 1200, prot)]
    reads = [refs[0][100:160], u.rand(rng, 300, prot), u.rand(rng, 70, prot + "z"), refs[2][50:400] + refs[2][420:700]]
    ctx.set_score_matrix(m)
    for tie in (0, 1):
        sc = (1, -1, -1, -10)
        b = u.run(ctx, refs, reads, sc, tie, mode, mode3=False)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, u.expect(refs, reads, sc, mode, tie=tie, matrix=mat), mode)
        b.free()
    ctx.clear_score_matrix()
    refs = [u.rand(rng, 500), u.rand(rng, 100)]
    reads = [u.rand(rng, 150), refs[0][40:300]]
    sc = (5, -3, -4, 0)                                           # gap_open = 0: still the mode-3 kernels
    b = u.run(ctx, refs, reads, sc, 0, mode, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, mode), mode)
    b.free()
    ctx.set_option("affine", 1)
    b = u.run(ctx, refs, reads, sc, 1, mode, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, mode, tie=1), mode)
    b.free()


# 6 -- the options that apply to mode-3 runs give the same results
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("opt", [("device_strings", 0), ("zero_copy", 0), ("scores_only", 1), ("cell_cap", 2),
                                 ("arena_words_per_pair", 1), ("max_workspace_bytes", 1 << 20)])
def test_ends_options(ctx, mode, opt):
    rng = random.Random(600)
    refs = ["ACGTTGCA" * 40, u.rand(rng, 900), "GATTACA" * 30 + u.rand(rng, 200), u.rand(rng, 64), u.rand(rng, 2500)]
    reads = ["ACGTTGCAAC", u.rand(rng, 150), "GATTACAGATTACA", u.rand(rng, 300), refs[4][1000:1400]]
    sc = (5, -3, -2, -6)
    ctx.set_option(*opt)
    b = u.run(ctx, refs, reads, sc, 0, mode, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, mode), mode, alignments=opt[0] != "scores_only")
    if opt[0] == "scores_only":
        assert [b.ref_total(r) for r in range(len(refs))] == \
            [sum(gr.align_numpy(rf, rd, sc, mode)[0] for rd in reads) for rf in refs]
    if opt[0] == "cell_cap" and mode == sw.ALIGN_FIT:
        assert b.timing().rerun_pairs >= 1
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    b.free()


# 7 -- run_async takes the mode set when it was asked for; the mirror's keyword
def test_ends_async_and_mirror(ctx):
    rng = random.Random(700)
    refs = [u.rand(rng, 500) for _ in range(3)]
    reads = [u.rand(rng, 120) for _ in range(4)]
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("align_mode", sw.ALIGN_FIT)
    ctx.set_option("debug_async_delay_us", 200000)
    b = ctx.upload(refs, reads).run_async(sw.make_params(sc[:3]))
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)                 # while the run has not started yet
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, sw.ALIGN_FIT), sw.ALIGN_FIT)
    b.free()
    for mode in MODES:
        got = sw.SmithWaterman.OptAlignments(ctx, align_mode=mode).call([refs[0], reads[0]], list(sc))
        assert got == gr.align_numpy(refs[0], reads[0], sc, mode)
        got = sw.DistributedSW.OptAlignments(ctx, align_mode=mode).call([refs[0], reads[0]], list(sc))
        assert got == gr.align_numpy(refs[0], reads[0], sc, mode, tie_mode=1)
        assert ctx.options["align_mode"] == sw.ALIGN_LOCAL and ctx.options["gap_open"] == sc[3]
    total, (ref, sites) = sw.Distribution.MapRef(ctx, align_mode=sw.ALIGN_FIT).call(((">r", refs[1]), reads, (list(sc), ["a", "i", "d", "-"])))
    exp = [gr.align_numpy(refs[1], q, sc, sw.ALIGN_FIT) for q in reads]
    assert total == sum(e[0] for e in exp)
    assert sites == sorted([a for e in exp for a in e[1]], key=lambda t: t[0])


# 8 -- a stream from a FASTA file (the slots copy the mode at open), records and scores only
@pytest.mark.parametrize("mode", MODES)
def test_ends_stream_from_fasta(ctx, tmp_path, mode):
    rng = random.Random(800 + mode)
    refs = [u.rand(rng, rng.randint(200, 800)) for _ in range(40)]
    reads = [u.rand(rng, 150), refs[17][100:250], "W" * 300]        # (the last: no base of it is in any reference)
    path = tmp_path / "refs.fa"
    with open(path, "w") as f:
        for k, r in enumerate(refs):
            f.write(">gi|ref%d\n" % k)
            for x in range(0, len(r), 70):
                f.write(r[x:x + 70] + "\n")
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    ctx.set_option("align_mode", mode)
    exp = [[gr.align_numpy(r, q, sc, mode) for q in reads] for r in refs]
    want = [sum(e[0] for e in row) for row in exp]
    assert min(want) < 0                                          # negative totals come through untouched
    st = ctx.stream(reads, sw.make_params(sc[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)                 # (the stream keeps the mode it was opened with)
    st.push_file(path).finish()
    assert [int(t) for t in st.totals()] == want
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            sites = sorted([a for e in exp[first + r] for a in e[1]], key=lambda t: t[0])
            assert c.ref_match_sites(r) == sites, first + r
    st.close()
    ctx.set_option("align_mode", mode)
    ctx.set_option("scores_only", 1)
    ctx.set_option("stream_keep_records", 0)
    st = ctx.stream(reads, sw.make_params(sc[:3]), slots=2, chunk_bytes=1 << 16)
    st.push_file(path).finish()
    assert [int(t) for t in st.totals()] == want
    st.close()


# 9 -- one batch under one mode after another (the prep cache keys on the mode); back to 0 is today's pipeline
def test_ends_rerun_under_another_mode(ctx):
    from oracle import sw_oracle as orc
    rng = random.Random(900)
    refs = [u.rand(rng, 400) for _ in range(3)]
    reads = [u.rand(rng, 100) for _ in range(3)] + [refs[1][30:200]]
    sc = (5, -3, -4, -6)
    b = ctx.upload(refs, reads)
    p = sw.make_params(sc[:3])
    ctx.set_option("gap_open", sc[3])
    for mode in (sw.ALIGN_FIT, sw.ALIGN_GLOBAL, sw.ALIGN_FIT, sw.ALIGN_LOCAL, sw.ALIGN_GLOBAL):
        ctx.set_option("align_mode", mode)
        b.run(p)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, u.expect(refs, reads, sc, mode), mode)
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)
    ctx.set_option("gap_open", 0)
    b.run(p)
    assert b.pipeline_mode() == 1                                # today's pipeline again
    for r, ref in enumerate(refs):
        for q, read in enumerate(reads):
            es, ea = orc.opt_alignments((ref, read), sc[:3], b"aid-", 0)
            assert b.score(r * len(reads) + q) == es
            if es:
                assert b.alignments(r * len(reads) + q) == [(a[0], tuple(a[1])) for a in ea]
    b.free()


# 10 -- an invalid value leaves the context as it was
def test_ends_invalid_value(ctx):
    ctx.set_option("align_mode", sw.ALIGN_FIT)
    for bad in (3, -1, 1 << 40):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("align_mode", bad)
        assert e.value.code == ERR_INVALID
    b = u.run(ctx, ["CGTCCAGACT"], ["AGGTCGAC"], (2, -3, -1, -3), mode3=False)       # (align_mode left as it is)
    assert (b.score(0), b.alignments(0)) == (2, [(2, ("__GTCCAGAC", "AGGTC__GAC"))])      # still fit
    b.free()


# 11 -- both sides of every bound, against the restatement in unbounded ints
def _scalar(ref, read, sc, mode):
    return gr.align_scalar(ref, read, sc, mode)


def test_ends_bounds_scores_and_read_length(ctx):
    rng = random.Random(1100)
    L = 1 << 20
    # inside: every score at its bound, the longest read; fit values reach gap_open + 1024 * gap - (gap_open + 2 * gap)
    read = u.rand(rng, 1024, "AC")
    ref = read[:500] + u.rand(rng, 40, "AC") + read[560:]
    for sc in ((L, -L, -L, -L), (L, L, -L, -L), (-L, -L, -L, 0)):
        for mode, rf in ((sw.ALIGN_FIT, ref), (sw.ALIGN_FIT, "CA"), (sw.ALIGN_GLOBAL, ref[:950])):
            b = u.run(ctx, [rf], [read], sc, 0, mode, mode3=False)
            assert (b.score(0), b.alignments(0)) == _scalar(rf, read, sc, mode), (sc, mode, len(rf))
            b.free()
    # outside: one more in any score, one more read base, a positive gap
    b = ctx.upload(["ACGT" * 10], ["ACG"])
    ctx.set_option("align_mode", sw.ALIGN_FIT)
    ctx.set_option("gap_open", -6)
    for bad in ((L + 1, -3, -4), (5, -(L + 1), -4), (5, -3, -(L + 1)), (5, -3, 1)):
        with pytest.raises(_capi.SwmiError) as e:
            b.run(sw.make_params(bad))
        assert e.value.code == ERR_UNSUPPORTED
    ctx.set_option("gap_open", -(L + 1))
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()
    ctx.set_option("gap_open", -6)
    b = ctx.upload(["ACGT" * 10], ["A" * 1025])
    for mode in MODES:
        ctx.set_option("align_mode", mode)
        with pytest.raises(_capi.SwmiError) as e:
            b.run(sw.make_params((5, -3, -4)))
        assert e.value.code == ERR_UNSUPPORTED
    b.free()


@pytest.mark.parametrize("o,m", [(0, 64), (-(1 << 20), 64), (-7, 100)])
def test_ends_bound_global_int32(ctx, o, m):
    """global mode: 3 * |gap_open| + (64 * ceil(m / 64) + n) * |gap| <= 2^31 -- the last n inside, the first outside"""
    rng = random.Random(1200 + m)
    e = -(1 << 20)
    rows = 64 * ((m + 63) // 64)
    n_ok = ((1 << 31) - 3 * -o) // -e - rows
    assert 3 * -o + (rows + n_ok) * -e <= 1 << 31 < 3 * -o + (rows + n_ok + 1) * -e
    read = u.rand(rng, m, "AC")
    ref = u.rand(rng, n_ok + 1, "AC")
    sc = (1 << 20, -3, e, o)
    b = u.run(ctx, [ref[:n_ok]], [read], sc, 0, sw.ALIGN_GLOBAL, mode3=False)
    assert (b.score(0), b.alignments(0)) == _scalar(ref[:n_ok], read, sc, sw.ALIGN_GLOBAL)
    b.free()
    ctx.set_option("align_mode", sw.ALIGN_GLOBAL)
    b = ctx.upload([ref], [read])
    with pytest.raises(_capi.SwmiError) as err:
        b.run(sw.make_params(sc[:3]))
    assert err.value.code == ERR_UNSUPPORTED
    ctx.set_option("align_mode", sw.ALIGN_FIT)                   # the same pair is inside the fit mode's bounds
    b.run(sw.make_params(sc[:3]))
    assert (b.score(0), b.alignments(0)) == _scalar(ref, read, sc, sw.ALIGN_FIT)
    b.free()


def test_ends_bound_path_lds(ctx):
    """a path has up to m + n moves, packed 16 per dword next to the 4096-dword tile and 128 dwords of scratch in 160 KB of LDS:
    (m + n + 15) // 16 <= 36735, so m + n = 587760 is the last pair inside"""
    limit = (160 * 1024 // 4 - 4096 - 128 - 1) * 16
    assert limit == 587760
    rng = random.Random(1300)
    ref = u.rand(rng, limit, "ACGT")
    sc = (2, -3, -1, -2)
    for mode in MODES:
        b = u.run(ctx, [ref[:limit - 1]], ["G"], sc, 0, mode, mode3=False)     # m + n = limit
        assert (b.score(0), b.alignments(0)) == _scalar(ref[:limit - 1], "G", sc, mode)
        b.free()
        ctx.set_option("align_mode", mode)
        b = ctx.upload([ref], ["G"])                              # m + n = limit + 1
        with pytest.raises(_capi.SwmiError) as err:
            b.run(sw.make_params(sc[:3]))
        assert err.value.code == ERR_UNSUPPORTED
        b.free()
    ctx.set_option("align_mode", sw.ALIGN_LOCAL)                 # a local path stays positive: the same pair runs
    b = ctx.upload([ref], ["G"]).run(sw.make_params(sc[:3]))
    assert b.score(0) == 2
    b.free()


# 12 -- the JNI shim's entry point from plain C99 (tests/c/shim_ends.c)
def test_c99_shim_sets_align_mode(tmp_path):
    out = u.run_shim(tmp_path, "shim_ends")
    assert out.splitlines() == ["2 1 2:__GTCCAGAC/AGGTC__GAC mode 3", "-4 1 1:_CGTCCAGACT/AGGTC__GAC_ mode 3",
                                       "7 1 2:GTCCAGAC/GTC__GAC mode 3"]
