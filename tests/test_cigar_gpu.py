"""Option "cigar" on the GPU (swmi_emit.h: SwmiCigar at the emit site of aff_traceback): every alignment's
CIGAR and nm against tests/cigar_reference.py applied to the strings the reference aligners return, and -- because the host then
expands the CIGAR where it expanded the packed ops -- every other accessor against the same aligners through affine_gpu_util.
All comparisons are exact.  set_option("cigar", ...) is what fails without the feature.

The cases are chosen where the emitter can go wrong: the 64-op iteration and its seams (a run boundary on lane 0, a carried run
closed by the first boundary lane, a last run of one column, more than 64 runs), gap runs at either end and longer than an
iteration, the equality rule, every traceback family, and the host machinery around a payload whose size the record alone does
not tell."""
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi

import adapt_reference as ar
import affine_gpu_util as u
import cigar_reference as cr
import gotoh_reference as gr
import twopiece_reference as tr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -5, -6       # swmi_status (include/swmi.h)
LOCAL, FIT, GLOBAL = sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL
SC = (5, -4, -3, -5)
DIAG = (5, -1, -20, -20)                                   # substitutions stay on the diagonal
CHEAP = (5, -4, -1, -2)                                    # long gaps are cheap


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def check_cigars(b, n_pairs, want_of, c, what=None):
    """Batch.cigar of every alignment of every pair against the contract applied to the expected strings; want_of(pair) =
    (score, alignments, cells)"""
    for pair in range(n_pairs):
        score, alns, cells = want_of(pair)[:3]
        n, flags = b.n_alignments(pair)
        assert n == len(alns), (what, pair)
        if flags & sw.PAIR_DEGENERATE:
            continue                                        # (test_degenerate_and_empty looks at these)
        got = b.cigars(pair)
        for k, ((begin, (ra, qa)), cell) in enumerate(zip(alns, cells)):
            ent, nm = cr.cigar(ra, qa, c)
            assert got[k] == (begin, cell[0], cell[1], ent, nm), (what, pair, k, sw.cigar_string(got[k][3]), sw.cigar_string(ent))
        with pytest.raises(_capi.SwmiError) as e:
            b.cigar(pair, n)
        assert e.value.code == ERR_RANGE


def both(ctx, refs, reads, sc, exp, mode=LOCAL, tie=0, w=None, extend=None, matrix=None, map_ref=True, **options):
    """the batch under cigar = 1 and 2: every accessor through affine_gpu_util.check, every CIGAR, and the pipeline"""
    exp = {key: v[:3] for key, v in exp.items()}
    for c in (1, 2):
        b = u.run(ctx, refs, reads, sc, tie, mode, w, extend, matrix, cigar=c, **options)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, exp, mode, map_ref=map_ref)
        check_cigars(b, len(refs) * len(reads), lambda p: exp[(p // len(reads), p % len(reads))], c, (c, tie, mode))
        b.free()


def cigars_of(want, c=2):
    return [cr.cigar(ra, qa, c)[0] for _, (ra, qa) in want[1]]


def sub(s, col):
    """s with the base of column `col` (1-based) substituted"""
    return s[:col - 1] + {"A": "C", "C": "G", "G": "T", "T": "A"}[s[col - 1]] + s[col:]


# ---- the 64-op iteration ---------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def test_identical_pairs_span_the_iteration_seams(ctx):
    """one '=' run over 0 to 3 seams on the diagonal of the batch; off it, a prefix against a longer sequence: '=' then one gap run"""
    base = u.rand(random.Random(9101), 200)
    seqs = [base[:n] for n in LENGTHS]
    exp = u.expect(seqs, seqs, SC, GLOBAL, cells=True)
    for x, n in enumerate(LENGTHS):
        assert cigars_of(exp[(x, x)]) == [[(n, "=")]]
    assert cigars_of(exp[(8, 3)]) == [[(64, "="), (136, "D")]] and cigars_of(exp[(3, 8)]) == [[(64, "="), (136, "I")]]
    both(ctx, seqs, seqs, SC, exp, GLOBAL)


@pytest.mark.parametrize("n", [65, 128, 129, 200])
def test_one_substitution_on_a_seam(ctx, n):
    """columns 64, 65 and the last, and -- the walk counts from the end -- the columns of ops 63 and 64: a boundary on the first lane
    of an iteration, a carried run closed by the first boundary lane, a one-column first or last run"""
    ref = u.rand(random.Random(9102 + n), n)
    cols = sorted({64, 65, n, n - 64, n - 63, 1})
    reads = [sub(ref, col) for col in cols]
    exp = u.expect([ref], reads, DIAG, GLOBAL, cells=True)
    for q, col in enumerate(cols):
        runs = [(col - 1, "="), (1, "X"), (n - col, "=")]
        assert cigars_of(exp[(0, q)]) == [[r for r in runs if r[0]]], col
    both(ctx, [ref], reads, DIAG, exp, GLOBAL)


def alternating_case():
    ref = u.rand(random.Random(9103), 130)
    read = "".join(sub(ref, k + 1)[k] if k % 2 else ref[k] for k in range(130))
    want = gr.align_numpy(ref, read, DIAG, GLOBAL, cells=True)
    assert want[1] == [(1, (ref, read))]                    # the gapless path
    assert cigars_of(want) == [[(1, "=X"[k % 2]) for k in range(130)]] and cigars_of(want, 1) == [[(130, "M")]]
    return ref, read, want


def test_alternating_columns_more_runs_than_lanes(ctx):
    ref, read, want = alternating_case()
    both(ctx, [ref], [read], DIAG, {(0, 0): want}, GLOBAL)


def test_gap_runs_at_either_end(ctx):
    """70 extra reference bases in front (the row-0 deletion loop of the walk), behind, 70 extra read bases in front (the column-0
    insertions), and an extend run whose maximum cell leaves a tail of both sequences"""
    rng = random.Random(9104)
    base, extra = u.rand(rng, 100), u.rand(rng, 70)
    refs = [extra + base, base + extra, base]
    reads = [base, extra + base]
    exp = u.expect(refs, reads, SC, GLOBAL, cells=True)
    assert cigars_of(exp[(0, 0)]) == [[(70, "D"), (100, "=")]] and cigars_of(exp[(1, 0)]) == [[(100, "="), (70, "D")]]
    assert cigars_of(exp[(2, 1)]) == [[(70, "I"), (100, "=")]]
    both(ctx, refs, reads, SC, exp, GLOBAL)
    ref, read = base[:80] + u.rand(rng, 40), base[:80] + u.rand(rng, 30)
    want = gr.align_numpy(ref, read, SC, GLOBAL, 0, True, cells=True)
    assert want[2][0][0] < len(read) and want[2][0][1] < len(ref)
    both(ctx, [ref], [read], SC, {(0, 0): want}, GLOBAL, extend=1)
    ctx.set_option("extend", 0)


def test_gaps_longer_than_an_iteration(ctx):
    rng = random.Random(9105)
    base, gap = u.rand(rng, 300), u.rand(rng, 100)
    with_gap = base[:130] + gap + base[130:]
    refs, reads = [with_gap, base], [base, with_gap]
    exp = u.expect(refs, reads, CHEAP, GLOBAL, cells=True)
    # (the gap slides one column left: the base before it equals its last base)
    assert cigars_of(exp[(0, 0)]) == [[(129, "="), (100, "D"), (171, "=")]]
    assert cigars_of(exp[(1, 1)]) == [[(129, "="), (100, "I"), (171, "=")]]
    both(ctx, refs, reads, CHEAP, exp, GLOBAL)


# ---- the equality rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", [0, 1])
def test_equality_is_the_canonical_code(ctx, tie):
    """lower and upper case mixed, symbols outside the fast set (K, *, bytes >= 0x80: 0xE9 upper-cases to 0xC9, 0xFF and 0xF7 only
    equal themselves)"""
    rng = random.Random(9106)
    alphabet = "ACGTacgtKk*N\xe9\xc9\xff\xdf\xf7\xd7"
    refs = [u.rand(rng, n, alphabet) for n in (90, 150)]
    reads = [u.mutate(rng, refs[0][10:80], 0.1, 0.02, alphabet), "".join(ch.swapcase() if ch.isascii() else ch for ch in refs[1][20:120]),
             u.mutate(rng, refs[1], 0.08, 0.02, alphabet)[:140]]
    for mode in (LOCAL, GLOBAL):
        exp = u.expect(refs, reads, SC, mode, tie=tie, cells=True)
        if mode == LOCAL:
            seen = "".join(sw.cigar_string(c) for e in exp.values() for c in cigars_of(e))
            assert "X" in seen and "=" in seen
        both(ctx, refs, reads, SC, exp, mode, tie)


@pytest.mark.parametrize("tie", [0, 1])
def test_equality_does_not_follow_the_score_matrix(ctx, tie):
    """A / A scores -2 and is still '='; read G against reference A scores +3 and is still X"""
    rows = [[-2, -4, -4, -4], [-4, 5, -4, -4], [3, -4, 5, -4], [-4, -4, -4, 5]]      # rows: read base; columns: reference base
    mat = ("ACGT", rows)
    rng = random.Random(9107)
    ref = u.rand(rng, 160)
    read = "".join("G" if ch == "A" and rng.random() < 0.4 else ch for ch in ref[5:150])
    exp = u.expect([ref], [read], SC, GLOBAL, tie=tie, matrix=mat, cells=True)
    ra, qa = exp[(0, 0)][1][0][1]
    cols = set(zip(ra, qa))
    assert ("A", "A") in cols and ("A", "G") in cols
    both(ctx, [ref], [read], SC, exp, GLOBAL, tie, matrix=mat)
    ctx.clear_score_matrix()


# ---- every traceback family ------------------------------------------------------------------------------------------------
def family_case():
    rng = random.Random(9108)
    base = u.rand(rng, 1100)
    refs = [base[:300], u.mutate(rng, base[200:520], 0.05, 0.02)]
    reads = [u.mutate(rng, base[100:100 + m + 20], 0.06, 0.02)[:m] for m in (40, 64, 65)] + [u.mutate(rng, base, 0.05, 0.01)[:1024]]
    assert [len(q) for q in reads] == [40, 64, 65, 1024]
    return refs, reads


@pytest.mark.parametrize("mode,extend", [(LOCAL, 0), (FIT, 0), (GLOBAL, 0), (GLOBAL, 1)])
def test_short_read_kernels(ctx, mode, extend):
    refs, reads = family_case()
    tie = mode & 1
    exp = u.expect(refs, reads, SC, mode, 0, bool(extend), tie, cells=True)
    both(ctx, refs, reads, SC, exp, mode, tie, extend=extend)


def long_case(m, n, seed):
    rng = random.Random(seed)
    base = u.rand(rng, max(m, n) + 50)
    return u.mutate(rng, base, 0.04, 0.01)[:n], u.mutate(rng, base, 0.04, 0.01)[:m]


@pytest.mark.parametrize("m,n,mode,extend", [(1025, 400, LOCAL, 0), (1025, 300, GLOBAL, 0), (2049, 300, FIT, 0), (2049, 350, GLOBAL, 1)])
def test_long_reads_cross_strips(ctx, m, n, mode, extend):
    ref, read = long_case(m, n, 9109 + m + n)
    if mode != GLOBAL or extend:
        ref = ref[:n // 3] + read[m - n // 3:] + ref[n // 3:n // 2]      # the alignment ends in the last strip and crosses the seams
    tie = (m + n) & 1
    want = gr.align_numpy(ref, read, SC, mode, 0, bool(extend), tie, cells=True)
    both(ctx, [ref], [read], SC, {(0, 0): want}, mode, tie, extend=extend, long_reads=1)


@pytest.mark.parametrize("mode,extend", [(LOCAL, 0), (GLOBAL, 1)])
def test_long_reads_band(ctx, mode, extend):
    ref, read = long_case(2049, 2060, 9110)
    want = gr.align_numpy(ref, read, SC, mode, 32, bool(extend), 0, cells=True)
    both(ctx, [ref], [read], SC, {(0, 0): want}, mode, 0, 32, extend, long_reads=1)


def test_long_reads_band_adapt_and_xdrop(ctx):
    """the adaptive band, stopped by xdrop behind a strip: the walk starts from the best cell so far"""
    rng = random.Random(9111)
    ref, read = long_case(2049, 2100, 9111)
    read = read[:1500] + u.rand(rng, 549)                    # the tail diverges
    sc, w, X = (2, -4, -2, -4), 32, 40
    want = ar.align(ref, read, sc, w, X, 0)
    assert want[4] < len(read)                                # stopped
    for c in (1, 2):
        b = u.run(ctx, [ref], [read], sc, 0, GLOBAL, w, 1, None, long_reads=1, band_adapt=1, xdrop=X, cigar=c)
        u.check_pair(b, 0, want[:3], GLOBAL)
        assert b.rows_swept(0) == want[4]
        check_cigars(b, 1, lambda p: want, c)
        b.free()
    free = ar.align(ref, read, sc, w, 0, 1)
    both(ctx, [ref], [read], sc, {(0, 0): free}, GLOBAL, 1, w, 1, long_reads=1, band_adapt=1, xdrop=0)


@pytest.mark.parametrize("m,n,w", [(700, 500, 0), (1025, 500, 0), (2049, 2080, 64)])
def test_two_piece_gaps(ctx, m, n, w):
    sc6 = (2, -4, -2, -4, -1, -24)                           # the pieces tie at 20 bases
    ref, read = long_case(m, n + 30, 9112 + m)
    ref = ref[:200] + ref[230:]                              # a 30-base insertion: piece 2's
    ref = ref[:n]
    ctx.set_option("gap_open2", sc6[5])
    ctx.set_option("gap2", sc6[4])
    want = tr.align_numpy(ref, read, sc6, GLOBAL, w, False, m & 1, cells=True)
    assert "_" * 21 in want[1][0][1][0]                      # longer than the 20 bases at which the pieces tie
    exp = {(0, 0): want}
    for c in (1, 2):
        b = u.run(ctx, [ref], [read], sc6[:4], m & 1, GLOBAL, w, 0, None, long_reads=1, cigar=c)
        u.check(b, [ref], [read], exp, GLOBAL)
        check_cigars(b, 1, lambda p: want, c)
        b.free()


def tied_case():
    unit = "ACGTTGCAAGCT"
    refs, reads = [unit * 9, "GG" + unit * 5], [unit, unit[3:] + unit[:5]]
    return refs, reads


@pytest.mark.parametrize("tie", [0, 1])
def test_tied_alignments_keep_their_order(ctx, tie):
    refs, reads = tied_case()
    exp = u.expect(refs, reads, SC, LOCAL, tie=tie, cells=True)
    assert len(exp[(0, 0)][1]) == 9
    both(ctx, refs, reads, SC, exp, LOCAL, tie)


def test_degenerate_and_empty(ctx):
    refs, reads = ["AAAAAA", "ACGTACGT", ""], ["CCC", "", "ACGT"]
    exp = u.expect(refs, reads, SC, LOCAL)
    for c in (1, 2):
        b = u.run(ctx, refs, reads, SC, 0, LOCAL, cigar=c)
        u.check(b, refs, reads, exp, LOCAL)
        assert b.n_alignments(0) == (18, sw.PAIR_DEGENERATE)
        assert b.cigar(0, 0) == (0, 1, 1, [], 0) and b.cigar(0, 17) == (0, 3, 6, [], 0)
        with pytest.raises(_capi.SwmiError) as e:
            b.cigar(0, 18)
        assert e.value.code == ERR_RANGE
        for pair in (1, 4, 6, 7, 8):                          # an empty side: no alignments
            assert b.cigars(pair) == []
            with pytest.raises(_capi.SwmiError) as e:
                b.cigar(pair, 0)
            assert e.value.code == ERR_RANGE
        assert b.cigars(5) == [(1, 4, 4, [(4, "=M"[c == 1])], 0), (5, 4, 8, [(4, "=M"[c == 1])], 0)]
        b.free()


# ---- host machinery --------------------------------------------------------------------------------------------------------
def test_exact_size_rerun(ctx):
    refs, reads = tied_case()
    exp = u.expect(refs, reads, SC, LOCAL, cells=True)
    for c in (1, 2):
        b = u.run(ctx, refs, reads, SC, 0, LOCAL, cigar=c, cell_cap=1)
        assert b.timing().rerun_pairs >= 1
        u.check(b, refs, reads, exp, LOCAL)
        check_cigars(b, 4, lambda p: exp[(p // 2, p % 2)], c)
        b.free()


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_arena_overflow_rerun(ctx, zero_copy):
    """arena_words_per_pair at its minimum: a launch's first arena holds max(pairs, 1024) dwords, twelve alternating pairs need 12 *
    132 under cigar = 2 -- the first attempt cannot hold them, so right results show the overflow re-run (the library has no
    counter of its own for it); one re-run suffices, the kernels having asked for what they need"""
    ref, read, want = alternating_case()
    reads = [read] * 12
    exp = {(0, q): want for q in range(12)}
    ctx.set_option("arena_words_per_pair", 1)
    ctx.set_option("zero_copy", zero_copy)
    b = u.run(ctx, [ref], reads, DIAG, 0, GLOBAL, cigar=2)
    words = sum(2 + len(b.cigar(q, 0)[3]) for q in range(12))
    assert words == 12 * 132 > max(12 * 1, 1024)
    u.check(b, [ref], reads, exp, GLOBAL)
    check_cigars(b, 12, lambda p: want, 2)
    b.free()
    both(ctx, [ref], reads, DIAG, exp, GLOBAL)                # (cigar = 1: 3 dwords a pair; and 2 again, the arena now grown)


@pytest.mark.parametrize("zero_copy", [0, 1])
def test_zero_copy_and_chunks(ctx, zero_copy):
    rng = random.Random(9113)
    base = u.rand(rng, 400)
    refs = [u.mutate(rng, base, 0.05, 0.02)[:300] for _ in range(8)]
    reads = [u.mutate(rng, base[20:], 0.05, 0.02)[:290] for _ in range(8)]
    exp = u.expect(refs, reads, SC, LOCAL, cells=True)
    ctx.set_option("zero_copy", zero_copy)
    both(ctx, refs, reads, SC, exp, LOCAL)
    ctx.set_option("max_workspace_bytes", 1 << 20)
    b = u.run(ctx, refs, reads, SC, 0, LOCAL, cigar=2)
    assert b.timing().fill_launches > 1                       # several launches: their records are copied out of the block
    u.check(b, refs, reads, exp, LOCAL)
    check_cigars(b, 64, lambda p: exp[(p // 8, p % 8)], 2)
    b.free()


def test_async_run_keeps_the_value_it_was_asked_with(ctx):
    ref, read, want = alternating_case()
    p = sw.make_params(DIAG[:3])
    ctx.set_option("gap_open", DIAG[3])
    ctx.set_option("align_mode", GLOBAL)
    ctx.set_option("cigar", 2)
    ctx.set_option("debug_async_delay_us", 20000)
    b = ctx.upload([ref], [read]).run_async(p)
    ctx.set_option("cigar", 0)                                # does not reach the run in flight
    b.wait()
    ctx.set_option("debug_async_delay_us", 0)
    check_cigars(b, 1, lambda k: want, 2)
    b.run(p)                                                  # ... but the next one
    u.check_pair(b, 0, want, GLOBAL)
    with pytest.raises(_capi.SwmiError) as e:
        b.cigar(0, 0)
    assert e.value.code == ERR_UNSUPPORTED and "cigar" in str(e.value)
    b.free()


def test_stream_of_two_chunks(ctx):
    rng = random.Random(9114)
    base = u.rand(rng, 300)
    refs = [u.mutate(rng, base, 0.05, 0.02) for _ in range(6)]
    reads = [base[30:180], u.mutate(rng, base[100:260], 0.05, 0.02)]
    ctx.set_option("gap_open", SC[3])
    ctx.set_option("cigar", 2)
    st = ctx.stream(reads, sw.make_params(SC[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.set_option("cigar", 0)                                # (the stream keeps the value it was opened with)
    st.push(refs[:3]).push(refs[3:]).finish()
    chunks = st.chunks()
    assert [first for first, _ in chunks] == [0, 3]
    for first, c in chunks:
        part = refs[first:first + 3]
        exp = u.expect(part, reads, SC, LOCAL, cells=True)
        assert c.pipeline_mode() == 3
        u.check(c, part, reads, exp, LOCAL)
        check_cigars(c, 6, lambda p: exp[(p // 2, p % 2)], 2)
    st.close()


def test_pair_list_forward_and_reversed(ctx):
    rng = random.Random(9115)
    src = u.rand(rng, 600)
    refs, reads = [src], [u.mutate(rng, src, 0.05, 0.02)]
    specs = [(0, 0, 100, 300, 90, 280), (0, 0, 100, 300, 90, 280, True), (0, 0)]
    for c in (1, 2):
        u_opts = dict(gap_open=SC[3], align_mode=GLOBAL, extend=1, cigar=c)
        for name, v in u_opts.items():
            ctx.set_option(name, v)
        b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
        assert b.pipeline_mode() == 3
        for k in range(len(specs)):
            ref, read = b.segments(k)
            want = gr.align_numpy(ref, read, SC, GLOBAL, 0, True, cells=True)
            u.check_pair(b, k, want, GLOBAL, k)
            one = ctx.upload([ref], [read]).run(sw.make_params(SC[:3]))
            assert b.cigars(k) == one.cigars(0)
            one.free()
        check_cigars(b, len(specs), lambda k: gr.align_numpy(*b.segments(k), SC, GLOBAL, 0, True, cells=True), c)
        b.free()


def test_refusals(ctx):
    refs, reads = tied_case()
    exp = u.expect(refs, reads, SC, LOCAL, cells=True)
    # values outside 0 .. 2 leave the context as it was
    ctx.set_option("cigar", 1)
    for bad in (3, -1):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("cigar", bad)
        assert e.value.code == ERR_INVALID and "cigar" in str(e.value)
    b = u.run(ctx, refs, reads, SC, 0, LOCAL)
    check_cigars(b, 4, lambda p: exp[(p // 2, p % 2)], 1)
    # scores_only wins
    ctx.set_option("scores_only", 1)
    b.run(sw.make_params(SC[:3]))
    assert b.score(0) == exp[(0, 0)][0]
    with pytest.raises(_capi.SwmiError) as e:
        b.cigar(0, 0)
    assert e.value.code == ERR_UNSUPPORTED and "scores_only" in str(e.value)
    ctx.set_option("scores_only", 0)
    # a run with cigar = 0: the accessor is refused and every result is as before, with either payload of old
    ctx.set_option("cigar", 0)
    for device_strings in (1, 0):
        ctx.set_option("device_strings", device_strings)
        b.run(sw.make_params(SC[:3]))
        with pytest.raises(_capi.SwmiError) as e:
            b.cigar(0, 0)
        assert e.value.code == ERR_UNSUPPORTED and "cigar" in str(e.value)
        u.check(b, refs, reads, exp, LOCAL)
    b.free()


def test_gap_open_0_gives_the_linear_results(ctx):
    """cigar = 2 with gap_open = 0 on the default scores takes the affine kernels and returns what the linear pipeline returns"""
    rng = random.Random(9116)
    base = u.rand(rng, 500)
    refs = [u.mutate(rng, base, 0.05, 0.02) for _ in range(4)] + ["ACGTTGCAAGCT" * 6]
    reads = [base[50:200], u.mutate(rng, base[200:360], 0.08, 0.03), "ACGTTGCAAGCT"]
    sc = sw.DEFAULT_SCORES + (0,)
    for tie in (0, 1):
        lin = u.run(ctx, refs, reads, sc, tie, LOCAL, mode3=False, cigar=0)
        assert lin.pipeline_mode() in (1, 2)
        want = [(lin.score(p), lin.alignments(p, with_cell=True)) for p in range(15)]
        lin.free()
        b = u.run(ctx, refs, reads, sc, tie, LOCAL, cigar=2)
        assert b.pipeline_mode() == 3
        assert [(b.score(p), b.alignments(p, with_cell=True)) for p in range(15)] == want
        for p in range(15):
            for k, (begin, (ra, qa), cell) in enumerate(want[p][1]):
                assert b.cigar(p, k) == (begin, cell[0], cell[1]) + cr.cigar(ra, qa, 2)
        b.free()
