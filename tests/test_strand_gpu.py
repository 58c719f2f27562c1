"""The minus strand on the GPU (SWMI_SPEC_READ_REVCOMP): a pair of a pair list names its strand, and
sw_gather_kernel cuts, reverses, complements and encodes the read segment from the resident source.

The contract is 8l's sentence, extended: pair k gives, bit for bit, what the library gives for the two segments cut, reversed
under SWMI_SPEC_REVERSE and -- the read -- reverse-complemented under SWMI_SPEC_READ_REVCOMP by the caller.  So every expected
value comes from the CPU references the other pair tests use (oracle.sw_oracle.opt_alignments, gotoh_reference, hits_reference,
cigar_reference), called on PairBatch.segments(), which is plain slicing plus sw.revcomp on the host (tests/test_strand_cpu.py).
All comparisons are exact.  The first upload of a "-" pair is what fails without the feature: flag 0x4 is refused."""
import ctypes as C
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from oracle import sw_oracle as orc

import affine_gpu_util as u
import cigar_reference as cr
import gotoh_reference as gr
import hits_reference as hr

pytestmark = pytest.mark.gpu

ERR_INVALID = -1                            # swmi_status (include/swmi.h)
WHOLE = _capi.SPEC_WHOLE
LOCAL, FIT, GLOBAL = sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL
TYPES = b"aid-"
FLAGS = [(False, "+"), (True, "+"), (False, "-"), (True, "-")]          # flags 0, 1, 4, 5


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


_ORACLE = {}


def linear_want(ref, read):
    """(score, alignments with cells) of the oracle for one pair under the default scores, computed once per pair of segments"""
    if (ref, read) not in _ORACLE:
        _ORACLE[(ref, read)] = orc.opt_alignments((ref, read), (5, -3, -4), TYPES, 0, with_cells=True)
    return _ORACLE[(ref, read)]


def check_linear_pair(b, pair, ref, read, what):
    """score, count, flags, every alignment's begin, both strings and its cell; a degenerate pair lists one (0, "", "") per cell"""
    es, ea = linear_want(ref, read)
    assert b.score(pair) == es, (what, b.score(pair), es)
    n, flags = b.n_alignments(pair)
    assert n == len(ea), (what, n, len(ea))
    if flags & sw.PAIR_DEGENERATE:
        assert flags == sw.PAIR_DEGENERATE and es == 0, what
        assert b.alignment(pair, n - 1, True) == (0, ("", ""), (len(read), len(ref))), what
        return
    assert flags == 0, (what, flags)
    assert b.alignments(pair, True) == ea, what


def check_linear(b):
    for k in range(b.n_pairs()):
        ref, read = b.segments(k)
        check_linear_pair(b, k, ref, read, (k, b.spec(k)))


def transformed(refs, reads, spec):
    """the two segments of a pair given with resolved lengths, transformed in plain Python -- not through the package"""
    r, q, rs, rl, qs, ql, rev = spec[:7]
    a, b = refs[r][rs:rs + rl], reads[q][qs:qs + ql]
    if len(spec) == 8 and spec[7] == "-":
        b = sw.revcomp(b)
    return (a[::-1], b[::-1]) if rev else (a, b)


# ---- 1: the gather loop ---------------------------------------------------------------------------------------------------------
READ_LENS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 260)


def _grid_sources():
    """a reference of 300 bytes and a read source of 272 that follows the reference's reverse complement with substitutions, so
    that the minus pairs have long alignments; ACGT, lower case, N, K, U and a non-letter byte on both.  The read source lies
    behind a first read of 32 bytes: it starts on a 16-byte boundary of the device copy, so read starts 0 .. 3 are the four
    alignments of the kernel's loads."""
    rng = random.Random(2001)
    alphabet = "ACGTACGTACGTacgtNnKkUu\xe9*"
    ref = u.rand(rng, 300, alphabet)
    read = [c if rng.random() < 0.9 else rng.choice(alphabet) for c in sw.revcomp(ref[14:286])]
    for k, c in enumerate("KkUuMmNn\xe9*"):                          # (whatever the substitutions chose)
        read[30 + 23 * k] = c
    return [u.rand(rng, 40), ref], [u.rand(rng, 32), "".join(read)]


def _grid_specs():
    specs = []
    for rev, strand in FLAGS:
        for start in range(4):
            for ln in READ_LENS:
                specs.append((1, 1, 5, 290, start, ln, rev, strand))
        # segments that end on the last byte of the last source, the whole sources, and the first sources
        specs += [(1, 1, 150, WHOLE, 272 - 65, WHOLE, rev, strand), (1, 1, 0, WHOLE, 0, WHOLE, rev, strand), (0, 0, 3, 33, 1, 31, rev, strand),
                  (1, 1, 299, 1, 271, 1, rev, strand)]
    return specs


def _fast_path_case():
    """an all-ACGT window of a read source that holds a K before and behind it, against an all-ACGT window of such a reference"""
    rng = random.Random(2002)
    ref = "K" + u.rand(rng, 200) + "kK"
    fwd = u.mutate(rng, ref[31:151])
    read = "NK" + sw.revcomp(fwd) + "K"
    return ref, read, (0, 0, 1, 200, 2, len(fwd)), fwd


@pytest.mark.parametrize("device_strings", [1, 0])
def test_gather_grid(ctx, device_strings):
    """every alignment of the read's start x every length class of sw_gather_kernel's dword loop x the four flag combinations"""
    refs, reads = _grid_sources()
    specs = _grid_specs()
    ctx.set_option("device_strings", device_strings)
    b = ctx.upload_pairs(refs, reads, specs)
    try:
        assert b.n_pairs() == len(specs)
        b.run()
        assert b.pipeline_mode() in (1, 2)
        for k, sp in enumerate(specs):
            got = b.spec(k)                                           # WHOLE resolved, the strand as given
            assert got[:3] + got[4:5] + got[6:] == sp[:3] + sp[4:5] + sp[6:7] + (("-",) if sp[7] == "-" else ()), k
            assert b.strand(k) == sp[7]
            ref, read = b.segments(k)
            assert (ref, read) == transformed(refs, reads, got), k
            check_linear_pair(b, k, ref, read, (k, sp))
        # the complemented bytes came through with their case: the minus alignments hold lower-case bases, K and k (the source's M
        # and m), the bytes that are their own complement, and no U (nothing is complemented to it; the source's became A)
        assert all(c in reads[1] for c in "ACGTacgtNnKkMmUu\xe9*")
        seen = "".join(a[1][1] for k in range(b.n_pairs()) if b.strand(k) == "-" and not b.n_alignments(k)[1] for a in b.alignments(k))
        assert all(c in seen for c in "acgtKkMmNn\xe9*") and "U" not in seen and "u" not in seen
        assert max(b.score(k) for k in range(b.n_pairs()) if b.strand(k) == "-") > 500
    finally:
        b.free()
    # a minus pair whose segment is all ACGT inside a source with a K elsewhere: what the plain batch of the two segments gives
    ref, read, spec, fwd = _fast_path_case()
    b = ctx.upload_pairs([ref], [read], [spec + (False, "-"), spec + (True, "-")]).run()
    try:
        for k, (a, q) in enumerate([(ref[1:201], fwd), (ref[1:201][::-1], fwd[::-1])]):
            assert b.segments(k) == (a, q)
            x = ctx.upload([a], [q]).run()
            assert (b.score(k), b.n_alignments(k), b.alignments(k, True)) == (x.score(0), x.n_alignments(0), x.alignments(0, True))
            assert b.score(k) > 400
            x.free()
            check_linear_pair(b, k, a, q, k)
    finally:
        b.free()


@pytest.mark.parametrize("device_strings", [1, 0])
def test_all_256_byte_values(ctx, device_strings):
    """a read source of every byte value once, on the minus strand against its own reverse complement: one alignment down the
    diagonal whose read string is the transformed segment, byte for byte (read through the length: the strings hold a NUL)"""
    source = bytes(range(256))
    want = sw.revcomp(source)
    assert want == bytes(sw.COMPLEMENT[x] for x in reversed(range(256)))
    ctx.set_option("device_strings", device_strings)
    b = ctx.upload_pairs([want], [source], [(0, 0, 0, WHOLE, 0, WHOLE, False, "-")]).run()
    try:
        assert b.score(0) == 5 * 256 and b.n_alignments(0) == (1, 0)
        beg, ei, ej = C.c_int32(), C.c_int32(), C.c_int32()
        r, q, ln = C.c_char_p(), C.c_char_p(), C.c_uint32()
        _capi.check(b._lib.swmi_pair_alignment(b._h, 0, 0, C.byref(beg), C.byref(ei), C.byref(ej), C.byref(r), C.byref(q), C.byref(ln)))
        assert (beg.value, ei.value, ej.value, ln.value) == (1, 256, 256, 256)
        assert C.string_at(C.cast(q, C.c_void_p).value, 256) == want
        assert C.string_at(C.cast(r, C.c_void_p).value, 256) == want
    finally:
        b.free()


# ---- 2: the affine kernels ------------------------------------------------------------------------------------------------------
SC = (5, -3, -2, -6)
ASYM = ("ACGT", [[4, -3, -1, -2], [-2, 5, -3, -1], [-1, -2, 3, -3], [-3, -1, -2, 6]])      # rows: the read's base; M[x][y] != M[y][x]


def _affine_case():
    """a 300-base stretch of the reference, mutated, as the read source's reverse complement; pair 0 on the minus strand, pair 1
    its left extension (REVERSE | READ_REVCOMP) and pair 2 the plus pair of the same bytes"""
    rng = random.Random(2003)
    ref = u.rand(rng, 900)
    fwd = u.mutate(rng, ref[100:400], 0.05, 0.02)
    read = u.rand(rng, 9) + sw.revcomp(fwd).lower() + u.rand(rng, 6)
    m = len(fwd)
    return [ref], [read], [(0, 0, 100, 320, 9, m, False, "-"), (0, 0, 80, 320, 9, m, True, "-"), (0, 0, 100, 320, 9, m, False, "+")], fwd


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


@pytest.mark.parametrize("mode,extend,matrix,cigar", [(LOCAL, 0, ASYM, 0), (FIT, 0, None, 0), (GLOBAL, 0, None, 0), (GLOBAL, 1, None, 2)],
                         ids=["local-matrix", "fit", "global", "extend-cigar2"])
def test_affine_modes(ctx, mode, extend, matrix, cigar):
    refs, reads, specs, fwd = _affine_case()
    _set_affine(ctx, SC, mode, extend, matrix, cigar=cigar)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(SC[:3]))
    try:
        assert b.pipeline_mode() == 3
        assert b.segments(0) == (refs[0][100:420], fwd.lower()) and b.segments(1) == (refs[0][80:400][::-1], fwd.lower()[::-1])
        for k in range(len(specs)):
            ref, read = b.segments(k)
            want = gr.align_numpy(ref, read, SC, mode, 0, bool(extend), 0, matrix, cells=True)
            u.check_pair(b, k, want, mode, (k, specs[k]))
            if cigar:                                                 # = / X and nm on the COMPLEMENTED read
                got = b.cigars(k)
                assert len(got) == len(want[1]) >= 1
                for x, ((begin, (ra, qa)), cell) in enumerate(zip(want[1], want[2])):
                    ent, nm = cr.cigar(ra, qa, 2)
                    assert got[x] == (begin, cell[0], cell[1], ent, nm), (k, x)
                    assert k == 2 or (nm < 60 and any(op == "X" for _, op in ent) and max(n for n, op in ent if op == "=") > 20)
        assert b.score(0) > 5 * 200 and (mode != LOCAL or b.score(2) < b.score(0) // 3)
        if matrix:
            # the matrix is not symmetric: the same pair scored with the roles of row and column exchanged differs, so the row is
            # the complemented read base
            ref, read = b.segments(0)
            swapped = (matrix[0], [list(col) for col in zip(*matrix[1])])
            assert gr.align_numpy(ref, read, SC, mode, 0, False, 0, swapped)[0] != b.score(0)
    finally:
        b.free()


def test_long_read_with_band(ctx):
    """a read of 1,100 bases on the minus strand, and its left extension, through the banded strip sweeps"""
    rng = random.Random(2004)
    ref = u.rand(rng, 1400)
    fwd = u.mutate(rng, ref[100:1260], 0.03, 0.002)[:1100]
    refs, reads = [ref], [sw.revcomp(fwd)]
    sc = (2, -4, -2, -4)
    specs = [(0, 0, 100, 1130, 0, 1100, False, "-"), (0, 0, 70, 1130, 0, 1100, True, "-")]
    _set_affine(ctx, sc, GLOBAL, 1, None, long_reads=1, band=64)
    b = ctx.upload_pairs(refs, reads, specs).run(sw.make_params(sc[:3]))
    try:
        assert b.pipeline_mode() == 3
        assert b.segments(0) == (ref[100:1230], fwd) and b.segments(1) == (ref[70:1200][::-1], fwd[::-1])
        for k in range(2):
            seg_ref, seg_read = b.segments(k)
            want = gr.align_numpy(seg_ref, seg_read, sc, GLOBAL, 64, True, 0, None, cells=True)
            u.check_pair(b, k, want, GLOBAL, k)
            assert b.rows_swept(k) == 1100
        assert b.score(0) > 2 * 900
    finally:
        b.free()


# ---- 3: subopt + hits on a minus pair, then the reverse extensions ----------------------------------------------------------------
HSC = (5, -4, -3, -5)


def _weaken(read, k):
    out = list(read)
    for x in range(k):
        p = (2 * x + 1) * len(read) // (2 * k)
        out[p] = "ACGT"[("ACGT".index(out[p]) + 1) % 4]
    return "".join(out)


def test_hits_and_hit_specs_on_a_minus_pair(ctx):
    """the read segment is the reverse complement of an 80-base stretch X; the reference holds X at byte 150 and X with five
    substitutions at byte 330.  The two best hits end on the copies' last bases, and the extend run over hit_specs ends -- in
    source coordinates -- on their first: reference bytes 150 and 330, read byte 7 + 79 (the read's order is reversed)."""
    rng = random.Random(2005)
    X = u.rand(rng, 80)
    ref = u.rand(rng, 150) + X + u.rand(rng, 100) + _weaken(X, 5) + u.rand(rng, 150)
    assert ref[150:230] == X and len(ref) == 560
    reads = [u.rand(rng, 7) + sw.revcomp(X) + u.rand(rng, 5)]
    specs = [(0, 0, 40, 500, 7, 80, False, "-"), (0, 0, 40, 500, 7, 80, True, "-")]
    _set_affine(ctx, HSC, LOCAL, 0, None, subopt=30, hits=4)
    b = ctx.upload_pairs([ref], reads, specs).run(sw.make_params(HSC[:3]))
    try:
        assert b.pipeline_mode() == 3 and b.segments(0) == (ref[40:540], X)
        want = hr.hits_numpy(ref[40:540], X, HSC, 30, 4)
        hits = b.hits(0)
        assert hits == want and hits[:2] == [(400, 80, 230 - 40), (355, 80, 410 - 40)]
        assert b.subopt(0) == (355, 370) and b.score(0) == 400
        assert b.to_source(0, 80, 190) == (7, 229) and b.to_source(0, 1, 190 - 79) == (86, 150)
        ext = b.hit_specs(0)
        assert ext == [(0, 0, 40, j, 7 + 80 - i, i, True, "-") for _, i, j in hits]
        with pytest.raises(ValueError):
            b.hit_specs(1)
    finally:
        b.free()
    _set_affine(ctx, HSC, GLOBAL, 1, None, subopt=0, hits=0)
    pb = ctx.upload_pairs([ref], reads, ext).run(sw.make_params(HSC[:3]))
    try:
        assert [pb.score(k) for k in range(len(ext))] == [h[0] for h in hits]
        starts = []
        for k in range(2):
            (_, _, (ei, ej)), = pb.alignments(k, True)
            starts.append(pb.to_source(k, ei, ej))
        assert starts == [(86, 150), (86, 330)]
    finally:
        pb.free()
        _set_affine(ctx, HSC, LOCAL, 0)


# ---- 4: both strands --------------------------------------------------------------------------------------------------------------
def test_both_strands_and_best_strand(ctx):
    rng = random.Random(2006)
    ref = u.rand(rng, 2000)
    planted, reads = [], []
    for q in range(8):
        at = 100 + 230 * q
        read = list(ref[at:at + 100])
        for p in rng.sample(range(5, 95), 3):
            read[p] = "ACGT"[("ACGT".index(read[p]) + 1) % 4]
        read = "".join(read)
        planted.append("-" if q % 2 else "+")
        reads.append(sw.revcomp(read) if q % 2 else read)
    pairs = sw.both_strands([(0, q) for q in range(8)])
    b = ctx.upload_pairs([ref], reads, pairs).run()
    try:
        assert b.n_pairs() == 16
        best = b.best_strand()
        assert [k // 2 for k in best] == list(range(8))
        assert [b.strand(k) for k in best] == planted
        for q, k in enumerate(best):
            assert b.score(k) >= 5 * 97 - 3 * 3 - 20 and b.score(k ^ 1) < 300, (q, b.score(k), b.score(k ^ 1))
            (_, _, (ei, ej)), = b.alignments(k, True)
            qi, rj = b.to_source(k, ei, ej)                            # the end cell lies on the planted diagonal
            at = 100 + 230 * q
            assert rj - at == (99 - qi if planted[q] == "-" else qi), q
        check_linear(b)
    finally:
        b.free()


# ---- 5: set_pairs -----------------------------------------------------------------------------------------------------------------
def _results(b):
    return [(b.score(k), b.n_alignments(k), b.alignments(k, True) if not b.n_alignments(k)[1] else None) for k in range(b.n_pairs())]


def test_set_pairs_grows_the_transformed_area_and_goes_back(ctx):
    rng = random.Random(2007)
    ref = u.rand(rng, 700, "ACGTacgtN")
    refs = [ref, u.rand(rng, 90)]
    reads = [u.mutate(rng, ref[50:250]), sw.revcomp(u.mutate(rng, ref[300:480])), u.rand(rng, 33)]
    plus = [(0, 0, 20, 300, 0, WHOLE), (0, 1, 250, 300, 0, WHOLE), (1, 2), (0, 0, 20, 300, 3, 150)]
    minus = [(0, 1, 250, 300, 0, WHOLE, False, "-"), (0, 1, 250, 300, 5, 170, True, "-"), (0, 0, 20, 300, 0, WHOLE, False, "-"), (1, 2),
             (0, 1, 280, 200, 1, 150, False, "-")] + [(0, 1, 250 + k, 300, k, 170, bool(k & 1), "-") for k in range(12)]
    b = ctx.upload_pairs(refs, reads, plus).run()
    try:
        # all plus (no transformed area) -> minus pairs (the area grows: the sources are uploaded again) -> back -> a smaller area
        # (the sources stay) -> the largest
        for step, lst in enumerate((plus, minus, plus, minus[:2], plus + minus)):
            if step:
                assert b.set_pairs(lst).n_pairs() == len(lst)
                with pytest.raises(sw.SwmiError):
                    b.score(0)                                       # the old results are gone
                b.run()
            fresh = ctx.upload_pairs(refs, reads, lst).run()
            assert _results(b) == _results(fresh), step
            assert [b.spec(k) for k in range(b.n_pairs())] == [fresh.spec(k) for k in range(len(lst))]
            fresh.free()
            check_linear(b)
            if lst is minus:
                assert b.score(0) > 5 * 120 and b.spec(0) == (0, 1, 250, 300, 0, len(reads[1]), False, "-")
    finally:
        b.free()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def _spec_array(rows):
    arr = (_capi.PairSpec * len(rows))()
    for k, row in enumerate(rows):
        arr[k] = _capi.PairSpec(*row)
    return arr


def test_flag_bits(ctx):
    lib = _capi.load()
    refs, reads = ["ACGTACGTAC" * 4, "TTGACCA" * 3], ["ACGTTGCAAC" * 3]
    good = [(0, 0, 2, 30, 1, 25, False, "-"), (1, 0, 0, WHOLE, 3, 20, True)]
    b = ctx.upload_pairs(refs, reads, good).run()
    try:
        check_linear(b)
        before = _results(b)
        rb, ro = _capi.pack(refs)
        qb, qo = _capi.pack(reads)
        ok = (0, 0, 0, 4, 0, 4, 0, 0)
        for flags in (0x2, 0x8, 0x6):
            arr = _spec_array([ok, ok, (0, 0, 0, 4, 0, 4, flags, 0), ok])
            h = C.c_void_p()
            assert lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 2, qb, qo, 1, arr, 4, C.byref(h)) == ERR_INVALID, flags
            assert b"pair 2" in lib.swmi_last_error() and not h.value, (flags, lib.swmi_last_error())
            assert lib.swmi_batch_set_pairs(ctx._h, b._h, arr, 4) == ERR_INVALID, flags
            assert b"pair 2" in lib.swmi_last_error(), (flags, lib.swmi_last_error())
        # the batch is as it was
        assert b.n_pairs() == 2 and b.spec(0) == (0, 0, 2, 30, 1, 25, False, "-") and b.spec(1) == (1, 0, 0, 21, 3, 20, True)
        assert _results(b) == before and _results(b.run()) == before
        for flags in (0x4, 0x5):
            arr = _spec_array([ok, (0, 0, 3, 20, 2, 18, flags, 0)])
            h = C.c_void_p()
            assert lib.swmi_batch_upload_pairs(ctx._h, rb, ro, 2, qb, qo, 1, arr, 2, C.byref(h)) == 0, (flags, lib.swmi_last_error())
            sp = _capi.PairSpec()
            assert lib.swmi_batch_pair_spec(h, 1, C.byref(sp)) == 0 and sp.flags == flags       # the flags as held
            lib.swmi_batch_free(ctx._h, h)
            assert lib.swmi_batch_set_pairs(ctx._h, b._h, arr, 2) == 0, flags
            check_linear(b.set_pairs([(0, 0, 3, 20, 2, 18, bool(flags & 1), "-")]).run())
    finally:
        b.free()
