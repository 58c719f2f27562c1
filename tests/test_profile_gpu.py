"""Per-read score profiles on the GPU (swmi_batch_set_read_profiles: the ten sw_affine_sweep_*profile* kernels of swmi_affine.hip,
DESIGN.md section 8t) against tests/profile_reference.py: every score, the flags, the number of alignments, every alignment's begin,
both strings and its maximum cell.  Batch.set_read_profiles is what fails without the feature.

  sweep kernel (sw_affine_sweep_...)              rows per lane   run by
  [fit_|global_|extend_|overlap_]profile_kernel        1 .. 4     test_rows_per_lane (R 1 .. 4), test_matrix_parity, test_ties_beyond_cell_cap,
                                                                  test_lifecycle*, test_payloads, test_path_bound
  [..]profile_wide_kernel                              5 .. 16    test_rows_per_lane (R 5 .. 16), test_matrix_parity, test_bounds*, test_chunking

  wavefronts per workgroup (swmi_affine_profile_waves)            run by
  4                                                               every test above but test_bounds*; test_wavefronts_per_workgroup[n8_R16]
  3                                 wide                          test_wavefronts_per_workgroup[n9_R16]
                                    narrow                        test_wavefronts_per_workgroup[n64_R3]
  2                                 wide                          test_wavefronts_per_workgroup[n15_R16], test_rerun_in_a_wide_class (the re-run)
                                    narrow                        test_wavefronts_per_workgroup[n64_R4]
  1                                 wide                          test_wavefronts_per_workgroup[n31_R16, n64_R7], test_bounds*
  narrow 4 + wide 2, one pair array                               test_mixed_classes_in_one_batch (n = 15), test_rerun_in_a_wide_class (first launch)
  narrow 2 + wide 1, one pair array                               test_mixed_classes_in_one_batch (n = 64)
  narrow 4 + wide 2, then narrow 4 + wide 4 (another r_max)       test_mixed_classes_chunked
The inputs come from tests/profile_cases.py, which states what each is built for; tests/test_profile_cpu.py holds them to it."""
import ctypes as C
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as mx

import affine_gpu_util as u
import cigar_reference as cr
import gotoh_reference as gr
import profile_cases as pc
import profile_reference as pr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _set(ctx, name, sc, **options):
    ctx.set_option("gap_open", sc[3])
    for k, v in dict(pc.options(name), **options).items():
        ctx.set_option(k, v)


def _run(ctx, refs, reads, profiles, name, tie=0, sc=pc.SC, alphabet=pc.ALPHABET, **options):
    _set(ctx, name, sc, **options)
    b = ctx.upload(refs, reads).set_read_profiles(alphabet, profiles)
    b.run(sw.make_params(sc[:3], None, tie))
    assert b.pipeline_mode() == 3
    return b


def _expect(refs, reads, profiles, name, tie=0, sc=pc.SC, alphabet=pc.ALPHABET):
    return {(r, q): pc.want(refs[r], reads[q], profiles[q], name, tie, sc, alphabet) for r in range(len(refs)) for q in range(len(reads))}


def _check(b, refs, reads, exp, name):
    u.check(b, refs, reads, exp, pc.MODES[name][0], map_ref=False)


# 1 -- every rows-per-lane class, all five modes, both tie orders
@pytest.mark.parametrize("name", list(pc.MODES))
@pytest.mark.parametrize("R", pc.RS)
def test_rows_per_lane(ctx, R, name):
    refs, reads, profiles = pc.grid(R)
    for tie in (0, 1):
        b = _run(ctx, refs, reads, profiles, name, tie)
        _check(b, refs, reads, pc.expected(R, name, tie), name)
        b.free()


# 2 -- matrix parity on the device
@pytest.mark.parametrize("name", ["local", "fit"])
def test_matrix_parity(ctx, name):
    """profile_from_matrix(BLOSUM62) gives, pair by pair, what the matrix run of the same context gives"""
    refs, reads = pc.protein_pairs()
    sc = pc.SC_PROTEIN
    _set(ctx, name, sc)
    ctx.set_score_matrix(mx.BLOSUM62)
    bm = ctx.upload(refs, reads).run(sw.make_params(sc[:3]))
    ctx.clear_score_matrix()
    profiles = [mx.profile_from_matrix(q, mx.BLOSUM62, None, sc[1]) for q in reads]
    bp = ctx.upload(refs, reads).set_read_profiles(mx.BLOSUM62.alphabet, profiles).run(sw.make_params(sc[:3]))
    assert bm.pipeline_mode() == bp.pipeline_mode() == 3
    for pair in range(36):
        assert bp.score(pair) == bm.score(pair), pair
        assert bp.n_alignments(pair) == bm.n_alignments(pair), pair
        assert bp.alignments(pair, with_cell=True) == bm.alignments(pair, with_cell=True), pair
    # ... and what the restatement gives
    exp = _expect(refs[:2], reads, profiles, name, 0, sc, mx.BLOSUM62.alphabet)
    for r in range(2):
        for q in range(6):
            u.check_pair(bp, r * 6 + q, exp[(r, q)], pc.MODES[name][0], (r, q))
    bm.free()
    bp.free()


# 3 -- bounds
def test_bounds_entries_at_the_limit(ctx):
    """entries of +2^20 and -2^20 on a 1024-row read: H reaches 2^30 on the diagonal of a short reference"""
    rng = random.Random(3)
    S = 1 << 20
    read = u.rand(rng, 1024)
    refs = [u.rand(rng, 40, "ACGTN"), "ACGTX" * 5]
    profile = [[rng.choice((S, -S, S, 3, -2)) for _ in pc.ALPHABET] for _ in range(1024)]
    for name in ("local", "global"):
        sc = (1, -S, -3, -5)
        b = _run(ctx, refs, [read], [profile], name, 0, sc)
        _check(b, refs, [read], _expect(refs, [read], [profile], name, 0, sc), name)
        b.free()
    with pytest.raises(ValueError):
        ctx.upload(refs, [read]).set_read_profiles(pc.ALPHABET, [[[S + 1] * 5] * 1024])


@pytest.mark.parametrize("n, m, ok", [(31, 1024, True), (32, 1024, False), (64, 448, True), (64, 449, False)])
def test_bounds_of_the_lds_table(ctx, n, m, ok):
    """M * (n + 1) <= 32768 with M = 64 * ceil(m / 64): at the bound the batch runs, one symbol or one row beyond it is refused
    with nothing launched"""
    rng = random.Random(n * m)
    alphabet = bytes(range(0x21, 0x21 + n))                 # '!' .. : no two of them one symbol (no lower-case letters)
    read = "".join(chr(rng.randrange(0x21, 0x21 + n)) for _ in range(m))
    ref = "".join(chr(rng.randrange(0x21, 0x21 + n + 1)) for _ in range(50))
    profile = pc.random_profile(rng, m, n)
    _set(ctx, "local", pc.SC)
    b = ctx.upload([ref], [read]).set_read_profiles(alphabet, [profile])
    if ok:
        b.run(sw.make_params(pc.SC[:3]))
        u.check_pair(b, 0, pc.want(ref, read, profile, "local", 0, pc.SC, alphabet.decode("latin-1")), 0)
    else:
        with pytest.raises(sw.SwmiError) as e:
            b.run(sw.make_params(pc.SC[:3]))
        assert e.value.code == ERR_UNSUPPORTED and "profile" in str(e.value) and str(n) in str(e.value)
        assert b.timing().fill_launches == 0
    b.free()


# 4 -- ties beyond cell_cap: the exact-size re-run sweeps under the profile too
@pytest.mark.parametrize("tie", [0, 1])
def test_ties_beyond_cell_cap(ctx, tie):
    ref, read, profile = pc.periodic_case()
    b = _run(ctx, [ref], [read], [profile], "local", tie, cell_cap=2)
    assert b.timing().rerun_pairs == 1
    u.check_pair(b, 0, pc.want(ref, read, profile, "local", tie), 0)
    b.free()


# 5 -- chunking under max_workspace_bytes
def test_chunking(ctx):
    refs, reads, profiles = pc.grid(16)
    b = _run(ctx, refs, reads, profiles, "fit", 0, max_workspace_bytes=1 << 20)
    assert b.timing().fill_launches > 1
    _check(b, refs, reads, pc.expected(16, "fit", 0), "fit")
    b.free()


# 6 -- lifecycle
def _small():
    rng = random.Random(66)
    refs = [pc.random_reference(rng, n) for n in (33, 58)]
    reads = [u.rand(rng, m, "ACGTacgt") for m in (21, 70, 46)]
    pa = [pc.random_profile(rng, len(q)) for q in reads]
    pb = [pc.random_profile(rng, len(q)) for q in reads]
    return refs, reads, pa, pb


def test_lifecycle_set_replace_clear(ctx):
    refs, reads, pa, pb = _small()
    params = sw.make_params(pc.SC[:3])
    b = _run(ctx, refs, reads, pa, "local")
    _check(b, refs, reads, _expect(refs, reads, pa, "local"), "local")
    b.set_read_profiles(pc.ALPHABET, pb)
    with pytest.raises(sw.SwmiError):
        b.score(0)                                              # the old results are dropped
    b.run(params)
    _check(b, refs, reads, _expect(refs, reads, pb, "local"), "local")
    b.run(params)                                               # the cached plan of the same profiles
    _check(b, refs, reads, _expect(refs, reads, pb, "local"), "local")
    b.set_read_profiles(None)
    b.run(params)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, pc.SC, cells=True), 0, map_ref=False)
    # two batches of one context, each with its own profiles
    b2 = ctx.upload(refs, reads).set_read_profiles(pc.ALPHABET, pa)
    b.set_read_profiles(pc.ALPHABET, pb)
    b2.run(params)
    b.run(params)
    _check(b2, refs, reads, _expect(refs, reads, pa, "local"), "local")
    _check(b, refs, reads, _expect(refs, reads, pb, "local"), "local")
    b.free()
    b2.free()


def test_lifecycle_changes_the_pipeline_and_back(ctx):
    """gap_open 0, affine as it is: the batch runs on the linear pipeline, under profiles on the affine kernels (mode 3), and with
    the profiles cleared on the linear pipeline again -- the schedule and the plan of one pipeline must not serve the other"""
    refs, reads, pa, _ = _small()
    sc = pc.SC[:3] + (0,)
    params = sw.make_params(sc[:3])
    plain = u.expect(refs, reads, sc, cells=True)
    b = ctx.upload(refs, reads).run(params)
    first = b.pipeline_mode()
    assert first != 3
    u.check(b, refs, reads, plain, 0, map_ref=False)
    for _ in range(2):
        b.set_read_profiles(pc.ALPHABET, pa).run(params)
        assert b.pipeline_mode() == 3
        _check(b, refs, reads, _expect(refs, reads, pa, "local", 0, sc), "local")
        b.set_read_profiles(None).run(params)
        assert b.pipeline_mode() == first
        u.check(b, refs, reads, plain, 0, map_ref=False)
    b.free()


def test_lifecycle_async(ctx):
    """the worker starts 50 ms after the call; the profiles are replaced after the wait"""
    refs, reads, pa, pb = _small()
    params = sw.make_params(pc.SC[:3], None, 1)
    _set(ctx, "fit", pc.SC, debug_async_delay_us=50000)
    b = ctx.upload(refs, reads).set_read_profiles(pc.ALPHABET, pa)
    b.run_async(params).wait()
    _check(b, refs, reads, _expect(refs, reads, pa, "fit", 1), "fit")
    b.set_read_profiles(pc.ALPHABET, pb)
    b.run_async(params).wait()
    _check(b, refs, reads, _expect(refs, reads, pb, "fit", 1), "fit")
    b.free()


def test_refusals_leave_the_batch_usable(ctx):
    refs, reads, pa, pb = _small()
    params = sw.make_params(pc.SC[:3])
    lib = ctx._lib
    # a pair list takes no profiles
    pl = ctx.upload_pairs(refs, reads, [(0, 0), (1, 2)])
    with pytest.raises(sw.SwmiError) as e:
        pl.set_read_profiles(pc.ALPHABET, [pa[0], pa[2]])
    assert e.value.code == ERR_UNSUPPORTED
    pl.free()
    b = _run(ctx, refs, reads, pa, "local")
    # refused when setting: the batch keeps its profiles
    flat = (C.c_int32 * (5 * sum(len(q) for q in reads)))()
    big = (C.c_int32 * len(flat))()
    big[7] = -(1 << 20) - 1
    wide = (C.c_int32 * (65 * sum(len(q) for q in reads)))()
    for alphabet, n, arr in ((b"ACGTa", 5, flat), (bytes(range(0x21, 0x21 + 65)), 65, wide), (b"ACGTN", 5, big), (None, 5, flat), (b"ACGTN", 5, None)):
        assert lib.swmi_batch_set_read_profiles(ctx._h, b._h, alphabet, n, arr) == ERR_INVALID, (alphabet, n)
    _check(b, refs, reads, _expect(refs, reads, pa, "local"), "local")           # (not even the results are dropped)
    # refused when running, before anything is launched; the message names the profile and the other value
    ctx.set_score_matrix(mx.uniform("ACGT", 5, -3))
    with pytest.raises(sw.SwmiError) as e:
        b.run(params)
    assert e.value.code == ERR_UNSUPPORTED and "profile" in str(e.value) and "matrix" in str(e.value)
    ctx.clear_score_matrix()
    for opts, word in ((dict(align_mode=2, gap_open2=-9, gap2=-1), "gap_open2 = -9"), (dict(subopt=5), "subopt = 5"),
                       (dict(subopt=-1, hits=3), "subopt = -1"), (dict(align_mode=2, extend=1, end_bonus=7), "end_bonus = 7")):
        for k, v in opts.items():
            ctx.set_option(k, v)
        with pytest.raises(sw.SwmiError) as e:
            b.run(params)
        assert e.value.code == ERR_UNSUPPORTED and "profile" in str(e.value) and word in str(e.value), (opts, str(e.value))
        for k in opts:
            ctx.set_option(k, 0)
    b.run(params)
    _check(b, refs, reads, _expect(refs, reads, pa, "local"), "local")
    b.free()
    # a read of more than 1024 bases
    rng = random.Random(5)
    long_read = u.rand(rng, 1025)
    ctx.set_option("long_reads", 1)
    bl = ctx.upload(refs, [long_read]).set_read_profiles(pc.ALPHABET, [pc.random_profile(rng, 1025)])
    with pytest.raises(sw.SwmiError) as e:
        bl.run(params)
    assert e.value.code == ERR_UNSUPPORTED and "1025" in str(e.value)
    bl.set_read_profiles(None)
    bl.run(params)
    assert bl.score(0) == gr.align_numpy(refs[0], long_read, pc.SC)[0]
    bl.free()


@pytest.mark.parametrize("name", ["local", "overlap"])
def test_payloads(ctx, name):
    """scores_only, cigar 1 and 2 (= / X compare the read's real bases), host-built strings, results copied instead of mapped"""
    refs, reads, pa, _ = _small()
    exp = _expect(refs, reads, pa, name)
    b = _run(ctx, refs, reads, pa, name, scores_only=1)
    assert [b.score(k) for k in range(6)] == [exp[(k // 3, k % 3)][0] for k in range(6)]
    b.free()
    ctx.set_option("scores_only", 0)
    for cigar in (1, 2):
        b = _run(ctx, refs, reads, pa, name, cigar=cigar, profiling=1)
        for (r, q), (score, alns, cells) in exp.items():
            pair = r * 3 + q
            assert b.score(pair) == score
            if name == "local" and score == 0:
                continue
            want = [(a[0], c[0], c[1]) + cr.cigar(a[1][0], a[1][1], cigar) for a, c in zip(alns, cells)]
            assert b.cigars(pair) == want, (cigar, r, q)
        b.free()
    ctx.set_option("cigar", 0)
    for opts in (dict(device_strings=0), dict(zero_copy=0)):
        b = _run(ctx, refs, reads, pa, name, **opts)
        _check(b, refs, reads, exp, name)
        b.free()


# 7 -- the workgroup sizes the launcher computes: min(4, 159 KiB / table) wavefronts, table = 64 r (n + 1) int32
#   configuration   table                      wavefronts   pairs   workgroups (the last one partial)
#   n8_R16          1024 x  9:  36 KiB         4            15      4
#   n9_R16          1024 x 10:  40 KiB         3            10      4
#   n15_R16         1024 x 16:  64 KiB         2            15      8
#   n31_R16         1024 x 32: 128 KiB         1             5      5
#   n64_R7           448 x 65: 114 KiB         1             5      5
#   n64_R4           256 x 65:  65 KiB         2 (narrow)   15      8
#   n64_R3           192 x 65:  49 KiB         3 (narrow)   10      4
def _waves(n, r_max, shape):
    return _capi.load().swmi_affine_profile_waves(n, r_max, shape)


@pytest.mark.parametrize("name", list(pc.MODES))
@pytest.mark.parametrize("config", list(pc.WAVE_CONFIGS))
def test_wavefronts_per_workgroup(ctx, config, name):
    """a launcher whose grid counts four wavefronts to a workgroup, or a kernel that finds its pair so, skips pairs wherever there
    are fewer: every pair of the launch is checked in full"""
    n, R, waves, shape = pc.WAVE_CONFIGS[config]
    assert _waves(n, R, shape) == waves
    alphabet, refs, reads, profiles = pc.wave_grid(config)
    for tie in (0, 1):
        b = _run(ctx, refs, reads, profiles, name, tie, alphabet=alphabet)
        _check(b, refs, reads, pc.wave_expected(config, name, tie), name)
        b.free()


def _mixed_waves(variant, reads):
    rs = [pc.rows_per_lane(len(q)) for q in reads if q]
    assert min(rs) <= 4 < max(rs)
    return _waves(pc.MIXED[variant][0], max(rs), 0), _waves(pc.MIXED[variant][0], max(rs), 1)


@pytest.mark.parametrize("name", list(pc.MODES))
def test_mixed_classes_in_one_batch(ctx, name):
    """the narrow and the wide kernel over one pair array, each with its own workgroup size and table size: 4 and 2 wavefronts
    (n = 15), 2 and 1 (n = 64).  The empty read's pairs have no alignments; the two equal reads get the results of their own
    profiles"""
    for variant in pc.MIXED:
        alphabet, refs, reads, profiles = pc.mixed_classes(variant)
        assert _mixed_waves(variant, reads) == pc.MIXED[variant][3]
        exp = pc.mixed_expected(variant, name)
        b = _run(ctx, refs, reads, profiles, name, pc.MIXED_TIE[name], alphabet=alphabet)
        assert b.timing().fill_launches == 1
        _check(b, refs, reads, exp, name)
        for r in range(len(refs)):
            empty, twin = r * len(reads) + 3, r * len(reads) + 10
            assert (b.score(empty), b.n_alignments(empty)) == (exp[(r, 3)][0], (0, 0)) and exp[(r, 3)][1] == []
            assert reads[10] == reads[11] and exp[(r, 10)][:2] != exp[(r, 11)][:2]
            assert (b.score(twin), b.score(twin + 1)) == (exp[(r, 10)][0], exp[(r, 11)][0])
        b.free()


def test_mixed_classes_chunked(ctx):
    """the n = 15 batch under max_workspace_bytes = 1 MiB: two launches, the second with reads of classes 1 to 5 only -- its wide
    sweep has 320-row tables and 4 wavefronts where the first launch's has 1024 rows and 2 (tests/test_profile_cpu.py holds the
    restated plan to that)"""
    alphabet, refs, reads, profiles = pc.mixed_classes("n15")
    tie = pc.MIXED_TIE["fit"]
    plan = pc.launches(refs, reads, pc.MIXED_CAP)
    need = 4 * sum(pc.dir_words(len(reads[q]), len(refs[r])) for ch in plan for r, q in ch)
    b = _run(ctx, refs, reads, profiles, "fit", tie, alphabet=alphabet)
    assert b.timing().fill_launches == 1 and b.timing().dir_bytes == need > pc.MIXED_CAP
    b.free()
    b = _run(ctx, refs, reads, profiles, "fit", tie, alphabet=alphabet, max_workspace_bytes=pc.MIXED_CAP)
    assert b.timing().fill_launches == len(plan) == 2 and b.timing().dir_bytes == need
    _check(b, refs, reads, pc.mixed_expected("n15", "fit"), "fit")
    b.free()


@pytest.mark.parametrize("tie", [0, 1])
def test_rerun_in_a_wide_class(ctx, tie):
    """the exact-size re-run has its own r_max, and so its own workgroup size: one pair of class 16 in a launch of its own (the wide
    sweep alone, 2 wavefronts), after a first launch over classes 1 to 16"""
    alphabet, ref, reads, profiles = pc.periodic_wide_case()
    assert (_waves(15, 16, 1), _waves(15, 16, 0)) == (2, 4)
    b = _run(ctx, [ref], reads, profiles, "local", tie, alphabet=alphabet, cell_cap=2)
    assert b.timing().rerun_pairs == 1
    for q, want in enumerate(pc.periodic_wide_expected(tie)):
        u.check_pair(b, q, want, 0, q)
    assert b.score(2) == 192 and b.n_alignments(2) == (239, 0)
    b.free()


def test_alphabet_edges(ctx):
    """row strides 2, 3, 64 and 65 of the staging loop against reads of 1, 63, 64 and 65 rows, and an alphabet above 0x7F"""
    for k, (alphabet, refs, reads, profiles) in enumerate(pc.alphabet_edges()):
        for name in ("local", "global"):
            b = _run(ctx, refs, reads, profiles, name, 0, alphabet=alphabet)
            _check(b, refs, reads, pc.edges_expected(k, name), name)
            b.free()


def test_mismatch_is_staged_per_run(ctx):
    """one batch, one set of profiles, two runs that differ in mismatch: column n of every table is the run's"""
    refs, reads, profiles = pc.mismatch_case()
    for name in ("local", "global"):
        _set(ctx, name, pc.SC)
        b = ctx.upload(refs, reads).set_read_profiles(pc.ALPHABET, profiles)
        for k in (0, 1, 0):
            assert pc.SC_MISMATCH[k][3] == pc.SC[3]
            b.run(sw.make_params(pc.SC_MISMATCH[k][:3]))
            assert b.pipeline_mode() == 3
            _check(b, refs, reads, pc.mismatch_expected(name, k), name)
        b.free()


# 8 -- the path bound takes the largest entry
def test_path_bound(ctx):
    """all entries <= 0: a local pair is degenerate.  Entries of 50 under match 1, gap -1: a 42-move path of score 60 where the bound
    read with match alone allows 2 + 2 moves (the analogue of test_matrix_gpu.py::test_path_longer_than_the_match_bound)"""
    refs, read = ["W" + "C" * 40 + "W", "xW" + "C" * 200 + "Wx"], "ab"
    for o in (0, -1):
        sc = (1, -1, -1, o)
        b = _run(ctx, refs, [read], [[[0, -1], [-2, 0]]], "local", 0, sc, "WC")
        for r, ref in enumerate(refs):
            assert b.score(r) == 0 and b.n_alignments(r) == (len(ref) * len(read), sw.PAIR_DEGENERATE)
        b.free()
        big = [[50, -1], [50, -1]]
        exp = _expect(refs, [read], [big], "local", 0, sc, "WC")
        assert exp[(0, 0)][0] == 60 + o and len(exp[(0, 0)][1][0][1][0]) == 42
        b = _run(ctx, refs, [read], [big], "local", 0, sc, "WC")
        _check(b, refs, [read], exp, "local")
        b.free()
