"""Per-read score profiles (swmi_batch_set_read_profiles) without a GPU: the two restatements of
tests/profile_reference.py against each other; the identity with a score matrix; which kernels the profile launcher gives a run (the
list AFF_PROFILE_SWEEPS of swmi_affine.hip) -- the test that fails on a library without the feature; the Python helpers; and the
condition on the grids of tests/profile_cases.py that a kernel which ignores the profile cannot meet; the wavefronts per workgroup
the profile launcher computes (swmi_affine_profile_waves) and what the recipes built on them are built for."""
import ctypes as C
import os
import random
import re

import pytest

import gotoh_reference as gr
import overlap_reference as ov
import profile_cases as pc
import profile_reference as pr
from affine_census import AffRun, dummy_matrix, load
from sparksmithwaterman_amd import matrix as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_OF = {"local": 0, "fit": 1, "global": 2, "extend": 3, "overlap": 4}      # AffRun.mode


# ---- the two restatements ----
@pytest.mark.parametrize("name", list(pc.MODES))
@pytest.mark.parametrize("tie", [0, 1])
def test_numpy_form_is_the_scalar_form(name, tie):
    """random small cases, reference bytes outside the alphabet and lower-case among them; every alignment rescored"""
    rng = random.Random(100 * tie + len(name))
    mode, extend, overlap = pc.MODES[name]
    for _ in range(60):
        m, n = rng.randint(1, 14), rng.randint(1, 16)
        alphabet = rng.choice(["AC", "ACGTN", "ACG"])
        read = "".join(rng.choice("ACgtN") for _ in range(m))
        ref = "".join(rng.choice(alphabet + alphabet.lower() + "X") for _ in range(n))
        profile = pc.random_profile(rng, m, len(alphabet), -4, 4)
        sc = (rng.randint(0, 4), rng.randint(-4, 1), rng.randint(-3, 0), rng.randint(-4, 0))
        a = pr.align_scalar(ref, read, alphabet, profile, sc, mode, extend, overlap, tie, cells=True)
        b = pr.align_numpy(ref, read, alphabet, profile, sc, mode, extend, overlap, tie, cells=True)
        assert a == b, (ref, read, alphabet, profile, sc)
        if not (mode == gr.LOCAL and a[0] == 0):
            for (begin, (ra, qa)), (i, j) in zip(a[1], a[2]):
                used = qa.replace("_", "")
                assert used == read[i - len(used):i]                    # the read side shows the real bases, with case
                assert pr.rescore(ra, qa, i, alphabet, profile, sc) == a[0], (name, ref, read)


def test_a_reference_byte_outside_the_alphabet_scores_mismatch():
    profile = [[7, -9], [7, -9]]
    for ch in "GxZ*":
        assert pr.cell_score(ch, 1, "AC", profile, -5) == -5
    assert pr.cell_score("a", 2, "AC", profile, -5) == 7 and pr.cell_score("C", 1, "AC", profile, -5) == -9
    # the read's letter scores nothing, the position does: match = 9 is never taken, and the read side shows the real bases
    for form in (pr.align_scalar, pr.align_numpy):
        assert form("AAAA", "Tg", "A", [[3], [-8]], (9, -1, -2, 0)) == (3, [(k, ("A", "T")) for k in (1, 2, 3, 4)])
        assert form("AAAA", "Tg", "A", [[3], [2]], (9, -1, -2, 0)) == (5, [(k, ("AA", "Tg")) for k in (1, 2, 3)])


# ---- the identity with a score matrix ----
@pytest.mark.parametrize("name", list(pc.MODES))
def test_profile_from_matrix_is_the_matrix(name):
    """a read inside the alphabet: the profile made of its matrix rows gives what the matrix gives (numpy forms), whatever the
    reference holds -- a reference byte outside the alphabet scores mismatch either way, as it equals no read base"""
    rng = random.Random(31 + len(name))
    mode, extend, overlap = pc.MODES[name]
    M = mx.BLOSUM62
    matrix = (M.alphabet.decode("latin-1"), M.scores)
    for tie in (0, 1):
        for _ in range(6):
            read = "".join(rng.choice(pc.PROTEIN + "ar") for _ in range(rng.randint(5, 60)))
            ref = "".join(rng.choice(pc.PROTEIN + "bzxJ1") for _ in range(rng.randint(5, 70)))
            prof = mx.profile_from_matrix(read, M, None, pc.SC_PROTEIN[1])
            got = pr.align_numpy(ref, read, M.alphabet, prof, pc.SC_PROTEIN, mode, extend, overlap, tie, cells=True)
            if overlap:
                ref_way = ov.align_numpy(ref, read, pc.SC_PROTEIN, mode, 0, False, tie, matrix, cells=True)
            else:
                ref_way = gr.align_numpy(ref, read, pc.SC_PROTEIN, mode, 0, extend, tie, matrix, cells=True)
            assert got == ref_way, (ref, read)


# ---- the kernel table ----
def _listed(macro):
    """the kernel names of the rows of a list of swmi_affine.hip, in order"""
    with open(os.path.join(ROOT, "sparksmithwaterman_amd", "csrc", "swmi_affine.hip")) as f:
        src = f.read()
    body = src[src.index("#define %s(X)" % macro):]
    rows = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*X\((sw_affine_\w+),", line)
        if not m:
            break
        rows.append(m.group(1))
    return rows


def _affrun(**kw):
    base = dict(gap_open=-5, gap_open2=0, gap2=0, mode=0, band=0, xdrop=0, adapt=0, mat=None, nn=0, cigar=0, subopt=0, hits=0, end_bonus=0)
    base.update(kw)
    return AffRun(**base)


def _profile_sweep_name(run, shape):
    lib = load()
    f = lib.swmi_affine_profile_sweep_name          # AttributeError on a library without the feature
    f.restype = C.c_char_p
    f.argtypes = [C.POINTER(AffRun), C.c_uint32]
    s = f(C.byref(run), shape)
    return s and s.decode()


def test_the_profile_launcher_names_the_ten_kernels():
    """fails on a library without the feature: it has no swmi_affine_profile_sweep_name"""
    got = []
    for name, mode in MODE_OF.items():
        for shape, wide in ((0, ""), (1, "_wide")):
            for gap_open in (0, -5):
                s = _profile_sweep_name(_affrun(mode=mode, gap_open=gap_open), shape)
                stem = "" if name == "local" else name + "_"
                assert s == "sw_affine_sweep_%sprofile%s_kernel" % (stem, wide), (name, shape)
            got.append(s)
    listed = _listed("AFF_PROFILE_SWEEPS")
    assert len(listed) == 10 and sorted(got) == sorted(listed)
    others = set(_listed("AFF_SWEEPS")) | set(_listed("AFF_OVERLAP_SWEEPS"))
    assert len(others) == 78 and not set(listed) & others
    # the options of the long shape do not count for a short sweep; the cigar payload is the walk's
    for kw in (dict(band=64), dict(mode=3, xdrop=50), dict(cigar=2)):
        assert _profile_sweep_name(_affrun(**kw), 0) is not None, kw


@pytest.mark.parametrize("refused", [dict(mode=2, gap_open2=-6, gap2=-1), dict(subopt=5), dict(subopt=-1), dict(subopt=5, hits=3), dict(hits=3),
                                     dict(mode=3, end_bonus=7), dict(mat=1), dict(mode=5)])
def test_the_profile_launcher_refuses(refused):
    kw = dict(refused)
    if kw.pop("mat", 0):
        kw.update(mat=dummy_matrix(), nn=5)
    for shape in (0, 1):
        assert _profile_sweep_name(_affrun(**kw), shape) is None, (refused, shape)


def test_the_long_shape_has_no_profile_sweep():
    for mode in MODE_OF.values():
        assert _profile_sweep_name(_affrun(mode=mode), 2) is None
        assert _profile_sweep_name(_affrun(mode=mode), 3) is None


def test_the_new_function_is_bound():
    from sparksmithwaterman_amd import _capi
    assert "swmi_batch_set_read_profiles" in [s[0] for s in _capi.SYMBOLS]
    assert _capi.load().swmi_abi_version() == 3


# ---- the Python helpers ----
def test_profile_from_matrix_rows():
    M = mx.ScoreMatrix(b"AC", ((1, -2), (-3, 4)))
    assert mx.profile_from_matrix("AcXa", M, None, -7) == [[1, -2], [-3, 4], [-7, -7], [1, -2]]
    assert mx.profile_from_matrix(b"CA", "AC", [[1, -2], [-3, 4]], 0) == [[-3, 4], [1, -2]]
    assert mx.profile_from_matrix("", M, None, 0) == []
    with pytest.raises(ValueError):
        mx.profile_from_matrix("A", "AA", [[1, 1], [1, 1]], 0)


def test_quality_profile_rows():
    def cost(q):
        return -1 if q < 10 else -4
    assert mx.quality_profile("AcN", [2, 40, 40], "ACGT", 5, cost) == [[5, -1, -1, -1], [-4, 5, -4, -4], [-4, -4, -4, -4]]
    with pytest.raises(ValueError):
        mx.quality_profile("AC", [1], "ACGT", 5, cost)
    # a mismatch at a low-quality base costs less: the alignment goes through it instead of opening a gap
    ref, read = "ACGTTGCA", "ACGATGCA"
    low = mx.quality_profile(read, [40, 40, 40, 2, 40, 40, 40, 40], "ACGT", 5, cost)
    high = mx.quality_profile(read, [40] * 8, "ACGT", 5, cost)
    sc = (5, -4, -2, -6)
    assert pr.align_scalar(ref, read, "ACGT", low, sc, gr.GLOBAL)[0] == 7 * 5 - 1
    assert pr.align_scalar(ref, read, "ACGT", high, sc, gr.GLOBAL)[0] == 7 * 5 - 4


# ---- the grids of the GPU tests ----
@pytest.mark.parametrize("R", pc.RS)
def test_class_grid_differs_from_plain_scoring(R):
    """by the reference, at least three quarters of the (pair, mode) cases of a class give a score or an alignment different from the
    same pair under match / mismatch (serial ties; the strict order changes no score): a kernel that ignores the profile cannot pass
    tests/test_profile_gpu.py.  The grid's geometry is what the docstring of tests/profile_cases.py says."""
    refs, reads, profiles = pc.grid(R)
    assert len(refs) == 3 and len(reads) == 5 and (len(refs) * len(reads)) % 4 != 0
    assert all((len(q) + 63) // 64 == R for q in reads) and len(reads[0]) == 64 * R - 3 and len({len(q) for q in reads}) == 5
    assert R != 16 or 1024 in [len(q) for q in reads]
    assert all(70 <= len(r) <= 130 for r in refs)
    for ref in refs:
        assert any(c in "XZ*xz" for c in ref) and any(c.islower() for c in ref)
    assert all(-6 <= v <= 7 for p in profiles for row in p for v in row)
    differ = total = 0
    for name in pc.MODES:
        exp = pc.expected(R, name, 0)
        for (r, q), e in exp.items():
            total += 1
            differ += e[:2] != pc.plain(refs[r], reads[q], name, 0)[:2]
    assert total == 75 and 4 * differ >= 3 * total, (R, differ, total)


# ---- the workgroup sizes of the profile launcher ----
def _waves(n, r_max, shape):
    from sparksmithwaterman_amd import _capi
    return _capi.load().swmi_affine_profile_waves(n, r_max, shape)     # AttributeError on a library without the function


def test_profile_waves_is_bound():
    from sparksmithwaterman_amd import _capi
    assert ("swmi_affine_profile_waves", C.c_uint32, [C.c_uint32] * 3) in _capi.LAUNCH_SYMBOLS
    assert "swmi_affine_profile_waves" not in [s[0] for s in _capi.SYMBOLS]         # (include/swmi.h does not declare it)


def test_profile_waves_table():
    """the seven configurations of tests/profile_cases.py: 4, 3, 2, 1, 1, 2, 3 wavefronts per workgroup"""
    assert [c[2] for c in pc.WAVE_CONFIGS.values()] == [4, 3, 2, 1, 1, 2, 3]
    for name, (n, R, waves, shape) in pc.WAVE_CONFIGS.items():
        assert _waves(n, R, shape) == waves, name
        assert (shape == 0) == (R <= 4), name


def test_profile_waves_bounds():
    """0 where one table does not fit SWMI_PROF_LDS_WORDS = 32768 dwords (what check_run_params refuses), and for arguments the
    launcher refuses; the narrow sweep's table has at most 256 rows whatever the launch's longest read"""
    for n, R, fits in ((31, 16, True), (32, 16, False), (64, 7, True), (64, 8, False), (64, 16, False), (1, 16, True)):
        assert (_waves(n, R, 1) > 0) == fits == (64 * R * (n + 1) <= 32768), (n, R)
    for n in (1, 15, 64):
        assert [_waves(n, R, 0) for R in range(4, 17)] == [_waves(n, 4, 0)] * 13
    assert _waves(0, 4, 0) == _waves(65, 4, 0) == _waves(5, 0, 0) == _waves(5, 17, 1) == _waves(5, 4, 2) == 0
    # every admitted size: as many tables as fit 159 KiB, at most four
    for n in range(1, 65):
        for R in range(1, 17):
            table = 64 * R * (n + 1) * 4
            assert _waves(n, R, 1) == (min(4, (159 << 10) // table) if table <= 32768 * 4 else 0), (n, R)


@pytest.mark.parametrize("config", list(pc.WAVE_CONFIGS))
def test_wave_grid_geometry(config):
    """the five lengths of the class, references of 50 to 70 bases over the whole alphabet with bytes outside it and lower-case
    letters, and a pair count that is no multiple of the wavefronts of a workgroup and at least twice them"""
    n, R, waves, _ = pc.WAVE_CONFIGS[config]
    alphabet, refs, reads, profiles = pc.wave_grid(config)
    assert (alphabet, R) == pc.wave_config(config) and len(alphabet) == n == len({gr.upper(c) for c in alphabet})
    assert [len(q) for q in reads] == pc.class_lengths(R) == [len(p) for p in profiles] and len(reads[0]) == 64 * R - 3
    assert R != 16 or 1024 in [len(q) for q in reads]
    assert all(len(row) == n for p in profiles for row in p)
    pairs = len(refs) * len(reads)
    assert pairs % waves != 0 or waves == 1
    assert pairs >= 2 * waves and pairs >= 5
    for ref in refs:
        assert 50 <= len(ref) <= 70
        assert any(pc.is_outside(c, alphabet) for c in ref) and any(c.islower() for c in ref)
    used = {gr.upper(c) for ref in refs for c in ref if not pc.is_outside(c, alphabet)}
    assert len(used) >= min(n, 8) and not used <= set(pc.ALPHABET)           # columns beyond ACGTN's five are read


def test_wave_grid_differs_from_plain_scoring():
    """the profile decides: every pair of the one-wavefront configuration scores differently under match / mismatch"""
    alphabet, refs, reads, profiles = pc.wave_grid("n64_R7")
    exp = pc.wave_expected("n64_R7", "local", 0)
    assert all(exp[(0, q)][:2] != pc.plain(refs[0], reads[q], "local", 0)[:2] for q in range(5))


@pytest.mark.parametrize("variant", list(pc.MIXED))
def test_mixed_classes_need_both_kernels(variant):
    n, lengths, ref_lengths, (narrow, wide) = pc.MIXED[variant]
    alphabet, refs, reads, profiles = pc.mixed_classes(variant)
    assert len(alphabet) == n and len(refs) == 3 and [len(r) for r in refs] == list(ref_lengths)
    assert [len(q) for q in reads] == list(lengths) + [pc.MIXED_TWIN] * 2 == [len(p) for p in profiles]
    assert lengths[:8] == (1, 64, 65, 0, 256, 257, 300, 130) and sorted(lengths) != list(lengths)
    rs = [pc.rows_per_lane(m) for m in lengths if m]
    r_min, r_max = min(rs), max(rs)
    assert r_min <= 4 < r_max
    assert (_waves(n, r_max, 0), _waves(n, r_max, 1)) == (narrow, wide) == {"n15": (4, 2), "n64": (2, 1)}[variant]
    # the two equal reads carry different profiles, and the difference shows
    assert reads[10] == reads[11] and profiles[10] != profiles[11]
    exp = pc.mixed_expected(variant, "local")
    assert all(exp[(r, 10)][:2] != exp[(r, 11)][:2] for r in range(3))
    # the empty read: no alignments in any mode
    for name in pc.MODES:
        assert all(pc.mixed_expected(variant, name)[(r, 3)] == (0, [], []) for r in range(3)), name
    assert set(pc.MIXED_TIE) == set(pc.MODES) and set(pc.MIXED_TIE.values()) == {0, 1}
    for ref in refs:
        assert any(pc.is_outside(c, alphabet) for c in ref) and any(c.islower() for c in ref)


def test_mixed_classes_chunk_with_another_r_max():
    """under MIXED_CAP the n = 15 batch takes two launches, and the second has reads of classes 1 to 5 only: its wide sweep gets
    320-row tables and 4 wavefronts where the whole batch's gets 1024 rows and 2"""
    alphabet, refs, reads, _ = pc.mixed_classes("n15")
    plan = pc.launches(refs, reads, pc.MIXED_CAP)
    assert [len(ch) for ch in plan] == [24, 9] and sum(len(ch) for ch in plan) == 3 * 11
    r_max = [max(pc.rows_per_lane(len(reads[q])) for _, q in ch) for ch in plan]
    r_min = [min(pc.rows_per_lane(len(reads[q])) for _, q in ch) for ch in plan]
    assert r_max == [16, 5] and r_min == [1, 1]
    assert [_waves(15, r, 1) for r in r_max] == [2, 4]
    assert pc.launches(refs, reads, 1 << 40) == [[p for ch in plan for p in ch]]
    # dir_words is swmi_aff_pair_dir_words: 1024 x 60 is 16 blocks of 16 x 64 dwords, 1 x 1 one block of 64
    assert pc.dir_words(1024, 60) == 16 * 1024 and pc.dir_words(1, 1) == 64 and pc.dir_words(65, 10) == (10 + 33 - 1 + 7) // 8 * 128


def test_periodic_wide_case():
    """score 192 in 239 tied maximum cells, in both tie modes; the four other pairs stay within cell_cap = 2"""
    alphabet, ref, reads, profiles = pc.periodic_wide_case()
    assert alphabet == pc.alphabet_of(15) and ref == "ACGT" * 12 and reads[2] == "ACGT" * 250
    assert [pc.rows_per_lane(len(q)) for q in reads] == [1, 2, 16, 3, 3]
    for tie in (0, 1):
        score, alns, cells = pc.want(ref, reads[2], profiles[2], "local", tie, pc.SC, alphabet)
        assert score == 192 and len(cells) == len(alns) == 239
        for q in (0, 1, 3, 4):
            other = pc.want(ref, reads[q], profiles[q], "local", tie, pc.SC, alphabet)
            assert other[0] > 0 and 1 <= len(other[2]) <= 2, q
    assert (_waves(15, 16, 1), _waves(15, 3, 0)) == (2, 4)


def test_alphabet_edges():
    """the two restatements agree on every pair; the row strides are 2, 3, 64, 65 and 7; both cases of e-acute reach its column"""
    cases = pc.alphabet_edges()
    assert [len(c[0]) + 1 for c in cases] == [2, 3, 64, 65, 7]
    for alphabet, refs, reads, profiles in cases:
        assert tuple(len(q) for q in reads) == pc.EDGE_READS == (1, 63, 64, 65)
        assert len({gr.upper(c) for c in alphabet}) == len(alphabet)
        for name in ("local", "global"):
            mode, extend, overlap = pc.MODES[name]
            for r, ref in enumerate(refs):
                for q, read in enumerate(reads):
                    a = pr.align_scalar(ref, read, alphabet, profiles[q], pc.SC, mode, extend, overlap, 0, cells=True)
                    assert a == pc.want(ref, read, profiles[q], name, 0, pc.SC, alphabet), (alphabet, name, r, q)
    alphabet, refs, reads, profiles = cases[-1]
    assert alphabet == "AC\xe9\xff\xf7\xd7"
    for ref in refs:
        assert all(c in ref for c in "\xc9\xe9\xff\xdf\xb5\xf7\xd7")
    assert [pc.is_outside(c, alphabet) for c in "\xc9\xe9\xff\xdf\xb5\xf7\xd7"] == [False, False, False, True, True, False, False]
    cls = pr._classes(alphabet)
    assert cls[0xC9] == cls[0xE9] == 2 and cls[0xFF] == 3 and cls[0xF7] == 4 and cls[0xD7] == 5 and cls[0xDF] == cls[0xB5] == -1
    # e-acute's column changed: a score changes; and with the upper-case bytes taken out of the reference it changes in another way
    q = 3
    bumped = [row[:2] + [row[2] + 40] + row[3:] for row in profiles[q]]
    base = [pc.want(ref, reads[q], profiles[q], "local", 0, pc.SC, alphabet)[0] for ref in refs]
    moved = [pc.want(ref, reads[q], bumped, "local", 0, pc.SC, alphabet)[0] for ref in refs]
    lower_only = [pc.want(ref.replace("\xc9", "\xdf"), reads[q], bumped, "local", 0, pc.SC, alphabet)[0] for ref in refs]
    assert moved != base and lower_only != moved


def test_mismatch_case_depends_on_mismatch():
    refs, reads, profiles = pc.mismatch_case()
    assert all(any(pc.is_outside(c, pc.ALPHABET) for c in ref) for ref in refs)
    assert pc.SC_MISMATCH[0][1] != pc.SC_MISMATCH[1][1] and pc.SC_MISMATCH[0][::2] == pc.SC_MISMATCH[1][::2]
    for name in ("local", "global"):
        a, b = ({(r, q): pc.want(refs[r], reads[q], profiles[q], name, 0, sc) for r in range(2) for q in range(3)} for sc in pc.SC_MISMATCH)
        assert sum(a[k][0] != b[k][0] for k in a) >= 3, name     # half the scores or more differ
    assert {pc.rows_per_lane(len(q)) for q in reads} == {1, 2, 5}       # the narrow and the wide sweep


def test_protein_pairs_and_the_periodic_case():
    refs, reads = pc.protein_pairs()
    assert len(refs) == len(reads) == 6 and all(40 <= len(s) <= 300 for s in refs + reads)
    assert {(len(q) + 63) // 64 for q in reads} == {1, 2, 3, 4, 5}          # narrow and wide sweeps
    ref, read, profile = pc.periodic_case()
    score, alns, cells = pc.want(ref, read, profile, "local", 0)
    assert score == 48 and len(cells) == 10 > 2
