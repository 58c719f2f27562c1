"""Per-read score profiles (swmi_batch_set_read_profiles) without a GPU: the two restatements of
tests/profile_reference.py against each other; the identity with a score matrix; which kernels the profile launcher gives a run (the
list AFF_PROFILE_SWEEPS of swmi_affine.hip) -- the test that fails on a library without the feature; the Python helpers; and the
condition on the grids of tests/profile_cases.py that a kernel which ignores the profile cannot meet."""
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


def test_protein_pairs_and_the_periodic_case():
    refs, reads = pc.protein_pairs()
    assert len(refs) == len(reads) == 6 and all(40 <= len(s) <= 300 for s in refs + reads)
    assert {(len(q) + 63) // 64 for q in reads} == {1, 2, 3, 4, 5}          # narrow and wide sweeps
    ref, read, profile = pc.periodic_case()
    score, alns, cells = pc.want(ref, read, profile, "local", 0)
    assert score == 48 and len(cells) == 10 > 2
