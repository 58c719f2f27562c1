"""Option "end_bonus" without a GPU (include/swmi.h): the restatement of tests/end_bonus_reference.py -- its
numpy form held to its scalar form, end_score as the best global score over the prefixes of the reference, the to-end alignment as
the global alignment of that prefix, the strict choice, the smallest column on a tie, the empty sides -- and the boundary: the
library exports the two accessors, _capi declares them, the bindings have their entry points."""
import os
import random

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi, aligner

import end_bonus_reference as er
import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = (5, -4, -3, -5)          # match, mismatch, gap, gap_open
TIE = (5, -3, -3, -5)
BLOSUM_LIKE = ("ARNDC", [[4, -1, -2, -2, 0], [-1, 5, 0, -2, -3], [-2, 0, 6, 1, -3], [-2, -2, 1, 6, -3], [0, -3, -3, -3, 9]])


def rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def both(ref, read, sc, b, w=0, tie=0, matrix=None, strip=1024):
    a = er.align_scalar(ref, read, sc, b, w, tie, matrix, strip)
    c = er.align(ref, read, sc, b, w, tie, matrix, strip)
    assert a == c, (a, c, len(ref), len(read), b, w, tie, strip)
    score, alns, cells, took, (mx, es, ec) = a
    if ref and read:
        assert es <= mx and score == (es if took else mx)
        assert took == (b > 0 and es + b > mx)
        if took:
            assert cells == [(len(read), ec)] and len(alns) == 1 and alns[0][0] == 1
            assert alns[0][1][0].replace(gr.GAP_CHAR, "") == ref[:ec] and alns[0][1][1].replace(gr.GAP_CHAR, "") == read
            assert gr.rescore(alns[0][1][0], alns[0][1][1], sc, matrix) == es
    return a


@pytest.mark.parametrize("seed", range(6))
def test_numpy_form_is_the_scalar_form_random(seed):
    rng = random.Random(300 + seed)
    for _ in range(5):
        m, n = rng.randint(1, 30), rng.randint(1, 60)
        read = rand(rng, m)
        ref = rng.choice((rand(rng, n), read[:m - 1] + rand(rng, n)))
        for b in (0, 1, 7, 1 << 30):
            both(ref, read, rng.choice((SC, TIE)), b, tie=seed & 1)


@pytest.mark.parametrize("m,n,w", [(17, 30, 3), (24, 24, 2), (33, 60, 5), (9, 40, 2)])
def test_numpy_form_is_the_scalar_form_banded_staircase(m, n, w):
    """strips of 8 rows: row m is read over the last strip's window only"""
    rng = random.Random(m * 100 + n)
    read = rand(rng, m)
    ref = (read[:m // 2] + rand(rng, 2) + read[m // 2:] + rand(rng, n))[:n]
    lo, hi = gr.windows(m, n, w, 8)[-1]
    for tie in (0, 1):
        for b in (1, 12, 1 << 30):
            a = both(ref, read, SC, b, w, tie, strip=8)
            assert lo <= a[4][2] <= hi
    free = both(ref, read, SC, 1 << 30, 0, 0, strip=8)
    assert free[3] and both(ref, read, SC, 1 << 30, w, 0, strip=8)[3]


def test_numpy_form_is_the_scalar_form_matrix():
    rng = random.Random(17)
    for _ in range(6):
        read = rand(rng, rng.randint(2, 25), "ARNDC")
        ref = read[:len(read) - 2] + rand(rng, rng.randint(1, 30), "ARNDCX")
        for b in (1, 9):
            both(ref, read, (1, -1, -1, -4), b, matrix=BLOSUM_LIKE)


@pytest.mark.parametrize("seed", range(4))
def test_end_score_is_the_best_global_score_over_the_reference_prefixes(seed):
    rng = random.Random(400 + seed)
    read = rand(rng, rng.randint(3, 20))
    ref = read[:len(read) // 2] + rand(rng, 1) + read[len(read) // 2:] + rand(rng, 12)
    glob = [gr.align_scalar(ref[:j], read, SC, gr.GLOBAL)[0] for j in range(1, len(ref) + 1)]
    _, _, _, _, (mx, es, ec) = both(ref, read, SC, 1)
    assert es == max(glob) and ec == 1 + glob.index(es)
    assert mx == gr.align_scalar(ref, read, SC, gr.GLOBAL, extend=True)[0]


@pytest.mark.parametrize("tie", [0, 1])
def test_to_end_alignment_is_the_global_alignment_of_the_prefix(tie):
    rng = random.Random(500 + tie)
    for _ in range(8):
        read = rand(rng, rng.randint(2, 24))
        ref = (read[:len(read) - 3] + rand(rng, 20))[:rng.randint(1, 40)]
        score, alns, cells, took, (mx, es, ec) = both(ref, read, SC, 1 << 30, tie=tie)
        assert took
        assert (score, alns) == gr.align_scalar(ref[:ec], read, SC, gr.GLOBAL, tie_mode=tie)


def test_choice_is_strict():
    """the read is a prefix of the reference with its last base substituted: the best cell is (m - 1, m - 1), row m is 4 worse"""
    rng = random.Random(600)
    ref = rand(rng, 40)
    m = 25
    read = ref[:m - 1] + next(c for c in "ACGT" if c not in ref[m - 1:m + 2])     # (nor does it match behind a short deletion)
    off = both(ref, read, SC, 0)
    assert not off[3] and off[0] == 5 * (m - 1) and off[2] == [(m - 1, m - 1)] and off[4] == (5 * (m - 1), 5 * (m - 1) - 4, m)
    assert off[:3] == gr.align_scalar(ref, read, SC, gr.GLOBAL, extend=True, cells=True)
    at = both(ref, read, SC, 4)                       # end_score + 4 == max_score: not taken, and everything as without the option
    assert not at[3] and at[:3] == off[:3] and at[4] == off[4]
    over = both(ref, read, SC, 5)
    assert over[3] and over[0] == 5 * (m - 1) - 4 and over[2] == [(m, m)] and over[4] == off[4]
    assert er.taken(10, 6, 4) is False and er.taken(10, 6, 5) is True and er.taken(10, 10, 0) is False


@pytest.mark.parametrize("tie", [0, 1])
def test_end_col_is_the_smallest_column_on_a_tie(tie):
    """P + "T" against P + "GT" + tail: a mismatch at column m and a one-base deletion to column m + 1 both cost 3"""
    rng = random.Random(610)
    P = rand(rng, 19)
    read, ref = P + "T", P + "GT" + rand(rng, 10)
    m = len(read)
    H = gr.align_scalar(ref, read, TIE, gr.GLOBAL, extend=True, tie_mode=tie, matrices=True)[2]
    assert H[m][m] == H[m][m + 1] == 5 * (m - 1) - 3 == max(H[m][1:])
    a = both(ref, read, TIE, 4, tie=tie)
    assert a[3] and a[4] == (5 * (m - 1), 5 * (m - 1) - 3, m) and a[2] == [(m, m)]


def test_empty_sides():
    for ref, read in (("", "ACGT"), ("ACGT", ""), ("", "")):
        for b in (0, 3):
            assert both(ref, read, SC, b) == er.EMPTY == (0, [], [], False, (0, 0, 0))


def test_end_score_may_be_negative():
    a = both("CCCCCC", "AAAA", SC, 1 << 30)
    assert a[3] and a[0] == a[4][1] < 0 and a[4][0] == -4


def test_library_exports_and_bindings():
    lib = _capi.load()
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name, nargs in (("swmi_pair_end_score", 5), ("swmi_batch_pair_end_scores", 5)):
        assert getattr(lib, name) is not None
        assert name in bound and len(bound[name][1]) == nargs
    assert sw.PAIR_TO_END == _capi.PAIR_TO_END == 0x2 and sw.PAIR_DEGENERATE == 0x1
    assert _capi.END_BONUS_MAX == 1 << 30
    assert callable(aligner.Batch.end_score) and callable(aligner.Batch.end_scores)
    header = open(os.path.join(ROOT, "include", "swmi.h")).read()
    assert "#define SWMI_PAIR_TO_END     0x2u" in header and "#define SWMI_PAIR_DEGENERATE 0x1u" in header
    assert "#define SWMI_ABI_VERSION" in header
    shim = open(os.path.join(ROOT, "bindings", "jni", "swmi_shim.h")).read()
    assert "swmi_shim_set_end_bonus(" in shim and "swmi_shim_pair_end_score(" in shim
    jni = open(os.path.join(ROOT, "bindings", "jni", "swmi_jni.c")).read()
    assert "Java_sw_GpuSmithWaterman_nativeSetEndBonus" in jni and "Java_sw_GpuSmithWaterman_nativePairEndScore" in jni
    java = open(os.path.join(ROOT, "bindings", "java", "sw", "GpuSmithWaterman.java")).read()
    for name in ("nativeSetEndBonus", "nativePairEndScore", "setEndBonus", "endScore"):
        assert name in java, name


def test_mirror_classes_and_driver_take_the_option():
    import inspect
    from sparksmithwaterman_amd import sharded_files
    from sparksmithwaterman_amd import sw as mirror
    for cls in (mirror.SmithWaterman.OptAlignments, mirror.Distribution.MapPartition, mirror.Distribution.MapRef):
        assert "end_bonus" in inspect.signature(cls.__init__).parameters, cls
    ap = sharded_files._parser()
    common = ["--ref-dir", "r", "--in-dir", "i", "--out-dir", "o"]
    ns = ap.parse_args(common + ["--scores", "5,-4,-3,-5", "--align-mode", "global", "--extend", "--end-bonus", "7"])
    assert ns.end_bonus == 7
    for bad in (["--end-bonus", "7"], ["--align-mode", "global", "--extend", "--end-bonus", "-1"],
                ["--align-mode", "global", "--extend", "--long-reads", "--xdrop", "50", "--end-bonus", "7"]):
        with pytest.raises(SystemExit):
            ap.parse_args(common + bad)
