"""Option "subopt" without a GPU (include/swmi.h): the restatement of tests/subopt_reference.py -- its numpy form
held to its scalar form, the mask's strict '>', AUTO, the degenerate and empty pairs, the smallest column on a tie -- and the
boundary: the library exports the two accessors, _capi declares them, aligner.Batch has subopt / subopts."""
import random

import pytest

from sparksmithwaterman_amd import _capi, aligner

import affine_grid_cases as gc
import subopt_reference as sr

SC = (5, -3, -4, -5)          # match, mismatch, gap, gap_open
LIN = (5, -3, -4, 0)
BLOSUM_LIKE = ("ARNDC", [[4, -1, -2, -2, 0], [-1, 5, 0, -2, -3], [-2, 0, 6, 1, -3], [-2, -2, 1, 6, -3], [0, -3, -3, -3, 9]])


def rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def weaken(read, k, alphabet="ACGT"):
    """the read with k substitutions at evenly spaced places (each base replaced by the next one of the alphabet)"""
    out = list(read)
    for x in range(k):
        p = (2 * x + 1) * len(read) // (2 * k)
        out[p] = alphabet[(alphabet.index(out[p]) + 1) % len(alphabet)]
    return "".join(out)


def planted(rng, read, gaps, loads, alphabet="ACGT"):
    """a reference of random stretches (lengths `gaps`, one more than copies) around copies of the read with `loads` substitutions
    each; returns it and the 1-based end column of every copy"""
    ref, ends = rand(rng, gaps[0], alphabet), []
    for g, load in zip(gaps[1:], loads):
        ref += weaken(read, load, alphabet)
        ends.append(len(ref))
        ref += rand(rng, g, alphabet)
    return ref, ends


def both(ref, read, sc, w, band=0, matrix=None, strip=1024):
    a = sr.subopt_scalar(ref, read, sc, w, band, 0, matrix, strip)
    b = sr.subopt_numpy(ref, read, sc, w, band, matrix, strip)
    assert a == b, (a, b, len(ref), len(read), w, band, strip)
    assert 0 <= a[1] < a[0] or a[:2] == (0, 0)
    assert (a[2] == 0) == (a[1] == 0)
    return a


@pytest.mark.parametrize("seed", range(6))
def test_numpy_form_is_the_scalar_form_random(seed):
    rng = random.Random(100 + seed)
    for _ in range(6):
        m, n = rng.randint(1, 40), rng.randint(1, 90)
        ref, read = rand(rng, n), rand(rng, m)
        for w in (1, 3, 15, sr.AUTO):
            both(ref, read, rng.choice((SC, LIN)), w)


def test_numpy_form_is_the_scalar_form_planted():
    rng = random.Random(7)
    read = rand(rng, 30)
    ref, ends = planted(rng, read, (20, 25, 30, 10), (0, 2, 4))
    for w in (1, 10, 29, 30, 54, 55, 56, 200):
        s, s2, e2 = both(ref, read, SC, w)
        assert s == 150


def test_numpy_form_is_the_scalar_form_staircase_and_matrix():
    rng = random.Random(11)
    for _ in range(4):
        m, n = rng.randint(17, 40), rng.randint(30, 70)
        read = rand(rng, m)
        ref = rand(rng, 5) + gc.mutate(rng, read, "ACGT", 0.1, 0.02) + rand(rng, max(0, n - m - 5))
        for band in (0, 4, 9):
            if not any(lo > hi for lo, hi in sr.gr.windows(m, len(ref), band, 8)):
                both(ref, read, SC, 3, band, None, 8)
    read = rand(rng, 20, "ARNDC")
    ref, _ = planted(rng, read, (10, 15, 10), (0, 3), "ARNDC")
    both(ref, read, (1, -1, -1, -3), 5, 0, BLOSUM_LIKE)


def test_mask_is_strict_on_both_sides():
    # two exact maximum columns at 10 and 30; everything else is weaker
    colmax = [0] * 41
    colmax[10] = colmax[30] = 9
    colmax[4], colmax[16], colmax[24], colmax[36] = 5, 6, 7, 8
    assert sr.reduce_colmax(colmax, 9, 5) == (8, 36)         # |36 - 30| = 6 > 5, and 16 / 24 are 6 away from a maximum column
    assert sr.reduce_colmax(colmax, 9, 6) == (0, 0)          # 6 > 6 fails on both sides of both
    colmax[3] = 4
    assert sr.reduce_colmax(colmax, 9, 6) == (4, 3)          # |3 - 10| = 7 > 6
    # the same through the whole pipeline: the second copy d columns behind the first
    rng = random.Random(3)
    read = rand(rng, 24)
    ref, ends = planted(rng, read, (12, 16, 12), (0, 2))
    d = ends[1] - ends[0]
    s, s2, e2 = both(ref, read, SC, d - 1)
    assert (s, e2) == (120, ends[1]) and s2 > 60
    s, s2b, e2b = both(ref, read, SC, d)
    assert s2b < s2 and e2b != ends[1]
    # ... and with the weaker copy on the left
    ref, ends = planted(rng, read, (12, 16, 12), (2, 0))
    d = ends[1] - ends[0]
    assert both(ref, read, SC, d - 1)[2] == ends[0]
    assert both(ref, read, SC, d)[2] != ends[0]


@pytest.mark.parametrize("m,w", [(20, 15), (30, 15), (31, 15), (100, 50)])
def test_auto_is_ssw_mask_len(m, w):
    assert sr.mask_width(sr.AUTO, m) == w
    rng = random.Random(m)
    read = rand(rng, m)
    ref, _ = planted(rng, read, (8, w + 3, 8), (0, 2))
    assert both(ref, read, SC, sr.AUTO) == both(ref, read, SC, w)


def test_degenerate_and_empty_pairs():
    assert both("CCCC", "AAAA", SC, 1) == (0, 0, 0)
    assert both("", "ACGT", SC, 1) == (0, 0, 0)
    assert both("ACGT", "", SC, sr.AUTO) == (0, 0, 0)
    assert both("ACGT", "ACGT", SC, 1 << 30) == (20, 0, 0)     # one maximum column, every other one masked


def test_end2_is_the_smallest_column_on_a_tie():
    rng = random.Random(5)
    read = rand(rng, 20)
    weak = read[:10] + ("A" if read[10] != "A" else "C") + read[11:]          # one substitution: both weak copies score the same
    ref = rand(rng, 10) + weak + rand(rng, 15) + read + rand(rng, 15) + weak + rand(rng, 10)
    s, s2, e2 = both(ref, read, SC, 20)
    assert (s, s2, e2) == (100, 92, 30)
    colmax = [0, 1, 7, 3, 7, 9, 2]
    assert sr.reduce_colmax(colmax, 9, 1) == (7, 2)


def test_library_exports_and_bindings():
    lib = _capi.load()
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name in ("swmi_pair_subopt", "swmi_batch_pair_subopt"):
        assert getattr(lib, name) is not None
        assert name in bound and len(bound[name][1]) == 4
    assert _capi.SUBOPT_AUTO == -1 == sr.AUTO
    assert callable(aligner.Batch.subopt) and callable(aligner.Batch.subopts)
