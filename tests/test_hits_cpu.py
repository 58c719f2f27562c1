"""Option "hits" without a GPU (include/swmi.h): the restatement of tests/hits_reference.py -- its numpy form
held to its scalar form (banded staircases of 8-row strips and a score matrix included), entry 1 against subopt_reference, the
smallest row and the smallest column on ties, the end of the list at the first 0, K = 1, the degenerate and empty pairs, the
reverse-extension property that makes the cells worth having -- and the boundary: the library exports the two accessors and the
shim's two functions exist, _capi declares the struct and the prototypes, aligner.Batch has hits / hits_all / hit_specs."""
import os
import random

import pytest

from sparksmithwaterman_amd import _capi, aligner

import affine_grid_cases as gc
import gotoh_reference as gr
import hits_reference as hr
import subopt_reference as sr

SC = (5, -3, -4, -5)          # match, mismatch, gap, gap_open
LIN = (5, -3, -4, 0)
BLOSUM_LIKE = ("ARNDC", [[4, -1, -2, -2, 0], [-1, 5, 0, -2, -3], [-2, 0, 6, 1, -3], [-2, -2, 1, 6, -3], [0, -3, -3, -3, 9]])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ref, ends = rand(rng, gaps[0], alphabet), []
    for g, load in zip(gaps[1:], loads):
        ref += weaken(read, load, alphabet)
        ends.append(len(ref))
        ref += rand(rng, g, alphabet)
    return ref, ends


def both(ref, read, sc, w, k, band=0, matrix=None, strip=1024):
    """the two forms agree; the list has the properties the contract names; entry 1 is subopt's pair"""
    a = hr.hits_scalar(ref, read, sc, w, k, band, 0, matrix, strip)
    b = hr.hits_numpy(ref, read, sc, w, k, band, matrix, strip)
    assert a == b, (a, b, len(ref), len(read), w, k, band, strip)
    s, s2, e2 = sr.subopt_scalar(ref, read, sc, w, band, 0, matrix, strip)
    assert len(a) <= k and (len(a) == 0) == (s == 0)
    if a:
        assert a[0][0] == s
        assert all(1 <= i <= len(read) and 1 <= j <= len(ref) and v > 0 for v, i, j in a)
        assert all(x[0] >= y[0] for x, y in zip(a[1:], a[2:]))
        wd = sr.mask_width(w, len(read))
        cols = [j for _, _, j in a]
        assert all(abs(x - y) > wd for n, x in enumerate(cols) for y in cols[n + 1:])
    if k >= 2 and s > 0:
        assert (a[1][0], a[1][2]) == (s2, e2) if s2 else len(a) == 1
    return a


@pytest.mark.parametrize("seed", range(6))
def test_numpy_form_is_the_scalar_form_random(seed):
    rng = random.Random(300 + seed)
    for _ in range(6):
        m, n = rng.randint(1, 40), rng.randint(1, 90)
        ref, read = rand(rng, n), rand(rng, m)
        for w, k in ((1, 16), (3, 4), (15, 2), (sr.AUTO, 16)):
            both(ref, read, rng.choice((SC, LIN)), w, k)


def test_numpy_form_is_the_scalar_form_staircase_and_matrix():
    rng = random.Random(311)
    done = 0
    for _ in range(4):
        m, n = rng.randint(17, 40), rng.randint(30, 70)
        read = rand(rng, m)
        ref = rand(rng, 5) + gc.mutate(rng, read, "ACGT", 0.1, 0.02) + rand(rng, max(0, n - m - 5))
        for band in (0, 4, 9):
            if not any(lo > hi for lo, hi in gr.windows(m, len(ref), band, 8)):
                both(ref, read, SC, 3, 16, band, None, 8)
                done += band > 0
    assert done
    read = rand(rng, 20, "ARNDC")
    ref, _ = planted(rng, read, (10, 15, 10, 10), (0, 3, 5), "ARNDC")
    assert len(both(ref, read, (1, -1, -1, -3), 5, 8, 0, BLOSUM_LIKE)) >= 3


def test_three_copies_in_order_and_k():
    rng = random.Random(312)
    read = rand(rng, 30)
    ref, ends = planted(rng, read, (20, 25, 30, 10), (2, 0, 4))
    full = both(ref, read, SC, 20, 16)
    assert [(v, j) for v, _, j in full[:3]] == [(150, ends[1]), (134, ends[0]), (118, ends[2])]
    assert [i for _, i, _ in full[:3]] == [30, 30, 30]
    for k in (1, 2, 3):
        assert both(ref, read, SC, 20, k) == full[:k]


def test_smallest_row_and_smallest_column_on_ties():
    # A x m against A: every row of column 1 holds the maximum
    assert both("A", "AAAAA", SC, 1, 4) == [(5, 1, 1)]
    # GAG against a read with A at rows 3, 4 and 7: column 1 (G) is 0, columns 2's maximum 5 is held by three rows
    assert both("CAC", "CCAACCA", SC, 1, 4)[0][0] == 10
    h = both("TAT", "CCAACCA", SC, 1, 4)
    assert h == [(5, 3, 2)]
    # two equally weak copies around the exact one: the smaller column first, then the other
    rng = random.Random(313)
    read = rand(rng, 20)
    weak = read[:10] + ("A" if read[10] != "A" else "C") + read[11:]
    ref = rand(rng, 10) + weak + rand(rng, 15) + read + rand(rng, 15) + weak + rand(rng, 10)
    h = both(ref, read, SC, 20, 3)
    assert h == [(100, 20, 65), (92, 20, 30), (92, 20, 100)]


def test_the_list_ends_at_the_first_zero():
    colmax = [0, 0, 3, 0, 0, 9, 0, 0, 4, 0, 0]
    rows = [0, 0, 2, 0, 0, 1, 0, 0, 5, 0, 0]
    assert hr.pick(colmax, rows, 9, 1, 16) == [(9, 1, 5), (4, 5, 8), (3, 2, 2)]
    assert hr.pick(colmax, rows, 9, 2, 16) == [(9, 1, 5), (4, 5, 8), (3, 2, 2)]
    assert hr.pick(colmax, rows, 9, 3, 16) == [(9, 1, 5)]              # |8 - 5| = 3 > 3 fails on both sides
    assert hr.pick(colmax, rows, 9, 1, 2) == [(9, 1, 5), (4, 5, 8)]
    # a neighbour within w of an earlier hit is skipped, one at distance w + 1 is taken
    colmax = [0, 9, 0, 0, 0, 0, 7, 0, 6, 5, 0]
    rows = [0] + [1] * 10
    assert hr.pick(colmax, rows, 9, 2, 16) == [(9, 1, 1), (7, 1, 6), (5, 1, 9)]


def test_degenerate_and_empty_pairs():
    assert both("CCCC", "AAAA", SC, 1, 16) == []
    assert both("", "ACGT", SC, 1, 16) == []
    assert both("ACGT", "", SC, sr.AUTO, 16) == []
    assert both("ACGT", "ACGT", SC, 1 << 30, 16) == [(20, 4, 4)]


@pytest.mark.parametrize("seed", range(4))
def test_reverse_extension_finds_every_hit(seed):
    """with gap_open + gap < 0: the extend score of the reversed prefixes that end in a hit's cell is the hit's score -- the best
    local alignment that ends in (i, j) is the best extension backwards from it"""
    rng = random.Random(320 + seed)
    read = rand(rng, rng.randint(20, 35))
    ref, _ = planted(rng, read, (12, 20, 25, 8), (0, 2, 4))
    ref = gc.mutate(rng, ref, "ACGT", 0.02, 0.02)
    hits = both(ref, read, SC, 10, 16)
    assert len(hits) >= 3
    for v, i, j in hits:
        ext = gr.align_scalar(ref[:j][::-1], read[:i][::-1], SC, gr.GLOBAL, 0, True)[0]
        assert ext == v, (v, i, j, ext)


def test_library_exports_and_bindings():
    lib = _capi.load()
    bound = {n: (res, args) for n, res, args in _capi.SYMBOLS}
    for name in ("swmi_pair_hits", "swmi_batch_pair_hits"):
        assert getattr(lib, name) is not None
        assert name in bound and len(bound[name][1]) == 5
    import ctypes
    assert ctypes.sizeof(_capi.Hit) == 16 and [f[0] for f in _capi.Hit._fields_] == ["score", "end_i", "end_j", "reserved"]
    assert _capi.HITS_MAX == 16 == hr.K_MAX
    for name in ("hits", "hits_all", "hit_specs"):
        assert callable(getattr(aligner.Batch, name))
    assert aligner.PairBatch._hit_spec is not aligner.Batch._hit_spec
    shim = open(os.path.join(ROOT, "bindings", "jni", "swmi_shim.h")).read()
    jni = open(os.path.join(ROOT, "bindings", "jni", "swmi_jni.c")).read()
    java = open(os.path.join(ROOT, "bindings", "java", "sw", "GpuSmithWaterman.java")).read()
    assert "swmi_shim_set_hits" in shim and "swmi_shim_pair_hits" in shim
    assert "nativeSetHits" in jni and "nativePairHits" in jni and "setHits" in java and "nativePairHits" in java
