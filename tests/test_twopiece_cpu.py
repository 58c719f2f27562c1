"""Two-piece affine gaps: the restated contract of tests/twopiece_reference.py, held to the one-piece reference
where the two must agree, its two forms held to each other, and its alignments to their own run costs.  No GPU."""
import random

import pytest

import gotoh_reference as gr
import twopiece_reference as tr

GLOBAL = gr.GLOBAL
CROSS = (2, -4, -2, -4, -1, -24)          # the pieces tie at k = 20: -4 - 2k = -24 - k


def rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def pairs(seed, count, lo, hi, alphabet="ACGT"):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        ref = rand(rng, rng.randint(lo, hi), alphabet)
        read = "".join(c for c in ref if rng.random() > 0.1)
        read = "".join(c if rng.random() > 0.1 else rng.choice(alphabet) for c in read) or "A"
        out.append((ref, read))
    return out


SMALL = pairs(11, 6, 5, 30) + pairs(12, 4, 5, 30, "AC") + [("A", "A"), ("ACGT", "A"), ("A", "ACGTACGT")]


@pytest.mark.parametrize("piece2", ["same", "never"])
@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("tie", [0, 1])
def test_scalar_equals_one_piece(piece2, extend, tie):
    """with piece 2 = piece 1, or a piece 2 that can never win (o2 = -2^20, e2 = e1), the scalar form is gotoh_reference's in full"""
    for sc4 in [(2, -3, -2, -4), (1, -1, -1, 0), (3, -2, -1, -6)]:
        sc6 = sc4 + ((sc4[2], sc4[3]) if piece2 == "same" else (sc4[2], -(1 << 20)))
        for ref, read in SMALL:
            want = gr.align_scalar(ref, read, sc4, GLOBAL, 0, extend, tie, cells=True)
            assert tr.align_scalar(ref, read, sc6, GLOBAL, 0, extend, tie, cells=True) == want, (sc6, ref, read)


@pytest.mark.parametrize("piece2", ["same", "never"])
@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("tie", [0, 1])
def test_scalar_equals_one_piece_staircase(piece2, extend, tie):
    """the same on staircases at strip 8"""
    sc4 = (2, -3, -2, -4)
    sc6 = sc4 + ((sc4[2], sc4[3]) if piece2 == "same" else (sc4[2], -(1 << 20)))
    for ref, read in pairs(21, 6, 20, 40):
        m, n = len(read), len(ref)
        for w in (3, 8, 9):
            if m <= 8 or gr.refused(m, n, w, GLOBAL, extend, strip=8):
                continue
            want = gr.align_scalar(ref, read, sc4, GLOBAL, w, extend, tie, strip=8, cells=True)
            assert tr.align_scalar(ref, read, sc6, GLOBAL, w, extend, tie, strip=8, cells=True) == want, (w, ref, read)


SCORES = [CROSS, (2, -2, -2, -2, -1, -8), (3, -4, -3, 0, -1, -9), (2, -3, -1, -10, -3, -2)]


@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("tie", [0, 1])
def test_numpy_equals_scalar(extend, tie):
    for sc in SCORES:
        for ref, read in SMALL:
            want = tr.align_scalar(ref, read, sc, GLOBAL, 0, extend, tie, cells=True)
            assert tr.align_numpy(ref, read, sc, GLOBAL, 0, extend, tie, cells=True) == want, (sc, ref, read)


@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("tie", [0, 1])
def test_numpy_equals_scalar_banded(extend, tie):
    seen = 0
    for sc in SCORES[:2]:
        for ref, read in pairs(31, 5, 20, 40) + pairs(32, 3, 20, 40, "AC"):
            m, n = len(read), len(ref)
            for w in (3, 8, 9):
                if m <= 8 or gr.refused(m, n, w, GLOBAL, extend, strip=8):
                    continue
                want = tr.align_scalar(ref, read, sc, GLOBAL, w, extend, tie, strip=8, cells=True)
                assert tr.align_numpy(ref, read, sc, GLOBAL, w, extend, tie, strip=8, cells=True) == want, (sc, w, ref, read)
                seen += 1
    assert seen > 10


@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("tie", [0, 1])
def test_rescore(extend, tie):
    """o1, o2 <= 0: the DP optimum and the run-cost optimum coincide, so every alignment's run cost is its score"""
    for sc in SCORES:
        for ref, read in SMALL:
            score, alns, cells = tr.align_numpy(ref, read, sc, GLOBAL, 0, extend, tie, cells=True)
            assert alns
            for (begin, (ra, qa)), (i, j) in zip(alns, cells):
                assert tr.rescore(ra, qa, sc) == score, (sc, ref, read, ra, qa)
                assert ra.replace("_", "") == ref[:j] and qa.replace("_", "") == read[:i]


def test_rescore_is_a_run_cost():
    assert tr.rescore("ACGT", "A__T", CROSS) == 2 + 2 + max(-4 - 4, -24 - 2)
    assert tr.rescore("A" + "C" * 30 + "T", "A" + "_" * 30 + "T", CROSS) == 4 + (-24 - 30)
    assert tr.rescore("A_C", "AGC", CROSS) == 4 - 6
    assert tr.rescore("__", "AC", CROSS) == -8


@pytest.mark.parametrize("k", [19, 20, 21])
@pytest.mark.parametrize("kind", ["ins", "del"])
def test_crossover(k, kind):
    """a planted gap of 19, 20 or 21 bases is aligned as one run, at the cost of the cheaper piece"""
    rng = random.Random(100 + k)
    left, right, gap = rand(rng, 40), rand(rng, 40), rand(rng, k)
    ref, read = (left + right, left + gap + right) if kind == "ins" else (left + gap + right, left + right)
    for form in (tr.align_scalar, tr.align_numpy):
        score, alns = form(ref, read, CROSS, GLOBAL)
        assert score == 2 * 80 + max(-4 - 2 * k, -24 - k)
        (begin, (ra, qa)), = alns
        gapped = ra if kind == "ins" else qa
        assert gapped.count("_") == k and "_" * k in gapped
        assert "_" not in (qa if kind == "ins" else ra)
