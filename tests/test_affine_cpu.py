"""The affine-gap contract without a GPU: the two restatements in tests/gotoh_reference.py against each other, against the
oracle at gap_open = 0, and against the hand-checked known answers (tests/golden/affine_kat.json); the host mirror's
four-entry alignScores."""
import json
import os
import random

import pytest

from oracle import sw_oracle as orc

import gotoh_reference as gr
import limit_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _oracle(ref, read, scores, tie):
    s, al = orc.opt_alignments((ref, read), scores, b"aid-", tie)
    return s, [(a[0], tuple(a[1])) for a in al]


@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree(tie):
    rng = random.Random(100 + tie)
    for _ in range(250):
        alphabet = rng.choice(["ACGT", "AC", "ACGTacgtN\xe9\xc9"])
        ref = _rand(rng, rng.randint(0, 30), alphabet)
        if rng.random() < 0.3:
            ref = (_rand(rng, rng.randint(2, 5), "ACGT") * 8)[:rng.randint(8, 40)]      # periodic: tied maxima
        read = _rand(rng, rng.randint(0, 16), alphabet)
        sc = (rng.randint(1, 6), rng.randint(-5, 0), rng.randint(-4, 0), rng.choice([0, -1, -2, -6, -12]))
        assert gr.align_scalar(ref, read, sc, tie_mode=tie) == gr.align_numpy(ref, read, sc, tie_mode=tie), (ref, read, sc)


@pytest.mark.parametrize("tie", [0, 1])
def test_gap_open_zero_is_the_linear_oracle(tie, kats):
    n = 0
    for k in kats:
        if k["scores"][2] > 0 or tuple(k.get("types", "aid-")) != tuple("aid-") or k["tie_mode"] != tie:
            continue
        sc = tuple(k["scores"]) + (0,)
        exp = (k["score"], [(a[0], (a[1], a[2])) for a in k["alignments"]])
        assert gr.align_scalar(k["ref"], k["read"], sc, tie_mode=tie) == exp, k["name"]
        assert gr.align_numpy(k["ref"], k["read"], sc, tie_mode=tie) == exp, k["name"]
        n += 1
    assert n >= 3
    rng = random.Random(200 + tie)
    for _ in range(150):
        ref, read = _rand(rng, rng.randint(0, 60), "ACGT"), _rand(rng, rng.randint(0, 25), "ACGT")
        sc = (rng.randint(1, 5), rng.randint(-4, 0), rng.randint(-5, 0))
        exp = _oracle(ref, read, sc, tie)
        assert gr.align_numpy(ref, read, sc + (0,), tie_mode=tie) == exp
        assert gr.align_scalar(ref, read, sc + (0,), tie_mode=tie) == exp


def test_affine_kats():
    kats = _golden("affine_kat.json")["kats"]
    assert len(kats) >= 5
    for k in kats:
        sc = tuple(k["scores"])
        exp = (k["score"], [(a[0], (a[1], a[2])) for a in k["alignments"]])
        got = gr.align_scalar(k["ref"], k["read"], sc, tie_mode=k["tie_mode"], matrices=True)
        assert got[:2] == exp, k["name"]
        assert gr.align_numpy(k["ref"], k["read"], sc, tie_mode=k["tie_mode"]) == exp, k["name"]
        H, E, F, D, XE, XF = got[2:]
        assert H == k["H"], k["name"]
        assert [[None if v == gr.NINF else v for v in row] for row in E] == k["E"], k["name"]
        assert [[None if v == gr.NINF else v for v in row] for row in F] == k["F"], k["name"]
        assert ["".join(r) for r in D] == k["T"], k["name"]
        assert ["".join(str(x) for x in r) for r in XE] == k["xE"], k["name"]
        assert ["".join(str(x) for x in r) for r in XF] == k["xF"], k["name"]
    by = {k["name"]: k for k in kats}
    # o changes the path: the same pair with o = 0 splits the gap
    k1 = by["AKAT-1"]
    assert gr.align_scalar(k1["ref"], k1["read"], tuple(k1["scores"][:3]) + (0,))[1] != gr.align_scalar(k1["ref"], k1["read"], tuple(k1["scores"]))[1]
    assert by["AKAT-3s"]["alignments"] != by["AKAT-3t"]["alignments"]
    assert by["AKAT-4"]["score"] == 0 and len(by["AKAT-4"]["alignments"]) == len(by["AKAT-4"]["ref"]) * len(by["AKAT-4"]["read"])
    assert by["AKAT-5"]["alignments"] == []


@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree_at_the_score_bounds(tie):
    """every score at +-2^20 (the GPU tests' inputs at reduced length): align_numpy's int64 against align_scalar's Python
    ints, which keeps the numpy restatement trustworthy where tests/test_affine_gpu.py leans on it"""
    for sc in lc.AFFINE_BOUND_SCORES:
        ref, read = lc.affine_bound_pair(160, 40, 20)
        got = gr.align_scalar(ref, read, sc, tie_mode=tie)
        assert got == gr.align_numpy(ref, read, sc, tie_mode=tie), sc
        assert got[0] >= 40 * lc.L
    read = lc.rand_seq(random.Random(1410), 96, "AC")
    sc = lc.AFFINE_BOUND_SCORES[0]
    assert gr.align_scalar(read, read, sc, tie_mode=tie) == gr.align_numpy(read, read, sc, tie_mode=tie) == (96 * lc.L, [(1, (read, read))])


class _FakeBatch:
    def __init__(self, log):
        self.log = log

    def run(self, params):
        self.log.append(("run", (params.match, params.mismatch, params.gap)))
        return self

    def score(self, pair):
        return 7

    def alignments(self, pair):
        return []

    def ref_total(self, ref):
        return 7

    def ref_match_sites(self, ref):
        return []

    def free(self):
        self.log.append(("free",))


class _FakeContext:
    """records what the mirror asks of a context (no GPU)"""

    def __init__(self):
        self.log, self.options = [], {}

    def set_option(self, name, value):
        self.log.append(("set_option", name, value))
        self.options[name] = value

    def upload(self, refs, reads):
        self.log.append(("upload",))
        return _FakeBatch(self.log)


def test_mirror_splits_four_entry_align_scores():
    import sparksmithwaterman_amd as sw
    c = _FakeContext()
    assert sw.SmithWaterman.OptAlignments(c).call(["ACGT", "CG"], [5, -3, -4, -6]) == (7, [])
    assert c.log == [("set_option", "gap_open", -6), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "gap_open", 0)]
    c = _FakeContext()
    sw.Distribution.MapRef(c).call(((">r", "ACGT"), ["CG"], ([2, -1, -1, -3], ["a", "i", "d", "-"])))
    assert c.log[0] == ("set_option", "gap_open", -3) and ("run", (2, -1, -1)) in c.log and c.log[-1] == ("set_option", "gap_open", 0)
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # three entries: the context's options are left alone
    c = _FakeContext()
    with pytest.raises(ValueError):
        sw.SmithWaterman.OptAlignments(c).call(["ACGT", "CG"], [5, -3, -4, 2])
    assert c.log == []                                           # rejected before anything reaches the library
    with pytest.raises(ValueError):
        sw.make_params((5, -3, -4, -6))                          # make_params itself stays three-entry
