"""End-to-end alignment modes (option "align_mode": fit, global) without a GPU: the two restatements of the contract in
tests/gotoh_reference.py against each other, against properties that hold by construction and against the known answers
(tests/golden/ends_kat.json); the host mirror's align_mode keyword on a fake context."""
import json
import os
import random

import pytest

import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "ends_kat.json")) as f:
        return json.load(f)["kats"]


def _matrix(name):
    if name is None:
        return None
    from sparksmithwaterman_amd import matrix as mx
    m = getattr(mx, name)
    alpha = m.alphabet if isinstance(m.alphabet, str) else bytes(m.alphabet).decode("latin-1")
    return alpha, [list(map(int, r)) for r in m.scores]


def _pairs(seed, count, max_len=12):
    rng = random.Random(seed)
    for _ in range(count):
        alpha = rng.choice(["AC", "ACGT", "A"])
        ref = "".join(rng.choice(alpha) for _ in range(rng.randint(1, max_len)))
        read = "".join(rng.choice(alpha) for _ in range(rng.randint(1, max_len)))
        sc = (rng.randint(0, 4), rng.randint(-4, 1), rng.randint(-3, 0), rng.randint(-4, 0))
        yield ref, read, sc


@pytest.mark.parametrize("mode", [gr.FIT, gr.GLOBAL])
@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree_and_alignments_rescore(mode, tie):
    for ref, read, sc in _pairs(100 + 2 * mode + tie, 400):
        got = gr.align_scalar(ref, read, sc, mode, tie_mode=tie)
        assert gr.align_numpy(ref, read, sc, mode, tie_mode=tie) == got, (ref, read, sc)
        score, alns = got
        assert len(alns) >= 1
        for begin, (ra, qa) in alns:
            assert len(ra) == len(qa)
            assert gr.rescore(ra, qa, sc) == score, (ref, read, sc, ra, qa)
            assert qa.replace("_", "") == read                    # the whole read
            used = ra.replace("_", "")
            if mode == gr.GLOBAL:
                assert used == ref and begin == 1                 # the whole reference
            elif used:
                assert ref[begin - 1:].startswith(used)
            assert 1 <= begin <= len(ref)


@pytest.mark.parametrize("tie", [0, 1])
def test_local_ge_fit_ge_global(tie):
    for ref, read, sc in _pairs(7 + tie, 500):
        loc = gr.align_numpy(ref, read, sc, gr.LOCAL, tie_mode=tie)[0]
        fit = gr.align_scalar(ref, read, sc, gr.FIT, tie_mode=tie)[0]
        glo = gr.align_scalar(ref, read, sc, gr.GLOBAL, tie_mode=tie)[0]
        assert loc >= fit >= glo, (ref, read, sc, loc, fit, glo)
        # and fit is the best global score over the stretches of the reference, never below the all-insertion alignment
        assert fit >= sc[3] + len(read) * sc[2]


def test_restatements_agree_with_a_matrix():
    m = _matrix("BLOSUM62")
    rng = random.Random(5)
    for _ in range(60):
        ref = "".join(rng.choice(m[0][:20] + "z") for _ in range(rng.randint(1, 14)))
        read = "".join(rng.choice(m[0][:20] + "z") for _ in range(rng.randint(1, 14)))
        sc = (1, -1, rng.randint(-2, 0), rng.randint(-11, 0))
        for mode in (gr.FIT, gr.GLOBAL):
            for tie in (0, 1):
                got = gr.align_scalar(ref, read, sc, mode, tie_mode=tie, matrix=m)
                assert gr.align_numpy(ref, read, sc, mode, tie_mode=tie, matrix=m) == got
                for _, (ra, qa) in got[1]:
                    assert gr.rescore(ra, qa, sc, m) == got[0]


def test_ends_kats():
    kats = _kats()
    by = {k["name"]: k for k in kats}
    for k in kats:
        sc, m = tuple(k["scores"]), _matrix(k["matrix"])
        exp = (k["score"], [(a[0], (a[1], a[2])) for a in k["alignments"]])
        got = gr.align_scalar(k["ref"], k["read"], sc, k["align_mode"], tie_mode=k["tie_mode"], matrix=m, matrices=True)
        assert got[:2] == exp, k["name"]
        assert gr.align_numpy(k["ref"], k["read"], sc, k["align_mode"], tie_mode=k["tie_mode"], matrix=m) == exp, k["name"]
        H, E, F, D, XE, XF = got[2:]
        assert H == k["H"], k["name"]
        assert [[None if v == gr.NINF else v for v in row] for row in E] == k["E"], k["name"]
        assert [[None if v == gr.NINF else v for v in row] for row in F] == k["F"], k["name"]
        assert ["".join(r) for r in D] == k["T"], k["name"]
        assert ["".join(str(x) for x in r) for r in XE] == k["xE"], k["name"]
        assert ["".join(str(x) for x in r) for r in XF] == k["xF"], k["name"]
    # the three answers checked by hand
    assert (by["EKAT-1"]["score"], by["EKAT-1"]["alignments"]) == (2, [[2, "__GTCCAGAC", "AGGTC__GAC"]])
    assert (by["EKAT-2"]["score"], by["EKAT-2"]["alignments"]) == (-4, [[1, "_CGTCCAGACT", "AGGTC__GAC_"]])
    for n in ("EKAT-3f", "EKAT-3g"):
        assert (by[n]["score"], by[n]["alignments"]) == (0, [[1, "__ACGT__", "TTACGTAA"]])
    # what the file is meant to cover
    assert by["EKAT-4"]["alignments"][0][1].startswith("_") and by["EKAT-4"]["alignments"][0][0] == 1     # the j = 0 tail
    assert len(by["EKAT-3f"]["read"]) > len(by["EKAT-3f"]["ref"])
    assert len(by["EKAT-5s"]["alignments"]) == 3
    assert by["EKAT-7s"]["alignments"] != by["EKAT-7t"]["alignments"] and by["EKAT-7s"]["score"] == by["EKAT-7t"]["score"]
    assert by["EKAT-8"]["score"] < 0
    assert by["EKAT-9"]["matrix"] == "BLOSUM62"


class _FakeBatch:
    def __init__(self, log):
        self.log = log

    def run(self, params):
        self.log.append(("run", (params.match, params.mismatch, params.gap)))
        return self

    def score(self, pair):
        return -4

    def alignments(self, pair):
        return []

    def ref_total(self, ref):
        return -4

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


def test_mirror_takes_align_mode_keyword():
    import sparksmithwaterman_amd as sw
    assert (sw.ALIGN_LOCAL, sw.ALIGN_FIT, sw.ALIGN_GLOBAL) == (0, 1, 2)
    c = _FakeContext()
    assert sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL).call(["ACGT", "CG"], [5, -3, -4, -6]) == (-4, [])
    assert c.log == [("set_option", "gap_open", -6), ("set_option", "align_mode", 2), ("upload",), ("run", (5, -3, -4)), ("free",),
                     ("set_option", "align_mode", 0), ("set_option", "gap_open", 0)]
    c = _FakeContext()
    c.options["align_mode"] = sw.ALIGN_GLOBAL                   # the context's own setting comes back after the call
    sw.DistributedSW.OptAlignments(c, align_mode=sw.ALIGN_FIT).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == [("set_option", "align_mode", 1), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "align_mode", 2)]
    c = _FakeContext()
    sw.Distribution.MapRef(c, align_mode=sw.ALIGN_FIT).call(((">r", "ACGT"), ["CG"], ([2, -1, -1], ["a", "i", "d", "-"])))
    assert c.log[0] == ("set_option", "align_mode", 1) and ("run", (2, -1, -1)) in c.log and c.log[-1] == ("set_option", "align_mode", 0)
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # no keyword: the context's options are left alone
    c = _FakeContext()
    with pytest.raises(ValueError):
        sw.SmithWaterman.OptAlignments(c, align_mode=3).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == []                                           # rejected before anything reaches the library
