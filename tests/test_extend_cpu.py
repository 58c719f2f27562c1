"""Host-side checks of seed extension (option "extend") that need no GPU: the two restatements of tests/gotoh_reference.py
agree, the hand-checkable vectors of tests/golden/extend_kat.json hold, an extend result is the global alignment of the prefixes
that end in its maximum cells (the same module's plain global mode, which the project already trusts), the mirror takes the
extend= keyword and the sharded driver's parser knows --extend."""
import json
import os
import random

import pytest

import gotoh_reference as gr

HERE = os.path.dirname(os.path.abspath(__file__))
SC = (2, -3, -1, -3)
SCORES = (SC, (5, -3, -2, -6), (5, -3, -2, 0), (2, -1, -1, -1), (0, -3, -1, -3), (1, 1, -1, -2))
MATRIX = ("ACGT", [[3, -2, 1, -4], [-1, 4, -3, 0], [2, -5, 5, -1], [-3, 1, -2, 2]])      # asymmetric; row = read base


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _scalar(ref, read, sc, w=0, tie=0, matrix=None, **more):
    return gr.align_scalar(ref, read, sc, gr.GLOBAL, w, True, tie, matrix, **more)


def _numpy(ref, read, sc, w=0, tie=0, matrix=None, **more):
    return gr.align_numpy(ref, read, sc, gr.GLOBAL, w, True, tie, matrix, **more)


def _kats():
    with open(os.path.join(HERE, "golden", "extend_kat.json")) as f:
        return json.load(f)


def _pairs(seed, count, lo, hi):
    rng = random.Random(seed)
    for _ in range(count):
        alphabet = rng.choice(["A", "AC", "ACGT", "ACGTX"])
        yield _rand(rng, rng.randint(lo, hi), alphabet), _rand(rng, rng.randint(lo, hi), alphabet), rng.choice(SCORES)


@pytest.mark.parametrize("matrix", [None, MATRIX])
def test_scalar_and_numpy_agree(matrix):
    n = 0
    for ref, read, sc in _pairs(9910 + (matrix is not None), 150, 0, 14):
        for tie in (0, 1):
            a = _scalar(ref, read, sc, 0, tie, matrix, cells=True)
            assert a == _numpy(ref, read, sc, 0, tie, matrix, cells=True), (ref, read, sc, tie)
            assert a[:2] == _scalar(ref, read, sc, 0, tie, matrix)
            for (beg, (ra, qa)), (i, j) in zip(a[1], a[2]):       # every alignment spells the prefixes and the score it claims
                assert beg == 1 and ra.replace(gr.GAP_CHAR, "") == ref[:j] and qa.replace(gr.GAP_CHAR, "") == read[:i]
                assert gr.rescore(ra, qa, sc, matrix) == a[0], (ref, read, sc, tie)
            if not ref or not read:
                assert a == (0, [], [])
            n += 1
    assert n == 300


@pytest.mark.parametrize("w", [1, 3, 8])
def test_scalar_and_numpy_agree_on_a_staircase(w):
    rng = random.Random(9920 + w)
    done = 0
    for _ in range(60):
        m = rng.randint(9, 40)
        n = max(1, m + rng.choice([-w, -1, 0, 1, w, 2 * w + 9]))       # (the last: a reference that runs on past the band)
        if gr.refused(m, n, w, gr.GLOBAL, True, strip=8):
            continue
        alphabet = rng.choice(["AC", "ACGT"])
        ref, read = _rand(rng, n, alphabet), _rand(rng, m, alphabet)
        sc = rng.choice(SCORES)
        matrix = rng.choice([None, MATRIX])
        for tie in (0, 1):
            a = _scalar(ref, read, sc, w, tie, matrix, strip=8, cells=True)
            assert a == _numpy(ref, read, sc, w, tie, matrix, strip=8, cells=True), (ref, read, sc, tie)
            win = gr.windows(m, n, w, 8)
            for (beg, (ra, qa)), (i, j) in zip(a[1], a[2]):
                assert win[(i - 1) // 8][0] <= j <= win[(i - 1) // 8][1]
                assert beg == 1 and gr.rescore(ra, qa, sc, matrix) == a[0]
        done += 1
    assert done >= 30


@pytest.mark.parametrize("kat", _kats(), ids=lambda k: k["name"].split()[0])
def test_kats(kat):
    for tie, key in ((0, "serial"), (1, "strict")):
        want = (kat[key]["score"], [(b, tuple(s)) for b, s in kat[key]["alignments"]], [tuple(c) for c in kat[key]["cells"]])
        for fn in (_scalar, _numpy):
            assert fn(kat["ref"], kat["read"], kat["scores"], kat["w"], tie, strip=kat["strip"], cells=True) == want, (key, fn.__name__)


def test_kats_cover_what_they_should():
    kats = {k["name"].split()[0]: k for k in _kats()}
    assert kats["XKAT-1"]["serial"] == kats["XKAT-1"]["strict"] == {"score": 8, "alignments": [[1, ["ACGT", "ACGT"]]], "cells": [[4, 4]]}
    assert kats["XKAT-2"]["serial"] == {"score": -3, "alignments": [[1, ["G", "C"]]], "cells": [[1, 1]]}
    assert kats["XKAT-3"]["serial"] == {"score": 0, "alignments": [[1, ["A", "A"]], [1, ["AA", "AA"]]], "cells": [[1, 1], [2, 2]]}
    assert (kats["XKAT-4"]["serial"]["score"], kats["XKAT-4"]["serial"]["cells"]) == (30, [[20, 20]])
    k = kats["XKAT-5"]
    assert k["serial"]["cells"][0][1] == len(k["ref"]) and k["serial"]["cells"][0][0] < len(k["read"])       # last column
    k = kats["XKAT-6"]
    assert k["serial"]["cells"][0][0] == len(k["read"]) and k["serial"]["cells"][0][1] < len(k["ref"])       # last row
    assert kats["XKAT-7"]["serial"]["alignments"][0][1][1].startswith("___A")                                # row 0 reached early
    assert kats["XKAT-8"]["serial"]["alignments"][0][1][0].startswith("___A")                                # column 0 reached early
    for name in ("XKAT-9", "XKAT-10"):                             # the two tie modes list the same cells in another order
        k = kats[name]
        assert k["serial"]["cells"] != k["strict"]["cells"] and sorted(k["serial"]["cells"]) == sorted(k["strict"]["cells"])
        assert k["serial"]["score"] == k["strict"]["score"]


def _prefix_property(ref, read, sc, w, tie, matrix, strip):
    """(score, alignments, cells) put together from global alignments of prefixes alone"""
    m, n = len(read), len(ref)
    win = gr.windows(m, n, w, strip)
    glob = {}
    for i, j in gr.order(m, n, tie == 1):                        # the contract's order of tied cells
        if win[(i - 1) // strip][0] <= j <= win[(i - 1) // strip][1]:
            glob[(i, j)] = gr.align_scalar(ref[:j], read[:i], sc, gr.GLOBAL, w, tie_mode=tie, matrix=matrix, strip=strip)     # (plain global)
    best = max(v[0] for v in glob.values())
    cells = [c for c, v in glob.items() if v[0] == best]
    alns = [glob[c][1][0] for c in cells]
    assert all(len(glob[c][1]) == 1 for c in cells)
    return best, alns, cells


@pytest.mark.parametrize("matrix", [None, MATRIX])
def test_prefix_property(matrix):
    """the independent pin: extend(ref, read) is the global alignment of ref[:j] with read[:i] for every maximum cell (i, j), and
    its score the largest global score over all prefix pairs"""
    for ref, read, sc in _pairs(9930 + (matrix is not None), 60, 1, 12):
        for tie in (0, 1):
            want = _prefix_property(ref, read, sc, 0, tie, matrix, 1024)
            assert _scalar(ref, read, sc, 0, tie, matrix, cells=True) == want, (ref, read, sc, tie)
            assert _numpy(ref, read, sc, 0, tie, matrix, cells=True) == want, (ref, read, sc, tie)


def test_prefix_property_banded():
    rng = random.Random(9940)
    done = 0
    for _ in range(40):
        w = rng.choice([1, 2, 3])
        m = rng.randint(9, 20)
        n = max(1, m + rng.choice([-w, 0, 1, w, 2 * w + 9]))
        if gr.refused(m, n, w, gr.GLOBAL, True, strip=8):
            continue
        ref, read = _rand(rng, n, "AC"), _rand(rng, m, "AC")
        sc = rng.choice(SCORES)
        matrix = rng.choice([None, MATRIX])
        for tie in (0, 1):
            want = _prefix_property(ref, read, sc, w, tie, matrix, 8)
            assert _scalar(ref, read, sc, w, tie, matrix, strip=8, cells=True) == want, (ref, read, sc, w, tie)
            assert _numpy(ref, read, sc, w, tie, matrix, strip=8, cells=True) == want, (ref, read, sc, w, tie)
        done += 1
    assert done >= 25


def test_a_band_over_everything_and_short_reads_are_unbanded():
    rng = random.Random(9950)
    for _ in range(10):
        m, n = rng.randint(9, 30), rng.randint(1, 30)
        ref, read = _rand(rng, n, "AC"), _rand(rng, m, "AC")
        for tie in (0, 1):
            assert _scalar(ref, read, SC, max(m, n), tie, strip=8) == _scalar(ref, read, SC, 0, tie)
    ref, read = _rand(rng, 30), _rand(rng, 8)
    assert _numpy(ref, read, SC, 1, strip=8) == _numpy(ref, read, SC)          # m = strip: not a long read


# ---- the mirror's extend= keyword on a fake context ----
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


def test_mirror_takes_extend_keyword():
    import sparksmithwaterman_amd as sw
    c = _FakeContext()
    assert sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, extend=True).call(["ACGT", "CG"], [5, -3, -4, -6]) == (-4, [])
    assert c.log == [("set_option", "gap_open", -6), ("set_option", "align_mode", 2), ("set_option", "extend", 1), ("upload",),
                     ("run", (5, -3, -4)), ("free",), ("set_option", "extend", 0), ("set_option", "align_mode", 0),
                     ("set_option", "gap_open", 0)]
    c = _FakeContext()
    c.options["extend"] = 1                                       # the context's own setting comes back after the call
    sw.DistributedSW.OptAlignments(c, extend=False).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == [("set_option", "extend", 0), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "extend", 1)]
    for make in (lambda c: sw.Distribution.MapRef(c, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=8, extend=True),
                 lambda c: sw.Distribution.MapPartition(c, align_mode=sw.ALIGN_GLOBAL, extend=True)):
        c = _FakeContext()
        t = ((">r", "ACGT"), ["CG"], ([2, -1, -1], ["a", "i", "d", "-"]))
        f = make(c)
        f.call(t) if isinstance(f, sw.Distribution.MapRef) else f.call([t])
        assert c.log.index(("set_option", "extend", 1)) < c.log.index(("run", (2, -1, -1))) < c.log.index(("set_option", "extend", 0))
        assert c.options["extend"] == 0 and c.options["align_mode"] == 0
    for cls in (sw.Distribution.NoDistribution, sw.Distribution.DistributeReference):          # the file drivers keep it for _scores
        assert cls(_FakeContext(), extend=True)._extend is True and cls(_FakeContext())._extend is None
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c, extend=None).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # None: the context's own value, no option call
    for bad in (1, 0, 2, "yes"):
        c = _FakeContext()
        with pytest.raises(ValueError):
            sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, extend=bad).call(["ACGT", "CG"], [5, -3, -4])
        assert c.log == []                                       # rejected before anything reaches the library


def test_sharded_files_parser_extend_needs_global(capsys):
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "R", "--in-dir", "I", "--out-dir", "O"]
    assert sharded_files._parser().parse_args(base).extend is False
    args = sharded_files._parser().parse_args(base + ["--align-mode", "global", "--extend", "--long-reads", "--band", "32"])
    assert args.extend is True and args.align_mode == "global" and args.band == 32
    for mode in ([], ["--align-mode", "local"], ["--align-mode", "fit"]):
        with pytest.raises(SystemExit) as e:
            sharded_files._parser().parse_args(base + mode + ["--extend"])
        assert e.value.code == 2                                  # an argparse error
        assert "--extend requires --align-mode global" in capsys.readouterr().err
