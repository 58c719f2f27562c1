"""The drop-off rule of seed extension (option "xdrop") without a GPU: the two forms of
tests/xdrop_reference.py against each other on staircases at strip 8, the properties the contract states (a stopped run equals
the extend run of the truncated read; an X nothing exceeds equals the extend run; the test is strict), and the parts of the
feature that need no GPU: the mirror keyword, the sharded_files arguments and the C ABI's symbol list."""
import random

import pytest

import gotoh_reference as gr
import xdrop_reference as xr

SCORES = ((2, -4, -2, -4), (5, -3, -2, -6), (2, -3, -1, -3), (2, -1, -1, -1), (1, -5, -3, 0))
MATRIX = ("ACGT", [[3, -2, 1, -4], [-1, 4, -3, 0], [2, -5, 5, -1], [-3, 1, -2, 2]])      # asymmetric; row = read base
STRIP = 8


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _extend(ref, read, sc, w=0, tie=0, matrix=None, strip=STRIP):
    return gr.align_scalar(ref, read, sc, gr.GLOBAL, w, True, tie, matrix, strip, cells=True)


def _staircases(seed, count):
    """pairs whose read shares its head with the reference and then goes its own way: differences of every size"""
    rng = random.Random(seed)
    done = 0
    while done < count:
        w = rng.choice([0, 2, 5])
        m = rng.randint(17, 40)
        n = max(1, m + rng.choice([-5, -1, 0, 1, 5, 14]))
        if gr.refused(m, n, w, gr.GLOBAL, True, strip=STRIP):
            continue
        alphabet = rng.choice(["AC", "ACGT"])
        head = _rand(rng, rng.randint(0, min(m, n)), alphabet)
        ref = head + _rand(rng, n - len(head), alphabet)
        read = head + _rand(rng, m - len(head), alphabet)
        done += 1
        yield ref, read, rng.choice(SCORES), w, rng.choice([None, MATRIX])


def _thresholds(dr):
    """every X at which the outcome can change, and one past the largest"""
    ds = sorted({b - s for b, s in dr if b - s >= 1})
    return sorted({x for d in ds for x in (d - 1, d) if x >= 1} | {max(ds + [0]) + 3})


def test_numpy_form_equals_the_scalar_form():
    stops = runs = 0
    for ref, read, sc, w, matrix in _staircases(9800, 70):
        dr = xr.drops_scalar(ref, read, sc, w, matrix, STRIP)
        assert dr == xr.drops(ref, read, sc, w, matrix, STRIP), (ref, read, sc, w)
        assert len(dr) == (len(read) + STRIP - 1) // STRIP - 1
        assert all(b >= s for b, s in dr) and all(dr[k][0] <= dr[k + 1][0] for k in range(len(dr) - 1))
        for tie in (0, 1):
            for X in _thresholds(dr):
                a = xr.align_scalar(ref, read, sc, X, w, tie, matrix, STRIP)
                assert a == xr.align(ref, read, sc, X, w, tie, matrix, STRIP), (ref, read, sc, w, tie, X)
                assert a[:2] + a[3:] == xr.align(ref, read, sc, X, w, tie, matrix, STRIP, cells=False)
                win = gr.windows(len(read), len(ref), w, STRIP)
                for (beg, (ra, qa)), (i, j) in zip(a[1], a[2]):   # every alignment spells the prefixes and the score it claims
                    assert i <= a[3] and win[(i - 1) // STRIP][0] <= j <= win[(i - 1) // STRIP][1]
                    assert beg == 1 and ra.replace(gr.GAP_CHAR, "") == ref[:j] and qa.replace(gr.GAP_CHAR, "") == read[:i]
                    assert gr.rescore(ra, qa, sc, matrix) == a[0]
                stops += a[3] < len(read)
                runs += 1
    assert stops >= 100 and runs - stops >= 100


def test_a_stopped_run_is_the_extend_run_of_the_truncated_read():
    """for s* >= 1 under the same band (the truncated read is still long: the same windows), for s* = 0 without a band only"""
    seen = {0: 0, 1: 0, 2: 0}
    for ref, read, sc, w, matrix in _staircases(9801, 90):
        dr = xr.drops_scalar(ref, read, sc, w, matrix, STRIP)
        for tie in (0, 1):
            for X in _thresholds(dr):
                s = xr.first_stop(dr, X)
                got = xr.align_scalar(ref, read, sc, X, w, tie, matrix, STRIP)
                if s is None:
                    assert got == _extend(ref, read, sc, w, tie, matrix) + (len(read),)
                    continue
                assert got[3] == STRIP * (s + 1) < len(read) and got[0] == dr[s][0]
                if s >= 1 or w == 0:
                    assert got[:3] == _extend(ref, read[:got[3]], sc, w, tie, matrix), (ref, read, sc, w, tie, X)
                    seen[min(s, 2)] += 1
    assert all(v >= 10 for v in seen.values()), seen


def test_a_large_x_zero_and_short_reads_equal_extend():
    rng = random.Random(9802)
    for ref, read, sc, w, matrix in _staircases(9802, 25):
        dr = xr.drops_scalar(ref, read, sc, w, matrix, STRIP)
        top = max(b - s for b, s in dr)
        want = _extend(ref, read, sc, w, 0, matrix) + (len(read),)
        for X in (0, max(top, 1), (1 << 31) - 1):
            assert xr.align_scalar(ref, read, sc, X, w, 0, matrix, STRIP) == want
            assert xr.align(ref, read, sc, X, w, 0, matrix, STRIP) == want
    for m in (1, 7, 8):                                           # at most one strip: never stopped, never banded
        ref, read = _rand(rng, 12) + "C" * 12, _rand(rng, m)
        assert xr.drops(ref, read, SCORES[0], 2, None, STRIP) == xr.drops_scalar(ref, read, SCORES[0], 2, None, STRIP) == []
        for f in (xr.align, xr.align_scalar):
            assert f(ref, read, SCORES[0], 1, 2, 0, None, STRIP) == _extend(ref, read, SCORES[0], 0) + (m,)
    for f in (xr.align, xr.align_scalar):                         # an empty side
        assert f("", "ACGT" * 5, SCORES[0], 1, 0, 0, None, STRIP) == (0, [], [], 20)
        assert f("ACGT", "", SCORES[0], 1, 0, 0, None, STRIP) == (0, [], [], 0)


def test_the_test_is_strict():
    """a head of 6 matches, then A's against C's: from the one maximum cell (6, 6) row 8 is reached by two insertions, so
    best(0) - seam(0) = |o| + 2 |e| and best(1) - seam(1) = |o| + 10 |e| -- X = d does not stop, X = d - 1 does"""
    sc = (2, -4, -2, -4)
    ref, read = "ACGTAC" + "C" * 18, "ACGTAC" + "A" * 14
    dr = xr.drops_scalar(ref, read, sc, 0, None, STRIP)
    assert dr == [(12, 12 - 8), (12, 12 - 24)]
    d0, d1 = 8, 24
    for f in (xr.align, xr.align_scalar):
        assert [f(ref, read, sc, X, 0, 0, None, STRIP)[3] for X in (d0 - 1, d0, d1 - 1, d1)] == [8, 16, 16, 20]
        for X in (d0 - 1, d1 - 1, d1):
            assert f(ref, read, sc, X, 0, 0, None, STRIP)[:3] == (12, [(1, ("ACGTAC", "ACGTAC"))], [(6, 6)])


# ---- what fails without the feature ------------------------------------------------------------------------------------------
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


def test_mirror_takes_xdrop_keyword():
    import sparksmithwaterman_amd as sw
    c = _FakeContext()
    f = sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, long_reads=True, extend=True, xdrop=300)
    assert f.call(["ACGT", "CG"], [2, -4, -2, -4]) == (-4, [])
    assert c.log == [("set_option", "gap_open", -4), ("set_option", "align_mode", 2), ("set_option", "long_reads", 1),
                     ("set_option", "extend", 1), ("set_option", "xdrop", 300), ("upload",), ("run", (2, -4, -2)), ("free",),
                     ("set_option", "xdrop", 0), ("set_option", "extend", 0), ("set_option", "long_reads", 0),
                     ("set_option", "align_mode", 0), ("set_option", "gap_open", 0)]
    c = _FakeContext()
    c.options["xdrop"] = 77                                       # the context's own setting comes back after the call
    sw.DistributedSW.OptAlignments(c, xdrop=0).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == [("set_option", "xdrop", 0), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "xdrop", 77)]
    for make in (lambda c: sw.Distribution.MapRef(c, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=8, extend=True, xdrop=9),
                 lambda c: sw.Distribution.MapPartition(c, align_mode=sw.ALIGN_GLOBAL, extend=True, xdrop=9)):
        c = _FakeContext()
        t = ((">r", "ACGT"), ["CG"], ([2, -1, -1], ["a", "i", "d", "-"]))
        f = make(c)
        f.call(t) if isinstance(f, sw.Distribution.MapRef) else f.call([t])
        assert c.log.index(("set_option", "xdrop", 9)) < c.log.index(("run", (2, -1, -1))) < c.log.index(("set_option", "xdrop", 0))
        assert c.options["xdrop"] == 0 and c.options["extend"] == 0
    for cls in (sw.Distribution.NoDistribution, sw.Distribution.DistributeReference):          # the file drivers keep it for _scores
        assert cls(_FakeContext(), xdrop=5)._xdrop == 5 and cls(_FakeContext())._xdrop is None
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c, xdrop=None).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # None: the context's own value, no option call
    for bad in (2.5, "300", True, -1, 1 << 31):
        c = _FakeContext()
        with pytest.raises(ValueError):
            sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, extend=True, xdrop=bad).call(["ACGT", "CG"], [5, -3, -4])
        assert c.log == []                                       # rejected before anything reaches the library
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c, xdrop=(1 << 31) - 1).call(["ACGT", "CG"], [5, -3, -4])
    assert ("set_option", "xdrop", (1 << 31) - 1) in c.log


def test_sharded_files_parser_xdrop_needs_extend(capsys):
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "R", "--in-dir", "I", "--out-dir", "O"]
    assert sharded_files._parser().parse_args(base).xdrop == 0
    args = sharded_files._parser().parse_args(base + ["--align-mode", "global", "--extend", "--long-reads", "--xdrop", "300"])
    assert args.xdrop == 300 and args.extend is True and args.long_reads is True
    assert sharded_files._parser().parse_args(base + ["--xdrop", "0"]).xdrop == 0          # off: no --extend needed
    for more in (["--xdrop", "300"], ["--align-mode", "global", "--xdrop", "300"], ["--align-mode", "local", "--xdrop", "1"]):
        with pytest.raises(SystemExit) as e:
            sharded_files._parser().parse_args(base + more)
        assert e.value.code == 2                                  # an argparse error
        assert "--xdrop requires --extend" in capsys.readouterr().err
    for bad in ("-1", str(1 << 31)):
        with pytest.raises(SystemExit) as e:
            sharded_files._parser().parse_args(base + ["--align-mode", "global", "--extend", "--xdrop=" + bad])
        assert e.value.code == 2
        assert "--xdrop takes a threshold" in capsys.readouterr().err


def test_rows_swept_is_a_declared_symbol():
    from sparksmithwaterman_amd import _capi
    import ctypes as C
    sym = {name: (res, args) for name, res, args in _capi.SYMBOLS}
    assert sym["swmi_pair_rows_swept"] == (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)])
    assert _capi.XDROP_MAX == (1 << 31) - 1
