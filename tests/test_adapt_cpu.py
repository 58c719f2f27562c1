"""The adaptive band of seed extension (option "band_adapt") without a GPU: the two forms of
tests/adapt_reference.py against each other on staircases at strip 8, the properties the contract states (monotone windows of
at most strip + 2w columns that are never empty, p(s) inside the window above and the window below, alignments that rescore to
the score and spell the prefixes, the window that stands still), the bound function of the host runtime against its Python
restatement, and the parts of the feature that need no GPU: the mirror keyword, the sharded_files arguments, the C ABI's symbol."""
import os
import random
import subprocess

import pytest

import adapt_reference as ar
import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = ((2, -4, -2, -4), (5, -3, -2, -6), (2, -3, -1, -3), (2, -1, -1, -1), (1, -5, -3, 0))
MATRIX = ("ACGT", [[3, -2, 1, -4], [-1, 4, -3, 0], [2, -5, 5, -1], [-3, 1, -2, 2]])      # asymmetric; row = read base
STRIP = 8


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _extend(ref, read, sc, w=0, tie=0, matrix=None, strip=STRIP):
    return gr.align_scalar(ref, read, sc, gr.GLOBAL, w, True, tie, matrix, strip, cells=True)


def _drifting(seed, count):
    """pairs whose reference is the read with runs of extra or missing bases here and there, or goes its own way for a stretch,
    with a reference that may be far shorter than the read"""
    rng = random.Random(seed)
    for _ in range(count):
        alphabet = rng.choice(["AC", "ACGT"])
        read = _rand(rng, rng.randint(17, 44), alphabet)
        ref, i = "", 0
        while i < len(read):
            k = rng.randint(3, 12)
            kind = rng.random()
            if kind < 0.25:
                ref += _rand(rng, rng.randint(1, 5), alphabet)              # extra reference bases
            elif kind < 0.4:
                i += rng.randint(1, 4)                                      # read bases the reference lacks
            elif kind < 0.55:
                ref += _rand(rng, k, alphabet)                              # an unrelated stretch
                i += k
                continue
            ref += read[i:i + k]
            i += k
        ref = (ref + _rand(rng, rng.choice([0, 0, 6]), alphabet))[:rng.choice([len(ref) + 6, len(ref) + 6, rng.randint(3, 12)])]
        yield ref, read, rng.choice(SCORES), rng.randint(1, 6), rng.choice([None, MATRIX])


def _thresholds(drops):
    ds = sorted({b - s for b, s in drops if b - s >= 1})
    return [0] + sorted({x for d in ds for x in (d - 1, d) if x >= 1})[:4]


def _check_windows(res, ps, ref, read, w, strip=STRIP):
    """the properties of the contract on one result's windows"""
    n, wins = len(ref), res[3]
    assert wins[0] == (1, min(n, strip + w))
    assert len(ps) >= len(wins) - 1
    for s, (lo, hi) in enumerate(wins):
        assert 1 <= lo <= hi <= n and hi - lo + 1 <= strip + 2 * w, (s, lo, hi)               # never empty, never wider
        if s:
            assert lo >= wins[s - 1][0] and hi >= wins[s - 1][1]                            # monotone
            assert wins[s - 1][0] <= ps[s - 1] <= wins[s - 1][1] and lo <= ps[s - 1] <= hi   # p(s - 1) in both windows


# 1, 4, 5 -- scalar against numpy, and what every result must satisfy
def test_numpy_form_equals_the_scalar_form():
    runs = stops = long_short = 0
    for ref, read, sc, w, matrix in _drifting(9900, 400):
        _, _, drops = ar.trace_scalar(ref, read, sc, w, 0, 0, matrix, STRIP)
        for tie in (0, 1):
            for X in _thresholds(drops):
                a, ps, dr = ar.trace_scalar(ref, read, sc, w, X, tie, matrix, STRIP)
                assert (a, ps, dr) == ar.trace(ref, read, sc, w, X, tie, matrix, STRIP), (ref, read, sc, w, tie, X)
                rows = a[4] if X else len(read)
                assert len(a[3]) == (rows + STRIP - 1) // STRIP
                _check_windows(a, ps, ref, read, w)
                for (beg, (ra, qa)), (i, j) in zip(a[1], a[2]):
                    lo, hi = a[3][(i - 1) // STRIP]
                    assert i <= rows and lo <= j <= hi
                    assert beg == 1 and ra.replace(gr.GAP_CHAR, "") == ref[:j] and qa.replace(gr.GAP_CHAR, "") == read[:i]
                    assert gr.rescore(ra, qa, sc, matrix) == a[0]
                runs += 1
                stops += rows < len(read)
                long_short += len(ref) + STRIP < len(read)
    assert runs >= 1500 and stops >= 100 and long_short >= 100, (runs, stops, long_short)


# 2 -- a band over everything is no band; a short read and w = 0 are not banded
def test_a_band_over_everything_is_the_unbanded_extend_run():
    for ref, read, sc, _, matrix in _drifting(9901, 40):
        want = _extend(ref, read, sc, 0, 0, matrix)
        for w in (len(ref), len(ref) + 5):
            for f in (ar.align_scalar, ar.align):
                got = f(ref, read, sc, w, 0, 0, matrix, STRIP)
                assert got[:3] == want and all(win == (1, len(ref)) for win in got[3]), (ref, read, w)
    rng = random.Random(9902)
    for m in (1, 7, 8):
        ref, read = _rand(rng, 20), _rand(rng, m)
        for f in (ar.align_scalar, ar.align):
            assert f(ref, read, SCORES[0], 2, 0, 0, None, STRIP) == _extend(ref, read, SCORES[0]) + ([(1, 20)],)
            assert f(ref, read, SCORES[0], 2, 5, 0, None, STRIP) == _extend(ref, read, SCORES[0]) + ([(1, 20)], m)
    for f in (ar.align_scalar, ar.align):
        assert f("", "ACGT" * 5, SCORES[0], 2, 0, 0, None, STRIP) == (0, [], [], [])
        assert f("ACGT", "", SCORES[0], 2, 3, 0, None, STRIP) == (0, [], [], [], 0)


# 3 -- identical sequences: the seam row's maximum lies on the main diagonal, and the windows are the static ones
def test_identical_sequences_keep_the_static_band():
    rng = random.Random(9903)
    for m, w, sc in ((40, 2, SCORES[0]), (33, 5, SCORES[1]), (24, 1, SCORES[2])):
        seq = _rand(rng, m)
        for tie in (0, 1):
            for tr in (ar.trace_scalar, ar.trace):
                got, ps, _ = tr(seq, seq, sc, w, 0, tie, None, STRIP)
                assert ps == [STRIP * (s + 1) for s in range((m - 1) // STRIP)]
                assert got[3] == gr.windows(m, m, w, STRIP)
                assert got[:3] == _extend(seq, seq, sc, w, tie)
                assert got[:3] == (m * sc[0], [(1, (seq, seq))], [(m, m)])


# 4 -- no window is empty where the static band has one: a reference that ends far above the read's last strips
def test_a_short_reference_is_taken():
    rng = random.Random(9904)
    taken = 0
    for _ in range(30):
        read = _rand(rng, rng.randint(30, 44))
        n = rng.randint(4, 12)
        ref, w = read[:n], rng.randint(1, 3)
        assert gr.refused(len(read), n, w, gr.GLOBAL, True, strip=STRIP)                     # the static band refuses it
        a, ps, _ = ar.trace_scalar(ref, read, SCORES[0], w, 0, 0, None, STRIP)
        assert a == ar.align(ref, read, SCORES[0], w, 0, 0, None, STRIP)
        _check_windows(a, ps, ref, read, w)
        assert a[3][-1][1] == n and len(a[3]) == (len(read) + STRIP - 1) // STRIP
        taken += 1
    assert taken == 30


# the drift the band is for: the static band of the same half-width loses the alignment, the adaptive one keeps it
def test_drift_is_followed():
    rng = random.Random(9905)
    read = _rand(rng, 40)
    ref = read[:4] + _rand(rng, 3) + read[4:12] + _rand(rng, 3) + read[12:20] + _rand(rng, 3) + read[20:28] + _rand(rng, 3) + read[28:] + _rand(rng, 8)
    sc, w = SCORES[1], 4
    free = _extend(ref, read, sc)
    static = _extend(ref, read, sc, w)
    for f in (ar.align_scalar, ar.align):
        got = f(ref, read, sc, w, 0, 0, None, STRIP)
        assert got[:3] == free and static[0] < free[0]
        assert got[3] != gr.windows(len(read), len(ref), w, STRIP)


# 6 -- the window that stands still: c_lo(s + 1) = c_lo(s) > 1, where column c_lo - 1 of the seam row was never written
def test_the_standing_centre_occurs():
    seen = 0
    for ref, read, sc, w, matrix in _drifting(9906, 400):
        a = ar.align(ref, read, sc, w, 0, 0, matrix, STRIP)
        wins = a[3]
        hit = [s for s in range(1, len(wins)) if wins[s][0] == wins[s - 1][0] > 1]
        if hit:
            seen += 1
            assert a == ar.align_scalar(ref, read, sc, w, 0, 0, matrix, STRIP)        # (the scalar form asserts a real predecessor)
    assert seen >= 40, seen


# 7 -- the bound: (2 NS + 1) |o| + (1024 NS + n) |e| <= 2^30, the host runtime's function against the restatement
def _edge_cases():
    lim = 1 << 30
    cases = []
    for m, o, e in ((1025, -6, -2), (3000, -(1 << 20), -1), (10000, -4, -(1 << 10)), (2048, 0, -3), (2049, -(1 << 20), -(1 << 20)),
                    (5000, -100, 0)):
        ns = (m + 1023) // 1024
        if e:
            n = (lim - (2 * ns + 1) * -o) // -e - 1024 * ns           # the largest n inside
            cases += [(m, n - 1, o, e), (m, n, o, e), (m, n + 1, o, e)]
        else:
            cases += [(m, 1 << 29, o, e)]
    # a strip more makes the difference: the same n, one more base of read
    cases += [(1024 * 3, 5000, -(1 << 20), -2), (1024 * 3 + 1, 5000, -(1 << 20), -2), (1024 * 255, 1000, -(1 << 20), -2047),
              (1024 * 255 + 1, 1000, -(1 << 20), -2047)]
    return cases


def test_bound_function_matches_its_restatement(tmp_path):
    cases = _edge_cases()
    want = [ar.bound_ok(m, n, (0, 0, e, o)) for m, n, o, e in cases]
    assert want.count(True) >= 8 and want.count(False) >= 6, want
    src = tmp_path / "adapt_bound.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "swmi_host.h"\n'
                   'int main(int argc, char **argv) {\n'
                   '    for (int k = 1; k + 3 < argc; k += 4)\n'
                   '        printf("%d %lld\\n", (int)swmi_adapt_bound_ok(strtoull(argv[k], 0, 10), strtoull(argv[k + 1], 0, 10), atoll(argv[k + 2]), atoll(argv[k + 3])),\n'
                   '               (long long)swmi_adapt_low(strtoull(argv[k], 0, 10), strtoull(argv[k + 1], 0, 10), atoll(argv[k + 2]), atoll(argv[k + 3])));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "adapt_bound"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1",
                           "-I", os.path.join(ROOT, "sparksmithwaterman_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)] + [str(x) for c in cases for x in c], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [ln.split() for ln in out.stdout.splitlines()]
    assert [g[0] == "1" for g in got] == want
    for (m, n, o, e), g in zip(cases, got):
        ns = (m + 1023) // 1024
        assert int(g[1]) == (2 * ns + 1) * o + (1024 * ns + n) * e


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


def test_mirror_takes_band_adapt_keyword():
    import sparksmithwaterman_amd as sw
    c = _FakeContext()
    f = sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=64, extend=True, band_adapt=True)
    assert f.call(["ACGT", "CG"], [2, -4, -2, -4]) == (-4, [])
    assert c.log == [("set_option", "gap_open", -4), ("set_option", "align_mode", 2), ("set_option", "long_reads", 1),
                     ("set_option", "band", 64), ("set_option", "extend", 1), ("set_option", "band_adapt", 1), ("upload",),
                     ("run", (2, -4, -2)), ("free",), ("set_option", "band_adapt", 0), ("set_option", "extend", 0),
                     ("set_option", "band", 0), ("set_option", "long_reads", 0), ("set_option", "align_mode", 0),
                     ("set_option", "gap_open", 0)]
    c = _FakeContext()
    c.options["band_adapt"] = 1                                   # the context's own setting comes back after the call
    sw.DistributedSW.OptAlignments(c, band_adapt=False).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == [("set_option", "band_adapt", 0), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "band_adapt", 1)]
    for make in (lambda c: sw.Distribution.MapRef(c, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=8, extend=True, band_adapt=True),
                 lambda c: sw.Distribution.MapPartition(c, align_mode=sw.ALIGN_GLOBAL, band=8, extend=True, band_adapt=True)):
        c = _FakeContext()
        t = ((">r", "ACGT"), ["CG"], ([2, -1, -1], ["a", "i", "d", "-"]))
        f = make(c)
        f.call(t) if isinstance(f, sw.Distribution.MapRef) else f.call([t])
        assert c.log.index(("set_option", "band_adapt", 1)) < c.log.index(("run", (2, -1, -1))) < c.log.index(("set_option", "band_adapt", 0))
        assert c.options["band_adapt"] == 0 and c.options["band"] == 0
    for cls in (sw.Distribution.NoDistribution, sw.Distribution.DistributeReference):          # the file drivers keep it for _scores
        assert cls(_FakeContext(), band_adapt=True)._band_adapt is True and cls(_FakeContext())._band_adapt is None
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c, band_adapt=None).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # None: the context's own value, no option call
    for bad in (1, 0, "yes", 2.5):
        c = _FakeContext()
        with pytest.raises(ValueError):
            sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_GLOBAL, band=8, extend=True, band_adapt=bad).call(["ACGT", "CG"], [5, -3, -4])
        assert c.log == []                                       # rejected before anything reaches the library


def test_sharded_files_parser_band_adapt_needs_band_and_extend(capsys):
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "r", "--in-dir", "i", "--out-dir", "o", "--align-mode", "global", "--long-reads"]
    ns = sharded_files._parser().parse_args(base + ["--band", "64", "--extend", "--band-adapt"])
    assert ns.band_adapt is True and ns.band == 64 and ns.extend
    assert sharded_files._parser().parse_args(base + ["--band", "64", "--extend"]).band_adapt is False
    for args in (["--band-adapt"], ["--band-adapt", "--extend"], ["--band-adapt", "--band", "64"]):
        with pytest.raises(SystemExit):
            sharded_files._parser().parse_args(base + args)
        assert "--band-adapt requires --band and --extend" in capsys.readouterr().err


def test_the_accessor_is_bound_and_exported():
    from sparksmithwaterman_amd import _capi
    assert "swmi_pair_band_window" in [s[0] for s in _capi.SYMBOLS]
    lib = _capi.load()
    assert lib.swmi_pair_band_window(None, 0, 0, None, None) == -1            # SWMI_ERR_INVALID: a null batch
    with open(os.path.join(ROOT, "include", "swmi.h")) as f:
        text = f.read()
    assert "swmi_pair_band_window(const swmi_batch *b, uint64_t pair, uint32_t strip, uint32_t *c_lo, uint32_t *c_hi)" in text
    assert "#define SWMI_ABI_VERSION 3" in text
