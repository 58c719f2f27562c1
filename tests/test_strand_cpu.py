"""The minus strand without a GPU (SWMI_SPEC_READ_REVCOMP): the flag's value against the header, the
complement table against a literal restatement, the eight-field tuples of normalise_pairs, and the host-side cutting and
coordinate mapping that tests/test_strand_gpu.py takes its expected inputs from (cut_segments, cell_to_source) against plain
slicing plus sw.revcomp, for all four combinations of the two flags."""
import os
import random
import re

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi, aligner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "swmi.h")).read()
WHOLE = _capi.SPEC_WHOLE

# the table, restated: every byte that does not map to itself
PAIRS = {"A": "T", "T": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D", "U": "A",
         "a": "t", "t": "a", "c": "g", "g": "c", "r": "y", "y": "r", "k": "m", "m": "k", "b": "v", "v": "b", "d": "h", "h": "d", "u": "a"}


def test_the_flag_is_4_in_the_header_and_in_python():
    assert int(re.search(r"#define SWMI_SPEC_READ_REVCOMP\s+(0x[0-9A-Fa-f]+)u", HEADER).group(1), 16) == _capi.SPEC_READ_REVCOMP == 4
    assert _capi.SPEC_REVERSE == 1 and not re.search(r"#define SWMI_SPEC_\w+\s+0x2u", HEADER)       # bit 0x2 stays undefined
    assert re.search(r"#define SWMI_ABI_VERSION\s+(\d+)", HEADER).group(1) == "3"


def test_the_complement_table():
    assert isinstance(sw.COMPLEMENT, bytes) and len(sw.COMPLEMENT) == 256
    for x in range(256):
        want = ord(PAIRS.get(chr(x), chr(x)))
        assert sw.COMPLEMENT[x] == want, (x, sw.COMPLEMENT[x], want)
    for c in "SWNswn-*. \x00\xe9\xff0":
        assert sw.COMPLEMENT[ord(c)] == ord(c)
    twice = bytes(sw.COMPLEMENT[sw.COMPLEMENT[x]] for x in range(256))
    assert [x for x in range(256) if twice[x] != x] == [ord("U"), ord("u")]
    assert twice[ord("U")] == ord("T") and twice[ord("u")] == ord("t")


def test_revcomp():
    assert sw.revcomp(b"AACGTNnKu") == b"aMnNACGTT" and sw.revcomp("AACGTNnKu") == "aMnNACGTT"
    assert sw.revcomp(b"") == b"" and sw.revcomp("") == "" and sw.revcomp("\xe9A") == "T\xe9"
    every = bytes(range(256))
    assert sw.revcomp(every) == every.translate(sw.COMPLEMENT)[::-1]


def test_normalise_pairs_takes_the_strand():
    got = sw.normalise_pairs([(2, 3, 4, 5, 6, 7, True, "-"), (2, 3, 4, 5, 6, 7, False, "+"), [2, 3, 4, None, 6, WHOLE, 0, "-"],
                              (2, 3, 4, 5, 6, 7, 1, "+"), (0, 1), (2, 3, 4, 5, 6, 7), (2, 3, 4, 5, 6, 7, True)])
    assert got == [(2, 3, 4, 5, 6, 7, True, "-"), (2, 3, 4, 5, 6, 7, False), (2, 3, 4, WHOLE, 6, WHOLE, False, "-"), (2, 3, 4, 5, 6, 7, True),
                   (0, 1, 0, WHOLE, 0, WHOLE, False), (2, 3, 4, 5, 6, 7, False), (2, 3, 4, 5, 6, 7, True)]
    assert sw.normalise_pairs(got) == got


@pytest.mark.parametrize("bad", [[(0, 1, 2, 3, 4, 5, True, "x")], [(0, 1, 2, 3, 4, 5, True, 0)], [(0, 1, 2, 3, 4, 5, True, None)],
                                 [(0, 1, 2, 3, 4, 5, True, "-", 0)], [(0, 1), (0, 1, 2, 3, 4, 5, False, "")], [(0, 1, 2, 3, 4, 5, False, "--")],
                                 [(0, 1, 2, 3, 4, 5, False, b"-")], [(0, 1, 2, 3, 4, 5, False, True)], [(0, 1, 2, 3, 4, 5, "-", "-")],
                                 [(0, 1, 2, 3, 4, -5, False, "-")], [(0, 1, 2, 3, 4, 5, 2, "-")]])
def test_normalise_pairs_refuses(bad):
    with pytest.raises(ValueError) as e:
        sw.normalise_pairs(bad)
    assert "pair %d" % (len(bad) - 1) in str(e.value)


def test_segments_and_to_source_against_plain_slicing():
    rng = random.Random(2)
    alphabet = b"ACGTacgtNnKkUuRYM\xe9-"
    refs = [bytes(rng.choice(alphabet) for _ in range(n)) for n in (50, 1, 0, 33)]
    reads = [bytes(rng.choice(alphabet) for _ in range(n)) for n in (20, 0, 7)] + [bytes(range(256))]
    for _ in range(300):
        r, q = rng.randrange(4), rng.randrange(4)
        rs, qs = rng.randrange(len(refs[r]) + 1), rng.randrange(len(reads[q]) + 1)
        rl, ql = rng.randrange(len(refs[r]) - rs + 1), rng.randrange(min(len(reads[q]) - qs, 25) + 1)
        for rev in (False, True):
            for minus in (False, True):
                for whole in (False, True):
                    spec, = sw.normalise_pairs([(r, q, rs, None if whole else rl, qs, WHOLE if whole else ql, rev, "-" if minus else "+")])
                    assert len(spec) == (8 if minus else 7)
                    n, m = (len(refs[r]) - rs, len(reads[q]) - qs) if whole else (rl, ql)
                    a, b = aligner.cut_segments(refs, reads, spec)
                    assert (len(a), len(b)) == (n, m)
                    read_reversed = rev != minus
                    for i in range(1, m + 1):
                        for j in ((1, n) if n else ()):
                            qi, rj = aligner.cell_to_source(spec, (n, m), i, j)
                            assert (qi, rj) == (qs + m - i if read_reversed else qs + i - 1, rs + n - j if rev else rs + j - 1)
                            src = reads[q][qi]
                            assert b[i - 1] == (sw.COMPLEMENT[src] if minus else src) and refs[r][rj] == a[j - 1]
                    assert a == (refs[r][rs:rs + n][::-1] if rev else refs[r][rs:rs + n])
                    cut = reads[q][qs:qs + m]
                    if minus:
                        cut = sw.revcomp(cut)
                    assert b == (cut[::-1] if rev else cut)


def _bare_batch(refs, reads, pairs):
    pb = sw.PairBatch.__new__(sw.PairBatch)
    pb._h = None
    pb._refs, pb._reads = refs, reads
    pb._specs = sw.normalise_pairs(pairs)
    return pb


def test_pair_batch_methods_need_no_library_state():
    pb = _bare_batch([b"ACGTACGTAC"], [b"ttgca"], [(0, 0, 2, 6, 1, 3, False, "-"), (0, 0, 2, 6, 1, 3, True, "-"), (0, 0), (0, 0, 0, None, 0, None, 0, "-")])
    assert pb.n_pairs() == 4 and [pb.strand(k) for k in range(4)] == ["-", "-", "+", "-"]
    assert pb.segments(0) == ("GTACGT", "gca") and pb.segments(1) == ("TGCATG", "acg") and pb.segments(3) == ("ACGTACGTAC", "tgcaa")
    # row 1 of the minus pair is the LAST byte of its read segment, row 1 of the reversed minus pair the first
    assert pb.to_source(0, 1, 1) == (3, 2) and pb.to_source(0, 3, 6) == (1, 7)
    assert pb.to_source(1, 1, 1) == (1, 7) and pb.to_source(1, 3, 6) == (3, 2)
    assert pb.to_source(3, 1, 10) == (4, 9) and pb.to_source(3, 5, 1) == (0, 0)


def test_hit_specs_of_a_minus_pair():
    """a hit (i, j) of (r, q, rs, rl, qs, ql, False, "-"): rows 1 .. i are the read segment's last i bytes, complemented, so the
    reverse extension is (r, q, rs, j, qs + ql - i, i, True, "-") -- and its segments are the two prefixes, reversed"""
    rng = random.Random(4)
    refs = [bytes(rng.choice(b"ACGTn") for _ in range(60))]
    reads = [bytes(rng.choice(b"ACGTk") for _ in range(40))]
    pb = _bare_batch(refs, reads, [(0, 0, 7, 40, 5, 30, False, "-"), (0, 0, 7, None, 5, None, False, "-"), (0, 0, 7, 40, 5, 30, True, "-"),
                                   (0, 0, 7, 40, 5, 30, False)])
    for pair, ql in ((0, 30), (1, 35)):
        a, b = aligner.cut_segments(refs, reads, pb._specs[pair])
        for i, j in ((1, 1), (ql, 40), (13, 29)):
            spec = pb._hit_spec(pair, i, j)
            assert spec == (0, 0, 7, j, 5 + ql - i, i, True, "-")
            norm, = sw.normalise_pairs([spec])
            assert aligner.cut_segments(refs, reads, norm) == (a[:j][::-1], b[:i][::-1])
            # cell (i', j') of the extension is cell (i + 1 - i', j + 1 - j') of the pair
            for ii, jj in ((1, 1), (i, j)):
                assert aligner.cell_to_source(norm, (j, i), ii, jj) == aligner.cell_to_source(pb._specs[pair], (len(a), len(b)), i + 1 - ii, j + 1 - jj)
    with pytest.raises(ValueError):
        pb._hit_spec(2, 3, 3)
    assert pb._hit_spec(3, 4, 6) == (0, 0, 7, 6, 5, 4, _capi.SPEC_REVERSE)


def test_both_strands_and_best_strand():
    got = sw.both_strands([(0, 1), (2, 3, 4, 5, 6, 7, True), (1, 1, 0, 9, 0, 9, False, "+")])
    assert got == [(0, 1, 0, WHOLE, 0, WHOLE, False), (0, 1, 0, WHOLE, 0, WHOLE, False, "-"), (2, 3, 4, 5, 6, 7, True), (2, 3, 4, 5, 6, 7, True, "-"),
                   (1, 1, 0, 9, 0, 9, False), (1, 1, 0, 9, 0, 9, False, "-")]
    assert sw.both_strands([]) == []
    with pytest.raises(ValueError) as e:
        sw.both_strands([(0, 1), (0, 1, 0, 4, 0, 4, False, "-")])
    assert "pair 1" in str(e.value)
    pb = _bare_batch([b"A"], [b"A"], got)
    pb.scores = lambda: [10, 12, 7, 7, 9, 3]
    assert pb.best_strand() == [1, 2, 4]                 # a tie goes to plus
    for other in ([(0, 0)], [(0, 0), (0, 0)], [(0, 0, 0, 1, 0, 1, False, "-"), (0, 0, 0, 1, 0, 1, False)], got[:2] + [got[2], got[5]]):
        pb = _bare_batch([b"A"], [b"A"], other)
        pb.scores = lambda: [0] * 4
        with pytest.raises(ValueError):
            pb.best_strand()
