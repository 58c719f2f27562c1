"""Pair lists without a GPU: the ctypes mirror of swmi_pair_spec against the header text, the tuple handling of
normalise_pairs, and the host-side cutting and coordinate mapping that tests/test_pairs_gpu.py takes its expected inputs from
(cut_segments, cell_to_source: what PairBatch.segments and PairBatch.to_source do) against plain slicing."""
import ctypes
import os
import random
import re

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi, aligner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "swmi.h")).read()
WHOLE = _capi.SPEC_WHOLE


def test_pair_spec_mirrors_the_header():
    body = re.search(r"typedef struct swmi_pair_spec \{(.*?)\} swmi_pair_spec;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint32_t "), decl
            fields += [name.strip() for name in decl[len("uint32_t "):].split(",")]
    assert fields == ["ref", "read", "ref_start", "ref_len", "read_start", "read_len", "flags", "reserved"]
    assert [name for name, _ in _capi.PairSpec._fields_] == fields
    assert all(t is ctypes.c_uint32 for _, t in _capi.PairSpec._fields_)
    assert ctypes.sizeof(_capi.PairSpec) == 32
    assert [getattr(_capi.PairSpec, name).offset for name in fields] == list(range(0, 32, 4))
    assert int(re.search(r"#define SWMI_SPEC_REVERSE\s+(0x[0-9A-Fa-f]+)u", HEADER).group(1), 16) == _capi.SPEC_REVERSE == 1
    assert int(re.search(r"#define SWMI_SPEC_WHOLE\s+(0x[0-9A-Fa-f]+)u", HEADER).group(1), 16) == WHOLE == 0xFFFFFFFF


def test_the_abi_version_stays_3():
    assert re.search(r"#define SWMI_ABI_VERSION\s+(\d+)", HEADER).group(1) == "3"
    assert _capi.load().swmi_abi_version() == 3


def test_the_three_functions_are_bound():
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS}
    for name in ("swmi_batch_upload_pairs", "swmi_batch_set_pairs", "swmi_batch_pair_spec"):
        assert name in bound and bound[name][0] is ctypes.c_int and hasattr(_capi.load(), name)
    assert len(bound["swmi_batch_upload_pairs"][1]) == 10 and len(bound["swmi_batch_set_pairs"][1]) == 4


def test_normalise_pairs_takes_the_three_forms():
    got = sw.normalise_pairs([(0, 1), [2, 3, 4, 5, 6, 7], (2, 3, 4, 5, 6, 7, True), (2, 3, 4, None, 6, WHOLE, 0), (1, 0, 0, 0, 0, 0, False)])
    assert got == [(0, 1, 0, WHOLE, 0, WHOLE, False), (2, 3, 4, 5, 6, 7, False), (2, 3, 4, 5, 6, 7, True), (2, 3, 4, WHOLE, 6, WHOLE, False),
                   (1, 0, 0, 0, 0, 0, False)]
    assert sw.normalise_pairs([]) == [] and sw.normalise_pairs(iter([(0, 0)])) == [(0, 0, 0, WHOLE, 0, WHOLE, False)]
    assert sw.normalise_pairs(sw.normalise_pairs([(0, 1), (2, 3, 4, 5, 6, 7, True)])) == sw.normalise_pairs([(0, 1), (2, 3, 4, 5, 6, 7, True)])
    import numpy as np
    assert sw.normalise_pairs([tuple(np.arange(6, dtype=np.int64))]) == [(0, 1, 2, 3, 4, 5, False)]       # integers of any kind


@pytest.mark.parametrize("bad", [[(0,)], [(0, 1, 2)], [(0, 1, 2, 3, 4)], [(0, 1, 2, 3, 4, 5, True, 0)], [5], [(0, 1), None],
                                 [(0, -1)], [(0, 1, 0, -2, 0, 3)], [(1 << 32, 0)], [(0, 1, 0, 1 << 32, 0, 0)], [(0.0, 1)], [("0", 1)],
                                 [(0, 1, 2, 3, 4, 5, 2)], [(0, 1, 2, 3, 4, 5, "yes")], [(0, 1, 2, 3, 4, 5, None)], [(True, 0)],
                                 [(None, 0)], [(0, 1, None, 3, 4, 5)]])
def test_normalise_pairs_refuses(bad):
    with pytest.raises(ValueError) as e:
        sw.normalise_pairs(bad)
    assert "pair %d" % (len(bad) - 1) in str(e.value)


def test_segments_and_to_source_against_plain_slicing():
    rng = random.Random(1)
    refs = [bytes(rng.randrange(256) for _ in range(n)) for n in (50, 1, 0, 33)]
    reads = [bytes(rng.randrange(256) for _ in range(n)) for n in (20, 0, 7)]
    for _ in range(300):
        r, q = rng.randrange(4), rng.randrange(3)
        rs, qs = rng.randrange(len(refs[r]) + 1), rng.randrange(len(reads[q]) + 1)
        rl, ql = rng.randrange(len(refs[r]) - rs + 1), rng.randrange(len(reads[q]) - qs + 1)
        for rev in (False, True):
            for whole in (False, True):
                spec, = sw.normalise_pairs([(r, q, rs, None if whole else rl, qs, WHOLE if whole else ql, rev)])
                n, m = (len(refs[r]) - rs, len(reads[q]) - qs) if whole else (rl, ql)
                a, b = aligner.cut_segments(refs, reads, spec)
                assert (len(a), len(b)) == (n, m)
                # byte j - 1 of the reference segment (column j) and byte i - 1 of the read segment (row i) are the source bytes
                # to_source names: start + j - 1 forward, start + len - j reversed (swmi.h)
                for i in range(1, m + 1):
                    for j in ((1, n) if n else ()):
                        qi, rj = aligner.cell_to_source(spec, (n, m), i, j)
                        assert (qi, rj) == ((qs + m - i, rs + n - j) if rev else (qs + i - 1, rs + j - 1))
                        assert reads[q][qi] == b[i - 1] and refs[r][rj] == a[j - 1]
                assert a == (refs[r][rs:rs + n][::-1] if rev else refs[r][rs:rs + n])
                assert b == (reads[q][qs:qs + m][::-1] if rev else reads[q][qs:qs + m])


def test_pair_batch_methods_need_no_library_state():
    """segments / to_source of a PairBatch are the two functions above on its own copy of the sources"""
    pb = sw.PairBatch.__new__(sw.PairBatch)
    pb._h = None
    pb._refs, pb._reads = [b"ACGTACGTAC"], [b"ttgca"]
    pb._specs = sw.normalise_pairs([(0, 0, 2, 6, 1, 3, True), (0, 0)])
    assert pb.n_pairs() == 2
    assert pb.segments(0) == ("TGCATG", "cgt") and pb.segments(1) == ("ACGTACGTAC", "ttgca")
    assert pb.to_source(0, 1, 1) == (3, 7) and pb.to_source(0, 3, 6) == (1, 2) and pb.to_source(1, 5, 10) == (4, 9)
