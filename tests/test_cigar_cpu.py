"""Option "cigar" without a device: the contract's restatement (tests/cigar_reference.py) on hand-written cases, the text form,
the edit distance of a known pair, and the boundary -- the library exports swmi_pair_cigar, Python's constants are the header's,
and the option is refused without a context."""
import os
import re

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi, aligner

import cigar_reference as cr
import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_empty_alignment():
    assert cr.cigar("", "", 2) == ([], 0)
    assert cr.cigar("", "", 1) == ([], 0)


def test_reference_one_column():
    assert cr.cigar("A", "A", 2) == ([(1, "=")], 0)
    assert cr.cigar("A", "C", 2) == ([(1, "X")], 1)
    assert cr.cigar("A", "C", 1) == ([(1, "M")], 1)


def test_reference_lone_gaps():
    # the column whose REFERENCE string has '_' consumes a read base: I; the one whose read string has '_' is D
    assert cr.cigar("_", "G", 2) == ([(1, "I")], 1)
    assert cr.cigar("G", "_", 2) == ([(1, "D")], 1)
    assert cr.cigar("AC__GT", "ACTTGT", 2) == ([(2, "="), (2, "I"), (2, "=")], 2)
    assert cr.cigar("ACTTGT", "AC__GT", 1) == ([(2, "M"), (2, "D"), (2, "M")], 2)


def test_reference_equality_is_upper_case_equality():
    assert cr.cigar("a", "A", 2) == ([(1, "=")], 0)
    assert cr.cigar("k*\xe9", "K*\xc9", 2) == ([(3, "=")], 0)         # e-acute: 0xE9 upper-cases to 0xC9
    assert cr.cigar("\xff\xf7", "\xdf\xd7", 2) == ([(2, "X")], 2)      # 0xFF and 0xF7 only equal themselves
    with pytest.raises(AssertionError):
        cr.cigar("_", "_", 2)                                           # no column is a gap on both sides


def test_reference_mode_1_merges_eq_and_x():
    assert cr.cigar("ACG", "ATG", 2) == ([(1, "="), (1, "X"), (1, "=")], 1)
    assert cr.cigar("ACG", "ATG", 1) == ([(3, "M")], 1)
    assert cr.cigar("ACG_T", "ATGCT", 1) == ([(3, "M"), (1, "I"), (1, "M")], 2)


def test_cigar_string_round_trip():
    ent = [(12, "="), (1, "X"), (3, "I"), (40, "=")]
    text = sw.cigar_string(ent)
    assert text == "12=1X3I40="
    assert [(int(n), op) for n, op in re.findall(r"(\d+)([MIDX=])", text)] == ent
    assert sw.cigar_string([]) == ""
    assert sw.cigar_string(cr.cigar("AC__GT", "ACTTGT", 1)[0]) == "2M2I2M"


def test_nm_of_a_known_pair():
    # global alignment of ACGTACGT (reference) with ACTTACG (read): one substitution, one deleted reference base
    score, alns = gr.align_scalar("ACGTACGT", "ACTTACG", (5, -3, -4, 0), gr.GLOBAL)[:2]
    assert score == 6 * 5 - 3 - 4
    (begin, (ra, qa)), = alns
    assert (ra, qa) == ("ACGTACGT", "ACTTACG_")
    assert cr.cigar(ra, qa, 2) == ([(2, "="), (1, "X"), (4, "="), (1, "D")], 2)
    assert cr.cigar(ra, qa, 1) == ([(7, "M"), (1, "D")], 2)


def test_library_exports_the_accessor_and_constants_match_the_header():
    lib = _capi.load()
    assert lib.swmi_pair_cigar is not None
    src = open(os.path.join(ROOT, "include", "swmi.h")).read()
    header = {name: int(val) for name, val in re.findall(r"#define\s+SWMI_CIGAR_(\w+)\s+(\d+)u", src)}
    assert header == {"M": 0, "I": 1, "D": 2, "EQ": 7, "X": 8}
    assert header == {"M": sw.CIGAR_M, "I": sw.CIGAR_I, "D": sw.CIGAR_D, "EQ": sw.CIGAR_EQ, "X": sw.CIGAR_X}
    assert (aligner.CIGAR_M, aligner.CIGAR_I, aligner.CIGAR_D, aligner.CIGAR_EQ, aligner.CIGAR_X) == (0, 1, 2, 7, 8)
    assert _capi.CIGAR_CHARS == {0: "M", 1: "I", 2: "D", 7: "=", 8: "X"}


def test_option_and_accessor_are_refused_without_a_context():
    lib = _capi.load()
    for v in (0, 1, 2, 3):
        assert lib.swmi_set_option(None, b"cigar", v) == _capi.ERR_INVALID
    assert lib.swmi_pair_cigar(None, 0, 0, None, None, None, None, None, None) == _capi.ERR_INVALID
