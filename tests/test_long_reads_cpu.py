"""Host-side checks of the long-read feature (option "long_reads") that need no GPU: the expected values of
tests/test_long_reads_gpu.py do not rest on one restatement, and the sharded driver's parser knows --long-reads."""
import pytest

import gotoh_reference as gr
import long_reads_cases as lc


@pytest.mark.parametrize("case", lc.seam_cases(), ids=lambda c: c[0])
def test_seam_cases_scalar_and_numpy_agree(case):
    name, ref, read, sc = case
    assert len(read) > lc.STRIP
    for tie in (0, 1):
        want = gr.align_scalar(ref, read, sc, tie_mode=tie)
        assert gr.align_numpy(ref, read, sc, tie_mode=tie) == want, (name, tie)
        assert want[0] > 0 and want[1]
    # what each case is there for
    s, al = gr.align_numpy(ref, read, sc)
    ends = [a[0] + len(a[1][0].replace(gr.GAP_CHAR, "")) - 1 for a in al]                 # last reference column
    spelled = [len(a[1][1].replace(gr.GAP_CHAR, "")) for a in al]                         # read bases
    if name == "diagonal":
        assert s >= 80 * sc[0] and ref[30:110] in al[0][1][0] and ref[30:110] in al[0][1][1]
    if name == "insertion":
        assert s == 200 * 2 - 6 - 40 and al[0][1][0] == ref[20:120] + gr.GAP_CHAR * 40 + ref[120:220]
    if name.startswith("deletion"):
        assert s >= 128 * 5 - 6 - 24 and ref[20:80] + gr.GAP_CHAR * 12 + ref[92:160] in al[0][1][1]
    if name == "ties_both_strips":
        assert len(al) == 2 and ends == [64, 64]
    if name in ("later_strip_higher", "later_strip_lower"):
        assert len(al) == 1 and s == 64 * 5 and spelled == [64]


@pytest.mark.parametrize("case", lc.ends_cases(), ids=lambda c: c[0])
def test_ends_cases_scalar_and_numpy_agree(case):
    """both tie modes; the two pairs with a 2500-base reference (2.5 and 5 million cells in the scalar restatement) under one
    tie mode each"""
    name, ref, read, sc, mode = case
    ties = {"global_1025_2500": (1,), "global_2049_2500": (0,)}.get(name, (0, 1))
    for tie in ties:
        want = gr.align_scalar(ref, read, sc, mode, tie_mode=tie)
        assert gr.align_numpy(ref, read, sc, mode, tie_mode=tie) == want, (name, tie)
        for begin, (ra, qa) in want[1]:
            assert qa.replace(gr.GAP_CHAR, "") == read
            if mode == lc.GLOBAL:
                assert ra.replace(gr.GAP_CHAR, "") == ref
        if name == "fit_head_overhang":
            assert all(a[1][0].startswith(gr.GAP_CHAR * 1100) and not a[1][0].startswith(gr.GAP_CHAR * 1101) for a in want[1])


def test_sharded_files_parser_accepts_long_reads():
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "r", "--in-dir", "i", "--out-dir", "o"]
    assert sharded_files._parser().parse_args(base).long_reads is False
    args = sharded_files._parser().parse_args(base + ["--long-reads", "--scores", "5,-3,-2,-6"])
    assert args.long_reads is True and args.align_mode == "local"
