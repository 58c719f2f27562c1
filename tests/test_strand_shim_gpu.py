"""The minus strand through the JNI shim's pair-list calls from plain C99: tests/c/shim_strand.c prints the dozen pairs of
shim_pairs.c with flags 4 and 5 on half of them (read 1 is the reverse complement of its stretch of the reference), and every
line is compared with the oracle on the segments cut, reversed and complemented here."""
import pytest

import sparksmithwaterman_amd as sw
from oracle import sw_oracle as orc

import affine_gpu_util as u

pytestmark = pytest.mark.gpu

ERR_INVALID = -1                            # swmi_status (include/swmi.h)


def lcg(x, n):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


SPECS = [(0, 0, 30, 160, 0, 120, 0), (0, 0, 30, 160, 0, 120, 1), (0, 0, 57, 93, 11, 64, 4), (0, 0, 57, 93, 11, 64, 5),
         (0, 1, 200, 101, 3, 50, 4), (0, 1, 203, -1, 1, -1, 5), (0, 1, 190, 70, 0, 0, 0), (1, 0, 0, 150, 40, 33, 0),
         (0, 0, 1, 5, 1, 6, 4), (0, 1, 399, 1, 59, 1, 5), (0, 1, 200, 101, 3, 50, 0), (0, 1, 201, 100, 0, 60, 5)]      # as in shim_strand.c


def test_shim_strand(tmp_path):
    refs = [lcg(1, 400), lcg(2, 150)]
    fwd = refs[0][210:270]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    reads = ["".join(("TGCA"[x & 3] if x % 17 == 16 else refs[0][40 + x]).lower() for x in range(120)),
             "".join(("TGCA"[x & 3] if x % 17 == 16 else comp[fwd[59 - x]]).lower() for x in range(60))]
    lines = u.run_shim(tmp_path, "shim_strand").splitlines()
    assert len(lines) == len(SPECS) + 1
    best = {}
    for line, (r, q, rs, rl, qs, ql, flags) in zip(lines, SPECS):
        ref = refs[r][rs:] if rl < 0 else refs[r][rs:rs + rl]
        read = reads[q][qs:] if ql < 0 else reads[q][qs:qs + ql]
        if flags & 4:
            read = sw.revcomp(read)
        if flags & 1:
            ref, read = ref[::-1], read[::-1]
        score, alns = orc.opt_alignments((ref, read), (5, -3, -4), b"aid-", 0, with_cells=True)
        if score == 0 and ref and read:                     # a degenerate pair: one (0, "", "") per cell, row-major
            want = ["0:%d:%d:/" % (i, j) for i in range(1, len(read) + 1) for j in range(1, len(ref) + 1)]
        else:
            want = ["%d:%d:%d:%s/%s" % (b, i, j, ra, qa) for b, (ra, qa), (i, j) in alns]
        assert line.split() == [str(score), str(len(want))] + want, (r, q, rs, rl, qs, ql, flags)
        assert len(want) < 200
        best[(rs, rl, qs, ql, flags)] = score
    # the flag did its work: the same bytes align on the minus strand and not on the plus strand
    assert best[(200, 101, 3, 50, 4)] > 5 * 40 > 2 * best[(200, 101, 3, 50, 0)]
    assert lines[-1] == "flag2 %d 1" % ERR_INVALID
