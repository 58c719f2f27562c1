"""The JNI shim's pair-list calls (swmi_shim_align_pairs, swmi_shim_pair_results, swmi_shim_pair_alignment) from plain C99:
tests/c/shim_pairs.c prints a dozen pairs, and every line is compared with the oracle on the segments cut -- and reversed -- here."""
import pytest

from oracle import sw_oracle as orc

import affine_gpu_util as u

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)


def lcg(x, n):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


SPECS = [(0, 0, 30, 160, 0, 120, 0), (0, 0, 30, 160, 0, 120, 1), (0, 0, 57, 93, 11, 64, 0), (0, 0, 57, 93, 11, 64, 1),
         (0, 1, 200, 101, 3, 50, 0), (0, 1, 203, -1, 1, -1, 1), (0, 1, 190, 70, 0, 0, 0), (1, 0, 0, 150, 40, 33, 0),
         (0, 0, 1, 5, 1, 6, 0), (0, 1, 399, 1, 59, 1, 1), (0, 0, 30, 160, 0, 120, 0), (0, 0, 31, 160, 1, 119, 1)]      # as in shim_pairs.c


def test_shim_pairs(tmp_path):
    refs = [lcg(1, 400), lcg(2, 150)]
    reads = ["".join(("TGCA"[x & 3] if x % 17 == 16 else refs[0][at + x]).lower() for x in range(n)) for at, n in ((40, 120), (210, 60))]
    lines = u.run_shim(tmp_path, "shim_pairs").splitlines()
    assert len(lines) == len(SPECS) + 3
    for line, (r, q, rs, rl, qs, ql, rev) in zip(lines, SPECS):
        ref = refs[r][rs:] if rl < 0 else refs[r][rs:rs + rl]
        read = reads[q][qs:] if ql < 0 else reads[q][qs:qs + ql]
        if rev:
            ref, read = ref[::-1], read[::-1]
        score, alns = orc.opt_alignments((ref, read), (5, -3, -4), b"aid-", 0, with_cells=True)
        if score == 0 and ref and read:                     # a degenerate pair: one (0, "", "") per cell, row-major
            want = ["0:%d:%d:/" % (i, j) for i in range(1, len(read) + 1) for j in range(1, len(ref) + 1)]
        else:
            want = ["%d:%d:%d:%s/%s" % (b, i, j, ra, qa) for b, (ra, qa), (i, j) in alns]
        assert line.split() == [str(score), str(len(want))] + want, (r, q, rs, rl, qs, ql, rev)
        assert len(want) < 200
    assert lines[-3:] == ["views %d" % ERR_UNSUPPORTED, "ints %d" % ERR_INVALID, "bad %d 1" % ERR_INVALID]
