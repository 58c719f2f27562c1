"""Option "end_bonus" through the JNI shim from plain C99 (tests/c/shim_end_bonus.c: swmi_shim_set_end_bonus,
swmi_shim_pair_end_score): one short and one long pair, under a bonus on either side of the short pair's choice, under the largest
bonus and with the option off, against tests/end_bonus_reference.py."""
import pytest

import affine_gpu_util as u
import end_bonus_reference as er

pytestmark = pytest.mark.gpu

SC = (5, -4, -3, -5)


def _lcg(n, x):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def test_c99_shim_sets_end_bonus_and_reads_it(tmp_path):
    out = u.run_shim(tmp_path, "shim_end_bonus")
    lng = _lcg(1100, 20261)
    ref = lng[:59] + "ACGT"[("ACGT".index(lng[59]) + 1) & 3] + lng[60:1090] + _lcg(30, 4243)
    want, taken = [], []
    for bonus in (3, 5, 1 << 30):
        for read in (lng[:60], lng):
            score, _, _, took, ends = er.align(ref, read, SC, bonus)
            want.append("%d %d %d %d %d mode 3" % ((score,) + ends + (int(took),)))
            taken.append(took)
    # the short read's last base meets the substituted one: row m is best behind a one-base deletion, at column 61 and 3 below the
    # best score (at cell (59, 59)), so bonus 3 is the tie that changes nothing; the long read's tail does not match
    assert taken == [False, False, True, False, True, True]
    assert want[0] == "295 295 292 61 0 mode 3" and want[2] == "292 295 292 61 1 mode 3"
    assert out.splitlines() == want + ["unsupported", "unsupported"]
