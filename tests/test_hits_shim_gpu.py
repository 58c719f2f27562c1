"""Option "hits" through the JNI shim from plain C99 (tests/c/shim_hits.c: swmi_shim_set_hits, swmi_shim_pair_hits): one short and one
long pair under subopt = 45 with hits = 3, 1 and 0, and a run with hits and without subopt, against tests/hits_reference.py."""
import pytest

import affine_gpu_util as u
import hits_reference as hr

pytestmark = pytest.mark.gpu

SC = (2, -3, -4, -6)


def _lcg(n, x):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def test_c99_shim_sets_hits_and_reads_them(tmp_path):
    out = u.run_shim(tmp_path, "shim_hits")
    lng = _lcg(1100, 20260)
    shrt = lng[900:940]
    ref = lng[100:260] + _lcg(50, 4242) + shrt + _lcg(50, 777) + lng[700:1100]
    want = []
    for k in (3, 1):
        for read in (shrt, lng):
            h = hr.hits_numpy(ref, read, SC, 45, k)
            want.append("%d :" % len(h) + "".join(" %d %d %d ;" % e for e in h) + " mode 3")
    # the short read lies in the reference twice (two maximum columns: the first one is the primary's); the long read's best alignment
    # is its last 400 bases, the runner-up its bases 100 .. 259 at the reference's start
    assert want[0].startswith("3 : 80 40 250 ; 14 ") and want[1].startswith("3 : 801 1100 700 ; 709 1054 654 ;")
    assert want[2] == "1 : 80 40 250 ; mode 3"
    assert out.splitlines() == want + ["unsupported", "unsupported", "refused"]
