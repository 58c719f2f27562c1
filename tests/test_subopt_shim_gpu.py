"""Option "subopt" through the JNI shim from plain C99 (tests/c/shim_subopt.c: swmi_shim_set_subopt, swmi_shim_pair_subopt): one short
and one long pair, under a fixed half-width, under AUTO and with the option off, against tests/subopt_reference.py."""
import pytest

import affine_gpu_util as u
import subopt_reference as sr

pytestmark = pytest.mark.gpu

SC = (2, -3, -4, -6)


def _lcg(n, x):
    out = []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def test_c99_shim_sets_subopt_and_reads_it(tmp_path):
    out = u.run_shim(tmp_path, "shim_subopt")
    lng = _lcg(1100, 20260)
    shrt = lng[900:940]
    ref = lng[100:260] + _lcg(50, 4242) + shrt + _lcg(50, 777) + lng[700:1100]
    want = []
    for w in (45, sr.AUTO):
        for read in (shrt, lng):
            s, s2, e2 = sr.subopt_numpy(ref, read, SC, w)
            want.append("%d %d %d mode 3" % (s, s2, e2))
    # the short read lies in the reference twice (it ends at columns 250 and 540: two maximum columns); the long read's best alignment
    # is its last 400 bases, and the runner-up under AUTO (w = 550) its bases 100 .. 259 at the reference's start
    assert want == ["80 14 469 mode 3", "801 709 654 mode 3", "80 38 229 mode 3", "801 298 149 mode 3"]
    assert out.splitlines() == want + ["unsupported", "unsupported"]
