"""Per-read profiles through the JNI shim from plain C99 (tests/c/shim_profile.c: swmi_shim_set_read_profiles): one pair in local
mode without profiles, under a profile that forgives one mismatch and with the profiles cleared, against tests/gotoh_reference.py and
tests/profile_reference.py, and the three refusals."""
import pytest

import affine_gpu_util as u
import gotoh_reference as gr
import profile_reference as pr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
SC = (2, -3, -1, -3)


def test_c99_shim_sets_read_profiles(tmp_path):
    out = u.run_shim(tmp_path, "shim_profile")
    ref, read = "GGACGTTCGAtt", "ACGATCGA"
    profile = [[0] * 4 if i == 3 else [2 if c == q else -3 for c in "ACGT"] for i, q in enumerate(read)]
    plain = gr.align_numpy(ref, read, SC)
    prof = pr.align_numpy(ref, read, "ACGT", profile, SC)
    assert prof == (14, [(3, ("ACGTTCGA", "ACGATCGA"))]) and plain[0] < prof[0]          # the whole read, through position 4
    line = lambda e: "%d %d" % (e[0], len(e[1])) + "".join(" %d:%s/%s" % (b, ra, qa) for b, (ra, qa) in sorted(e[1], key=lambda a: a[0])) + " mode 3"
    assert out.splitlines() == [line(plain), line(prof), line(plain), "refused %d" % ERR_INVALID, "refused %d" % ERR_INVALID, line(plain),
                                "refused %d" % ERR_UNSUPPORTED]
