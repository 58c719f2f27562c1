"""Option "overlap" through the JNI shim from plain C99 (tests/c/shim_overlap.c: swmi_shim_set_overlap): one dovetail pair in fit
mode with the option on and off, against tests/overlap_reference.py and tests/gotoh_reference.py, and the refusal in global mode."""
import pytest

import affine_gpu_util as u
import gotoh_reference as gr
import overlap_reference as ov

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -5
SC = (2, -3, -1, -3)


def test_c99_shim_sets_overlap(tmp_path):
    out = u.run_shim(tmp_path, "shim_overlap")
    ref, read = "TTTTTACGCGGA", "ACGCGGAAAAAAA"
    o = ov.align_numpy(ref, read, SC)
    f = gr.align_numpy(ref, read, SC, gr.FIT)
    assert o == (14, [(6, ("ACGCGGA", "ACGCGGA"))]) and f[0] < o[0]           # the reference's tail is the read's head
    line = lambda e: "%d %d" % (e[0], len(e[1])) + "".join(" %d:%s/%s" % (b, ra, qa) for b, (ra, qa) in sorted(e[1], key=lambda a: a[0])) + " mode 3"
    assert out.splitlines() == [line(o), line(f), "refused %d" % ERR_UNSUPPORTED]
