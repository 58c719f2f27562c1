"""swmi_shim_set_cigar / swmi_shim_pair_cigar -- what nativeSetCigar and nativePairCigar of bindings/jni/swmi_jni.c forward to --
from plain C99 (tests/c/shim_cigar.c): one global pair's entries and nm against tests/cigar_reference.py, and the shim's
refusals (null context, value 3, negative pair, alignment out of range: checked inside the program; a run with cigar = 0)."""
import pytest

from sparksmithwaterman_amd import _capi

import affine_gpu_util as u
import cigar_reference as cr
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

REF, READ = "GGCCCAGTCCAGCCCAACTAACGAATAAGTAGAATCCTCGGAAGT", "GGCCTAGTCCAGATCCTCGGAAGT"
SC = (2, -4, -2, -4)


def test_c99_shim_returns_the_cigar(tmp_path):
    score, alns, cells = gr.align_scalar(REF, READ, SC, gr.GLOBAL, cells=True)
    (begin, (ra, qa)), = alns
    assert "_" * 21 in qa
    lines = []
    for c in (2, 1):
        ent, nm = cr.cigar(ra, qa, c)
        assert nm == 22
        ops = " ".join("%d:%d" % (n, {v: k for k, v in _capi.CIGAR_CHARS.items()}[op]) for n, op in ent)
        lines.append("mode 3 begin %d cell %d %d nm %d %s" % (begin, cells[0][0], cells[0][1], nm, ops))
    assert lines[0].endswith("nm 22 4:7 1:8 7:7 21:2 12:7") and lines[1].endswith("nm 22 12:0 21:2 12:0")
    out = u.run_shim(tmp_path, "shim_cigar")
    assert out.splitlines() == lines + ["refused %d" % _capi.ERR_UNSUPPORTED]
