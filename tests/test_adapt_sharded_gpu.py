"""sharded_files --align-mode global --extend --long-reads --band 48 --band-adapt on one MI355X, two ranks: three reads, one of two
strips, against nine references of about 1.3 kbp.  The winning reference is the long read without two stretches of 40 bases, so
that on row 1024 the alignment stands 80 columns left of the diagonal: the static band of half-width 48 loses it in strip 1,
the adaptive band follows it.  The result file must be what the mirror classes' own file driver writes with the same options,
hold the total tests/adapt_reference.py gives, and differ from the file written without --band-adapt."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import adapt_reference as ar
import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (2, -4, -2, -4)
W = 48


def _fasta(recs):
    out = []
    for meta, seq in recs:
        out.append(meta)
        out.extend(seq[k:k + 80] for k in range(0, len(seq), 80))
    return "\n".join(out) + "\n"


def _body(text):
    head, rest = text.split(os.linesep, 1)
    assert head.startswith("Execution Time = ") and head.endswith(" ms")
    return rest


def test_sharded_files_band_adapt(tmp_path):
    rng = random.Random(9990)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir, off_dir = (tmp_path / d for d in ("reference", "input", "out", "control", "off"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir, off_dir):
        d.mkdir()
    near = rand(1300)
    long_read = near[:300] + rand(40) + near[300:700] + rand(40) + near[700:1220]
    reads = [long_read, long_read[:70], rand(50)]
    refs = [(">gi|r%d" % k, rand(rng.randint(1290, 1330))) for k in range(8)]
    refs.insert(5, (">gi|near", near))
    (ref_dir / "a.fa").write_text(_fasta(refs[:4]))
    (ref_dir / "b.fa").write_text(_fasta(refs[4:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    adaptive = ar.align(near, long_read, SCORES, W)
    static = gr.align_numpy(near, long_read, SCORES, gr.GLOBAL, W, True, cells=True)
    assert adaptive[0] > static[0] and adaptive[3][1] != gr.windows(1300, 1300, W)[1]
    assert adaptive[:3] == gr.align_numpy(near, long_read, SCORES, gr.GLOBAL, 0, True, cells=True)     # what no band at all finds
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "global", "--extend", "--long-reads", "--band", str(W), "--band-adapt"]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    ctx = sw.Context(0)
    try:
        for out, adapt in ((ctl_dir, True), (off_dir, None)):
            sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=W, extend=True, band_adapt=adapt).call(
                [str(ref_dir), str(in_dir), None, str(out), None, None], (list(SCORES), None))
            assert ctx.options.get("band_adapt", 0) == 0          # (put back after the call)
    finally:
        ctx.close()
    # the winner's total as the file states it: the long read under the adaptive band, and the two short reads in full
    short = [gr.align_numpy(near, q, SCORES, gr.GLOBAL, 0, True)[0] for q in reads[1:]]
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    off = open(off_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want) != _body(off)
    assert ">gi|near" in got and ">gi|near" in off
    from sparksmithwaterman_amd import io as swio
    site = lambda e: swio.TAB + e[1][0][1][0] + swio.NEWLINE + swio.TAB + e[1][0][1][1] + swio.NEWLINE
    assert "Maximum alignment score = %d%s" % (adaptive[0] + sum(short), swio.NEWLINE) in got and site(adaptive) in got and site(static) not in got
    assert "Maximum alignment score = %d%s" % (static[0] + sum(short), swio.NEWLINE) in off and site(static) in off
