"""sharded_files --align-mode global --extend --long-reads --xdrop on one MI355X, two ranks: three reads, one of three strips,
against nine references of about 2.1 kbp.  The winning reference shares the long read's first 700 bases and its last 900, with
500 unrelated bases between them: without the drop-off rule the extension runs on to the common tail, with it the sweep ends
behind strip 0 and the head is the answer.  The result file must be what the mirror classes' own file driver writes with the
same options, hold the total tests/xdrop_reference.py gives, and differ from the file written without --xdrop."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import gotoh_reference as gr
import xdrop_reference as xr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (2, -4, -2, -4)


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


def test_sharded_files_xdrop(tmp_path):
    rng = random.Random(9790)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir, off_dir = (tmp_path / d for d in ("reference", "input", "out", "control", "off"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir, off_dir):
        d.mkdir()
    head, tail = rand(700), rand(900)
    long_read = head + rand(500) + tail
    near = head + rand(500) + tail
    reads = [long_read, long_read[:70], rand(50)]
    refs = [(">gi|r%d" % k, rand(rng.randint(2090, 2130))) for k in range(8)]
    refs.insert(5, (">gi|near", near))
    (ref_dir / "a.fa").write_text(_fasta(refs[:4]))
    (ref_dir / "b.fa").write_text(_fasta(refs[4:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    d = [best - seam for best, seam in xr.drops(near, long_read, SCORES, 0)]
    X = d[0] - 1
    assert len(d) == 2 and X >= 1
    stopped, full = xr.align(near, long_read, SCORES, X), xr.align(near, long_read, SCORES, 0)
    assert stopped[0] == 1400 and stopped[3] == 1024 and full[0] > 1400 and full[3] == 2100
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "global", "--extend", "--long-reads", "--xdrop", str(X)]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    ctx = sw.Context(0)
    try:
        for out, xdrop in ((ctl_dir, X), (off_dir, None)):
            sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_GLOBAL, long_reads=True, extend=True, xdrop=xdrop).call(
                [str(ref_dir), str(in_dir), None, str(out), None, None], (list(SCORES), None))
            assert ctx.options.get("xdrop", 0) == 0               # (put back after the call)
    finally:
        ctx.close()
    # the winner's total as the file states it: the stopped long read, and the two short reads in full
    short = [gr.align_numpy(near, q, SCORES, gr.GLOBAL, 0, True)[0] for q in reads[1:]]
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    off = open(off_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want) != _body(off)
    assert ">gi|near" in got and ">gi|near" in off
    from sparksmithwaterman_amd import io as swio
    site = lambda e: swio.TAB + e[1][0][1][0] + swio.NEWLINE + swio.TAB + e[1][0][1][1] + swio.NEWLINE
    assert "Maximum alignment score = %d%s" % (stopped[0] + sum(short), swio.NEWLINE) in got and site(stopped) in got and site(full) not in got
    assert "Maximum alignment score = %d%s" % (full[0] + sum(short), swio.NEWLINE) in off and site(full) in off
