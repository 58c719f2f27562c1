"""sharded_files --align-mode fit --overlap --long-reads on one MI355X, two ranks: three reads, one of two strips, against eight
references of 300 to 700 bases in two files.  The winning reference's tail continues into the long read (a dovetail of 250 bases
with 850 read bases hanging over), its head is the tail of another read and the third read lies inside it: fit pays for every
overhang and gives that reference 1,199 less.  The result file must be what the mirror classes' own file driver writes with
overlap=True, hold the total tests/overlap_reference.py gives, and differ from the file written without --overlap."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import gotoh_reference as gr
import overlap_reference as ov

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (5, -3, -2, -6)


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


def test_sharded_files_overlap(tmp_path):
    rng = random.Random(8820)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir, off_dir = (tmp_path / d for d in ("reference", "input", "out", "control", "off"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir, off_dir):
        d.mkdir()
    near = rand(600)
    reads = [near[350:] + rand(850), near[100:300], rand(80) + near[:120]]
    assert len(reads[0]) == 1100
    refs = [(">gi|r%d" % k, rand(rng.randint(300, 700))) for k in range(7)]
    refs.insert(5, (">gi|near", near))
    (ref_dir / "a.fa").write_text(_fasta(refs[:4]))
    (ref_dir / "b.fa").write_text(_fasta(refs[4:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    exp = [ov.align_numpy(near, q, SCORES) for q in reads]
    assert [e[0] for e in exp] == [5 * 250, 5 * 200, 5 * 120] and all(len(e[1]) == 1 for e in exp)
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "fit", "--overlap", "--long-reads"]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    ctx = sw.Context(0)
    try:
        for out, overlap in ((ctl_dir, True), (off_dir, None)):
            sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_FIT, long_reads=True, overlap=overlap).call(
                [str(ref_dir), str(in_dir), None, str(out), None, None], (list(SCORES), None))
            assert ctx.options.get("overlap", 0) == 0                 # (put back after the call)
    finally:
        ctx.close()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    off = open(off_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want) != _body(off)
    from sparksmithwaterman_amd import io as swio
    site = lambda e: swio.TAB + e[1][0][1][0] + swio.NEWLINE + swio.TAB + e[1][0][1][1] + swio.NEWLINE
    assert "Maximum alignment score = %d%s" % (sum(e[0] for e in exp), swio.NEWLINE) in got and ">gi|near" in got
    assert all(site(e) in got for e in exp)
    fit = sum(gr.align_numpy(near, q, SCORES, gr.FIT)[0] for q in reads)       # fit pays for the overhangs
    assert fit < sum(e[0] for e in exp) - 1000 and "Maximum alignment score = %d%s" % (fit, swio.NEWLINE) in off
