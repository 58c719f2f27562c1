"""sharded_files --align-mode global with six-entry scores (two-piece gaps) on one MI355X, two ranks: three reads against seven
references of about 300 bases.  The winning reference is the first read without a stretch of 30 bases, so that its alignment holds
one long insertion, which the second piece charges 24 + 30 where the first charges 4 + 60.  The result file must be what the mirror
classes' own file driver writes with the same scores, hold the total tests/twopiece_reference.py gives, and differ from the file
written with the first four entries alone."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import gotoh_reference as gr
import twopiece_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (2, -4, -2, -4, -1, -24)


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


def test_sharded_files_two_piece(tmp_path):
    rng = random.Random(8820)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir, one_dir = (tmp_path / d for d in ("reference", "input", "out", "control", "one"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir, one_dir):
        d.mkdir()
    near = rand(300)
    reads = [near[:140] + rand(30) + near[140:], near[:290], near[20:]]
    refs = [(">gi|r%d" % k, rand(rng.randint(290, 310))) for k in range(6)]
    refs.insert(4, (">gi|near", near))
    (ref_dir / "a.fa").write_text(_fasta(refs[:3]))
    (ref_dir / "b.fa").write_text(_fasta(refs[3:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    two = [tr.align_numpy(near, q, SCORES) for q in reads]
    one = [gr.align_numpy(near, q, SCORES[:4], gr.GLOBAL) for q in reads]
    assert two[0][0] == one[0][0] + 30 - 20 and "_" * 30 in two[0][1][0][1][0]
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores=" + ",".join(map(str, SCORES)), "--align-mode", "global"]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    ctx = sw.Context(0)
    try:
        for out, sc in ((ctl_dir, SCORES), (one_dir, SCORES[:4])):
            sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_GLOBAL).call(
                [str(ref_dir), str(in_dir), None, str(out), None, None], (list(sc), None))
            assert ctx.options.get("gap_open2", 0) == 0 and ctx.options.get("gap2", 0) == 0      # (put back after the call)
    finally:
        ctx.close()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    off = open(one_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want) != _body(off)
    assert ">gi|near" in got and ">gi|near" in off
    from sparksmithwaterman_amd import io as swio
    assert "Maximum alignment score = %d%s" % (sum(e[0] for e in two), swio.NEWLINE) in got
    assert "Maximum alignment score = %d%s" % (sum(e[0] for e in one), swio.NEWLINE) in off
    for e in two:
        assert swio.TAB + e[1][0][1][0] + swio.NEWLINE + swio.TAB + e[1][0][1][1] + swio.NEWLINE in got
