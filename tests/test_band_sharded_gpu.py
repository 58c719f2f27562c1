"""sharded_files --band --long-reads --align-mode on one MI355X, two ranks: a 1300-base read against two small reference files.
The result file must be what the mirror classes' own file driver writes with the same options, and the winner's alignment must
be the one tests/gotoh_reference.py builds."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (5, -3, -2, -6)
W = 30


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


def test_sharded_files_band(tmp_path):
    rng = random.Random(9950)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir = (tmp_path / d for d in ("reference", "input", "out", "control"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir):
        d.mkdir()
    read = rand(1300)
    # the winner holds the read 300 columns to the right of the diagonal: outside the band from row 755 to row 1024
    shifted = rand(300) + read
    near = read[:600] + rand(20) + read[620:]
    refs_a = [(">gi|a1", rand(1290)), (">gi|near", near)]
    refs_b = [(">gi|shifted", shifted), (">gi|b2", rand(1310))]
    (ref_dir / "a.fa").write_text(_fasta(refs_a))
    (ref_dir / "b.fa").write_text(_fasta(refs_b))
    (in_dir / "input1.txt").write_text(">gi reads\n" + read + "\n")
    banded = {name: gr.align_numpy(seq, read, SCORES, 1, W) for name, seq in refs_a + refs_b}
    assert banded[">gi|shifted"] != gr.align_numpy(shifted, read, SCORES, 1)
    assert max(banded, key=lambda k: banded[k][0]) == ">gi|near"          # (unbanded, the shifted copy would win)
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--long-reads", "--band", str(W), "--align-mode", "fit"]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    ctx = sw.Context(0)
    try:
        sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_FIT, long_reads=True, band=W).call(
            [str(ref_dir), str(in_dir), None, str(ctl_dir), None, None], (list(SCORES), None))
        assert ctx.options["band"] == 0                           # (put back after the call)
    finally:
        ctx.close()
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want)
    # ... and the file the reference's own output routine builds from gotoh_reference: the one winner, its sites sorted by begin
    from sparksmithwaterman_amd import io as swio
    score, alns = banded[">gi|near"]
    built = swio.InOutOps.GetOutputStr().call([read], ((4, 1), score, 0), [([">gi|near", near], sorted(alns, key=lambda t: t[0]))])
    assert _body(got) == _body(built)
