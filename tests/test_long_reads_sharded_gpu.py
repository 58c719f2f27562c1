"""sharded_files --long-reads on one MI355X: a 1300-base read against a two-file reference set; the result file must be what
the mirror classes' own file driver writes with long_reads=True."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

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


def test_sharded_files_long_reads(tmp_path):
    rng = random.Random(8210)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir = (tmp_path / d for d in ("reference", "input", "out", "control"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir):
        d.mkdir()
    win = rand(400)
    (ref_dir / "a.fa").write_text(_fasta([(">gi|a1", rand(300)), (">gi|win", win), (">gi|a3", rand(150))]))
    (ref_dir / "b.fa").write_text(_fasta([(">gi|b1", rand(500)), (">gi|win2", win), (">gi|b3", rand(90))]))
    read = rand(1300)
    read = read[:960] + win[100:300] + read[1160:]                # (the winners' alignment crosses row 1024)
    (in_dir / "input1.txt").write_text(">gi reads\n" + read + "\n")
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
            "--out-dir", str(out_dir), "--world", "1", "--scores", ",".join(map(str, SCORES))]
    rc = subprocess.run(base + ["--long-reads"], cwd=ROOT, env=env, timeout=600)
    assert rc.returncode == 0
    ctx = sw.Context(0)
    try:
        sw.Distribution.NoDistribution(ctx, long_reads=True).call(
            [str(ref_dir), str(in_dir), None, str(ctl_dir), None, None], (list(SCORES), None))
        assert ctx.options["long_reads"] == 0                     # (put back after the call)
    finally:
        ctx.close()
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want)
    assert got.count(win) >= 2                                    # (both copies of the winner are listed)
