"""sharded_files --align-mode global --extend --end-bonus on one MI355X, two ranks: three reads against eight references of 300
to 700 bases in two files.  The winning reference starts with the first 200 bases of the first read, whose last 8 bases do not
match it: the best extension stops 8 bases short of the read's end, and with a bonus of 40 the pair is taken to the end instead
(end_bonus_reference.taken).  The result file must be what the mirror classes' own file driver writes with the same bonus, hold
the total tests/end_bonus_reference.py gives, and differ from the file written without --end-bonus."""
import os
import random
import subprocess
import sys

import pytest

import sparksmithwaterman_amd as sw

import end_bonus_reference as eb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = (2, -4, -2, -4)
BONUS = 40


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


def test_sharded_files_end_bonus(tmp_path):
    rng = random.Random(8821)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir, off_dir = (tmp_path / d for d in ("reference", "input", "out", "control", "off"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir, off_dir):
        d.mkdir()
    near = rand(500)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    reads = [near[:200] + "".join(other[c] for c in near[200:208]), near[:120], rand(60)]
    refs = [(">gi|r%d" % k, rand(rng.randint(300, 700))) for k in range(7)]
    refs.insert(5, (">gi|near", near))
    (ref_dir / "a.fa").write_text(_fasta(refs[:4]))
    (ref_dir / "b.fa").write_text(_fasta(refs[4:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    on = [eb.align(near, q, SCORES, BONUS) for q in reads]
    plain = [eb.align(near, q, SCORES, 0) for q in reads]
    max_score, end_score, end_col = on[0][4]
    assert max_score == 400 and plain[0][:3] == (400, plain[0][1], [(200, 200)]) and not plain[0][3]      # stops short of the end
    assert end_score < max_score < end_score + BONUS and eb.taken(max_score, end_score, BONUS)
    assert on[0][3] and on[0][0] == end_score and on[0][2] == [(208, end_col)] and on[0][1] != plain[0][1]
    assert sum(e[0] for e in on) != sum(e[0] for e in plain)
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "global", "--extend", "--end-bonus", str(BONUS)]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    ctx = sw.Context(0)
    try:
        for out, bonus in ((ctl_dir, BONUS), (off_dir, None)):
            sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_GLOBAL, extend=True, end_bonus=bonus).call(
                [str(ref_dir), str(in_dir), None, str(out), None, None], (list(SCORES), None))
            assert ctx.options.get("end_bonus", 0) == 0               # (put back after the call)
    finally:
        ctx.close()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    off = open(off_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want) != _body(off)
    assert ">gi|near" in got and ">gi|near" in off
    from sparksmithwaterman_amd import io as swio
    site = lambda e: swio.TAB + e[1][0][1][0] + swio.NEWLINE + swio.TAB + e[1][0][1][1] + swio.NEWLINE
    assert "Maximum alignment score = %d%s" % (sum(e[0] for e in on), swio.NEWLINE) in got and site(on[0]) in got and site(plain[0]) not in got
    assert "Maximum alignment score = %d%s" % (sum(e[0] for e in plain), swio.NEWLINE) in off and site(plain[0]) in off
