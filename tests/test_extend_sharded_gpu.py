"""sharded_files --align-mode global --extend --long-reads --band on one MI355X, two ranks: three reads, one of two strips,
against two dozen references of about 2.1 kbp -- longer than 1024 * 2 + band, which a plain banded global run refuses.  The
result file must be what a driver loop over tests/gotoh_reference.py builds, and what the mirror classes' own file driver
writes with the same options."""
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
W = 32


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


def test_sharded_files_extend(tmp_path):
    rng = random.Random(9980)
    rand = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    ref_dir, in_dir, out_dir, ctl_dir = (tmp_path / d for d in ("reference", "input", "out", "control"))
    for d in (ref_dir, in_dir, out_dir, ctl_dir):
        d.mkdir()
    long_read = rand(1100)
    reads = [long_read, long_read[:70], rand(50)]
    # the winner starts with the long read, a few bases changed and 20 replaced: the extension runs through all of it
    near = long_read[:600] + rand(20) + long_read[620:] + rand(1000)
    refs = [(">gi|r%d" % k, rand(rng.randint(2090, 2130))) for k in range(23)]
    refs.insert(13, (">gi|near", near))
    assert all(len(seq) > 1024 * 2 + W for _, seq in refs)           # (m, n) outside the band: extend runs take them
    (ref_dir / "a.fa").write_text(_fasta(refs[:12]))
    (ref_dir / "b.fa").write_text(_fasta(refs[12:]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    # the driver loop (Distribution.java:573,600-613): the running maximum of the references' totals from 0, ties kept
    best, opt = 0, []
    for meta, seq in refs:
        res = [gr.align_numpy(seq, q, SCORES, gr.GLOBAL, W, True) for q in reads]
        total = sum(r[0] for r in res)
        sites = sorted([a for r in res for a in r[1]], key=lambda t: t[0])
        if total > best:
            best, opt = total, [([meta, seq], sites)]
        elif total == best:
            opt.append(([meta, seq], sites))
    assert [o[0][0] for o in opt] == [">gi|near"] and best > 5 * 1000
    assert gr.align_numpy(near, long_read, SCORES, gr.GLOBAL, W, True, cells=True)[2][0][0] == 1100        # to the end of the read, not of the reference
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "2", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "global", "--extend", "--long-reads", "--band", str(W)]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=600).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    from sparksmithwaterman_amd import io as swio
    built = swio.InOutOps.GetOutputStr().call(reads, ((len(refs), len(reads)), best, 0), sorted(opt, key=lambda v: v[0][0]))
    assert _body(got) == _body(built)
    ctx = sw.Context(0)
    try:
        sw.Distribution.NoDistribution(ctx, align_mode=sw.ALIGN_GLOBAL, long_reads=True, band=W, extend=True).call(
            [str(ref_dir), str(in_dir), None, str(ctl_dir), None, None], (list(SCORES), None))
        assert ctx.options["extend"] == 0                         # (put back after the call)
    finally:
        ctx.close()
    want = open(ctl_dir / "result1.txt", newline="", encoding="latin-1").read()
    assert _body(got) == _body(want)
