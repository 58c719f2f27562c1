"""sharded_files --align-mode fit on one MI355X (every rank on GPU 0, gloo for the exchange) against a test-side driver loop:
the control driver's loop (oracle/io_oracle_py's file pieces, `int max = 0`, ties kept, its writer) with the fit-mode
restatement of tests/gotoh_reference.py as the aligner."""
import json
import os
import subprocess
import sys

import pytest

from oracle import io_oracle_py as ioo

import gotoh_reference as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "CCTGGGTCCTGCCTCGCATCTGACCAGGGCAGGTGGCCTCCTCATCACACTGCTGCCTCTGCTGTTGGCCCTGCTCATGA"
SCORES = (5, -3, -2, -6)


def _fasta(recs):
    out = []
    for meta, seq in recs:
        out.append(meta)
        out.extend(seq[k:k + 80] for k in range(0, len(seq), 80))
    return "\n".join(out) + "\n"


def _tree(root):
    ref_dir, in_dir = root / "reference", root / "input"
    for d in (ref_dir, in_dir, ref_dir / "sub"):
        d.mkdir(parents=True)
    a = [(">gi|ref1", REF * 3), (">gi|dup", REF[::-1] * 2), (">gi|x1", REF[7:] + REF[:7]), (">gi|ref1 mid", REF * 3),
         (">gi|x2", (REF[::-1] * 3)[:200]), (">gi|x3", REF[::2] * 4), (">gi|ref1", REF * 3)]
    (ref_dir / "a.fa").write_text(_fasta(a))
    (ref_dir / "sub" / "b.fa").write_text(_fasta([(">gi|dup", REF * 3), (">gi|b1", "ACGT" * 30), (">gi|b2", REF[5:70] + "ACGT" * 9)]))
    # input1: reads of the periodic reference, the second with two bases that only fit with the ends paid for;
    # input2: reads no reference holds -- every total is negative, so nothing beats `int max = 0` and no reference is listed
    (in_dir / "input1.txt").write_text(">gi reads\n" + REF[10:50] + "\nTT" + REF[30:60] + "AA\n")
    (in_dir / "input2.txt").write_text("WWWWWWWWWWWW\nWWWWW\n")
    return ref_dir, in_dir


def _driver(ref_dir, in_dir, out_dir, mode, tie=0):
    texts = []
    for input_num, in_file in enumerate(ioo._files_sorted(str(in_dir)), 1):
        reads = ioo.get_reads(in_file, ">gi")
        num_refs, mx, opt = 0, 0, []
        for ref_file in ioo._files_sorted(str(ref_dir)):
            ref_seqs = ioo.get_ref_seqs(ref_file, ">gi")
            num_refs += len(ref_seqs)
            for ref in ref_seqs:
                res = [gr.align_numpy(ref[1], q, SCORES, mode, tie_mode=tie) for q in reads]
                total = sum(r[0] for r in res)
                sites = sorted([a for r in res for a in r[1]], key=lambda t: t[0])
                if total > mx:
                    mx, opt = total, [(ref, sites)]
                elif total == mx:
                    opt.append((ref, sites))
        opt.sort(key=lambda t: t[0][0])
        texts.append(ioo.get_output_str(reads, (num_refs, len(reads)), mx, 0, opt))
    return texts


def _body(text):
    head, rest = text.split(os.linesep, 1)
    assert head.startswith("Execution Time = ") and head.endswith(" ms")
    return rest


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_files_fit_mode(tmp_path, world):
    ref_dir, in_dir = _tree(tmp_path)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", str(world), "--stream-chunk-bytes", "65536", "--scores", ",".join(map(str, SCORES)),
           "--align-mode", "fit", "--stats", str(out_dir / "rank<r>.json")]
    rc = subprocess.run(cmd, cwd=ROOT, env=env, timeout=900)     # the launcher makes no GPU call; the ranks are its children
    assert rc.returncode == 0
    expect = _driver(ref_dir, in_dir, out_dir, gr.FIT)
    local = _driver(ref_dir, in_dir, out_dir, gr.LOCAL)
    assert _body(expect[0]) != _body(local[0])                  # the mode shows in the result
    assert "Maximum alignment score = 0" in expect[1] and "Reference:" not in expect[1]     # negative totals never win
    for k, text in enumerate(expect, 1):
        got = open(out_dir / ("result%d.txt" % k), newline="", encoding="latin-1").read()
        assert _body(got) == _body(text), k
    stats = [json.load(open(out_dir / ("rank%d.json" % r))) for r in range(world)]
    assert sum(st["records"] for st in stats) == 2 * 10
