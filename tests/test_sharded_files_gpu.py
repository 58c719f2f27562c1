"""The sharded file-to-file driver (sparksmithwaterman_amd.sharded_files) end to end on one MI355X: every rank process on GPU 0,
gloo for the exchange (SWMI_ONE_GPU=1), at most three ranks at once.  Every result file must equal the control driver's
(oracle/io_oracle_py.no_distribution, Distribution.java:482-634; with --tie strict, tests/control_driver_oracle.py) apart from
the wall-clock line (InOutOps.java:249)."""
import json
import os
import subprocess
import sys

import pytest

from sparksmithwaterman_amd import io as swio
from oracle import io_oracle_py as ioo
from oracle import sw_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from control_driver_oracle import control_driver     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "CCTGGGTCCTGCCTCGCATCTGACCAGGGCAGGTGGCCTCCTCATCACACTGCTGCCTCTGCTGTTGGCCCTGCTCATGA"   # EngineerData.java:23
READ_20 = "ACTGACTGACTGACTGACTG"                                                            # EngineerData.java:29


def _fasta(recs, eol="\n"):
    out = []
    for meta, seq in recs:
        out.append(meta)
        out.extend(seq[k:k + 80] for k in range(0, len(seq), 80))
    return eol.join(out) + eol


def _tree(root):
    """two reads files; three reference files, one in a subdirectory.  The periodic EngineerData reference REF*3 sits at the
    start, middle and end of a.fa and in sub/b.fa, so the winning total ties across the ranks' shards; ">gi|dup" is in both
    a.fa and sub/b.fa; c.fa has one record, fewer than the ranks."""
    ref_dir, in_dir = root / "reference", root / "input"
    for d in (ref_dir, in_dir, ref_dir / "sub"):
        d.mkdir(parents=True)
    a = [(">gi|ref1", REF * 3), (">gi|dup", REF[::-1] * 2), (">gi|x1", REF[7:] + REF[:7]), (">gi|ref1 mid", REF * 3),
         (">gi|x2", (REF[::-1] * 3)[:200]), (">gi|dup", REF * 2 + "ACGT"), (">gi|x3", REF[::2] * 4), (">gi|ref1", REF * 3)]
    (ref_dir / "a.fa").write_text(_fasta(a))
    b = [(">gi|dup", REF * 3), (">gi|b1", "ACGT" * 30), (">gi|b2", REF[5:70] + "ACGT" * 9)]
    with open(ref_dir / "sub" / "b.fa", "w", newline="") as f:
        f.write(_fasta(b, "\r\n"))
    (ref_dir / "c.fa").write_text(_fasta([(">gi|single", REF[5:70] + "ACGT" * 9)]))
    (in_dir / "input1.txt").write_text(">gi reads\n" + REF[10:50] + "\n" + READ_20 + "\n")
    (in_dir / "input2.txt").write_text("TTTTTTTTGGGGG\nGCATCTGACCAGGG\n")
    return ref_dir, in_dir


def _run(ref_dir, in_dir, out_dir, world, *extra):
    out_dir.mkdir(exist_ok=True)
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", str(world), "--stream-chunk-bytes", "65536",
           "--stats", str(out_dir / "rank<r>.json")] + list(extra)
    rc = subprocess.run(cmd, cwd=ROOT, env=env, timeout=900)     # the launcher makes no GPU call; the ranks are its children
    assert rc.returncode == 0
    return [json.load(open(out_dir / ("rank%d.json" % r))) for r in range(world)]


def _body(text):
    head, rest = text.split(os.linesep, 1)
    assert head.startswith("Execution Time = ") and head.endswith(" ms")
    return rest


def _check_against_oracle(ref_dir, in_dir, out_dir, oracle_dir, tie_mode=orc.TIE_SERIAL):
    oracle_dir.mkdir(exist_ok=True)
    if tie_mode == orc.TIE_SERIAL:
        expect = ioo.no_distribution(str(ref_dir), str(in_dir), ">gi", str(oracle_dir))
    else:                                   # DistributeAlgorithm's aligner in the control loop (tests/control_driver_oracle.py)
        expect = control_driver(str(ref_dir), str(in_dir), ">gi", str(oracle_dir), tie_mode=tie_mode)
    n_refs = sum(len(ioo.get_ref_seqs(p, ">gi")) for p in ioo._files_sorted(str(ref_dir)))
    for k, text in enumerate(expect, 1):
        got = open(out_dir / ("result%d.txt" % k), newline="", encoding="latin-1").read()
        assert _body(got) == _body(text), k
        assert "# Reference Sequences = %d%s" % (n_refs, os.linesep) in got
    assert not (out_dir / ("result%d.txt" % (len(expect) + 1))).exists()
    return expect


def _check_stats(ref_dir, stats, world, n_reads_files):
    files = list(ioo._files_sorted(str(ref_dir)))
    for st in stats:
        # each rank streamed exactly its own byte-range shard of every reference file, for every reads file
        mine = [len(swio.read_refs_shard_packed(p, ">gi", st["rank"], world)) for p in files]
        assert [f["records_per_ref_file"] for f in st["files"]] == [mine] * n_reads_files
        assert st["records"] == sum(mine) * n_reads_files
        assert st["backend"] == ("gloo" if world > 1 else "none")
        for phase in ("parse_s", "push_s", "sweep_s", "reduce_s", "realign_s", "gather_s", "write_s"):
            assert st[phase] >= 0
    whole = [len(swio.read_refs_packed(p, ">gi")) for p in files]
    assert [sum(x) for x in zip(*[st["files"][0]["records_per_ref_file"] for st in stats])] == whole


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_files_match_the_control_driver(tmp_path, world):
    ref_dir, in_dir = _tree(tmp_path)
    stats = _run(ref_dir, in_dir, tmp_path / "out", world)
    _check_against_oracle(ref_dir, in_dir, tmp_path / "out", tmp_path / "oracle")
    _check_stats(ref_dir, stats, world, 2)
    # the tree was built so that c.fa leaves a rank empty and the winners of input1 tie across ranks
    assert min(st["files"][0]["records_per_ref_file"][1] for st in stats) == 0
    assert sum(1 for st in stats if st["winners_owned"] > 0) >= 2


@pytest.mark.gpu
def test_sharded_files_strict_ties(tmp_path):
    ref_dir, in_dir = _tree(tmp_path)
    stats = _run(ref_dir, in_dir, tmp_path / "out", 2, "--tie", "strict")
    strict = _check_against_oracle(ref_dir, in_dir, tmp_path / "out", tmp_path / "oracle", orc.TIE_STRICT)
    _check_stats(ref_dir, stats, 2, 2)
    serial = ioo.no_distribution(str(ref_dir), str(in_dir), ">gi", str(tmp_path / "oracle"))
    assert strict != serial                # (the periodic references have tied directions on their paths)


@pytest.mark.gpu
def test_sharded_files_max_zero_every_reference_wins(tmp_path):
    """a read sharing no base with any reference: every total is 0 = `int max = 0`, so every reference is a winner, each
    with m*n degenerate (0, "", "") sites per read (SmithWaterman.java:154,182-185) -- nothing may be cut"""
    ref_dir, in_dir = tmp_path / "reference", tmp_path / "input"
    for d in (ref_dir, in_dir, ref_dir / "sub"):
        d.mkdir(parents=True)
    (ref_dir / "a.fa").write_text(_fasta([(">gi|z%d" % k, ("ACGGCA" * 3)[k:k + 9 + k]) for k in range(5)]))
    (ref_dir / "sub" / "b.fa").write_text(_fasta([(">gi|z1", "CAGCAG"), (">gi|y", "GGGACCA" * 2)]))
    (in_dir / "reads.txt").write_text(">gi none\nTTTTT\nTT\n")
    stats = _run(ref_dir, in_dir, tmp_path / "out", 2)
    expect = _check_against_oracle(ref_dir, in_dir, tmp_path / "out", tmp_path / "oracle")
    assert "Maximum alignment score = 0" in expect[0] and expect[0].count("Reference:") == 7
    assert sum(st["winners_owned"] for st in stats) == 7
    _check_stats(ref_dir, stats, 2, 1)


@pytest.mark.gpu
def test_world_one_is_no_distribution(tmp_path):
    import sparksmithwaterman_amd as sw
    ref_dir, in_dir = _tree(tmp_path)
    stats = _run(ref_dir, in_dir, tmp_path / "out", 1)
    _check_stats(ref_dir, stats, 1, 2)
    ctl = tmp_path / "ctl"
    ctl.mkdir()
    ctx = sw.Context(0)
    try:
        sw.Distribution.NoDistribution(ctx).call([str(ref_dir), str(in_dir), ">gi", str(ctl), None, None], None)
    finally:
        ctx.close()
    for k in (1, 2):
        got = open(tmp_path / "out" / ("result%d.txt" % k), "rb").read()
        want = open(ctl / ("result%d.txt" % k), "rb").read()
        assert got.split(os.linesep.encode(), 1)[1] == want.split(os.linesep.encode(), 1)[1]
    _check_against_oracle(ref_dir, in_dir, tmp_path / "out", tmp_path / "oracle")
