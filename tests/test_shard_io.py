"""CPU checks of the sharded file driver's pieces: the byte-range shard rule of a reference file (swmi_io_read_refs_shard,
include/swmi_io.h) and the strict-tie control driver of the tests (control_driver_oracle.py: DistributeAlgorithm's aligner, Distribution.java:140-210)."""
import os
import random
import sys

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import io as swio
from oracle import io_oracle_py as ioo
from oracle import sw_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from control_driver_oracle import control_driver     # noqa: E402


def _records_at_cuts():
    """four 25-byte records: for S = 2 and 4 the cuts floor(n*s/S) fall exactly on metadata lines"""
    recs = [">gi|%d\n%s\n" % (k, "ACGTACGTACGTACGTAC"[:25 - 6 - 1]) for k in range(4)]
    assert all(len(r) == 25 for r in recs)
    return "".join(recs)


CASES = {
    "crlf.fa": ">gi|1\r\nACGT\r\nAC GT \r\n>gi|2\r\n\r\nTT\r\n>gi|3\r\nG\r\n>gi|4\r\nCCCC\r\nAAAA\r\n",
    "lonecr.fa": ">gi|1\rACGT\rAC\r>gi|2\rGG\r>gi|3\r>gi|4\rTTTTTTTT\r",
    "mixed.fa": ">gi|1\r\nAC\n>gi|2\rGG\r\n\r>gi|3\nT\r>gi|4\r\n",
    "straddle.fa": ">gi|head\nA\n>gi|long\n" + ("ACGTACGTAC" * 8 + "\n") * 40 + ">gi|tail\nC\n",
    "at_cut.fa": _records_at_cuts(),
    "dups.fa": "".join(">gi|same\n%s\n" % ("ACGT" * (k + 1)) for k in range(6)) + ">gi|other\nTT\n>gi|same\nG",
    "few.fa": ">gi|x\nACGT\n>gi|y\nTTTT\n",
    "one.fa": ">gi|only\nACGTACGT",
    "not_meta_mid.fa": ">gi|1\nAC>gi|not\n x>gi\n>gi|2\n>gi\n\n>gi|3\nA\n",
}
ERRORS = {"empty.fa": "", "no_meta.fa": "ACGT\n>gi|1\nAC\n", "blank_first.fa": "\n>gi|1\nAC\n"}


def _write(d, name, text):
    p = d / name
    with open(p, "w", newline="") as f:
        f.write(text)
    return p


def _whole(path):
    s = swio.read_refs_packed(path, ">gi")
    return s.metadata, s.sequences(), s.positions


def _concat(path, n_shards):
    meta, seqs, pos = [], [], []
    for k in range(n_shards):
        s = swio.read_refs_shard_packed(path, ">gi", k, n_shards)
        assert len(s.positions) == len(s)
        meta += s.metadata
        seqs += s.sequences()
        pos += s.positions
    return meta, seqs, pos


def test_shard_symbols_exported():
    lib = sw._capi.load()
    for name in ("swmi_io_read_refs_shard", "swmi_seqset_positions"):
        assert any(n == name for n, _, _ in swio.IO_SYMBOLS)
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("name", list(CASES))
def test_shards_concatenate_to_the_whole_file(tmp_path, name):
    path = _write(tmp_path, name, CASES[name])
    whole = _whole(path)
    assert whole[0] == [r[0] for r in ioo.get_ref_seqs(path, ">gi")]
    data = open(path, "rb").read()
    for meta, pos in zip(whole[0], whole[2]):          # a position is where the metadata line starts
        assert data[pos:pos + len(meta)].decode("latin-1") == meta
        assert pos == 0 or data[pos - 1:pos] in (b"\n", b"\r")
    for n_shards in range(1, 8):
        assert _concat(path, n_shards) == whole, n_shards


def test_shard_rule_is_the_byte_range_of_the_metadata_line(tmp_path):
    path = _write(tmp_path, "at_cut.fa", CASES["at_cut.fa"])
    n = os.path.getsize(path)
    for n_shards in range(1, 8):
        for k in range(n_shards):
            s = swio.read_refs_shard_packed(path, ">gi", k, n_shards)
            lo, hi = n * k // n_shards, n * (k + 1) // n_shards
            assert all(lo <= p < hi for p in s.positions), (n_shards, k, s.positions)
    # a metadata line exactly at a cut belongs to the shard the cut opens
    assert swio.read_refs_shard_packed(path, ">gi", 1, 4).positions == [25]
    assert swio.read_refs_shard_packed(path, ">gi", 1, 2).positions == [50, 75]


def test_more_shards_than_records(tmp_path):
    path = _write(tmp_path, "few.fa", CASES["few.fa"])
    counts = [len(swio.read_refs_shard_packed(path, ">gi", k, 7)) for k in range(7)]
    assert sum(counts) == 2 and counts.count(0) == 5
    path = _write(tmp_path, "straddle.fa", CASES["straddle.fa"])
    counts = [len(swio.read_refs_shard_packed(path, ">gi", k, 7)) for k in range(7)]
    assert sum(counts) == 3 and counts[0] == 2 and counts[-1] == 1      # the long record's shard is the first


@pytest.mark.parametrize("name", list(ERRORS))
def test_error_files_fail_on_every_shard(tmp_path, name):
    path = _write(tmp_path, name, ERRORS[name])
    with pytest.raises(sw.SwmiError):
        swio.read_refs_packed(path, ">gi")
    for n_shards in (1, 3, 7):
        for k in range(n_shards):
            with pytest.raises(sw.SwmiError) as e:
                swio.read_refs_shard_packed(path, ">gi", k, n_shards)
            assert e.value.code == -1


def test_shard_out_of_range(tmp_path):
    path = _write(tmp_path, "few.fa", CASES["few.fa"])
    for k, n in ((2, 2), (0, 0), (7, 3)):
        with pytest.raises(sw.SwmiError) as e:
            swio.read_refs_shard_packed(path, ">gi", k, n)
        assert e.value.code == -1


def test_random_files_every_line_ending(tmp_path):
    rng = random.Random(20261015)
    for trial in range(120):
        lines = [">gi|%d" % rng.randrange(5)]
        for _ in range(rng.randrange(1, 30)):
            r = rng.random()
            if r < 0.25:
                lines.append(">gi|%d %s" % (rng.randrange(5), "x" * rng.randrange(4)))
            elif r < 0.3:
                lines.append("")
            else:
                lines.append("".join(rng.choice("ACGT >g") for _ in range(rng.randrange(1, 40))))
        text = "".join(ln + rng.choice(["\n", "\r\n", "\r"]) for ln in lines)
        if rng.random() < 0.3:
            text = text.rstrip("\r\n")
        path = _write(tmp_path, "r%d.fa" % trial, text)
        whole = _whole(path)
        for n_shards in range(1, 8):
            assert _concat(path, n_shards) == whole, (trial, n_shards, text)


def test_strict_oracle_differs_from_serial_exactly_where_kat3_says(tmp_path, kats):
    """KAT-3: the same scores, and the strict aligner's (4,4) traceback a,i,a,a gives (2, AA_A/AACA)
    where the serial one gives (2, AA/AA); after MapRef's sort by begin the two site lists differ in order and that one site."""
    k3s = [k for k in kats if k["name"] == "KAT-3-serial"][0]
    k3t = [k for k in kats if k["name"] == "KAT-3-strict"][0]
    ref_dir, in_dir, out_s, out_t = (tmp_path / d for d in ("ref", "in", "out_s", "out_t"))
    for d in (ref_dir, in_dir, out_s, out_t, ref_dir / "sub"):
        d.mkdir()
    _write(ref_dir, "a.fa", ">gi|kat3\n%s\n>gi|low\nGGGG\n" % k3s["ref"])
    _write(ref_dir / "sub", "b.fa", ">gi|kat3 again\n%s\n" % k3s["ref"])
    _write(in_dir, "reads.txt", ">gi reads\n%s\n" % k3s["read"])
    serial = ioo.no_distribution(str(ref_dir), str(in_dir), ">gi", str(out_s), scores=tuple(k3s["scores"]))
    strict = control_driver(str(ref_dir), str(in_dir), ">gi", str(out_t), scores=tuple(k3s["scores"]), tie_mode=orc.TIE_STRICT)
    # the test-side driver with the serial aligner is the oracle's control driver
    assert serial == control_driver(str(ref_dir), str(in_dir), ">gi", str(out_s), scores=tuple(k3s["scores"]),
                                    tie_mode=orc.TIE_SERIAL)

    def expect(sites):
        sites = [(b, (r, q)) for b, r, q in sites]
        opt = [([">gi|kat3", k3s["ref"]], sites), ([">gi|kat3 again", k3s["ref"]], sites)]
        return ioo.get_output_str([k3s["read"]], (3, 1), 2, 0, opt)

    strict_sorted = sorted(k3t["alignments"], key=lambda s: s[0])
    assert serial == [expect(k3s["map_ref_sorted"])]
    assert strict == [expect(strict_sorted)]
    a, b = serial[0].split(ioo.NEWLINE), strict[0].split(ioo.NEWLINE)
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(a) == len(b) and diff
    # every differing line is a site line (Index / refAligned / readAligned) of one of the two winners
    assert all(a[i].startswith(ioo.TAB) and b[i].startswith(ioo.TAB) for i in diff)
    assert a[:a.index("Reference:")] == b[:b.index("Reference:")]


def test_config_file_generator(tmp_path):
    """tools/write_config_files.py: configs[3]-shaped files -- synth.config_multi_read's references as >gi|ref<k> records over
    several files (one in a subdirectory), the reads behind a leading >gi line"""
    import subprocess
    import sys
    from sparksmithwaterman_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "write_config_files.py"), "--config", "3", "--n-refs", "30",
                        "--n-reads", "4", "--ref-files", "3", "--subdir", "--out", str(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    refs, reads = synth.config_multi_read(30, 4, seed=3)
    files = list(ioo._files_sorted(str(tmp_path / "reference")))
    assert any(os.sep + "sub" + os.sep in f for f in files) and len(files) == 3
    got = {}
    for f in files:
        got.update({m: q for m, q in ioo.get_ref_seqs(f, ">gi")})
    assert got == {">gi|ref%d" % k: r.decode() for k, r in enumerate(refs)}
    assert all(len(ln) <= 80 for ln in open(files[0]).read().splitlines())
    assert ioo.get_reads(str(tmp_path / "input" / "reads1.txt"), ">gi") == [q.decode() for q in reads]
