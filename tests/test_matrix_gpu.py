"""Substitution score matrices on the GPU (swmi_set_score_matrix, the matrix sweeps of swmi_affine.hip).

Checked against the oracle where the matrix changes nothing (the identity matrix at gap_open = 0) and against the numpy
restatement of the contract in tests/gotoh_reference.py otherwise."""
import os
import random
import subprocess
import sys
import time

import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from sparksmithwaterman_amd import matrix as M
from oracle import io_oracle_py as ioo
from oracle import sw_oracle as orc

import affine_gpu_util as u
import gotoh_reference as gr
import limit_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)


def _golden(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name), encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _kat_matrix(kat):
    """a known answer's matrix: {"alphabet", "rows"}, or the name of a built-in one ("BLOSUM62")"""
    m = kat["matrix"]
    if isinstance(m, str):
        b = getattr(M, m)
        return b.alphabet.decode("latin-1"), [list(r) for r in b.scores]
    return m["alphabet"], m["rows"]


def _expect_linear(refs, reads, scores, tie):
    exp = {}
    for r, ref in enumerate(refs):
        for q, read in enumerate(reads):
            s, al = orc.opt_alignments((ref, read), scores[:3], b"aid-", tie)
            exp[(r, q)] = (s, [(a[0], tuple(a[1])) for a in al])
    return exp


def _rand_matrix(rng, alphabet, lo=-6, hi=8):
    return alphabet, [[rng.randint(lo, hi) for _ in alphabet] for _ in alphabet]


# 1 -- the identity matrix over ACGT gives the oracle's results bit for bit
@pytest.mark.parametrize("tie", [0, 1])
def test_identity_matrix_matches_the_oracle(ctx, tie):
    rng = random.Random(101 + tie)
    refs = [u.rand(rng, rng.randint(1, 700), rng.choice(["ACGT", "ACGTN", "ACGTacgtN"])) for _ in range(16)]
    refs[3] = "ACGTTGCA" * 60                           # periodic: a tied maximum per period
    reads = [u.rand(rng, rng.randint(1, 220), rng.choice(["ACGT", "acgtN"])) for _ in range(30)]
    reads[5] = "ACGTTGCAAC"
    b = u.run(ctx, refs, reads, (5, -3, -4, 0), tie, matrix=tuple(M.uniform("ACGT", 5, -3)), mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, _expect_linear(refs, reads, (5, -3, -4), tie))
    b.free()


# 2 -- random matrices against the restatement, every rows-per-lane instantiation
@pytest.mark.parametrize("tie", [0, 1])
def test_random_matrices_every_read_length(ctx, tie):
    rng = random.Random(111 + tie)
    reads = [u.rand(rng, m, "ACGTNacgtX") for m in (1, 2, 63, 64, 65, 128, 129, 200, 256, 257, 320, 384, 448, 512, 513, 640,
                                                   704, 768, 832, 896, 960, 1000, 1024)]
    refs = [u.rand(rng, 300, "ACGTNacgtX"), u.rand(rng, 1100, "ACGTN")]
    for o, mat in ((-6, _rand_matrix(rng, "ACGTN")),                       # asymmetric, positive off-diagonal entries
                   (0, _rand_matrix(rng, "acgt", -3, 9)),
                   (-2, _rand_matrix(rng, "AC"))):
        sc = (4, -3, -2, o)
        b = u.run(ctx, refs, reads, sc, tie, matrix=mat, mode3=False)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, u.expect(refs, reads, sc, tie=tie, matrix=mat))
        b.free()


def test_kats(ctx):
    for k in _golden("matrix_kat.json")["kats"]:
        mat = _kat_matrix(k)
        b = u.run(ctx, [k["ref"]], [k["read"]], tuple(k["scores"]), k["tie_mode"], matrix=mat, mode3=False)
        assert b.score(0) == k["score"], k["name"]
        assert [[x[0], x[1][0], x[1][1]] for x in b.alignments(0)] == k["alignments"], k["name"]
        b.free()


def test_blosum62_protein(ctx):
    rng = random.Random(121)
    aa = "ARNDCQEGHILKMFPSTWYV"
    refs = [u.rand(rng, rng.randint(50, 900), aa) for _ in range(6)]
    reads = [u.rand(rng, rng.randint(20, 400), aa) for _ in range(5)] + [refs[2][100:260]]
    sc = (1, -1, -1, -11)
    b = u.run(ctx, refs, reads, sc, 0, matrix=M.BLOSUM62, mode3=False)
    u.check(b, refs, reads, u.expect(refs, reads, sc, matrix=(M.BLOSUM62.alphabet, M.BLOSUM62.scores)))
    b.free()


# 3 -- ties, the cell-overflow re-run, and a path longer than the match-based bound
@pytest.mark.parametrize("tie", [0, 1])
def test_ties_and_cell_overflow(ctx, tie):
    ctx.set_option("cell_cap", 2)
    refs = ["CCTGGGTCCTGCCTCG" * 25, "AGAGAGAG" * 30, "acgtNNacgtRYacgt" * 12]
    reads = ["CCTGGGTCCTGC", "AG", "ACGTNNACG", "GA"]
    mat = ("AGC", [[3, -1, 0], [-1, 3, 0], [0, 0, 1]])
    sc = (3, -2, -3, -1)
    b = u.run(ctx, refs, reads, sc, tie, matrix=mat, mode3=False)
    assert b.timing().rerun_pairs >= 1
    u.check(b, refs, reads, u.expect(refs, reads, sc, tie=tie, matrix=mat))
    b.free()


def test_path_longer_than_the_match_bound(ctx):
    # match 1, gap -1: the match-based bound allows about 2 * m + m / 1 moves; W/W = 50 makes a 42-move path of score 60
    refs = ["W" + "C" * 40 + "W", "xW" + "C" * 200 + "Wx"]
    reads = ["WW"]
    mat = ("WC", [[50, -1], [-1, 1]])
    sc = (1, -1, -1, 0)
    for o in (0, -1):
        s = sc[:3] + (o,)
        b = u.run(ctx, refs, reads, s, 0, matrix=mat, mode3=False)
        exp = u.expect(refs, reads, s, matrix=mat)
        u.check(b, refs, reads, exp)
        assert len(exp[(0, 0)][1][0][1][0]) == 42
        b.free()


# 4 -- options, async (a matrix swap while the run is in flight), a stream from a file, a batch re-run under two matrices
@pytest.mark.parametrize("opt", [("scores_only", 1), ("device_strings", 0), ("max_workspace_bytes", 1 << 20)])
def test_options(ctx, opt):
    rng = random.Random(131)
    refs = ["ACGTTGCA" * 40, u.rand(rng, 900, "ACGTN"), u.rand(rng, 2500)]
    reads = ["ACGTTGCAAC", u.rand(rng, 150), u.rand(rng, 300), u.rand(rng, 400)]
    mat = _rand_matrix(rng, "ACGT")
    sc = (5, -3, -2, -6)
    ctx.set_option(*opt)
    b = u.run(ctx, refs, reads, sc, 0, matrix=mat, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc, matrix=mat), alignments=opt[0] != "scores_only")
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    b.free()


def test_async_swap_and_rerun(ctx):
    rng = random.Random(141)
    refs = [u.rand(rng, 1500) for _ in range(40)]
    reads = [u.rand(rng, 150) for _ in range(20)]
    m1, m2 = _rand_matrix(rng, "ACGT"), _rand_matrix(rng, "ACGT", -2, 12)
    sc = (5, -3, -2, -4)
    ctx.set_option("gap_open", sc[3])
    ctx.set_score_matrix(*m1)
    b = ctx.upload(refs, reads)
    # the worker starts the run 0.3 s after the call (test knob): the swap below certainly comes before the run starts, so the
    # run must take the matrix set when it was asked for, not the one set when it starts
    ctx.set_option("debug_async_delay_us", 300000)
    t0 = time.perf_counter()
    b.run_async(sw.make_params(sc[:3]))
    ctx.set_score_matrix(*m2)
    t_swap = time.perf_counter() - t0
    b.wait()
    assert t_swap < 0.25 and time.perf_counter() - t0 >= 0.3
    ctx.set_option("debug_async_delay_us", 0)
    sub = [0, 7, 39]
    e1 = {(r, q): gr.align_numpy(refs[r], reads[q], sc, matrix=m1) for r in sub for q in range(len(reads))}
    for (r, q), (s, al) in e1.items():
        assert b.score(r * len(reads) + q) == s
        assert b.alignments(r * len(reads) + q) == al
    b.run(sw.make_params(sc[:3]))                       # the same batch again: now m2 (no stale plan)
    for r in sub:
        for q in range(len(reads)):
            s, al = gr.align_numpy(refs[r], reads[q], sc, matrix=m2)
            assert b.score(r * len(reads) + q) == s
            assert b.alignments(r * len(reads) + q) == al
    b.free()


def test_stream_from_fasta(ctx, tmp_path):
    rng = random.Random(151)
    refs = [u.rand(rng, rng.randint(200, 800), "ACGTN") for _ in range(40)]
    reads = [u.rand(rng, 150), refs[17][100:250], u.rand(rng, 64)]
    path = tmp_path / "refs.fa"
    with open(path, "w") as f:
        for k, r in enumerate(refs):
            f.write(">gi|ref%d\n" % k)
            for x in range(0, len(r), 70):
                f.write(r[x:x + 70] + "\n")
    mat = _rand_matrix(rng, "ACGTN")
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    ctx.set_score_matrix(*mat)
    st = ctx.stream(reads, sw.make_params(sc[:3]), slots=2, chunk_bytes=1 << 16)
    ctx.clear_score_matrix()                           # (the stream keeps the matrix set when it was opened)
    st.push_file(path).finish()
    exp = [[gr.align_numpy(r, q, sc, matrix=mat) for q in reads] for r in refs]
    assert [int(t) for t in st.totals()] == [sum(e[0] for e in row) for row in exp]
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            if (first + r) % 7 == 3 or first + r == 17:
                sites = sorted([a for e in exp[first + r] for a in e[1]], key=lambda t: t[0])
                assert c.ref_match_sites(r) == sites, first + r
    st.close()


def test_clearing_returns_to_mode_1(ctx):
    rng = random.Random(161)
    refs = [u.rand(rng, 400) for _ in range(3)]
    reads = [u.rand(rng, 100) for _ in range(3)]
    b = ctx.upload(refs, reads)
    ctx.set_score_matrix("ACGT", [[9, 0, 0, 0], [0, 9, 0, 0], [0, 0, 9, 0], [0, 0, 0, 9]])
    assert b.run(sw.make_params()).pipeline_mode() == 3
    ctx.clear_score_matrix()
    b.run(sw.make_params())
    assert b.pipeline_mode() == 1
    u.check(b, refs, reads, _expect_linear(refs, reads, (5, -3, -4), 0))
    b.free()


# 5 -- bounds and error codes
def test_bounds(ctx):
    lib = ctx._lib

    def raw_set(alpha, scores):
        arr = (_capi.C.c_int32 * max(len(scores), 1))(*scores)
        return lib.swmi_set_score_matrix(ctx._h, alpha, len(alpha), arr)

    ctx.set_score_matrix("AC", [[2, 0], [0, 2]])
    assert raw_set(b"Aa", [1, 2, 3, 4]) == ERR_INVALID                       # duplicate after canonicalisation
    assert raw_set(b"\xe9\xc9", [1, 2, 3, 4]) == ERR_INVALID
    assert raw_set(bytes(range(0x21, 0x21 + 65)), [0] * 65 * 65) == ERR_INVALID
    assert raw_set(b"AC", [0, 0, 0, (1 << 20) + 1]) == ERR_INVALID
    assert raw_set(b"AC", [0, 0, -(1 << 20) - 1, 0]) == ERR_INVALID
    assert lib.swmi_set_score_matrix(None, b"A", 1, (_capi.C.c_int32 * 1)(0)) == ERR_INVALID
    b = ctx.upload(["ACAC"], ["CA"])                 # the failed calls left the matrix as it was
    assert b.run(sw.make_params((1, -1, -1))).score(0) == 4
    assert raw_set(bytes(range(0x21, 0x21 + 64)), [1 << 20] * 64 * 64) == 0
    b.free()
    ctx.set_score_matrix("AC", [[2, 0], [0, 2]])
    b = ctx.upload(["ACGT" * 10], ["A" * 1025])
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()
    b = ctx.upload(["ACGT" * 10], ["ACG"])
    for bad in ((5, -3, 1), ((1 << 20) + 1, -3, -4)):
        with pytest.raises(_capi.SwmiError) as e:
            b.run(sw.make_params(bad))
        assert e.value.code == ERR_UNSUPPORTED
    b.free()
    with pytest.raises(ValueError):
        ctx.set_score_matrix("Aa", [[1, 2], [3, 4]])
    for bad in (-1, 10000001):
        with pytest.raises(_capi.SwmiError) as e:
            ctx.set_option("debug_async_delay_us", bad)
        assert e.value.code == ERR_INVALID


# 5b -- the largest matrix the ABI takes, at the entry bound, in local mode
@pytest.mark.parametrize("tie", [0, 1])
def test_64_symbols_at_the_entry_bound(ctx, tie):
    """64 symbols (a 65 x 65 table, 16.9 KB of LDS), bytes at and above 0x80, lower-case letters in the sequences, entries
    random in +-2^20 with both extremes present, two bytes outside the alphabet; every rows-per-lane class boundary of the
    narrow sweep and the longest read; gap_open 0 and at its bound.  The scalar restatement (Python ints) checks the short
    reads, the numpy one (int64; tests/test_matrix_cpu.py holds it to the scalar one on these inputs) the longest."""
    mat, draw = lc.big_matrix()
    rng = random.Random(1510 + tie)
    reads = [lc.rand_seq(rng, m, draw) for m in (1, 64, 65, 1024)]
    refs = [lc.rand_seq(rng, 40, draw), reads[3][500:700] + lc.rand_seq(rng, 100, draw)]
    assert any(ord(c) >= 0x80 for c in refs[1]) and any(c.islower() for c in refs[1])
    L = lc.L
    for o in (0, -L):
        sc = (L, -L, -L, o)
        b = u.run(ctx, refs, reads, sc, tie, matrix=mat, mode3=False)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, {(r, q): (gr.align_scalar if len(read) <= 65 else gr.align_numpy)(ref, read, sc, tie_mode=tie, matrix=mat)
                                 for r, ref in enumerate(refs) for q, read in enumerate(reads)})
        b.free()


def test_all_entries_at_the_bound(ctx):
    """the matrix test_bounds installs -- 64 symbols, every entry 2^20 -- run on a small pair"""
    alpha = bytes(range(0x21, 0x21 + 64)).decode("latin-1")
    mat = (alpha, [[1 << 20] * 64 for _ in range(64)])
    refs, reads = ["ACGTAC#!~xA", "Z9"], ["CGT!a~", "z"]          # (~ is outside: match / mismatch; x is the symbol X)
    for sc, tie in (((5, -3, -4, -6), 0), ((1 << 20, -(1 << 20), -(1 << 20), 0), 1)):
        b = u.run(ctx, refs, reads, sc, tie, matrix=mat, mode3=False)
        exp = {(r, q): gr.align_scalar(ref, read, sc, tie_mode=tie, matrix=mat) for r, ref in enumerate(refs) for q, read in enumerate(reads)}
        u.check(b, refs, reads, exp)
        assert exp[(1, 1)][0] == 1 << 20                          # read z / reference Z: one symbol
        b.free()


# 6 -- the JNI shim's entry point from plain C99 (tests/c/shim_matrix.c)
def test_c99_shim_sets_the_matrix(tmp_path):
    out = u.run_shim(tmp_path, "shim_matrix")
    # ref CAGCA, read ACAG; read A vs reference C = 5 (tests/golden/matrix_kat.json "asymmetric, longer")
    s, al = gr.align_numpy("CAGCA", "ACAG", (1, -1, -2, -1), matrix=("AC", [[2, 5], [-3, 2]]))
    assert out.split() == [str(s), str(len(al))] + ["%d:%s/%s" % (a[0], a[1][0], a[1][1]) for a in al] + ["cleared", "1"]


# 7 -- the sharded file driver with --matrix at world 1
def test_sharded_files_matrix(tmp_path):
    rng = random.Random(171)
    ref_dir, in_dir = tmp_path / "reference", tmp_path / "input"
    ref_dir.mkdir()
    in_dir.mkdir()
    refs = [u.rand(rng, rng.randint(100, 300)) for _ in range(12)]
    with open(ref_dir / "a.fa", "w") as f:
        for k, r in enumerate(refs):
            f.write(">gi|r%d\n%s\n" % (k, r))
    reads = [refs[4][20:70], u.rand(rng, 40)]
    (in_dir / "input1.txt").write_text(">gi reads\n" + "\n".join(reads) + "\n")
    mfile = tmp_path / "m.txt"
    mfile.write_text("# ACGT, transitions score 1\n   A  C  G  T\nA  5 -3  1 -3\nC -3  5 -3  1\nG  1 -3  5 -3\nT -3  1 -3  5\n")
    env = dict(os.environ, SWMI_ONE_GPU="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out_dir = tmp_path / "out"
    cmd = [sys.executable, "-m", "sparksmithwaterman_amd.sharded_files", "--ref-dir", str(ref_dir), "--in-dir", str(in_dir),
           "--out-dir", str(out_dir), "--world", "1", "--matrix", str(mfile)]
    assert subprocess.run(cmd, cwd=ROOT, env=env, timeout=900).returncode == 0
    got = open(out_dir / "result1.txt", newline="", encoding="latin-1").read()
    # the control driver's file, every alignment from the restatement
    mat = M.load(str(mfile))
    best, opt = 0, []
    for k, r in enumerate(refs):
        per = [gr.align_numpy(r, q, (5, -3, -4, 0), matrix=(mat.alphabet, mat.scores)) for q in reads]
        total = sum(e[0] for e in per)
        sites = sorted([a for e in per for a in e[1]], key=lambda t: t[0])
        if total > best:
            best, opt = total, [((">gi|r%d" % k, r), sites)]
        elif total == best:
            opt.append(((">gi|r%d" % k, r), sites))
    expect = ioo.get_output_str(reads, (len(refs), len(reads)), best, 0, opt)
    assert got.split(os.linesep, 1)[1] == expect.split(os.linesep, 1)[1]
    # (the matrix changes the winner's total: transitions score 1 instead of -3)
    assert best != max(orc.map_ref((">gi|r%d" % k, r), reads)[0] for k, r in enumerate(refs))
