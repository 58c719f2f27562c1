"""Score matrices without a GPU: the two restatements of the contract (tests/gotoh_reference.py) against each other, against the
linear oracle and the affine restatement where the matrix changes nothing, against hand-derived known answers, and the Python
side of the API (NCBI parser, BLOSUM62, validation)."""
import json
import os
import random

import pytest

from oracle import sw_oracle as orc
from sparksmithwaterman_amd import matrix as M

import gotoh_reference as gr
import limit_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "matrix_kat.json"), encoding="utf-8") as f:
        return json.load(f)["kats"]


def _kat_matrix(kat):
    """a known answer's matrix: {"alphabet", "rows"}, or the name of a built-in one ("BLOSUM62")"""
    m = kat["matrix"]
    if isinstance(m, str):
        b = getattr(M, m)
        return b.alphabet.decode("latin-1"), [list(r) for r in b.scores]
    return m["alphabet"], m["rows"]


def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _rand_matrix(rng, alphabet, lo=-6, hi=8):
    return alphabet, [[rng.randint(lo, hi) for _ in alphabet] for _ in alphabet]


@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree(tie):
    rng = random.Random(11 + tie)
    for _ in range(60):
        mat = _rand_matrix(rng, rng.choice(["ACGT", "ACGTN", "AC", "acgT"]))
        sc = (rng.randint(-2, 5), rng.randint(-5, 2), -rng.randint(0, 4), -rng.randint(0, 5))
        ref, read = _rand(rng, rng.randint(0, 14), "ACGTNacgtX"), _rand(rng, rng.randint(0, 10), "ACGTNacgtX")
        assert gr.align_scalar(ref, read, sc, tie_mode=tie, matrix=mat) == gr.align_numpy(ref, read, sc, tie_mode=tie, matrix=mat), (ref, read, sc, mat)


@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree_at_the_entry_bound(tie):
    """the 64-symbol matrix with entries in +-2^20 of tests/test_matrix_gpu.py at reduced length: align_numpy (int64, a
    256 x 256 table built through the case rule) against align_scalar (Python ints, a dict)"""
    mat, draw = lc.big_matrix()
    assert max(max(r) for r in mat[1]) == lc.L and min(min(r) for r in mat[1]) == -lc.L
    assert any(mat[1][i][j] != mat[1][j][i] for i in range(64) for j in range(64))
    rng = random.Random(1520 + tie)
    reads = [lc.rand_seq(rng, m, draw) for m in (1, 33, 65, 128)]
    refs = [lc.rand_seq(rng, 40, draw), reads[3][20:90] + lc.rand_seq(rng, 30, draw)]
    for o in (0, -lc.L):
        sc = (lc.L, -lc.L, -lc.L, o)
        for ref in refs:
            for read in reads:
                assert gr.align_scalar(ref, read, sc, tie_mode=tie, matrix=mat) == gr.align_numpy(ref, read, sc, tie_mode=tie, matrix=mat), (ref, read, o)


@pytest.mark.parametrize("tie", [0, 1])
def test_identity_matrix_is_the_linear_oracle(tie):
    rng = random.Random(3 + tie)
    for _ in range(40):
        match, mismatch, gap = rng.randint(1, 6), -rng.randint(0, 5), -rng.randint(1, 5)
        mat = M.uniform("ACGT", match, mismatch)
        ref, read = _rand(rng, rng.randint(1, 30), "ACGTNacgt"), _rand(rng, rng.randint(1, 12), "ACGTNacgt")
        s, al = orc.opt_alignments((ref, read), (match, mismatch, gap), b"aid-", tie)
        exp = (s, [(a[0], tuple(a[1])) for a in al])
        for f in (gr.align_scalar, gr.align_numpy):
            assert f(ref, read, (match, mismatch, gap, 0), tie_mode=tie, matrix=mat) == exp, (ref, read)


@pytest.mark.parametrize("tie", [0, 1])
def test_identity_matrix_is_the_affine_restatement(tie):
    rng = random.Random(5 + tie)
    for _ in range(40):
        sc = (rng.randint(1, 6), -rng.randint(0, 5), -rng.randint(0, 3), -rng.randint(1, 8))
        mat = M.uniform("acgt", sc[0], sc[1])
        ref, read = _rand(rng, rng.randint(1, 30), "ACGTNacgt"), _rand(rng, rng.randint(1, 12), "ACGTNacgt")
        exp = gr.align_numpy(ref, read, sc, tie_mode=tie)
        assert gr.align_scalar(ref, read, sc, tie_mode=tie, matrix=mat) == exp
        assert gr.align_numpy(ref, read, sc, tie_mode=tie, matrix=mat) == exp


@pytest.mark.parametrize("k", range(len(_kats())))
def test_known_answers(k):
    kat = _kats()[k]
    mat = _kat_matrix(kat)
    sc, tie = tuple(kat["scores"]), kat["tie_mode"]
    exp = (kat["score"], [(a[0], (a[1], a[2])) for a in kat["alignments"]])
    got = gr.align_scalar(kat["ref"], kat["read"], sc, tie_mode=tie, matrix=mat, matrices=True)
    assert got[:2] == exp, kat["name"]
    assert got[2] == kat["H"], kat["name"]
    assert gr.align_numpy(kat["ref"], kat["read"], sc, tie_mode=tie, matrix=mat) == exp, kat["name"]


def test_kat_asymmetric_pins_row_as_read():
    kats = {k["name"]: k for k in _kats()}
    assert kats["asymmetric: read A vs reference C scores 5 (row = read)"]["score"] == 5
    assert kats["asymmetric: read C vs reference A scores -3 (degenerate)"]["score"] == 0


def test_cell_score_rule():
    mat = ("Acé", [[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    sc = (10, -10, -1, 0)
    assert gr.cell_score("C", "a", sc, mat) == 2             # read a (row 0), reference C (column 1)
    assert gr.cell_score("a", "C", sc, mat) == 4
    assert gr.cell_score("\xc9", "\xe9", sc, mat) == 9       # É / é: one symbol
    assert gr.cell_score("G", "g", sc, mat) == 10            # outside the alphabet: equal -> match
    assert gr.cell_score("G", "A", sc, mat) == -10           # one side outside: mismatch
    assert gr.cell_score("\xff", "\xff", sc, mat) == 10 and gr.cell_score("\xff", "\xdf", sc, mat) == -10


def test_blosum62():
    b = M.BLOSUM62
    assert b.alphabet == b"ARNDCQEGHILKMFPSTWYVBZX*"
    idx = {c: k for k, c in enumerate(b.alphabet.decode())}
    assert b.scores[idx["W"]][idx["W"]] == 11
    assert b.scores[idx["A"]][idx["A"]] == 4
    assert b.scores[idx["C"]][idx["C"]] == 9
    assert b.scores[idx["*"]][idx["*"]] == 1
    n = len(b.alphabet)
    assert all(b.scores[i][j] == b.scores[j][i] for i in range(n) for j in range(n))


def test_parse_ncbi(tmp_path):
    text = "# a comment\n\n   A  C  g\nA  1 -2  3\nC -4  5 -6\ng  7 -8  9\n"
    m = M.parse_ncbi(text)
    assert m.alphabet == b"ACg" and m.scores == ((1, -2, 3), (-4, 5, -6), (7, -8, 9))
    p = tmp_path / "m.txt"
    p.write_bytes(text.encode())
    assert M.load(str(p)) == m
    for bad in ("   A C\nA 1 2\n",                          # a row missing
                "   A C\nA 1 2\nC 1\n",                     # a short row
                "   A C\nC 1 2\nA 1 2\n",                   # rows out of order
                "   A a\nA 1 2\na 1 2\n",                   # one symbol twice
                "   A C\nA 1 x\nC 1 2\n",                   # not an integer
                "   AB C\nAB 1 2\nC 1 2\n",                 # a symbol of two characters
                ""):
        with pytest.raises(ValueError):
            M.parse_ncbi(bad)


def test_validate():
    sym, flat = M.validate("AC", [[1, 2], [3, 4]])
    assert sym == b"AC" and flat == [1, 2, 3, 4]
    assert M.validate(["A", "c"], ((1, 2), (3, 4)))[0] == b"Ac"
    assert len(M.validate("".join(chr(0x21 + k) for k in range(64)), [[0] * 64] * 64)[0]) == 64
    with pytest.raises(ValueError):
        M.validate("", [])
    with pytest.raises(ValueError):
        M.validate("".join(chr(0x21 + k) for k in range(65)), [[0] * 65] * 65)
    for dup in ("Aa", "\xe9\xc9", "AA"):
        with pytest.raises(ValueError):
            M.validate(dup, [[0, 0], [0, 0]])
    assert M.validate("\xf7\xd7", [[0, 0], [0, 0]])[0] == b"\xf7\xd7"        # (0xF7 has no upper case: two symbols)
    with pytest.raises(ValueError):
        M.validate("AC", [[1 << 20, 0], [0, (1 << 20) + 1]])
    M.validate("AC", [[1 << 20, -(1 << 20)], [0, 0]])
    with pytest.raises(ValueError):
        M.validate("AC", [[1, 2], [3]])
    with pytest.raises(ValueError):
        M.validate("AC", [[1, 2.5], [3, 4]])
