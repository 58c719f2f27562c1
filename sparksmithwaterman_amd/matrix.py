"""Substitution score matrices (swmi_set_score_matrix): the NCBI text format, a built-in BLOSUM62, and
the checks the library makes when a matrix is set.

A matrix is an alphabet of n symbols (1..64, pairwise distinct after Character.toUpperCase on ISO-8859-1) and n x n integer
scores, row = READ base, column = REFERENCE base.  Context.set_score_matrix takes one.
"""
import collections

MAX_SYMBOLS = 64
MAX_ABS_SCORE = 1 << 20           # every sum of the affine recurrence stays within int32

ScoreMatrix = collections.namedtuple("ScoreMatrix", "alphabet scores")   # alphabet: bytes; scores: tuple of n row tuples


def canonical(byte):
    """The symbol a byte stands for: Character.toUpperCase on ISO-8859-1 (a-z and 0xE0-0xFE except 0xF7 drop 0x20)."""
    return byte - 32 if (0x61 <= byte <= 0x7A or (0xE0 <= byte <= 0xFE and byte != 0xF7)) else byte


def _symbols(alphabet):
    if isinstance(alphabet, str):
        return alphabet.encode("latin-1")
    if isinstance(alphabet, (bytes, bytearray)):
        return bytes(alphabet)
    return b"".join(_symbols(a) for a in alphabet)          # a list of one-symbol strings


def validate(alphabet, scores):
    """(alphabet bytes, row-major list of n*n ints) for a valid matrix; ValueError otherwise (the library's checks:
    1 <= n <= 64, symbols distinct after canonicalisation, |entry| <= 2^20)."""
    sym = _symbols(alphabet)
    n = len(sym)
    if n < 1 or n > MAX_SYMBOLS:
        raise ValueError("a score matrix has 1 to %d symbols, got %d" % (MAX_SYMBOLS, n))
    seen = {}
    for k, c in enumerate(sym):
        u = canonical(c)
        if u in seen:
            raise ValueError("score matrix symbols %d and %d (%r, %r) are the same symbol" % (seen[u], k, chr(sym[seen[u]]), chr(c)))
        seen[u] = k
    rows = [list(r) for r in scores]
    if len(rows) != n or any(len(r) != n for r in rows):
        raise ValueError("a score matrix over %d symbols needs %d rows of %d entries" % (n, n, n))
    flat = []
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            if int(v) != v:
                raise ValueError("score matrix entry [%d][%d] = %r is not an integer" % (i, j, v))
            if abs(int(v)) > MAX_ABS_SCORE:
                raise ValueError("score matrix entry [%d][%d] = %d: |entries| must be <= 2^20" % (i, j, int(v)))
            flat.append(int(v))
    return sym, flat


def parse_ncbi(text):
    """A matrix in the NCBI text format: '#' comment lines, a header row of column symbols, then one row per symbol that starts
    with its symbol.  The rows must name the header's symbols in the header's order."""
    header, rows = None, []
    for ln, line in enumerate(text.splitlines(), 1):
        f = line.split()
        if not f or f[0].startswith("#"):
            continue
        if header is None:
            header = f
            if any(len(s) != 1 for s in header):
                raise ValueError("line %d: header symbols must be single characters" % ln)
            continue
        if len(rows) >= len(header) or f[0] != header[len(rows)]:
            raise ValueError("line %d: unexpected row %r (rows follow the header's order)" % (ln, f[0]))
        if len(f) != len(header) + 1:
            raise ValueError("line %d: %d scores for %d symbols" % (ln, len(f) - 1, len(header)))
        try:
            rows.append(tuple(int(x) for x in f[1:]))
        except ValueError:
            raise ValueError("line %d: scores must be integers" % ln) from None
    if header is None or len(rows) != len(header):
        raise ValueError("incomplete matrix: %d rows for %d symbols" % (len(rows), 0 if header is None else len(header)))
    sym, _ = validate("".join(header), rows)
    return ScoreMatrix(sym, tuple(rows))


def load(path):
    """parse_ncbi of a file (ISO-8859-1)."""
    with open(path, "rb") as f:
        return parse_ncbi(f.read().decode("latin-1"))


def uniform(alphabet, match, mismatch):
    """match on the diagonal, mismatch off it: the same scores as no matrix."""
    sym = _symbols(alphabet)
    return ScoreMatrix(sym, tuple(tuple(match if i == j else mismatch for j in range(len(sym))) for i in range(len(sym))))


def profile_from_matrix(read, alphabet, scores, default):
    """The per-read profile (Batch.set_read_profiles) that scores as the matrix does: row i is the matrix row
    of read[i]'s symbol, M[class(read[i])][.], and a row of `default` for a read base outside the alphabet (give `mismatch`: such
    a base scores that against every symbol of the alphabet -- it can equal none).  alphabet, scores: as for validate, or a
    ScoreMatrix as `alphabet` with scores None.  Returns a list of m rows of n ints."""
    if isinstance(alphabet, ScoreMatrix) and scores is None:
        alphabet, scores = alphabet.alphabet, alphabet.scores
    sym, flat = validate(alphabet, scores)
    n = len(sym)
    cls = {canonical(c): k for k, c in enumerate(sym)}
    rd = read if isinstance(read, (bytes, bytearray)) else read.encode("latin-1")
    out = []
    for b in rd:
        k = cls.get(canonical(b))
        out.append([int(default)] * n if k is None else flat[k * n:(k + 1) * n])
    return out


def quality_profile(read, quals, alphabet, match, mismatch_of_q):
    """A quality-aware profile for a mapper: row i scores `match` in the column of read[i]'s symbol and mismatch_of_q(quals[i])
    in every other column (a mismatch at a Q2 base costs less than one at a Q40 base).  A read base outside the alphabet
    mismatches every symbol.  quals: one integer per base; mismatch_of_q: a function of it."""
    sym = _symbols(alphabet)
    n = len(sym)
    cls = {canonical(c): k for k, c in enumerate(sym)}
    rd = read if isinstance(read, (bytes, bytearray)) else read.encode("latin-1")
    if len(quals) != len(rd):
        raise ValueError("%d qualities for a read of %d bases" % (len(quals), len(rd)))
    out = []
    for b, q in zip(rd, quals):
        mm = int(mismatch_of_q(q))
        row = [mm] * n
        k = cls.get(canonical(b))
        if k is not None:
            row[k] = int(match)
        out.append(row)
    return out


# BLOSUM62 (Henikoff & Henikoff 1992) as NCBI distributes it
BLOSUM62_TEXT = """\
#  Matrix made by matblas from blosum62.iij
#  BLOSUM Clustered Scoring Matrix in 1/2 Bit Units
   A  R  N  D  C  Q  E  G  H  I  L  K  M  F  P  S  T  W  Y  V  B  Z  X  *
A  4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0 -2 -1  0 -4
R -1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3 -1  0 -1 -4
N -2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3  3  0 -1 -4
D -2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3  4  1 -1 -4
C  0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1 -3 -3 -2 -4
Q -1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2  0  3 -1 -4
E -1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4
G  0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3 -1 -2 -1 -4
H -2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3  0  0 -1 -4
I -1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3 -3 -3 -1 -4
L -1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1 -4 -3 -1 -4
K -1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2  0  1 -1 -4
M -1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1 -3 -1 -1 -4
F -2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1 -3 -3 -1 -4
P -1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2 -2 -1 -2 -4
S  1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2  0  0  0 -4
T  0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0 -1 -1  0 -4
W -3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3 -4 -3 -2 -4
Y -2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1 -3 -2 -1 -4
V  0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4 -3 -2 -1 -4
B -2 -1  3  4 -3  0  1 -1  0 -3 -4  0 -3 -3 -2  0 -1 -4 -3 -3  4  1 -1 -4
Z -1  0  0  1 -3  3  4 -2  0 -3 -3  1 -1 -3 -1  0 -1 -3 -2 -2  1  4 -1 -4
X  0 -1 -1 -1 -2 -1 -1 -1 -1 -1 -1 -1 -1 -1 -2  0  0 -2 -1 -1 -1 -1 -1 -4
* -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4 -4  1
"""

BLOSUM62 = parse_ncbi(BLOSUM62_TEXT)
