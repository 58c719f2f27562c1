"""The pairs of the rows-per-lane grid tests, shared by tests/test_affine_grid_gpu.py and tests/test_affine_grid_cpu.py.

swmi_affine.hip compiles one sweep body per rows-per-lane value R = ceil(m / 64), R = 1 .. 16, for a read of m bases; lane l owns
the read rows l * R + 1 .. l * R + R, so row i sits in row slot (i - 1) % R of lane (i - 1) // R.  Everything here is
deterministic (fixed seeds) and TEST INFRASTRUCTURE ONLY (no test_ prefix: pytest does not collect it).

Shape grid: three read lengths per class R -- 64 R - 63 (the first: fewer than 64 lanes own rows for R >= 2; row m sits in slot
-64 mod R, which is slot 0 only where R divides 64), 64 R (the last: row m in slot R - 1 of lane 63) and one in between whose
row m sits in a slot strictly between 0 and R - 1 (for R >= 3; m % R != 0 for R >= 2 -- no length has m % 1 != 0) -- 48 reads.
The walk grid's reads have m = 1 (mod R): their row m sits in slot 0 for every R.  Every read holds a mutated copy of (a stretch of) the
long reference, about 150 bases with a repeat planted in it, at a position that differs from read to read.  The short reference
(37 bases: fewer columns than lanes, no multiple of 8) is a stretch of the long one.

Walk grid: one pair per R whose alignment is long and has a long run of either gap kind: the reference is the read with
substitutions, one run of read bases taken out of it (the walk inserts them: state INS over more than 16 rows, so across lane
boundaries for every R) and one run of extra columns put into it (the walk deletes them; for R >= 6 the run is longer than one
traceback tile of 4096 // (64 R) eight-step blocks).  Scores WALK_SCORES make both runs cheaper than breaking the alignment.

Matrix cases draw from "ACGTNacgtX": lower case folds onto upper case, X is outside the matrix's alphabet "ACGTN" and so keeps
the match / mismatch rule."""
import random

RS = tuple(range(1, 17))
PLAIN_ALPHABET = "ACGT"
MATRIX_DRAW = "ACGTNacgtX"
MATRIX_ALPHABET = "ACGTN"

SHAPE_SCORES = {False: (5, -3, -2, -6), True: (4, -3, -2, -6)}      # by matrix: (match, mismatch, gap, gap_open)
WALK_SCORES = (5, -3, -1, -4)

TILE_WORDS = 4096                                                   # SWMI_AFF_TILE_WORDS: dwords of the traceback's LDS tile


def rows_per_lane(m):
    """swmi_aff_rows_per_lane (csrc/swmi_device.h)"""
    r = (m + 63) // 64
    return 1 if r < 1 else r


def row_slot(i, R):
    """the row slot of read row i (1-based) in the lane that owns it"""
    return (i - 1) % R


def _middle(R):
    """a length strictly inside class R with m % R != 0 and row m strictly between slot 0 and slot R - 1 (R >= 3)"""
    m = 64 * R - 31
    if R == 1:
        return m
    while m % R == 0 or (R >= 3 and not 0 < row_slot(m, R) < R - 1):
        m += 1
    return m


GRID_LENGTHS = tuple(m for R in RS for m in (64 * R - 63, _middle(R), 64 * R))
FIRST_OF_CLASS = tuple(range(0, 48, 3))                             # indices into GRID_LENGTHS (and into the grid's reads)

assert len(GRID_LENGTHS) == 48 and len(set(GRID_LENGTHS)) == 48
assert [sum(rows_per_lane(m) == R for m in GRID_LENGTHS) for R in RS] == [3] * 16           # each class exactly three times
for _R in RS:
    _first, _mid, _last = GRID_LENGTHS[3 * (_R - 1):3 * _R]
    assert _first == 64 * _R - 63 and _last == 64 * _R and _first < _mid < _last
    assert rows_per_lane(_first - 1) == _R - 1 or _R == 1
    assert rows_per_lane(_last + 1) == _R + 1
    assert row_slot(_first, _R) == -64 % _R and row_slot(_last, _R) == _R - 1 and (_last - 1) // _R == 63
    assert _R < 2 or (_mid % _R != 0 and (_first + _R - 1) // _R < 64)
    assert _R < 3 or 0 < row_slot(_mid, _R) < _R - 1


def rand_seq(rng, n, alphabet=PLAIN_ALPHABET):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _substitute(rng, s, alphabet, rate, keep=()):
    """s with about `rate` of its bases redrawn; positions in `keep` stay"""
    return "".join(rng.choice(alphabet) if rng.random() < rate and x not in keep else c for x, c in enumerate(s))


def mutate(rng, s, alphabet=PLAIN_ALPHABET, subs=0.05, indels=0.01):
    """a copy of s with substitutions and a few one-base insertions and deletions"""
    out = []
    for c in s:
        x = rng.random()
        if x < indels:
            continue
        if x < 2 * indels:
            out.append(rng.choice(alphabet))
        out.append(rng.choice(alphabet) if rng.random() < subs else c)
    return "".join(out)


def score_matrix():
    """(alphabet, rows): asymmetric, the diagonal positive and some off-diagonal entries too (row = read base, column =
    reference base, as swmi_set_score_matrix takes it).  The off-diagonal entries are random as in _rand_matrix of
    tests/test_matrix_gpu.py; the diagonal is kept positive so that the planted copies stay the best alignments."""
    rng = random.Random(7301)
    k = len(MATRIX_ALPHABET)
    rows = [[rng.randint(5, 8) if a == b else rng.randint(-6, 3) for b in range(k)] for a in range(k)]
    assert rows != [list(c) for c in zip(*rows)]                                              # asymmetric
    assert sum(rows[a][b] > 0 for a in range(k) for b in range(k) if a != b) >= 2
    assert sum(rows[a][b] < 0 for a in range(k) for b in range(k) if a != b) >= 10
    return MATRIX_ALPHABET, rows


_SHAPE = {}


def shape_grid(matrix=False):
    """(refs, reads): refs = [the long reference, the short one], reads = the 48 of GRID_LENGTHS in that order.  The issue pairs
    the short reference with the reads FIRST_OF_CLASS only; a caller that can afford it pairs it with all of them."""
    if matrix not in _SHAPE:
        rng = random.Random(7101 + int(matrix))
        draw = MATRIX_DRAW if matrix else PLAIN_ALPHABET
        body = rand_seq(rng, 150, draw)
        unit = body[20:34]
        long_ref = body[:96] + unit + body[110:]                    # a 14-base repeat: columns 21 .. 34 and 97 .. 110
        assert len(long_ref) == 150 and long_ref.count(unit) >= 2
        short_ref = long_ref[60:97]
        reads = []
        for x, m in enumerate(GRID_LENGTHS):
            span = min(m, 130)                                      # bases of the reference the read copies
            at = (11 * x) % (150 - span + 1)
            copy = mutate(rng, long_ref[at:at + span], draw)[:m]
            pos = (29 * x + 5) % (m - len(copy) + 1)                # where the copy lies in the read
            read = rand_seq(rng, pos, draw) + copy
            reads.append(read + rand_seq(rng, m - len(read), draw))
        assert tuple(len(r) for r in reads) == GRID_LENGTHS
        _SHAPE[matrix] = ([long_ref, short_ref], reads)
    return _SHAPE[matrix]


# ---- the option grids: subopt and hits run the shape grid; end_bonus has a grid of its own ----
GRID_SUBOPT = 10                                                    # the mask half-width of test_grid_subopt and test_grid_hits
GRID_HITS = 4
ENDB_BONUSES = (1, 12)

_ENDB = {}


def endb_grid(R, matrix=False):
    """(refs, reads) of class R for option end_bonus.  The shape grid's references end far before a long read does, so there only
    the classes up to 7 ever take a pair to the end.  Here the reads are the three prefixes of one base sequence of 64 R bases with
    the class's GRID_LENGTHS, and the references are cut from mutated copies of it: one ends a few bases before the shortest read
    does, one between the ends of the two longer reads, one is a whole copy; each has a random tail, the last one 20 bases of it."""
    if (R, matrix) not in _ENDB:
        rng = random.Random(7500 + 16 * int(matrix) + R)
        draw = MATRIX_DRAW if matrix else PLAIN_ALPHABET
        base = rand_seq(rng, 64 * R, draw)
        first, mid, last = GRID_LENGTHS[3 * (R - 1):3 * R]
        reads = [base[:m] for m in (first, mid, last)]
        refs = [mutate(rng, base, draw, 0.05, 0.01)[:cut] + rand_seq(rng, tail, draw)
                for cut, tail in ((max(1, first - 4), 5), ((mid + last) // 2, 7), (last + 64, 20))]       # (the last: the whole copy)
        _ENDB[(R, matrix)] = (refs, reads)
    return _ENDB[(R, matrix)]


# ---- the banded matrix run of subopt and hits: sw_affine_sweep_band_{subopt,hits}_matrix_kernel ----
BAND_MATRIX_W, BAND_MATRIX_SUBOPT, BAND_MATRIX_HITS = 32, 60, 8
_BAND_MATRIX = []


def band_matrix_case():
    """(ref, read): a read of 1100 bases -- two strips, 76 rows in the second -- and a mutated copy of it plus 40 random bases"""
    if not _BAND_MATRIX:
        rng = random.Random(7551)
        read = rand_seq(rng, 1100, MATRIX_DRAW)
        _BAND_MATRIX.append((mutate(rng, read, MATRIX_DRAW, 0.04, 0.004) + rand_seq(rng, 40, MATRIX_DRAW), read))
    return _BAND_MATRIX[0]


def walk_plan(R):
    """(m, inserted read bases, deleted reference columns) of the walk-grid pair of class R.  The reads of R = 1 and 2 (51 and
    115 bases) are too short for a run of 40 and one of 24 next to stretches that pay for them: 8 and 8, and 20 and 16."""
    m = 64 * R - 13
    m -= row_slot(m, R)                                             # row m in slot 0
    if R == 1:
        return m, 8, 8
    if R == 2:
        return m, 20, 16
    return m, 40, 8 * (TILE_WORDS // (64 * R)) + 8 if R >= 6 else 24


_WALK = {}


def walk_grid(matrix=False):
    """[(R, ref, read)] for R = 1 .. 16.  The read is three stretches A | I | B C with I the inserted run; the reference is
    A' | B' | D | C' with D the deleted run and X' a copy of X with substitutions (none within 6 bases of a run's edge)."""
    if matrix not in _WALK:
        rng = random.Random(7201 + int(matrix))
        draw = MATRIX_DRAW if matrix else PLAIN_ALPHABET
        out = []
        for R in RS:
            m, ins, dele = walk_plan(R)
            assert rows_per_lane(m) == R and row_slot(m, R) == 0
            assert R < 3 or ins > 16
            assert R < 6 or dele > 8 * (TILE_WORDS // (64 * R))      # more columns than one tile's blocks hold steps
            a = (m - ins) // 3                                      # A, B and C share the rest of the read
            b = (m - ins - a) // 2
            read = rand_seq(rng, m, draw)
            A, B, C = read[:a], read[a + ins:a + ins + b], read[a + ins + b:]
            edges = lambda s: set(range(6)) | set(range(len(s) - 6, len(s)))
            ref = (_substitute(rng, A, draw, 0.04, edges(A)) + _substitute(rng, B, draw, 0.04, edges(B)) + rand_seq(rng, dele, draw) +
                   _substitute(rng, C, draw, 0.04, edges(C)))
            assert len(ref) == m - ins + dele <= m + 100
            out.append((R, ref, read))
        _WALK[matrix] = out
    return _WALK[matrix]


def longest_run(s, c="_"):
    """the longest run of character c in s"""
    best = cur = 0
    for x in s:
        cur = cur + 1 if x == c else 0
        best = max(best, cur)
    return best


# ---- the mixed launches of fit and global mode: narrow (R = 4), wide (R = 5) and strip pairs in one batch ----
MIXED_LENGTHS = (256, 257, 1025)
MIXED_SUBSETS = ((0, 2), (1, 2), (0, 1, 2), (2,), (0, 1))           # indices into MIXED_LENGTHS
MIXED_BAND = 16
assert [rows_per_lane(m) for m in MIXED_LENGTHS[:2]] == [4, 5] and MIXED_LENGTHS[2] > 1024

_MIXED = {}


def mixed_launch(matrix=False):
    """(refs, reads): two related references of about 1060 bases; reads of MIXED_LENGTHS bases, each holding a mutated stretch
    of the first reference.  The longest read's copy starts 30 rows down, so its row 1025 meets a column left of 1025 -
    MIXED_BAND, the first one of its second strip's window: the band changes that read's result."""
    if matrix not in _MIXED:
        rng = random.Random(7401 + int(matrix))
        draw = MATRIX_DRAW if matrix else PLAIN_ALPHABET
        base = rand_seq(rng, 1060, draw)
        refs = [base, mutate(rng, base, draw, 0.03, 0.004)]
        reads = []
        for m, head, at in zip(MIXED_LENGTHS, (0, 0, 30), (300, 610, 0)):
            read = rand_seq(rng, head, draw) + mutate(rng, base[at:at + m - head + 12], draw, 0.04, 0.004)
            reads.append(read[:m] + rand_seq(rng, m - len(read), draw))
        assert tuple(len(r) for r in reads) == MIXED_LENGTHS and all(1040 <= len(r) <= 1080 for r in refs)
        _MIXED[matrix] = (refs, reads)
    return _MIXED[matrix]
