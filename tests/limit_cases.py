"""Inputs at the limits of the score arithmetic, shared by the CPU and the GPU tests -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).

Linear pipelines: DESIGN.md section 2 promises Java `int` wrap-around (every score add/sub in uint32).  WRAP_SCORES are score
sets under which sums do wrap on inputs of a few dozen bases; a wrapped sum is a positive H plus a positive score that comes
out negative and must lose to 0.  tests/test_oracle.py proves on small batches that the wrap changes the answer, so a kernel
that widened a sum or compared through the sign of a difference would be caught by tests/test_gpu_parity.py.

Affine kernels: every score at +-2^20 (include/swmi.h), the largest matrix the ABI takes (64 symbols).
"""
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRAP_SCORES = [
    (1 << 30, -3, -4),                  # the second match of a run wraps
    (10 ** 9, -3, -4),                  # two matches fit, the third wraps
    (715827883, -3, -4),                # 3 * 715827883 = 2^31 + 1
    (2 ** 31 - 1, -2 ** 31, -2 ** 31),  # both ends of int
    (10 ** 9, -10 ** 9, -1),            # a huge H with nearly free gaps
    (1 << 30, 1 << 29, -4),             # positive mismatch (the kernels' mode 1 falls to mode 2)
    (10 ** 9, 5, 7),                    # positive gap, long paths
]
# a positive gap that makes a GAP sum wrap (H + gap past 2^31 - 1): defined by the reference, agreed on by both oracles,
# refused by the library (include/swmi.h: the documented deviation)
POSITIVE_GAP_WRAP_SCORES = [(10 ** 9, 5, 10 ** 9), (5, -3, 2 ** 31 - 1)]


def positive_gap_accepted(scores, moves):
    """the rule of include/swmi.h for gap > 0, restated: moves = longest read + longest reference of the batch"""
    B = 2 ** 31 - 1
    if scores[2] <= 0:
        return True
    pos = sorted({x for x in scores if x > 0}, reverse=True)
    h_max = min(moves, B // pos[0]) * pos[0] + (min(moves, B // pos[1]) * pos[1] if len(pos) > 1 else 0)
    return min(B, h_max) + scores[2] <= B


# large operands on both sides of every compare, and no wrap at all (reads of at most 300 bases)
LARGE_SCORES = [(1 << 20, -(1 << 20), -(1 << 19)), (7000000, -1, -6999999)]


def score_id(sc):
    return "_".join(str(x) for x in sc)


def wrap_kats():
    """hand-derived known answers under wrapping scores, in the format of kat.json (tests/golden/wrap_kat.json)"""
    with open(os.path.join(ROOT, "tests", "golden", "wrap_kat.json")) as f:
        return json.load(f)["kats"]


def rand_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def small_wrap_batch(k):
    """3 references of 20-80 bases x 4 reads of 3-40 bases over AC and ACGT for score set k: small enough for the pure-Python
    twin, repetitive enough for runs of matches (which is where a sum wraps)"""
    rng = random.Random(7100 + k)
    refs = [rand_seq(rng, rng.randint(20, 80), a) for a in ("AC", "ACGT", "AC")]
    reads = [rand_seq(rng, rng.randint(3, 40), a) for a in ("AC", "ACGT", "AC")]
    reads.append(refs[1][5:5 + rng.randint(10, 15)])            # an exact cut: a run of matches that certainly wraps
    return refs, reads


# ---- affine kernels ------------------------------------------------------------------------------------------------
L = 1 << 20
# (match, mismatch, gap, gap_open): every score at its bound; a positive mismatch; gap_open = 0; a free extension
AFFINE_BOUND_SCORES = [(L, -L, -L, -L), (L, L, -L, -L), (L, -L, -L, 0), (L, -L, 0, -L)]


def affine_bound_pair(m, cut, n_side, seed=1400):
    """a read of m bases over AC and a reference that holds a cut of `cut` bases of it between 2 * n_side random ones"""
    rng = random.Random(seed)
    read = rand_seq(rng, m, "AC")
    at = (m - cut) // 2
    return rand_seq(rng, n_side, "AC") + read[at:at + cut] + rand_seq(rng, n_side, "AC"), read


def big_matrix(seed=1500):
    """The largest matrix swmi_set_score_matrix takes: 64 symbols -- A-Z, 0-9, 23 accented capitals (bytes 0xC0-0xD6) and five
    punctuation marks --, entries random in [-2^20, 2^20], asymmetric, both extremes present.  Returns (matrix, sequence
    alphabet): sequences are drawn from the symbols, the lower-case forms of the letters (one symbol with their capitals)
    and two bytes outside the alphabet, which score match / mismatch."""
    rng = random.Random(seed)
    alpha = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789" + "".join(chr(c) for c in range(0xC0, 0xD7)) + "!#$%&"
    assert len(alpha) == 64
    rows = [[rng.randint(-L, L) for _ in alpha] for _ in alpha]
    rows[3][5], rows[5][3], rows[7][7], rows[63][0] = L, -L, -L, L
    draw = alpha + "abcdefghijklmnopqrstuvwxyz" + "".join(chr(c) for c in range(0xE0, 0xF7)) + "~\xf7"
    return (alpha, rows), draw
