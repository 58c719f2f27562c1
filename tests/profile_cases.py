"""Inputs of the per-read profile tests and their expected values -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  tests/test_profile_cpu.py holds every recipe to what it is built for, on the restatements
of tests/profile_reference.py alone; tests/test_profile_gpu.py runs them on the GPU.

The class grid.  One batch per rows-per-lane class R = 1 .. 16 of swmi_affine.hip (R = ceil(m / 64)): five reads of different
lengths in the class -- 64 R - 3 first, 64 (R - 1) + 1 last, for R = 16 also 1024 -- against three references of 70 to 130 bases over
the five-symbol alphabet ACGTN, with bytes outside it and lower-case letters among them.  That is 15 pairs, no multiple of the four
wavefronts of a workgroup, and four different tables in every workgroup.  The entries are random in -6 .. 7."""
import functools
import random

import gotoh_reference as gr
import overlap_reference as ov
import profile_reference as pr

ALPHABET = "ACGTN"
SC = (5, -3, -2, -6)                                    # (match, mismatch, gap, gap_open)
RS = tuple(range(1, 17))
# the five runs a profile is built for: gotoh_reference's mode, extend, overlap
MODES = {"local": (gr.LOCAL, False, False), "fit": (gr.FIT, False, False), "global": (gr.GLOBAL, False, False),
         "extend": (gr.GLOBAL, True, False), "overlap": (gr.FIT, False, True)}


def options(name):
    """the context options of a run of MODES[name]"""
    mode, extend, overlap = MODES[name]
    return dict(align_mode=mode, extend=int(extend), overlap=int(overlap))


def random_profile(rng, m, n=len(ALPHABET), lo=-6, hi=7):
    return [[rng.randint(lo, hi) for _ in range(n)] for _ in range(m)]


def random_reference(rng, n):
    """over ACGTN, about one byte in twelve outside the alphabet and one in eight lower-case"""
    out = []
    for _ in range(n):
        c = rng.choice("XZ*") if rng.random() < 0.08 else rng.choice(ALPHABET)
        out.append(c.lower() if rng.random() < 0.12 else c)
    return "".join(out)


@functools.lru_cache(maxsize=None)
def grid(R):
    """(refs, reads, profiles) of class R"""
    rng = random.Random(7700 + R)
    lengths = [64 * R - 3, 64 * R - 20, 64 * R - 41, 64 * R if R == 16 else 64 * R - 9, 64 * (R - 1) + 1]
    assert len(set(lengths)) == 5 and all((m + 63) // 64 == R for m in lengths)
    reads = ["".join(rng.choice("ACGTacgtN") for _ in range(m)) for m in lengths]
    refs = [random_reference(rng, n) for n in (70, 101, 130)]
    return tuple(refs), tuple(reads), tuple(random_profile(rng, m) for m in lengths)


def want(ref, read, profile, name, tie, sc=SC, alphabet=ALPHABET):
    mode, extend, overlap = MODES[name]
    return pr.align_numpy(ref, read, alphabet, profile, sc, mode, extend, overlap, tie, cells=True)


def plain(ref, read, name, tie, sc=SC):
    """the same pair under match / mismatch"""
    mode, extend, overlap = MODES[name]
    if overlap:
        return ov.align_numpy(ref, read, sc, mode, 0, False, tie, None, cells=True)
    return gr.align_numpy(ref, read, sc, mode, 0, extend, tie, None, cells=True)


@functools.lru_cache(maxsize=None)
def expected(R, name, tie):
    """{(r, q): (score, alignments, cells)} of the class grid"""
    refs, reads, profiles = grid(R)
    return {(r, q): want(refs[r], reads[q], profiles[q], name, tie) for r in range(len(refs)) for q in range(len(reads))}


# ---- matrix parity: 6 x 6 protein pairs of 40 to 300 residues under BLOSUM62 ----
PROTEIN = "ARNDCQEGHILKMFPSTWYV"
SC_PROTEIN = (1, -4, -1, -11)                           # BLOSUM62 with gaps -11 / -1 (match is not read inside the alphabet)


@functools.lru_cache(maxsize=None)
def protein_pairs():
    rng = random.Random(6262)
    base = "".join(rng.choice(PROTEIN) for _ in range(400))
    reads, refs = [], []
    for m in (40, 77, 129, 200, 257, 300):
        at = rng.randrange(0, 400 - m)
        reads.append("".join(rng.choice(PROTEIN) if rng.random() < 0.15 else c for c in base[at:at + m]))
    for n in (40, 90, 150, 210, 260, 300):
        at = rng.randrange(0, 400 - n)
        refs.append("".join(rng.choice(PROTEIN + "BZX") if rng.random() < 0.1 else c for c in base[at:at + n]))
    return tuple(refs), tuple(reads)


# ---- ties beyond cell_cap: a periodic profile against a periodic reference ----
def periodic_case():
    """(ref, read, profile): the read's profile rewards ACGT at rows 0..3 with period 4, the reference is ACGT x 12: a local run ties in
    many cells, far more than cell_cap = 2"""
    read = "ACGT" * 3
    profile = [[4 if c == i % 4 else -3 for c in range(len(ALPHABET))] for i in range(len(read))]
    return "ACGT" * 12, read, profile
