"""Inputs for the pick kernels of options "subopt" and "hits" (sw_subopt_kernel / sw_hits_kernel of swmi_subopt.hip, DESIGN.md 8n and
8p), deterministic -- TEST INFRASTRUCTURE ONLY, shared by tests/test_pick_cpu.py and tests/test_pick_gpu.py.

Not collected by pytest (no test_ prefix).  The other option tests place their cases where the SWEEPS can write the row of column
maxima wrongly; these place the maximum columns, the runner-up and the earlier hits of a row where the PASS over it can go wrong:
against the 64-column step edges and the 256-column edge of its unrolled loop, in every in-flight load of its lookahead, at every
row-end length, densely, in sixteen rounds, and in partly filled workgroups.

THE COMB.  READ is 8 bases over ACG; a reference is all T with exact copies of READ ending at chosen 1-based columns and weak
copies, in which the first k of the read positions 2, 4, 6 are T.  Under SC = (5, -4, -3, -5) an isolated exact copy ending at e
leaves exactly PROFILE on the columns e - 7 .. e + 11 and 0 elsewhere: 5 .. 35 on the way up, 40 at e, then the gap's tail 32,
29 .. 2.  A weak copy reaches 31, 22 or 13 at its end.  So under w = 1 a single copy's runner-up is the left one (e - 2, 30), under
w = 2 the right one (e + 3, 26), and where every maximum column and every runner-up lies is chosen, not found.

Every family is a list of Case(name, ref, read, w, k, band, sc): w the mask half-width, k the K of the "hits" run.  The claims
the families make (which seam has a runner-up on which side, which row ends occur, how many entries a list has) are asserted by
tests/test_pick_cpu.py from the column maxima of subopt_reference.local_h, which rows() hands out once per (ref, read, band).
"""
import collections
import random

import subopt_reference as sr

SC = (5, -4, -3, -5)            # match, mismatch, gap, gap_open: the comb
LOG = (2, -3, -4, -6)           # the band family: keeps random sequence in the logarithmic phase
WAVE = 64
_rng = random.Random(9500)
READ = "".join(_rng.choice("ACG") for _ in range(8))
A8 = "AAAAAAAA"                 # against all T: a degenerate pair; against a comb: many tied maximum columns
PROFILE = [5, 10, 15, 20, 25, 30, 35, 40, 32, 29, 26, 23, 20, 17, 14, 11, 8, 5, 2]      # columns e - 7 .. e + 11
AUTO = sr.AUTO

Case = collections.namedtuple("Case", "name ref read w k band sc")


def case(name, ref, w, k, read=READ, band=0, sc=SC):
    return Case(name, ref, read, w, k, band, sc)


def weak_read(k):
    """READ with the first k of the positions 2, 4, 6 (1-based) replaced by T: its copy reaches 40 - 9 k"""
    out = list(READ)
    for p in (1, 3, 5)[:k]:
        out[p] = "T"
    return "".join(out)


def comb(n, exact=(), weak=()):
    """all T, n columns, with exact copies ending at the 1-based columns `exact` and weak ones at `weak` = [(end, k)]; copies do
    not overlap"""
    ref = ["T"] * n
    taken = set()
    for e, k in [(e, 0) for e in exact] + list(weak):
        assert 8 <= e <= n and not taken & set(range(e - 8, e)), (n, exact, weak)
        taken |= set(range(e - 8, e))
        ref[e - 8:e] = weak_read(k)
    return "".join(ref)


# ---- what a case's row holds (the restatement's column maxima; memoised: the CPU tests share them) -----------------------------
_rows = {}


def cols_of(c):
    """the columns the pick reads: n, or the last strip's window end under a band (swmi_aff_colmax_cols)"""
    m, n = len(c.read), len(c.ref)
    return min(n, 1024 * ((m + 1023) // 1024) + c.band) if c.band and m > 1024 else n


def rows(c):
    """(s, colmax, row): the pair's score and, for the columns 1 .. cols_of(c) at index 0 .., the column maximum and the smallest
    row that holds it.  (0, [], []) for a pair with an empty side"""
    key = (c.ref, c.read, c.band, c.sc)
    if key not in _rows:
        if not c.ref or not c.read:
            _rows[key] = (0, [], [])
        else:
            H = sr.local_h(c.ref, c.read, c.sc, c.band)
            n = cols_of(c)
            cm = [int(x) for x in H[1:].max(axis=0)[1:n + 1]]
            rw = [int(x) + 1 for x in H[1:].argmax(axis=0)[1:n + 1]]
            assert max(int(x) for x in H[1:].max(axis=0)) == max(cm)        # (nothing right of the last window: those cells do not exist)
            _rows[key] = (max(cm), cm, rw)
    return _rows[key]


def width(c):
    return sr.mask_width(c.w, len(c.read))


# ---- slide: one copy moved across every step edge --------------------------------------------------------------------------------
SLIDE_N = 321                   # one unrolled quad (columns 1 .. 256), a whole tail step and a partial one of one column


def slide(w):
    """one exact copy ending at e, for every e within w + 2 of a multiple of 64 up to 320, and e = 8 and e = n.  Claim: for each of
    the five seams some case has its runner-up in the step before its maximum column's, and some case in the step after"""
    ends = {8, SLIDE_N}
    for seam in range(WAVE, SLIDE_N, WAVE):
        ends |= {seam + d for d in range(-(w + 2), w + 3) if 8 <= seam + d <= SLIDE_N}
    return [case("slide-w%d-e%d" % (w, e), comb(SLIDE_N, [e]), w, 3) for e in sorted(ends)]


# ---- row ends: every length class of the two loops -------------------------------------------------------------------------------
# the issue's fourteen lengths, and 128 and 191: without them (cols - 1) % 256 // 64 = 1 has no whole last step and = 2 no partial one
ROW_END_N = (8, 63, 64, 65, 128, 191, 192, 193, 255, 256, 257, 448, 449, 511, 512, 513)


def row_ends():
    """the exact copy at e = n with a weak one at the front (w = 1: the runner-up is two columns left of the row's end; w = 12: the
    weak copy), and the other way round: end2 = n, in lane 0 or 63 of the last step where n allows.  Claim: every value of
    (cols - 1) % 256 // 64 occurs with the last step partial and with it whole; end2 = n occurs in lane 0 and in lane 63"""
    out = []
    for n in ROW_END_N:
        front = [(8, 1)] if n >= 29 else []
        for w in (1, 12):
            out.append(case("end-n%d-w%d-max-last" % (n, w), comb(n, [n], front), w, 3))
        if n >= 29:
            out.append(case("end-n%d-w12-weak-last" % n, comb(n, [8], [(n, 1)]), 12, 3))
    return out


# ---- lookahead: the next maximum column in each in-flight load, a quad skipped, the row exhausted, kept, searched again ------------
LOOK_DELTA = {1: 0, 2: 33, 3: 17, 4: 34, 5: 3, 9: 21}         # (29 + delta < 64: the second copy ends in step d)


def lookahead():
    """w = 20; a first exact copy ends at 30, a second one 64 d + delta behind it.  A weak copy (31) lies 64 columns before the
    second one where that is between the two (d >= 2), and in a second variant 45 behind it.  `short-nxt`: the weak copy ends in lane
    63 of step 0 and the second exact one in lane 9 of step t -- found by load t - 1 of the first search; a `nxt` that is t - 1 steps
    short would lie 10 columns behind the weak copy and mask it"""
    out = []
    for n in (700, 1100):
        for d, delta in LOOK_DELTA.items():
            e2 = 30 + WAVE * d + delta
            if d >= 2:
                out.append(case("look-n%d-d%d-between" % (n, d), comb(n, [30, e2], [(e2 - WAVE, 1)]), 20, 3))
            out.append(case("look-n%d-d%d-behind" % (n, d), comb(n, [30, e2], [(e2 + 45, 1)]), 20, 3))
        for t in (2, 3, 4):
            out.append(case("look-n%d-short-nxt-%d" % (n, t), comb(n, [30, WAVE * t + 10], [(WAVE, 1)]), 20, 3))
        out.append(case("look-n%d-alone" % n, comb(n, [30], [(400, 1)]), 20, 3))
        out.append(case("look-n%d-three" % n, comb(n, [30, 30 + 2 * WAVE + 9, 30 + 7 * WAVE + 40], [(300, 1), (n - 20, 2)]), 20, 3))
        out.append(case("look-n%d-nothing-eligible" % n, comb(n, [30, n - 30]), n // 2, 3))
    out.append(case("look-checked-700", comb(700, [30, 100], [(400, 1)]), 20, 3))
    out.append(case("look-checked-1100", comb(1100, [30, 700], [(500, 2)]), 40, 3))
    return out


LOOK_CHECKED = {"look-checked-700": (31, 400), "look-checked-1100": (22, 500)}


# ---- dense: a maximum column every 16 columns ------------------------------------------------------------------------------------
def dense():
    """an exact copy every 16 columns over 600.  w = 7 leaves one eligible column per period (all equal: the smallest wins, and
    sixteen rounds list sixteen of them); w = 8 leaves none, unless one copy is left out: then the only eligible columns straddle the
    step edge 64 | 65; w = 3 as well"""
    out = []
    for off in (0, 6):
        ends = [e for e in range(16 + off, 600, 16)]
        for w in (3, 7, 8):
            out.append(case("dense-off%d-w%d" % (off, w), comb(600, ends), w, 16))
        out.append(case("dense-off%d-w8-one-out" % off, comb(600, [e for e in ends if e != 64 + off]), 8, 16))
    return out


# ---- rounds: sixteen entries ------------------------------------------------------------------------------------------------------
ROUNDS_EXACT = 7                # the step that holds the exact copy
ROUNDS_STRENGTH = (1, 3, 2, 1, 2, 3, 1, 0, 3, 2, 1, 2, 3, 1, 2, 3)


def rounds_ends():
    """one copy per 64-column step of 1,024 columns: column 8 in step 0 (within w of column 0: where a test of lane 0's pj would
    mask), then lane 0, lane 63 and mid-step in turn"""
    return [8] + [WAVE * t + (31, 1, 64, 41)[t % 4] for t in range(1, 16)]


def rounds():
    """one exact copy and 15 weak ones, strengths 31, 22 and 13 in no order of columns: 16 entries under w = 12, equal ones listing
    the smaller column first.  Then two weak copies d = 16 columns apart across the step edge 128 | 129, under w = d - 1 (both
    listed) and w = d (the second one masked by the first: the strict mask around an earlier entry)"""
    ends = rounds_ends()
    ref = comb(1024, [ends[ROUNDS_EXACT]], [(e, k) for e, k in zip(ends, ROUNDS_STRENGTH) if k])
    out = [case("rounds-k%d" % k, ref, 12, k) for k in (1, 2, 3, 16)]
    pair = comb(321, [30], [(120, 1), (136, 2)])
    return out + [case("rounds-apart-w15", pair, 15, 4), case("rounds-apart-w16", pair, 16, 4)]


# ---- wide masks -------------------------------------------------------------------------------------------------------------------
def wide():
    """w = 63, 64, 65 with a weak copy 64, 65 and 66 columns right and left of the exact one; w = 2^30 on 513 columns (nothing is
    eligible; j + w passes 2^31 in 32 bits); AUTO (15 for this read) with the weak copy 15 and 16 columns away"""
    out = []
    for w in (63, 64, 65):
        for d in (64, 65, 66):
            out.append(case("wide-w%d-right%d" % (w, d), comb(321, [100], [(100 + d, 1)]), w, 3))
            out.append(case("wide-w%d-left%d" % (w, d), comb(321, [100 + d], [(100, 1)]), w, 3))
    out.append(case("wide-w2^30", comb(513, [200], [(500, 1)]), 1 << 30, 3))
    for d in (15, 16):
        out.append(case("wide-auto-%d" % d, comb(321, [100], [(100 + d, 1), (100 - d, 2)]), AUTO, 3))
    return out


# ---- layout: partly filled workgroups, a degenerate and an empty pair inside one ------------------------------------------------------
def layout_cut(q, r):
    """the first 4 q + r slide cases of w = 1: the last workgroup of SUB_WAVES = 4 pairs holds r"""
    return slide(1)[:4 * q + r]


def layout_mixed():
    """(refs, reads, w, k): slide, dense and rounds references against [READ, A8], pair = 2 * ref + read.  Reference 2 is all T
    (its pair with A8, pair 5, is degenerate: second of its workgroup) and reference 4 is empty (its two pairs are in no launch, so
    every later pair's place in the launch differs from its place in the results).  Large enough for two launches under the
    smallest max_workspace_bytes"""
    refs = [c.ref for c in slide(2)]
    refs[2:2] = ["T" * SLIDE_N]
    refs[4:4] = [""]
    refs += [c.ref for c in dense()] + [c.ref for c in rounds()[:1]] * 3
    return refs, [READ, A8], 2, 3


# ---- band: the row ends at the last window's end ------------------------------------------------------------------------------------
BAND = 50                       # m = 1100: the last window ends at column 2048 + 50 = 2098 = 32 * 64 + 50


def band():
    """two pairs, read of 1,100 bases against 2,300 columns under band 50, scores LOG: swmi_aff_colmax_cols = 2098, no multiple of 64.
    The best alignment (rows 1025 .. 1100) ends in the last swept column; a copy of rows 901 .. 1050 right of it scores more and
    must not count -- with the band off it wins.  Pair 0: the runner-up is a copy in strip 0's columns (w = 100).  Pair 1: the best
    alignment's own prefix under w = 5, in the last, partial step"""
    rng = random.Random(9501)
    read = "".join(rng.choice("ACGT") for _ in range(1100))
    out = []
    for pair in (0, 1):
        ref = [rng.choice("ACGT") for _ in range(2300)]
        ref[2022:2098] = read[1024:1100]
        ref[2110:2260] = read[900:1050]
        if pair == 0:
            ref[400:460] = read[380:440]
        out.append(case("band-%d" % pair, "".join(ref), (100, 5)[pair], 4, read, BAND, LOG))
    return out


def comb_families():
    """{family: cases}, the comb families in the order of the module"""
    return {"slide": slide(1) + slide(2), "row_ends": row_ends(), "lookahead": lookahead(), "dense": dense(), "rounds": rounds(),
            "wide": wide()}


def mixed_cases():
    """layout_mixed() as cases, one per pair with both sides non-empty"""
    refs, reads, w, k = layout_mixed()
    return [case("mixed-r%d-q%d" % (r, q), ref, w, k, read) for r, ref in enumerate(refs) for q, read in enumerate(reads) if ref]


def all_cases():
    """every pair the GPU module runs"""
    out = [c for fam in comb_families().values() for c in fam]
    return out + mixed_cases() + band()
