"""Gap-heavy alignments at the column-chunk halo and at the path-length bound -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  tests/test_gap_paths_cpu.py proves on the CPU that every input below is as sharp
as it claims to be; tests/test_gap_paths_gpu.py runs them through the kernels.

Two pieces of host arithmetic (csrc/swmi_plan.h) are restated here WITHOUT looking at the library: the halo of a column chunk
(path_span, col_chunk, and the chunk lists of Planner::take_cols / take_strips) and the longest possible traceback
(path_bound).  The inputs are RATCHET pairs, the only kind of pair whose optimum comes near either: a walked path has every
prefix score in (0, final], so the gaps have to be paid for as they come.  The gapless sequence is cut into segments of k
bases over ACG, the other sequence holds the same segments separated by runs of the filler base T; every run costs almost
what the path has earned so far, and the score reaches its maximum in the last cell only.
"""
import functools
import random
from collections import namedtuple

import numpy as np

FILLER = "T"
STEP_W = 32                        # anti-diagonal steps (= columns of lane 0) per checkpoint window
RMAX = 4                           # rows per lane of the widest sweep: strips of 256 read rows


# ---- the ratchet -----------------------------------------------------------------------------------------------------------
def ratchet(rng, m, scores, k, kind, tight=0, gap_open=0):
    """(body_ref, read, gaps): m bases over ACG cut into segments of k (the last one takes the remainder) -- the read of a
    deletion ratchet (kind "del"), the reference of an insertion ratchet ("ins") -- and the other sequence with a run of T
    between consecutive segments.  gaps: the gap moves of the intended path, which has m alignment moves.
    The runs: d = (match * k - 1 + gap_open) // |gap| bases each, so that a cycle nets a small positive amount and the peaks
    climb; tight=F > 0 (linear gaps) instead lets every run spend the score down to the smallest value of at least F, and
    shortens the last run until the final score exceeds every earlier peak -- with F = 1 the longest path there is for the
    segments."""
    match, _, gap = scores
    g = -gap
    assert kind in ("del", "ins") and match > 0 and g > 0 and gap_open <= 0 and m >= 2 * k
    segs = ["".join(rng.choice("ACG") for _ in range(k)) for _ in range(m // k - 1)]
    segs.append("".join(rng.choice("ACG") for _ in range(k + m % k)))
    runs = []
    if not tight:
        runs = [(match * k - 1 + gap_open) // g] * (len(segs) - 1)
    else:
        assert gap_open == 0
        s, peaks = 0, []
        for x, seg in enumerate(segs[:-1]):
            s += match * len(seg)
            peaks.append(s)
            d = (s - tight) // g
            if x == len(segs) - 2:                 # the last run: the final cell must be the only maximum
                while d > 0 and s - d * g + match * len(segs[-1]) <= max(peaks):
                    d -= 1
            runs.append(d)
            s -= d * g
    assert all(d > 0 for d in runs)
    gapped = segs[0] + "".join(FILLER * d + seg for d, seg in zip(runs, segs[1:]))
    plain = "".join(segs)
    return (gapped, plain, sum(runs)) if kind == "del" else (plain, gapped, sum(runs))


def planted(body, n, end_col):
    """body padded with T on both sides to n bases, its last base at 1-based column end_col"""
    assert len(body) <= end_col <= n
    return FILLER * (end_col - len(body)) + body + FILLER * (n - end_col)


# ---- swmi_plan.h, restated ---------------------------------------------------------------------------------------------------
def rows_per_lane(m):
    return min(RMAX, max(1, (m + 63) // 64))


def path_span(m, scores):
    """columns a positive-score path of an m-base read can span"""
    match, _, gap = scores
    return m + max(match, 0) * m // (-gap if gap < 0 else 1) + 1


def ck_windows(n):
    return ((n + 63 + 15) // 16 + 1) // 2


def col_chunk(g_lo, wpc, n_ck, n, span):
    """(g_lo, g_hi, col0) of the chunk that owns the windows from g_lo on"""
    g_hi = min(g_lo + wpc, n_ck)
    if g_hi < n_ck and g_hi * STEP_W > n:
        g_hi = n_ck
    c0 = g_lo * STEP_W - 64 - span - 1
    return g_lo, g_hi, (0 if g_lo == 0 or c0 <= 0 else c0 // STEP_W * STEP_W)


def path_bound(n, m, scores, align_mode=0):
    """moves of the longest possible traceback of an n x m pair"""
    match, mismatch, gap = scores
    path = n + m
    if align_mode == 0 and match > 0 and gap < 0 and mismatch <= match:
        path = min(path, m + min(n, match * m // -gap), n + min(m, match * n // -gap))
    return path


def _chunks_possible(scores, n_pairs, col_chunks):
    match, mismatch, gap = scores
    return (match > 0 and gap < 0 and mismatch <= 0 and match <= 7 and mismatch >= -8 and
            (n_pairs <= 512 or col_chunks > 1) and col_chunks != 1)


def _chunk_list(chunks, n, span):
    n_ck = ck_windows(n)
    wpc = (n_ck + chunks - 1) // chunks
    out = []
    for g_lo in range(0, n_ck, wpc):
        out.append(col_chunk(g_lo, wpc, n_ck, n, span))
        if out[-1][1] == n_ck:
            break
    return out


def plan_chunks(m, n, scores, n_pairs, col_chunks):
    """the column chunks [(g_lo, g_hi, col0)] of an m x n pair (fast symbols) in a launch of n_pairs pairs under option
    col_chunks; [] where the pair is swept whole.  Planner::take_cols for a read of one strip, Planner::take_strips (a chunk
    body may be as short as a quarter of the halo; the automatic budget is shared by the strips) for a longer one"""
    if not _chunks_possible(scores, n_pairs, col_chunks):
        return []
    span = path_span(m, scores)
    budget = col_chunks if col_chunks > 1 else max(1, 1024 // max(n_pairs, 1))
    if m <= 64 * RMAX:
        if budget <= 1:
            return []
        chunks = min(budget, n // max(span + 64, 256), ck_windows(n))
    else:
        strips = (m + 64 * RMAX - 1) // (64 * RMAX)
        if col_chunks <= 1:
            budget //= strips
        chunks = min(budget, n // max((span + 64) // 4, 256), ck_windows(n))
    return _chunk_list(chunks, n, span) if chunks >= 2 else []


def end_lane(m):
    """lane that owns the read's last row, in the strip that holds it"""
    R = rows_per_lane(m)
    return (m - 1) % (64 * R) // R


def end_step(m, col):
    """0-based anti-diagonal step at which the cell (last read row, 1-based column col) is computed: lane l works on column
    t - l + 1 at step t"""
    return col + end_lane(m) - 1


def owner(chunks, m, col):
    """index of the chunk that owns the window of the cell (last read row, col)"""
    g = end_step(m, col) // STEP_W
    return next(x for x, (g_lo, g_hi, _) in enumerate(chunks) if g_lo <= g < g_hi)


# LDS dwords of a resident pair's wavefront (Planner::res_need_words; sw_resident_pairs_kernel) and the pairs option
# "resident" = 1 accepts (Planner::res_size_fits)
def res_need_words(m, n, scores):
    R = rows_per_lane(m)
    lact = (m + R - 1) // R
    nblk = (n + lact - 1 + 15) // 16
    n_ck = (nblk + 1) // 2
    opw = (path_bound(n, m, scores) + 15) // 16 + 1
    return nblk * R * 64 + ((n_ck + 1) & ~1) + 2 * 128 + 64 * opw + (n + 3) // 4 + 1 + (m + 3) // 4 + 1 + 8 + 128


def res_size_fits(m, n, scores):
    return m <= 64 * RMAX and res_need_words(m, n, scores) * 4 <= 40 * 1024


# ---- the plain sweep -----------------------------------------------------------------------------------------------------------
def cut_sweep_max(ref, read, scores, col0):
    """maximum H of a linear-gap local sweep that starts from zero at column col0 + 1: what a chunk wavefront with that col0
    can see of the pair"""
    match, mismatch, gap = scores
    rb = np.frombuffer(ref[col0:].encode("latin-1"), dtype=np.uint8)
    n = len(rb)
    if n == 0:
        return 0
    ramp = gap * np.arange(n + 1, dtype=np.int64)
    prev = np.zeros(n + 1, dtype=np.int64)
    best = 0
    for c in read.encode("latin-1"):
        tmp = np.zeros(n + 1, dtype=np.int64)
        np.maximum(prev[:-1] + np.where(rb == c, match, mismatch), prev[1:] + gap, out=tmp[1:])
        np.maximum(tmp, 0, out=tmp)
        # H[j] = max over j' <= j of tmp[j'] + gap * (j - j')
        prev = np.maximum.accumulate(tmp - ramp) + ramp
        best = max(best, int(prev.max()))
    return best


def path_columns(alignment):
    """(first column, columns spanned, moves) of an oracle alignment (begin, (refAligned, readAligned)); begin is the 1-based
    column of the path's first cell"""
    begin, (ra, _) = alignment
    return begin, sum(1 for c in ra if c != "_"), len(ra)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# The ratchet of a score set: (k for reads of one or two rows per lane, k for longer reads, tight).  A short read loses a
# larger share of its span to the first segment, which no run precedes, and takes a k that wastes less.  At the default scores
# the mismatch is cheaper than the gap, and a ratchet whose score keeps coming back to 1 .. 4 loses to paths that begin further
# right with a few chance matches (seen with k = 5): longer segments and a floor of 6 keep it the optimum.  (4, -6, -5) is the
# set with |gap| > match > 1.  tests/test_gap_paths_cpu.py proves every choice.
HALO_SCORES = ((5, -3, -4), (7, -8, -1), (4, -6, -5))
RATCHET = {(5, -3, -4): (9, 9, 6), (7, -8, -1): (3, 8, 1), (4, -6, -5): (4, 4, 1)}


def ratchet_params(m, scores):
    k_short, k_long, tight = RATCHET[scores]
    return (k_short if m <= 128 else k_long), tight


HALO_SINGLE_M = (99, 255, 256)                # rows per lane 2, 4, 4
HALO_MULTI_M = (300, 520)                     # two and three strips
FORCED_CHUNKS = 7

HaloCase = namedtuple("HaloCase", "m scores k n read body_cols gaps chunks places refs")
Place = namedtuple("Place", "label end_col chunk")     # chunk: index of the chunk that owns the end cell


def _first_behind_a_halo(chunks):
    return next(x for x, c in enumerate(chunks) if c[2] > 0)


def _enough_chunks(chunks):
    return sum(1 for c in chunks if c[2] > 0) >= 3


@functools.lru_cache(maxsize=None)
def halo_case(m, scores):
    """One read of m bases and five references of one length n: the smallest n that the plan cuts into at least three chunks
    behind a halo (col0 > 0) at col_chunks = 7, the ratchet's end cell
      a   at the first anti-diagonal step of the first window of the first such chunk,
      b   at that window's last step,
      ca, cb   the same in the pair's last chunk (the one that runs to the reference's end),
      d   past the first window of the chunk after a's, the body begun as far back as the first window of a's chunk where it
          is long enough: the walk crosses a chunk edge (several where a chunk body is shorter than the halo)."""
    k, tight = ratchet_params(m, scores)
    rng = random.Random(20261019 + 1000 * m + 7 * scores[0] - scores[2])
    body, read, gaps = ratchet(rng, m, scores, k, "del", tight=tight)
    cols, lane = len(body), end_lane(m)
    n = cols
    while True:
        chunks = plan_chunks(m, n, scores, 4, FORCED_CHUNKS)
        if _enough_chunks(chunks):
            first, last = _first_behind_a_halo(chunks), len(chunks) - 1
            a = chunks[first][0] * STEP_W - lane + 1
            ca = chunks[last][0] * STEP_W - lane + 1
            d = max(chunks[first][0] * STEP_W + cols, chunks[first + 1][0] * STEP_W + STEP_W + 16 - lane + 1)
            d = min(d, n)
            if a >= cols and ca + STEP_W - 1 <= n and owner(chunks, m, d) > first:
                break
        n += 1
    places = [Place("a", a, first), Place("b", a + STEP_W - 1, first), Place("ca", ca, last), Place("cb", ca + STEP_W - 1, last),
              Place("d", d, owner(chunks, m, d))]
    for p in places:
        assert owner(chunks, m, p.end_col) == p.chunk
    refs = tuple(planted(body, n, p.end_col) for p in places)
    return HaloCase(m, scores, k, n, read, cols, gaps, tuple(chunks), tuple(places), refs)


HALO_SINGLE = [(m, sc) for m in HALO_SINGLE_M for sc in HALO_SCORES]
HALO_MULTI = [(m, sc) for m in HALO_MULTI_M for sc in HALO_SCORES]
HALO_BATCHES = ((0, 4), (4, 5))               # the references of a case go in launches of at most 4 pairs


def halo_id(case):
    m, sc = case
    return "m%d-%d_%d_%d" % ((m,) + tuple(sc))


# Path-bound cases: name -> (scores, refs, reads, (r, q) of the near-bound pair).  Every batch but "shapes-2x2" is one pair.
BoundCase = namedtuple("BoundCase", "name scores refs reads near")
INS_SEAM_FRONT = 12        # rows 256 and 257 of "ins-40x330-seam" (the seam of its two strips) are rows of one insertion run


def _pad_read(gapped, m, front):
    """an insertion ratchet's read padded with T (the reference has none) to m bases, `front` of them in front"""
    assert len(gapped) + front <= m
    return FILLER * front + gapped + FILLER * (m - len(gapped) - front)


@functools.lru_cache(maxsize=None)
def bound_cases():
    rng = random.Random(20261020)
    S7, S5 = (7, -8, -1), (5, -3, -4)
    out = []
    # the transposed kernel's limits: m <= 256, n <= 2560, int4 scores
    body, read, _ = ratchet(rng, 256, S7, 8, "del")
    out.append(BoundCase("del-256x2000", S7, (planted(body, 2000, 1990),), (read,), (0, 0)))
    # the default scores, R = 4 with a partial last lane
    body, read, _ = ratchet(rng, 255, S5, 5, "del")
    out.append(BoundCase("del-255x600-default", S5, (planted(body, 600, 590),), (read,), (0, 0)))
    # pairs small enough for one wavefront's share of LDS (option "resident" = 1): a small one, and one that fills the share
    body, read, _ = ratchet(rng, 24, S7, 1, "del", tight=1)
    out.append(BoundCase("del-24x200-resident", S7, (planted(body, 200, 195),), (read,), (0, 0)))
    body, read, _ = ratchet(rng, 90, S7, 1, "del", tight=1)
    out.append(BoundCase("del-90x740-resident", S7, (planted(body, 740, 735),), (read,), (0, 0)))
    # insertion ratchets: the reference is the body alone
    ref, gapped, _ = ratchet(rng, 32, S7, 1, "ins", tight=1)
    out.append(BoundCase("ins-32x256", S7, (ref,), (_pad_read(gapped, 256, 4),), (0, 0)))
    ref, gapped, _ = ratchet(rng, 40, S7, 1, "ins", tight=1)
    out.append(BoundCase("ins-40x330-seam", S7, (ref,), (_pad_read(gapped, 330, INS_SEAM_FRONT),), (0, 0)))
    # Two reference lengths x two read lengths in one launch, the near-bound pair last in upload order.  Plain mixed-shape
    # coverage: the run schedules its pairs longest first (schedule() below), so the planner meets the near-bound pair FIRST and
    # its memo of the last pair's bound is not under test here -- memo_case() is the batch for that.
    body, read, _ = ratchet(rng, 128, S7, 8, "del", tight=1)
    short_ref = "".join(rng.choice("ACG") for _ in range(40))
    out.append(BoundCase("shapes-2x2", S7, (short_ref, planted(body, 1040, 1030)), (short_ref[5:29], read), (1, 1)))
    return tuple(out)


def bound_case(name):
    return next(c for c in bound_cases() if c.name == name)


BOUND_NAMES = ("del-256x2000", "del-255x600-default", "del-24x200-resident", "del-90x740-resident", "ins-32x256",
               "ins-40x330-seam", "shapes-2x2")
RESIDENT_NAMES = ("del-24x200-resident", "del-90x740-resident")


# ---- the order in which the planner meets the pairs (swmi_run.cpp: build_schedule, next_launch), restated ------------------------
# plan_chunk keeps the bound of the last pair's lengths (pb_m, pb_n, pb_val: "runs of equal lengths") and max_path is the maximum
# over a launch.  The schedule is longest first -- references by descending length (stable), under each the reads by descending
# length -- and path_bound never decreases as either length grows, so within a launch a larger bound can follow a smaller one
# only where the launch begins in the middle of one reference's reads and goes on into a reference of the same length.  A
# launch ends where the next pair's workspace would pass option max_workspace_bytes (at least 1 MiB).
def dir_words(m, n, mode):
    """dwords of workspace a pair is charged (swmi_device.h: swmi_dir_words; no transposed pairs: n > 2560)"""
    R = rows_per_lane(m)
    strips = (m + 64 * R - 1) // (64 * R)
    wblocks = (n + 63 + 15) // 16
    if mode == 0:
        return strips * wblocks * R * 64
    n_ck = (wblocks + 1) // 2
    return strips * (n_ck * (R + 2) * 64 + (((n_ck + 63) & ~63) if mode == 1 else 0))


def schedule(ref_lens, read_lens):
    """[(r, q)] in the planner's order, for references that are not all of one length and no empty sequence"""
    assert len(set(ref_lens)) > 1 and min(ref_lens) > 0 and min(read_lens) > 0
    ro = sorted(range(len(ref_lens)), key=lambda r: -ref_lens[r])            # (sorted is stable)
    qo = sorted(range(len(read_lens)), key=lambda q: -read_lens[q])
    return [(r, q) for r in ro for q in qo]


def launches(ref_lens, read_lens, mode, cap_bytes):
    """the schedule cut into launches"""
    out, words = [], 0
    for r, q in schedule(ref_lens, read_lens):
        dw = dir_words(read_lens[q], ref_lens[r], mode)
        if out and (words + dw) * 4 <= cap_bytes:
            out[-1].append((r, q))
            words += dw
        else:
            out.append([(r, q)])
            words = dw
    return out


def planned_max_path(launch, ref_lens, read_lens, scores, key="mn"):
    """max_path of a launch as plan_chunk derives it, with the memo refreshed when the lengths named in `key` change ("mn": the
    library's; "n", "m", "": broken memos, the last one never refreshed after the first pair)"""
    last, val, best = None, 0, 0
    for x, (r, q) in enumerate(launch):
        m, n = read_lens[q], ref_lens[r]
        now = tuple(v for c, v in (("m", m), ("n", n)) if c in key)
        if x == 0 or now != last:
            last, val = now, path_bound(n, m, scores)
        best = max(best, val)
    return best


MemoCase = namedtuple("MemoCase", "scores refs reads near")
MEMO_N = 24000              # long enough for two pairs' workspace to pass 1 MiB in every mode


@functools.lru_cache(maxsize=None)
def memo_case():
    """Two references of MEMO_N bases and a short one x reads of 128, 64 and 24 bases; the 128-base read and the SECOND long
    reference are a ratchet.  Under memo_cap(mode) the second launch is [(first long reference, 24-base read), (the ratchet
    pair)]: a small bound, then the near-bound pair of the same reference length."""
    rng = random.Random(20261022)
    scores = (7, -8, -1)
    body, read, _ = ratchet(rng, 128, scores, 8, "del", tight=1)
    mid = "".join(rng.choice("ACG") for _ in range(64))
    small = "".join(rng.choice("ACG") for _ in range(24))
    other = planted(mid + FILLER * 40 + small + FILLER * 9 + read[:100], MEMO_N, 9000)
    short_ref = "".join(rng.choice("ACG") for _ in range(40))
    return MemoCase(scores, (other, planted(body, MEMO_N, MEMO_N - 500), short_ref), (read, mid, small), (1, 0))


def memo_cap(mode):
    """max_workspace_bytes that ends the first launch after the two longest reads of the first reference"""
    return 4 * (dir_words(128, MEMO_N, mode) + dir_words(64, MEMO_N, mode))


# the affine kernels' ops_words: gap_open -1 on top of (7, -8, -1), runs of d = 7k - 2
AFFINE_SCORES = (7, -8, -1, -1)
AFFINE_K = 8


@functools.lru_cache(maxsize=None)
def affine_case():
    rng = random.Random(20261021)
    body, read, gaps = ratchet(rng, 256, AFFINE_SCORES[:3], AFFINE_K, "del", gap_open=AFFINE_SCORES[3])
    assert gaps == (256 // AFFINE_K - 1) * (7 * AFFINE_K - 2)
    return planted(body, 2000, 1990), read, 256 + gaps
