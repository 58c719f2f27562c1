"""The affine-gap (Gotoh) contract of DESIGN.md sections 8b-8g, restated once -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Two entry points with the same arguments and the same return value:
align_scalar is the specification (Python ints, a true -inf, one loop over the cells); align_numpy sweeps whole anti-diagonals
in int64 with -2^60 for -inf, for the 1,025-3,100 base shapes of the GPU tests, and the CPU tests hold it to the scalar form.

Arguments.  scores = (match, mismatch, gap, gap_open): gap is the per-base extension e, gap_open the extra cost o of opening a
gap, both <= 0.  matrix = None or (alphabet, rows), rows[a][b] the score of READ symbol alphabet[a] against REFERENCE symbol
alphabet[b]; s(i,j) is the matrix entry when both bases, upper-cased as Character.toUpperCase does on ISO-8859-1, are in the
alphabet, else match for equal bases and mismatch otherwise.  mode = LOCAL, FIT (the whole read against any stretch of the
reference) or GLOBAL (the whole read against the whole reference); extend=True is a GLOBAL run that ends where the score is
best.  w is the band's half-width and strip the sweep's strip height (a parameter so that CPU tests run staircases at strip 8).

Recurrence, for i = 1..m over the read and j = 1..n over the reference:
  E(i,j) = max(H(i,j-1) + o + e, E(i,j-1) + e)    xE = 1 iff E(i,j-1) + e > H(i,j-1) + o + e
  F(i,j) = max(H(i-1,j) + o + e, F(i-1,j) + e)    xF = 1 iff F(i-1,j) + e > H(i-1,j) + o + e
  H(i,j) = E 'd', then F 'i', then H(i-1,j-1) + s 'a', each replacing on '>=' (serial tie mode) or '>' (strict);
           local mode floors at 0: the chain starts from 0 '-'

Band.  Row i is in strip (i - 1) // strip, and cell (i, j) exists iff c_lo(s) <= j <= c_hi(s).  When w > 0 and m > strip,
c_lo(s) = max(1, strip * s + 1 - w) and c_hi(s) = min(n, strip * (s + 1) + w); otherwise every window is (1, n).  A strip
with an empty window is an assertion.  A cell outside the band reads as H = 0, E = F = -inf in local mode and as
H = E = F = -inf in the other modes.

Boundaries, set only where they lie in the band (row 0 up to c_hi(0); column 0 in the strips with c_lo = 1):
  local:  H = 0, E = F = -inf
  fit:    H(0,j) = 0; H(i,0) = F(i,0) = o + i*e
  global: H(0,0) = 0; H(0,j) = E(0,j) = o + j*e; H(i,0) = F(i,0) = o + i*e          (extend: the same)

Maximum.  local: over the in-band cells from 0 up; a maximum of 0 yields one (0, ("", "")) per in-band cell.  fit: row m over
the last strip's window, ascending j.  global: the one cell (m, n), asserted in band.  extend: over the in-band cells with no
floor, so the score may be <= 0.  Tied cells of local and extend come row-major (serial, SmithWaterman.java:157-185) or per
anti-diagonal with ascending j (strict, DistributedSW.java:209-239); in strict mode the alignments are then stably sorted by
`beginning` (:480).

Walk.  State H picks M/F/E from the direction; M moves diagonally; F and E stay in their gap while the x bit is set.  Local
stops at H = 0 (also how a banded walk ends when it leaves a window).  The others run to row 0, inserting the read's head
once at column 0; global and extend then delete the rest of the reference.  `beginning` is the column of the last reference
base taken.

Return.  (score, [(beginning, (refAligned, readAligned)), ...]) as OptAlignments.call returns; with cells=True then the
maximum cells [(i, j), ...] in the order of the alignments; with matrices=True (scalar only) then H, E, F, D, XE, XF as
lists of rows, -inf as NINF, D in '-aid'.  A pair with an empty side scores 0 with no alignments (and no cells) in every mode.
"""
import functools

import numpy as np

NINF = float("-inf")
NEG = -(1 << 60)          # the numpy form's -inf: far below anything a sum of the bounded scores can reach
GAP_CHAR = "_"
LOCAL, FIT, GLOBAL = 0, 1, 2


def _s(x):
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x


def upper(c):
    o = ord(c)
    if 0x61 <= o <= 0x7A or (0xE0 <= o <= 0xFE and o != 0xF7):
        return chr(o - 32)
    return c                                           # (0xFF's upper case is outside Latin-1: only itself)


def windows(m, n, w, strip=1024):
    """[(c_lo(s), c_hi(s))] for the strips of a read of m bases: the band's where it applies, else the whole reference"""
    ns = (m + strip - 1) // strip
    if w > 0 and m > strip:
        return [(max(1, strip * s + 1 - w), min(n, strip * (s + 1) + w)) for s in range(ns)]
    return [(1, n)] * ns


def in_band_cells(m, n, w, strip=1024):
    """the number of in-band cells with 1 <= i <= m"""
    return sum(max(0, hi - lo + 1) * (min(m, strip * (s + 1)) - strip * s) for s, (lo, hi) in enumerate(windows(m, n, w, strip)))


def refused(m, n, w, mode, extend=False, strip=1024):
    """what check_run_params refuses for the geometry alone: an empty window, or (m, n) outside the band in global mode"""
    win = windows(m, n, w, strip)
    return any(lo > hi for lo, hi in win) or (mode == GLOBAL and not extend and bool(win) and n > win[-1][1])


def order(m, n, strict):
    """the cells in the order the tied maxima are reported: row-major, or per anti-diagonal with ascending j"""
    if not strict:
        return [(i, j) for i in range(1, m + 1) for j in range(1, n + 1)]
    return [(d - j, j) for d in range(2, m + n + 1) for j in range(max(1, d - m), min(n, d - 1) + 1)]


def score_fn(scores, matrix):
    """s of the contract as a function of one (reference, read) character pair"""
    match, mismatch = scores[0], scores[1]
    idx = {} if matrix is None else {upper(c): k for k, c in enumerate(_s(matrix[0]))}

    @functools.lru_cache(maxsize=None)
    def s(ref_char, read_char):
        r, q = upper(ref_char), upper(read_char)
        if r in idx and q in idx:
            return int(matrix[1][idx[q]][idx[r]])
        return match if r == q else mismatch
    return s


def cell_score(ref_char, read_char, scores, matrix):
    return score_fn(scores, matrix)(ref_char, read_char)


def score_table(scores, matrix):
    """256 x 256 int64: [read byte, reference byte] -> s."""
    up = np.array([ord(upper(chr(b))) for b in range(256)], dtype=np.int64)
    T = np.where(up[:, None] == up[None, :], scores[0], scores[1]).astype(np.int64)
    if matrix is not None:
        cls = np.full(256, -1, dtype=np.int64)
        for k, c in enumerate(_s(matrix[0])):
            cls[up == up[ord(c)]] = k
        M = np.asarray(matrix[1], dtype=np.int64)
        inside = (cls[:, None] >= 0) & (cls[None, :] >= 0)
        T = np.where(inside, M[np.maximum(cls, 0)[:, None], np.maximum(cls, 0)[None, :]], T)
    return T


def rescore(ref_al, read_al, scores, matrix=None):
    """the score of an alignment given as its two strings: a gap of length k costs gap_open + k * gap"""
    s = score_fn(scores, matrix)
    e, o = scores[2], scores[3]
    total, prev = 0, None
    for r, q in zip(ref_al, read_al):
        if r == GAP_CHAR or q == GAP_CHAR:           # (test sequences never hold '_' themselves)
            kind = "i" if r == GAP_CHAR else "d"
            total += e + (o if kind != prev else 0)
            prev = kind
        else:
            total += s(r, q)
            prev = None
    return total


def _walk(cell, ref, read, H, D, XE, XF, mode):
    i, j = cell
    st, beginning, stack = "H", j, []
    while H[i][j] > 0 if mode == LOCAL else i > 0:
        if j == 0:                                     # (not local: H(i,0) = 0 there) the read's head, inserted
            stack.append((GAP_CHAR, read[i - 1]))
            i -= 1
            continue
        if st == "H":
            st = {"a": "M", "i": "F", "d": "E"}[D[i][j]]
        if st == "M":
            beginning = j
            stack.append((ref[j - 1], read[i - 1]))
            i, j, st = i - 1, j - 1, "H"
        elif st == "F":
            stack.append((GAP_CHAR, read[i - 1]))
            st = "F" if XF[i][j] else "H"
            i -= 1
        else:
            beginning = j
            stack.append((ref[j - 1], GAP_CHAR))
            st = "E" if XE[i][j] else "H"
            j -= 1
    if mode == GLOBAL:
        while j > 0:
            beginning = j
            stack.append((ref[j - 1], GAP_CHAR))
            j -= 1
    stack.reverse()
    return beginning, ("".join(p[0] for p in stack), "".join(p[1] for p in stack))


def _finish(ref, read, mode, strict, score, cells, n_degenerate, H, D, XE, XF, want_cells):
    if mode == LOCAL and score == 0:                    # every in-band cell ties at 0 and yields (0, "", "")
        opt = [(0, ("", ""))] * n_degenerate
    else:
        both = [(_walk(c, ref, read, H, D, XE, XF, mode), c) for c in cells]
        if strict:
            both.sort(key=lambda t: t[0][0])
        opt, cells = [a for a, _ in both], [c for _, c in both]
    return (int(score), opt, cells) if want_cells else (int(score), opt)


def align_scalar(ref, read, scores, mode=LOCAL, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, matrices=False,
                 cells=False):
    assert mode == GLOBAL or not extend, "extend is an option of global mode"
    ref, read = _s(ref), _s(read)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    H = [[0 if mode == LOCAL else NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    res = (0, [], []) if cells else (0, [])
    if m and n:
        win = windows(m, n, w, strip)
        assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
        s = score_fn(scores, matrix)
        H[0][0] = 0
        for j in range(1, win[0][1] + 1):               # row 0 and column 0 of the mode, where they are in the band
            if mode == GLOBAL:
                H[0][j] = E[0][j] = o + j * e
            else:
                H[0][j] = 0
        for i in range(1, m + 1):
            if win[(i - 1) // strip][0] == 1:
                if mode == LOCAL:
                    H[i][0] = 0
                else:
                    H[i][0] = F[i][0] = o + i * e
        ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
        best, best_cells = (0 if mode == LOCAL else None), []
        for i, j in order(m, n, strict):
            lo, hi = win[(i - 1) // strip]
            if not lo <= j <= hi:
                continue
            ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
            E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
            ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
            F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
            a = H[i - 1][j - 1] + s(ref[j - 1], read[i - 1])
            mx, t = E[i][j], "d"
            if mode == LOCAL:
                mx, t = (E[i][j], "d") if ge(E[i][j], 0) else (0, "-")
            if ge(F[i][j], mx):
                mx, t = F[i][j], "i"
            if ge(a, mx):
                mx, t = a, "a"
            assert mx != NINF, (i, j)                   # every in-band cell has a real predecessor
            H[i][j], D[i][j] = mx, t
            if mode == LOCAL or extend:
                if best is None or mx > best:
                    best, best_cells = mx, [(i, j)]
                elif mx == best:
                    best_cells.append((i, j))
        if mode == FIT:
            lo, hi = win[-1]
            best = max(H[m][lo:hi + 1])
            best_cells = [(m, j) for j in range(lo, hi + 1) if H[m][j] == best]
        elif mode == GLOBAL and not extend:
            assert win[-1][0] <= n <= win[-1][1], "(m, n) outside the band"
            best, best_cells = H[m][n], [(m, n)]
        res = _finish(ref, read, mode, strict, best, best_cells, len(best_cells), H, D, XE, XF, cells)
    if matrices:
        return res + (H, E, F, D, XE, XF)
    return res


def align_numpy(ref, read, scores, mode=LOCAL, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, cells=False):
    assert mode == GLOBAL or not extend, "extend is an option of global mode"
    ref, read = _s(ref), _s(read)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    win = windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    T = score_table(scores, matrix)
    rb = np.frombuffer(ref.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(read.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    rows = np.arange(1, m + 1, dtype=np.int64)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]      # by row - 1
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    H = np.full((m + 1, n + 1), 0 if mode == LOCAL else NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.full((m + 1, n + 1), "-", dtype="U1")
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    H[0, 0] = 0
    j0 = np.arange(1, win[0][1] + 1, dtype=np.int64)
    i0 = rows[lo_of == 1]
    if mode == GLOBAL:
        H[0, j0] = E[0, j0] = o + e * j0
    else:
        H[0, j0] = 0
    if mode == LOCAL:
        H[i0, 0] = 0
    else:
        H[i0, 0] = F[i0, 0] = o + e * i0
    # the band is a staircase, so the in-band rows of an anti-diagonal are one run: found once for every diagonal
    diag = np.arange(m + n + 1)
    first = np.searchsorted(rows + hi_of, diag, "left") + 1         # the first row with d - i <= c_hi
    last = np.searchsorted(rows + lo_of, diag, "right")             # the last row with c_lo <= d - i
    letters = np.array(list("-aid"))
    for d in range(2, m + n + 1):
        i = np.arange(first[d], last[d] + 1)
        if i.size == 0:
            continue
        j = d - i
        ext, opn = E[i, j - 1] + e, H[i, j - 1] + o + e
        ev = np.maximum(opn, ext)
        XE[i, j] = ext > opn
        ext, opn = F[i - 1, j] + e, H[i - 1, j] + o + e
        fv = np.maximum(opn, ext)
        XF[i, j] = ext > opn
        a = H[i - 1, j - 1] + T[qb[i - 1], rb[j - 1]]
        h = np.maximum(np.maximum(ev, fv), a)
        if mode == LOCAL:
            h = np.maximum(h, 0)
        if strict:      # '>' chain: the first candidate (above 0 in local mode) that reaches the maximum wins: d, then i, then a
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
            if mode == LOCAL:
                dd = np.where(h == 0, 0, dd)
        else:           # '>=' chain: the last candidate that reaches the maximum wins: a, then i, then d, then local's 0
            dd = np.where(a == h, 1, np.where(fv == h, 2, np.where(ev == h, 3, 0)))
        E[i, j], F[i, j], H[i, j], D[i, j] = ev, fv, h, letters[dd]
    n_band = in_band_cells(m, n, w, strip)
    if mode == LOCAL or extend:
        cols = np.arange(n + 1)[None, :]
        inb = np.zeros((m + 1, n + 1), dtype=bool)
        inb[1:] = (cols >= lo_of[:, None]) & (cols <= hi_of[:, None])
        best = int(H[inb].max())
        best_cells = []
        if cells or not (mode == LOCAL and best == 0):
            best_cells = [tuple(int(x) for x in c) for c in np.argwhere(inb & (H == best))]      # row-major
            if strict:
                best_cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    elif mode == FIT:
        lo, hi = win[-1]
        best = int(H[m, lo:hi + 1].max())
        best_cells = [(m, j) for j in range(lo, hi + 1) if H[m, j] == best]
    else:
        assert win[-1][0] <= n <= win[-1][1], "(m, n) outside the band"
        best, best_cells = int(H[m, n]), [(m, n)]
    return _finish(ref, read, mode, strict, best, best_cells, n_band, H, D, XE, XF, cells)
