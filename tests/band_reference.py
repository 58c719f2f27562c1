"""Two restatements of the banded alignment contract (option "band") -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  The band is a staircase with the sweep's strip height: row i (1-based) is in strip
s = (i - 1) // strip, and cell (i, j) exists iff c_lo(s) <= j <= c_hi(s) with

    c_lo(s) = max(1, strip * s + 1 - w)        c_hi(s) = min(n, strip * (s + 1) + w)

Row 0 and column 0 are the mode's where c_lo(s) = 1.  A cell outside the band reads as H = 0, E = F = -inf in local mode and as
H = E = F = -inf in fit and global mode; inside, the recurrence, the tie chains, the x bits, the order of the tied maxima and the
walk are those of affine_reference / ends_reference (imported, not copied).  The band applies to reads of MORE than `strip`
bases; a shorter read, or w = 0, is handed to ends_reference unchanged.

scores = (match, mismatch, gap, gap_open), mode 0 local / 1 fit / 2 global, matrix = None or (alphabet, rows).
Both return (score, [(beginning, (refAligned, readAligned)), ...]); local mode with maximum 0 returns one (0, ("", "")) per
IN-BAND cell.  align_scalar works in Python ints with a true -inf (a float); align_numpy sweeps anti-diagonals in int64 with
-2^60, for the shapes of the GPU tests.  `strip` is a parameter so that the CPU tests run a whole staircase at strip = 8.
"""
import numpy as np

import affine_reference as _ar
import ends_reference as _er

NINF = float("-inf")
NEG = _er.NEG
GAP_CHAR = _ar.GAP_CHAR
LOCAL, FIT, GLOBAL = 0, 1, 2
_s = _ar._s


def windows(m, n, w, strip=1024):
    """[(c_lo(s), c_hi(s))] for the strips of a read of m bases"""
    return [(max(1, strip * s + 1 - w), min(n, strip * (s + 1) + w)) for s in range((m + strip - 1) // strip)]


def in_band_cells(m, n, w, strip=1024):
    """the number of in-band cells with 1 <= i <= m"""
    return sum(max(0, hi - lo + 1) * (min(m, strip * (s + 1)) - strip * s) for s, (lo, hi) in enumerate(windows(m, n, w, strip)))


def refused(m, n, w, mode, strip=1024):
    """what check_run_params refuses for the geometry alone: an empty window, or (m, n) outside the band in global mode"""
    ns = (m + strip - 1) // strip
    return n < strip * (ns - 1) + 1 - w or (mode == GLOBAL and n > strip * ns + w)


def _banded(read, w, strip):
    return w > 0 and len(read) > strip


def _finish(ref, read, mode, strict, score, cells, H, D, XE, XF, n_band):
    """the walks of the contract over direction letters D[i][j] in '-aid'"""
    if mode == LOCAL:
        if score == 0:
            return 0, [(0, ("", ""))] * n_band
        opt = [_ar._walk(c, ref, read, H, D, XE, XF) for c in cells]
    else:
        opt = [_er._walk(c, ref, read, D, XE, XF, mode) for c in cells]
    if strict:
        opt.sort(key=lambda t: t[0])
    return int(score), opt


def align_scalar(ref, read, scores, mode, w, tie_mode=0, matrix=None, strip=1024):
    ref, read = _s(ref), _s(read)
    if not _banded(read, w, strip) or not ref:
        return _er.align_scalar(ref, read, scores, mode, tie_mode, matrix)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    win = windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    sfn = _er._score_fn(scores, matrix)
    out_h = 0 if mode == LOCAL else NINF
    H = [[out_h] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    # row 0 and column 0 of the mode, where they are in the band
    H[0][0] = 0
    for j in range(1, win[0][1] + 1):
        H[0][j] = 0 if mode != GLOBAL else o + j * e
        if mode == GLOBAL:
            E[0][j] = o + j * e
    for i in range(1, m + 1):
        if win[(i - 1) // strip][0] == 1:
            H[i][0] = 0 if mode == LOCAL else o + i * e
            if mode != LOCAL:
                F[i][0] = o + i * e
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    best, cells = (0 if mode == LOCAL else None), []
    band = lambda i, j: win[(i - 1) // strip][0] <= j <= win[(i - 1) // strip][1]
    for i, j in _ar._order(m, n, strict):
        if not band(i, j):
            continue
        ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
        E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
        ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
        F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
        a = H[i - 1][j - 1] + sfn(ref[j - 1], read[i - 1])
        if mode == LOCAL:
            mx, t = 0, "-"
            if ge(E[i][j], mx):
                mx, t = E[i][j], "d"
        else:
            mx, t = E[i][j], "d"
        if ge(F[i][j], mx):
            mx, t = F[i][j], "i"
        if ge(a, mx):
            mx, t = a, "a"
        assert mx != NINF, (i, j)                   # every in-band cell has a real predecessor
        H[i][j], D[i][j] = mx, t
        if mode == LOCAL:
            if mx > best:
                best, cells = mx, [(i, j)]
            elif mx == best:
                cells.append((i, j))
    if mode == FIT:
        row = [(H[m][j], j) for j in range(win[-1][0], win[-1][1] + 1)]
        best = max(v for v, _ in row)
        cells = [(m, j) for v, j in row if v == best]
    elif mode == GLOBAL:
        assert band(m, n), "(m, n) outside the band"
        best, cells = H[m][n], [(m, n)]
    return _finish(ref, read, mode, strict, best, cells, H, D, XE, XF, in_band_cells(m, n, w, strip))


class _Letters:
    """D codes 0..3 of a numpy array read as the letters '-aid' by [i][j]"""

    def __init__(self, D):
        self._D = D

    def __getitem__(self, i):
        row = self._D[i]
        return _Row(row)


class _Row:
    def __init__(self, row):
        self._row = row

    def __getitem__(self, j):
        return "-aid"[int(self._row[j])]


def align_numpy(ref, read, scores, mode, w, tie_mode=0, matrix=None, strip=1024):
    ref, read = _s(ref), _s(read)
    if not _banded(read, w, strip) or not ref:
        return _er.align_numpy(ref, read, scores, mode, tie_mode, matrix)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    win = windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    S = _er._score_table(ref, read, scores, matrix)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]      # by row - 1
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    H = np.full((m + 1, n + 1), 0 if mode == LOCAL else NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int8)          # 0 '-', 1 'a', 2 'i', 3 'd'
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    H[0, 0] = 0
    j0 = np.arange(1, win[0][1] + 1, dtype=np.int64)
    H[0, j0] = 0 if mode != GLOBAL else o + e * j0
    if mode == GLOBAL:
        E[0, j0] = o + e * j0
    i0 = np.flatnonzero(lo_of == 1) + 1
    H[i0, 0] = 0 if mode == LOCAL else o + e * i0
    if mode != LOCAL:
        F[i0, 0] = o + e * i0
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        keep = (lo_of[i - 1] <= j) & (j <= hi_of[i - 1])
        i, j = i[keep], j[keep]
        if i.size == 0:
            continue
        ext, opn = E[i, j - 1] + e, H[i, j - 1] + o + e
        ev = np.maximum(opn, ext)
        XE[i, j] = ext > opn
        ext, opn = F[i - 1, j] + e, H[i - 1, j] + o + e
        fv = np.maximum(opn, ext)
        XF[i, j] = ext > opn
        a = H[i - 1, j - 1] + S[i - 1, j - 1]
        h = np.maximum(np.maximum(ev, fv), a)
        if mode == LOCAL:
            h = np.maximum(h, 0)
            if strict:
                dd = np.where(h == 0, 0, np.where(ev == h, 3, np.where(fv == h, 2, 1)))
            else:
                dd = np.where(a == h, 1, np.where(fv == h, 2, np.where(ev == h, 3, 0)))
        elif strict:
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
        else:
            dd = np.where(a == h, 1, np.where(fv == h, 2, 3))
        E[i, j], F[i, j], H[i, j], D[i, j] = ev, fv, h, dd
    if mode == LOCAL:
        inb = np.zeros((m + 1, n + 1), dtype=bool)
        cols = np.arange(n + 1)[None, :]
        inb[1:] = (cols >= lo_of[:, None]) & (cols <= hi_of[:, None])
        best = int(H[inb].max())
        cells = [tuple(int(x) for x in c) for c in np.argwhere(inb & (H == best))] if best > 0 else []
        if strict:
            cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    elif mode == FIT:
        lo, hi = win[-1]
        best = int(H[m, lo:hi + 1].max())
        cells = [(m, int(j)) for j in range(lo, hi + 1) if H[m, j] == best]
    else:
        assert win[-1][0] <= n <= win[-1][1], "(m, n) outside the band"
        best, cells = int(H[m, n]), [(m, n)]
    return _finish(ref, read, mode, strict, best, cells, H, _Letters(D), XE, XF, in_band_cells(m, n, w, strip))
