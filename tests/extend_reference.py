"""Two restatements of the seed-extension contract (option "extend") -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  An extend run is a global run (ends_reference, mode 2) that ends where the score is
best: E, F, H, the x bits, the tie chains and the boundaries H(0,0) = 0, H(0,j) = o + j*e, H(i,0) = o + i*e are global mode's,
the score is the maximum of H(i,j) over 1 <= i <= m, 1 <= j <= n -- row 0 and column 0 do not compete, so it may be zero or
negative -- and every tied cell is a maximum cell, in local mode's order: row-major (serial tie mode) or per anti-diagonal with
ascending j (strict), then the stable sort of the alignments by `beginning`.  The walk is global mode's walk started at the
maximum cell (i, j): the alignment spells read[:i] and ref[:j] and `beginning` is 1.

Under a band of half-width w (reads of MORE than `strip` bases; band_reference's staircase) a cell outside the band reads as
H = E = F = -inf and the maximum is taken over the in-band cells.  The end cell is free, so the reference may run on past the
band; a strip with an empty window is refused as ever.

scores = (match, mismatch, gap, gap_open), matrix = None or (alphabet, rows).  Both return
(score, [(beginning, (refAligned, readAligned)), ...]); with cells=True a third entry, the maximum cells [(i, j), ...] in the
order of the alignments.  A pair with an empty side scores 0 with no alignments.  align_scalar works in Python ints with a true
-inf (a float); align_numpy sweeps anti-diagonals in int64 with -2^60, for the shapes of the GPU tests.  The walk, the score
function, the cell order and the windows are imported, not copied.
"""
import numpy as np

import affine_reference as _ar
import band_reference as _br
import ends_reference as _er

NINF = float("-inf")
NEG = _er.NEG
GAP_CHAR = _ar.GAP_CHAR
_s = _ar._s


def windows(m, n, w, strip=1024):
    """[(c_lo(s), c_hi(s))] for the strips of a read of m bases: the band's where it applies, else the whole reference"""
    if w > 0 and m > strip:
        return _br.windows(m, n, w, strip)
    return [(1, n)] * ((m + strip - 1) // strip)


def refused(m, n, w, strip=1024):
    """what check_run_params refuses for the geometry alone: a strip with an empty window"""
    return any(lo > hi for lo, hi in windows(m, n, w, strip))


def _finish(ref, read, strict, score, cells, D, XE, XF, want_cells):
    opt = [(_er._walk(c, ref, read, D, XE, XF, _er.GLOBAL), c) for c in cells]
    if strict:
        opt.sort(key=lambda t: t[0][0])                 # (stable; `beginning` is 1 throughout, so the order stays)
    alns = [a for a, _ in opt]
    return (int(score), alns, [c for _, c in opt]) if want_cells else (int(score), alns)


def align_scalar(ref, read, scores, w=0, tie_mode=0, matrix=None, strip=1024, cells=False):
    ref, read = _s(ref), _s(read)
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    win = windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    sfn = _er._score_fn(scores, matrix)
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    H[0][0] = 0
    for j in range(1, win[0][1] + 1):                   # row 0 and column 0 of global mode, where they are in the band
        H[0][j] = o + j * e
    for i in range(1, m + 1):
        if win[(i - 1) // strip][0] == 1:
            H[i][0] = o + i * e
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    best, best_cells = None, []
    for i, j in _ar._order(m, n, strict):
        lo, hi = win[(i - 1) // strip]
        if not lo <= j <= hi:
            continue
        ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
        E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
        ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
        F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
        a = H[i - 1][j - 1] + sfn(ref[j - 1], read[i - 1])
        mx, t = E[i][j], "d"
        if ge(F[i][j], mx):
            mx, t = F[i][j], "i"
        if ge(a, mx):
            mx, t = a, "a"
        assert mx != NINF, (i, j)                       # every in-band cell has a real predecessor
        H[i][j], D[i][j] = mx, t
        if best is None or mx > best:
            best, best_cells = mx, [(i, j)]
        elif mx == best:
            best_cells.append((i, j))
    return _finish(ref, read, strict, best, best_cells, D, XE, XF, cells)


def align_numpy(ref, read, scores, w=0, tie_mode=0, matrix=None, strip=1024, cells=False):
    ref, read = _s(ref), _s(read)
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    win = windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    S = _er._score_table(ref, read, scores, matrix)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]      # by row - 1
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    H = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int8)          # 1 'a', 2 'i', 3 'd'
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    H[0, 0] = 0
    j0 = np.arange(1, win[0][1] + 1, dtype=np.int64)
    H[0, j0] = o + e * j0
    i0 = np.flatnonzero(lo_of == 1) + 1
    H[i0, 0] = o + e * i0
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
        if strict:
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
        else:
            dd = np.where(a == h, 1, np.where(fv == h, 2, 3))
        E[i, j], F[i, j], H[i, j], D[i, j] = ev, fv, h, dd
    inb = np.zeros((m + 1, n + 1), dtype=bool)
    cols = np.arange(n + 1)[None, :]
    inb[1:] = (cols >= lo_of[:, None]) & (cols <= hi_of[:, None])
    best = int(H[inb].max())
    best_cells = [tuple(int(x) for x in c) for c in np.argwhere(inb & (H == best))]      # row-major
    if strict:
        best_cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    return _finish(ref, read, strict, best, best_cells, _br._Letters(D), XE, XF, cells)
