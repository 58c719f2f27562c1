"""The drop-off rule of seed extension (option "xdrop"), restated on tests/gotoh_reference.py -- TEST
INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  An xdrop run is an extend run (gotoh_reference: mode GLOBAL, extend=True) whose strip
sweep may end at a seam.  For a read of m > strip bases, NS = ceil(m / strip) strips with the windows c_lo(s) .. c_hi(s) of
gotoh_reference.windows, and s = 0 .. NS - 2:

  best(s) = the maximum of H(i, j) over the existing cells with 1 <= i <= strip * (s + 1), j >= 1
  seam(s) = the maximum of H(strip * (s + 1), j) over c_lo(s) <= j <= c_hi(s)
  s*      = the smallest s with best(s) - seam(s) > X        (strict; Python ints, so the difference is exact)

Without an s* -- always so for m <= strip and for X = 0, which is "off" -- the result is the extend result and rows_swept = m.
With one, rows_swept = strip * (s* + 1), the score is best(s*), the maximum cells are the cells of rows <= rows_swept that tie
at it, in extend's order (the full order filtered by row), and each is walked as extend walks it.

Two forms with the same arguments and return values: drops_scalar / align_scalar are the specification (Python ints, over the
matrices gotoh_reference.align_scalar returns); drops / align take the matrices of gotoh_reference.align_numpy, for the
2,049-3,100 base shapes of the GPU tests, and tests/test_xdrop_cpu.py holds them to the scalar form.  align_numpy hands its
matrices to gotoh_reference._finish only, so the numpy form takes them from there.

  drops(ref, read, scores, w, matrix=None, strip=1024)                     -> [(best(s), seam(s)) for s = 0 .. NS - 2]
                                                                               (the numpy form also takes tie_mode: see there)
  align(ref, read, scores, X, w=0, tie_mode=0, matrix=None, strip=1024, cells=True)
                                                                            -> (score, alignments, cells, rows_swept)
                                                                               (cells=False: (score, alignments, rows_swept))
"""
from unittest import mock

import numpy as np

import gotoh_reference as gr


def first_stop(dr, X):
    """s* for the differences dr = [(best(s), seam(s))], or None"""
    if X > 0:
        for s, (best, seam) in enumerate(dr):
            if best - seam > X:
                return s
    return None


# ---- the scalar form: the specification -------------------------------------------------------------------------------------
def _matrices_scalar(ref, read, scores, w, tie_mode, matrix, strip):
    res = gr.align_scalar(ref, read, scores, gr.GLOBAL, w, True, tie_mode, matrix, strip, matrices=True, cells=True)
    return res[:3], res[3], res[6], res[7], res[8]                 # the extend result, H, D, XE, XF


def _drops_scalar(H, m, n, w, strip):
    win = gr.windows(m, n, w, strip)
    out, best = [], None
    for s in range(len(win) - 1):
        lo, hi = win[s]
        for i in range(strip * s + 1, strip * (s + 1) + 1):
            for j in range(lo, hi + 1):
                best = H[i][j] if best is None else max(best, H[i][j])
        out.append((best, max(H[strip * (s + 1)][j] for j in range(lo, hi + 1))))
    return out


def drops_scalar(ref, read, scores, w, matrix=None, strip=1024):
    ref, read = gr._s(ref), gr._s(read)
    if not ref or len(read) <= strip:
        return []
    return _drops_scalar(_matrices_scalar(ref, read, scores, w, 0, matrix, strip)[1], len(read), len(ref), w, strip)


def align_scalar(ref, read, scores, X, w=0, tie_mode=0, matrix=None, strip=1024, cells=True):
    ref, read = gr._s(ref), gr._s(read)
    m, n = len(read), len(ref)
    full, H, D, XE, XF = _matrices_scalar(ref, read, scores, w, tie_mode, matrix, strip)
    s = first_stop(_drops_scalar(H, m, n, w, strip), X) if n and m > strip else None
    if s is None:
        res, rows = full, m
    else:
        win = gr.windows(m, n, w, strip)
        rows = strip * (s + 1)
        inside = [(i, j) for i, j in gr.order(m, n, tie_mode == 1)
                  if i <= rows and win[(i - 1) // strip][0] <= j <= win[(i - 1) // strip][1]]
        best = max(H[i][j] for i, j in inside)
        tied = [c for c in inside if H[c[0]][c[1]] == best]
        res = gr._finish(ref, read, gr.GLOBAL, tie_mode == 1, best, tied, 0, H, D, XE, XF, True)
    return res + (rows,) if cells else res[:2] + (rows,)


# ---- the numpy form ---------------------------------------------------------------------------------------------------------
_KEPT = {}          # the matrices of the last sweeps, by their arguments: a test runs several X on one pair, and a mixed launch
_KEPT_CELLS = 20 << 20      # takes its X from the differences of several pairs.  At most this many cells (about 14 bytes each)


def _matrices_numpy(ref, read, scores, w, tie_mode, matrix, strip):
    key = (ref, read, tuple(scores), w, tie_mode, repr(matrix), strip)
    if key in _KEPT:
        return _KEPT[key]
    got = {}
    finish = gr._finish

    def keep(ref_, read_, mode, strict, score, best_cells, n_deg, H, D, XE, XF, want_cells):
        got.update(H=H, D=D, XE=XE, XF=XF)
        return finish(ref_, read_, mode, strict, score, best_cells, n_deg, H, D, XE, XF, want_cells)
    with mock.patch.object(gr, "_finish", keep):
        full = gr.align_numpy(ref, read, scores, gr.GLOBAL, w, True, tie_mode, matrix, strip, cells=True)
    cells = lambda k: (len(k[0]) + 1) * (len(k[1]) + 1)
    while _KEPT and sum(cells(k) for k in _KEPT) + cells(key) > _KEPT_CELLS:
        del _KEPT[next(iter(_KEPT))]                               # (the oldest)
    _KEPT[key] = (full, got.get("H"), got.get("D"), got.get("XE"), got.get("XF"))
    return _KEPT[key]


def _in_band(m, n, w, strip):
    """bool (m + 1, n + 1): the existing cells with i, j >= 1"""
    win = gr.windows(m, n, w, strip)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    cols = np.arange(n + 1)[None, :]
    inb = np.zeros((m + 1, n + 1), dtype=bool)
    inb[1:] = (cols >= lo_of[:, None]) & (cols <= hi_of[:, None])
    return inb


def _drops_numpy(H, m, n, w, strip):
    win = gr.windows(m, n, w, strip)
    out, best = [], None
    for s in range(len(win) - 1):
        lo, hi = win[s]
        here = int(H[strip * s + 1:strip * (s + 1) + 1, lo:hi + 1].max())
        best = here if best is None else max(best, here)
        out.append((best, int(H[strip * (s + 1), lo:hi + 1].max())))
    return out


def drops(ref, read, scores, w, matrix=None, strip=1024, tie_mode=0):
    """tie_mode changes no H: it only names the sweep whose matrices are kept for the align() that follows"""
    ref, read = gr._s(ref), gr._s(read)
    if not ref or len(read) <= strip:
        return []
    return _drops_numpy(_matrices_numpy(ref, read, scores, w, tie_mode, matrix, strip)[1], len(read), len(ref), w, strip)


def align(ref, read, scores, X, w=0, tie_mode=0, matrix=None, strip=1024, cells=True):
    ref, read = gr._s(ref), gr._s(read)
    m, n = len(read), len(ref)
    full, H, D, XE, XF = _matrices_numpy(ref, read, scores, w, tie_mode, matrix, strip)
    s = first_stop(_drops_numpy(H, m, n, w, strip), X) if n and m > strip else None
    if s is None:
        res, rows = full, m
    else:
        rows = strip * (s + 1)
        inb = _in_band(m, n, w, strip)
        inb[rows + 1:] = False
        best = int(H[inb].max())
        tied = [tuple(int(x) for x in c) for c in np.argwhere(inb & (H == best))]          # row-major
        if tie_mode == 1:
            tied.sort(key=lambda c: (c[0] + c[1], c[1]))
        res = gr._finish(ref, read, gr.GLOBAL, tie_mode == 1, best, tied, 0, H, D, XE, XF, True)
    return res + (rows,) if cells else res[:2] + (rows,)
