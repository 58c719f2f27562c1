"""The adaptive band of seed extension (option "band_adapt"), restated on tests/gotoh_reference.py -- TEST
INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  An adaptive run is a banded extend run (gotoh_reference: mode GLOBAL, extend=True,
w > 0) whose windows follow the alignment.  For a read of m > strip bases, NS = ceil(m / strip) strips, each with a centre,
starting from c(-1) = 0:

  c_lo(s) = max(1, c(s - 1) + 1 - w)      c_hi(s) = min(n, c(s - 1) + strip + w)        (strip 0: the static window)
  p(s)    = the smallest column j in c_lo(s) .. c_hi(s) at which H(strip * (s + 1), j) is largest,   s <= NS - 2
  c(s)    = max(c(s - 1), p(s))

Everything else is gotoh_reference's banded extend run with these windows: a cell outside its strip's window does not exist,
the score is the maximum over the existing cells, tied cells come in extend's order, the walk is the global walk.  A read of at
most `strip` bases, or w = 0, is the plain extend run with the windows (1, n).

With X > 0 the drop-off rule of tests/xdrop_reference.py runs on these windows, before a window is placed: with best(s) the
maximum over the existing cells of rows <= strip * (s + 1) and seam(s) the maximum of the seam row over window s, the first s
with best(s) - seam(s) > X ends the sweep -- no further window exists, rows_swept = strip * (s + 1), and the result is the
extend result of (ref, read[:rows_swept]) under the windows placed so far.

How it is computed.  gotoh_reference's sweeps take their windows from gotoh_reference.windows; here that function is replaced
by the list placed so far.  The window of strip s + 1 hangs on the seam row of strip s, so the pair is swept NS times: the
prefix read[:strip * (s + 1)] under windows 0 .. s gives p(s) -- and is the result when the drop-off rule stops there -- and the
last sweep, of the whole read, is the result.  The windows are monotone, which gotoh_reference's numpy form relies on.

Two forms with the same arguments and return values: align_scalar is the specification (Python ints, a true -inf) and align takes
the matrices of gotoh_reference.align_numpy; tests/test_adapt_cpu.py holds them to each other.

  align(ref, read, scores, w, X=0, tie_mode=0, matrix=None, strip=1024)
      -> (score, alignments, cells, windows)                  windows = [(c_lo(s), c_hi(s))] of the strips swept
      -> (score, alignments, cells, windows, rows_swept)      when X > 0
  trace(...)  the same arguments -> (result as above, [p(s)], [(best(s), seam(s))]) for the seams the sweep looked at
"""
from unittest import mock

import gotoh_reference as gr


def window(c, n, w, strip=1024):
    """(c_lo, c_hi) of a strip whose centre is c"""
    return max(1, c + 1 - w), min(n, c + strip + w)


def bound_ok(m, n, scores, strip=1024):
    """the arithmetic bound of an adaptive run: (2 NS + 1) |o| + (strip * NS + n) |e| <= 2^30, NS = ceil(m / strip)"""
    ns = (m + strip - 1) // strip
    return (2 * ns + 1) * abs(scores[3]) + (strip * ns + n) * abs(scores[2]) <= 1 << 30


def _sweep(numpy_form, ref, read, scores, wins, w, tie_mode, matrix, strip):
    """the banded extend run of (ref, read) under the window list `wins`: (score, alignments, cells), H"""
    fixed = lambda m_, n_, w_, strip_=1024: list(wins[:(m_ + strip_ - 1) // strip_])
    with mock.patch.object(gr, "windows", fixed):
        if not numpy_form:
            res = gr.align_scalar(ref, read, scores, gr.GLOBAL, w, True, tie_mode, matrix, strip, matrices=True, cells=True)
            return res[:3], res[3]
        got = {}
        finish = gr._finish

        def keep(ref_, read_, mode, strict, score, best_cells, n_deg, H, D, XE, XF, want_cells):
            got["H"] = H
            return finish(ref_, read_, mode, strict, score, best_cells, n_deg, H, D, XE, XF, want_cells)
        with mock.patch.object(gr, "_finish", keep):
            res = gr.align_numpy(ref, read, scores, gr.GLOBAL, w, True, tie_mode, matrix, strip, cells=True)
        return res, got["H"]


def _run(numpy_form, ref, read, scores, w, X, tie_mode, matrix, strip):
    ref, read = gr._s(ref), gr._s(read)
    m, n = len(read), len(ref)
    tail = lambda rows: (rows,) if X > 0 else ()
    if m == 0 or n == 0:
        return (0, [], [], []) + tail(m), [], []
    ns = (m + strip - 1) // strip
    if w <= 0 or m <= strip:
        res, _ = _sweep(numpy_form, ref, read, scores, [(1, n)] * ns, 0, tie_mode, matrix, strip)
        return res + ([(1, n)] * ns,) + tail(m), [], []
    c, wins, ps, drops = 0, [window(0, n, w, strip)], [], []
    for s in range(ns):
        rows = min(m, strip * (s + 1))
        res, H = _sweep(numpy_form, ref, read[:rows], scores, wins, w, tie_mode, matrix, strip)
        if s == ns - 1:
            return res + (wins,) + tail(m), ps, drops
        lo, hi = wins[s]
        seam_row = [int(H[rows][j]) for j in range(lo, hi + 1)]
        seam = max(seam_row)
        drops.append((res[0], seam))                       # (res[0]: the extend score of the prefix = best(s))
        if X > 0 and res[0] - seam > X:
            return res + (wins,) + tail(rows), ps, drops
        p = lo + seam_row.index(seam)                      # the smallest such column
        ps.append(p)
        c = max(c, p)
        wins.append(window(c, n, w, strip))


def trace_scalar(ref, read, scores, w, X=0, tie_mode=0, matrix=None, strip=1024):
    return _run(False, ref, read, scores, w, X, tie_mode, matrix, strip)


def trace(ref, read, scores, w, X=0, tie_mode=0, matrix=None, strip=1024):
    return _run(True, ref, read, scores, w, X, tie_mode, matrix, strip)


def align_scalar(ref, read, scores, w, X=0, tie_mode=0, matrix=None, strip=1024):
    return _run(False, ref, read, scores, w, X, tie_mode, matrix, strip)[0]


def align(ref, read, scores, w, X=0, tie_mode=0, matrix=None, strip=1024):
    return _run(True, ref, read, scores, w, X, tie_mode, matrix, strip)[0]
