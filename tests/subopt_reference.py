"""The second-best local score of option "subopt" (include/swmi.h), restated -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  With H the local matrix of tests/gotoh_reference.py (band and strip included: a cell
outside its strip's window does not exist and reads 0 there), s the pair's score and w the mask half-width:

  colmax(j) = max of H(i, j) over 1 <= i <= m        (0 for a column without an existing cell: H >= 0 in local mode)
  j* is a maximum column   iff colmax(j*) == s
  j is eligible            iff |j - j*| > w for every maximum column        (strict, as in SSW)
  score2 = the largest colmax over the eligible columns, 0 if there are none
  end2   = the smallest eligible column with colmax == score2 if score2 > 0, else 0

w = AUTO (-1) is max(m // 2, 15), SSW's maskLen.  A degenerate pair (s == 0) and a pair with an empty side give (0, 0).

subopt_scalar takes H from align_scalar(..., matrices=True) and applies the rule with plain loops: the specification.
subopt_numpy sweeps H alone, whole anti-diagonals in int64, for the shapes above 1,024 rows; tests/test_subopt_cpu.py holds it to
the scalar form.  Both return (score, score2, end2).
"""
import numpy as np

import gotoh_reference as gr

AUTO = -1


def mask_width(w, m):
    return max(m // 2, 15) if w == AUTO else w


def reduce_colmax(colmax, s, w):
    """(score2, end2) from colmax[1..n] (index 0 unused), the pair's score s > 0 and the half-width w >= 1: the rule, in plain loops"""
    n = len(colmax) - 1
    tops = [j for j in range(1, n + 1) if colmax[j] == s]
    score2, end2 = 0, 0
    for j in range(1, n + 1):
        if all(abs(j - t) > w for t in tops) and colmax[j] > score2:
            score2, end2 = int(colmax[j]), j
    return score2, end2


def subopt_scalar(ref, read, scores, w, band=0, tie_mode=0, matrix=None, strip=1024):
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, 0, 0
    res = gr.align_scalar(ref, read, scores, gr.LOCAL, band, False, tie_mode, matrix, strip, matrices=True)
    s, H = res[0], res[2]
    if s == 0:
        return 0, 0, 0
    colmax = [0] + [max(H[i][j] for i in range(1, m + 1)) for j in range(1, n + 1)]
    assert max(colmax) == s
    return (s,) + reduce_colmax(colmax, s, mask_width(w, m))


def local_h(ref, read, scores, band=0, matrix=None, strip=1024):
    """H of the local recurrence alone, (m + 1) x (n + 1) int64, whole anti-diagonals at a time (the sweep of gr.align_numpy without
    its directions; the tie mode does not change a value)"""
    ref, read = gr._s(ref), gr._s(read)
    e, o = int(scores[2]), int(scores[3])
    m, n = len(read), len(ref)
    win = gr.windows(m, n, band, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    T = gr.score_table(scores, matrix)
    rb = np.frombuffer(ref.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(read.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    rows = np.arange(1, m + 1, dtype=np.int64)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), gr.NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), gr.NEG, dtype=np.int64)
    diag = np.arange(m + n + 1)
    first = np.searchsorted(rows + hi_of, diag, "left") + 1
    last = np.searchsorted(rows + lo_of, diag, "right")
    for d in range(2, m + n + 1):
        i = np.arange(first[d], last[d] + 1)
        if i.size == 0:
            continue
        j = d - i
        ev = np.maximum(H[i, j - 1] + o + e, E[i, j - 1] + e)
        fv = np.maximum(H[i - 1, j] + o + e, F[i - 1, j] + e)
        a = H[i - 1, j - 1] + T[qb[i - 1], rb[j - 1]]
        E[i, j], F[i, j] = ev, fv
        H[i, j] = np.maximum(np.maximum(np.maximum(ev, fv), a), 0)
    return H


def subopt_numpy(ref, read, scores, w, band=0, matrix=None, strip=1024):
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, 0, 0
    colmax = local_h(ref, read, scores, band, matrix, strip)[1:].max(axis=0)     # (index 0: column 0, all 0)
    s = int(colmax.max())
    if s == 0:
        return 0, 0, 0
    w = mask_width(w, m)
    cols = np.arange(n + 1)
    tops = cols[colmax == s]
    tops = tops[tops >= 1]
    # the distance to the nearest maximum column, by its two neighbours in the sorted list
    k = np.searchsorted(tops, cols)
    left = np.where(k > 0, cols - tops[np.maximum(k - 1, 0)], n + w + 1)
    right = np.where(k < len(tops), tops[np.minimum(k, len(tops) - 1)] - cols, n + w + 1)
    ok = (left > w) & (right > w)
    ok[0] = False
    if not ok.any():
        return s, 0, 0
    vals = np.where(ok, colmax, 0)
    score2 = int(vals.max())
    if score2 == 0:
        return s, 0, 0
    return s, score2, int(np.argmax(vals == score2))
