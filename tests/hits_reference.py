"""The K best local hits with their end cells of option "hits" (include/swmi.h), restated -- TEST
INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  In the terms of tests/subopt_reference.py -- H the local matrix with band and strips,
colmax(j) its column maxima over the existing cells, s the pair's score, w the mask half-width (AUTO: max(m // 2, 15)):

  row(j)   = the smallest row i, 1 <= i <= m, with H(i, j) == colmax(j)           (an absent cell reads 0: it never holds a maximum > 0)
  entry 0  = (s, row(j0), j0), j0 the smallest maximum column
  entry k  = (v, row(j), j), 1 <= k < K: column j is eligible iff |j - c| > w for every maximum column c and for c = the column of
             every entry 1 .. k - 1; v = the largest colmax over the eligible columns -- the list ends when that is 0 --, j the
             smallest eligible column that holds it

So entry 1 is (score2, end2) of option "subopt".  A degenerate pair (s == 0) and a pair with an empty side have no entries.

hits_scalar takes H from gotoh_reference.align_scalar(..., matrices=True) and applies the rule with plain loops: the specification.
hits_numpy takes H from subopt_reference.local_h, for the shapes above 1,024 rows; tests/test_hits_cpu.py holds it to the scalar
form.  Both return a list of (score, end_i, end_j).
"""
import numpy as np

import gotoh_reference as gr
import subopt_reference as sr

AUTO = sr.AUTO
K_MAX = 16


def pick(colmax, rows, s, w, k_max):
    """the list from colmax[1..n] and rows[1..n] (index 0 unused), the pair's score s > 0, the half-width w >= 1: the rule, in plain loops"""
    n = len(colmax) - 1
    tops = [j for j in range(1, n + 1) if colmax[j] == s]
    out = [(int(s), int(rows[tops[0]]), tops[0])]
    taken = []
    while len(out) < k_max:
        best, bj = 0, 0
        for j in range(1, n + 1):
            if all(abs(j - c) > w for c in tops) and all(abs(j - c) > w for c in taken) and colmax[j] > best:
                best, bj = int(colmax[j]), j
        if best == 0:
            break
        out.append((best, int(rows[bj]), bj))
        taken.append(bj)
    return out


def hits_scalar(ref, read, scores, w, k_max, band=0, tie_mode=0, matrix=None, strip=1024):
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return []
    res = gr.align_scalar(ref, read, scores, gr.LOCAL, band, False, tie_mode, matrix, strip, matrices=True)
    s, H = res[0], res[2]
    if s == 0:
        return []
    colmax, rows = [0], [0]
    for j in range(1, n + 1):
        best, bi = -1, 0
        for i in range(1, m + 1):
            if H[i][j] > best:
                best, bi = H[i][j], i
        colmax.append(best)
        rows.append(bi)
    assert max(colmax) == s
    return pick(colmax, rows, s, sr.mask_width(w, m), k_max)


def hits_numpy(ref, read, scores, w, k_max, band=0, matrix=None, strip=1024):
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return []
    H = sr.local_h(ref, read, scores, band, matrix, strip)
    colmax = H[1:].max(axis=0)                   # (index 0: column 0, all 0)
    rows = H[1:].argmax(axis=0) + 1              # (argmax: the first row that holds the maximum)
    s = int(colmax.max())
    if s == 0:
        return []
    w = sr.mask_width(w, m)
    cols = np.arange(n + 1)
    tops = cols[colmax == s]
    tops = tops[tops >= 1]
    ok = np.ones(n + 1, dtype=bool)
    ok[0] = False
    for c in tops:
        ok[max(int(c) - w, 0):int(c) + w + 1] = False
    out = [(s, int(rows[tops[0]]), int(tops[0]))]
    while len(out) < k_max:
        vals = np.where(ok, colmax, 0)
        best = int(vals.max())
        if best == 0:
            break
        j = int(np.argmax(vals == best))
        out.append((best, int(rows[j]), j))
        ok[max(j - w, 0):j + w + 1] = False
    return out
