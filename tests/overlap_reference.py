"""The overlap (ends-free) contract of DESIGN.md section 8s, restated twice -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  align_scalar is the specification (Python ints, a true -inf, one loop over the cells);
align_numpy sweeps whole anti-diagonals in int64 for the 1,025-3,100 base shapes of the GPU tests, and the CPU tests hold it to the
scalar form.  Both take the arguments of tests/gotoh_reference.py and return what its functions return; an overlap run is a fit run
without a band, so mode must be FIT, w 0 and extend False (strip is accepted and changes nothing: every window is the reference).

E, F, the x bits and the tie chains are gotoh_reference's (fit mode: no floor, the direction is never '-').
  Boundaries.  H(0,j) = 0 for j = 0..n, H(i,0) = 0 for i = 1..m; E(i,0) = F(0,j) = -inf.
  Score.       The maximum of H over C = {(m,j): 1 <= j <= n} | {(i,n): 1 <= i <= m}: it may be <= 0 and is never degenerate.
  Cells.       Every cell of C that holds the score, (m,n) once, in gotoh_reference.order restricted to C; in strict tie mode the
               alignments are then stably sorted by `beginning`.
  Walk.        From the cell in state H with global mode's moves to the first cell with i == 0 or j == 0; nothing is appended there.
               `beginning` is the column of the last reference base taken, the end column if none is.
A pair with an empty side scores 0 with no alignments (and no cells).
"""
import numpy as np

from gotoh_reference import FIT, GAP_CHAR, NEG, NINF, _s, score_fn, score_table


def competing(m, n, strict):
    """C in the order the tied maxima are reported: row-major, or per anti-diagonal with ascending j"""
    cells = [(i, n) for i in range(1, m)] + [(m, j) for j in range(1, n + 1)]
    return sorted(cells, key=lambda c: (c[0] + c[1], c[1])) if strict else cells


def span(cell, alignment):
    """(read_first, end_i, begin, end_j) of an alignment (beginning, (refAligned, readAligned)) that ends at `cell`"""
    used = sum(1 for c in alignment[1][1] if c != GAP_CHAR)
    return cell[0] - used + 1, cell[0], alignment[0], cell[1]


def _walk(cell, ref, read, D, XE, XF):
    i, j = cell
    st, beginning, stack = "H", j, []
    while i > 0 and j > 0:
        if st == "H":
            st = {"a": "M", "i": "F", "d": "E"}[str(D[i][j])]
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
    stack.reverse()
    return beginning, ("".join(p[0] for p in stack), "".join(p[1] for p in stack))


def _finish(ref, read, strict, score, cells, D, XE, XF, want_cells):
    both = [(_walk(c, ref, read, D, XE, XF), c) for c in cells]
    if strict:
        both.sort(key=lambda t: t[0][0])
    opt, cells = [a for a, _ in both], [c for _, c in both]
    return (int(score), opt, cells) if want_cells else (int(score), opt)


def _check_args(mode, w, extend):
    assert mode == FIT and w == 0 and not extend, "an overlap run is an unbanded fit run"


def align_scalar(ref, read, scores, mode=FIT, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, matrices=False, cells=False):
    _check_args(mode, w, extend)
    ref, read = _s(ref), _s(read)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    res = (0, [], []) if cells else (0, [])
    if m and n:
        s = score_fn(scores, matrix)
        for j in range(n + 1):
            H[0][j] = 0
        for i in range(1, m + 1):
            H[i][0] = 0
        ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
        for i in range(1, m + 1):
            for j in range(1, n + 1):
                ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
                E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
                ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
                F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
                a = H[i - 1][j - 1] + s(ref[j - 1], read[i - 1])
                mx, t = E[i][j], "d"
                if ge(F[i][j], mx):
                    mx, t = F[i][j], "i"
                if ge(a, mx):
                    mx, t = a, "a"
                H[i][j], D[i][j] = mx, t
        C = competing(m, n, strict)
        best = max(H[i][j] for i, j in C)
        res = _finish(ref, read, strict, best, [c for c in C if H[c[0]][c[1]] == best], D, XE, XF, cells)
    if matrices:
        return res + (H, E, F, D, XE, XF)
    return res


def align_numpy(ref, read, scores, mode=FIT, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, cells=False):
    _check_args(mode, w, extend)
    ref, read = _s(ref), _s(read)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    T = score_table(scores, matrix)
    rb = np.frombuffer(ref.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(read.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    H = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.full((m + 1, n + 1), "-", dtype="U1")
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    H[0, :] = 0
    H[:, 0] = 0
    letters = np.array(list("-aid"))
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        ext, opn = E[i, j - 1] + e, H[i, j - 1] + o + e
        ev = np.maximum(opn, ext)
        XE[i, j] = ext > opn
        ext, opn = F[i - 1, j] + e, H[i - 1, j] + o + e
        fv = np.maximum(opn, ext)
        XF[i, j] = ext > opn
        a = H[i - 1, j - 1] + T[qb[i - 1], rb[j - 1]]
        h = np.maximum(np.maximum(ev, fv), a)
        if strict:      # '>' chain: the first candidate that reaches the maximum wins: d, then i, then a
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
        else:           # '>=' chain: the last candidate that reaches the maximum wins: a, then i, then d
            dd = np.where(a == h, 1, np.where(fv == h, 2, 3))
        E[i, j], F[i, j], H[i, j], D[i, j] = ev, fv, h, letters[dd]
    best = max(int(H[m, 1:].max()), int(H[1:, n].max()))
    best_cells = [c for c in competing(m, n, strict) if H[c[0], c[1]] == best]
    return _finish(ref, read, strict, best, best_cells, D, XE, XF, cells)
