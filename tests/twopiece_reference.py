"""The two-piece affine-gap contract of DESIGN.md section 8j, restated -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Two entry points with the arguments and the return value of
gotoh_reference.align_scalar / align_numpy: align_scalar is the specification (Python ints, a true -inf, one loop over the
cells); align_numpy sweeps whole anti-diagonals in int64 with -2^60 for -inf, for the shapes of the GPU tests, and the CPU tests
hold it to the scalar form.  The geometry (windows, the order of the cells) is gotoh_reference's.

Arguments.  scores = (match, mismatch, gap, gap_open, gap2, gap_open2): a gap of length k costs
max(gap_open + k * gap, gap_open2 + k * gap2); write o1, e1, o2, e2.  mode is GLOBAL, with or without extend; w, strip,
tie_mode and cells= as in gotoh_reference.

Recurrence, for i = 1..m over the read and j = 1..n over the reference, p = 1, 2:
  Ep(i,j) = max(H(i,j-1) + op + ep, Ep(i,j-1) + ep)    xEp = 1 iff the extension is strictly better
  Fp(i,j) = max(H(i-1,j) + op + ep, Fp(i-1,j) + ep)    xFp likewise
  E = max(E1, E2), pE = 1 iff E2 > E1; F, pF likewise (piece 1 wins a tie, in both tie modes)
  H(i,j) = E 'd', then F 'i', then H(i-1,j-1) + s 'a', each replacing on '>=' (serial tie mode) or '>' (strict)
Boundaries, where they lie in the band: H(0,0) = 0, H(0,j) = max(o1 + j*e1, o2 + j*e2), H(i,0) the same in i; every gap
state of row 0 and column 0 is -inf, so the first real cell opens (x = 0, the value H + op + ep).  A cell outside the band
reads as -inf in all five values.

Walk.  State H reads the direction; 'd' enters E2 if pE is set, else E1; 'i' enters F2 if pF is set, else F1; a gap state stays
while its own x bit is set.  At column 0 the read's head is inserted, at row 0 the rest of the reference is deleted; `beginning`
is the column of the last reference base taken.  An extend run lists its tied maximum cells in extend's order.
"""
import numpy as np

import gotoh_reference as gr

NINF, NEG, GAP_CHAR, GLOBAL = gr.NINF, gr.NEG, gr.GAP_CHAR, gr.GLOBAL


def gap_cost(k, scores):
    return max(scores[3] + k * scores[2], scores[5] + k * scores[4])


def rescore(ref_al, read_al, scores):
    """the score of an alignment given as its two strings: a gap run of length k costs max(o1 + k*e1, o2 + k*e2)"""
    s = gr.score_fn(scores, None)
    total, prev, run = 0, None, 0
    for r, q in list(zip(ref_al, read_al)) + [("x", "x")]:
        kind = "i" if r == GAP_CHAR else ("d" if q == GAP_CHAR else None)
        if kind != prev and prev is not None:
            total += gap_cost(run, scores)
            run = 0
        if kind is None:
            total += s(r, q)
        else:
            run += 1
        prev = kind
    return total - s("x", "x")


def _walk(cell, ref, read, D, X, P):
    """X = (XE1, XE2, XF1, XF2), P = (PE, PF), indexed [i][j]"""
    i, j = cell
    st, beginning, stack = "H", j, []
    while i > 0:
        if j == 0:
            stack.append((GAP_CHAR, read[i - 1]))
            i -= 1
            continue
        if st == "H":
            t = D[i][j]
            if t == "a":
                st = "M"
            elif t == "i":
                st = "F2" if P[1][i][j] else "F1"
            else:
                st = "E2" if P[0][i][j] else "E1"
        if st == "M":
            beginning = j
            stack.append((ref[j - 1], read[i - 1]))
            i, j, st = i - 1, j - 1, "H"
        elif st[0] == "F":
            stack.append((GAP_CHAR, read[i - 1]))
            st = st if X[2 if st == "F1" else 3][i][j] else "H"
            i -= 1
        else:
            beginning = j
            stack.append((ref[j - 1], GAP_CHAR))
            st = st if X[0 if st == "E1" else 1][i][j] else "H"
            j -= 1
    while j > 0:
        beginning = j
        stack.append((ref[j - 1], GAP_CHAR))
        j -= 1
    stack.reverse()
    return beginning, ("".join(p[0] for p in stack), "".join(p[1] for p in stack))


def _finish(ref, read, strict, score, cells, D, X, P, want_cells):
    both = [(_walk(c, ref, read, D, X, P), c) for c in cells]
    if strict:
        both.sort(key=lambda t: t[0][0])
    opt, cells = [a for a, _ in both], [c for _, c in both]
    return (int(score), opt, cells) if want_cells else (int(score), opt)


def align_scalar(ref, read, scores, mode=GLOBAL, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, cells=False):
    assert mode == GLOBAL and matrix is None, "two-piece gaps: global and extend runs without a score matrix"
    ref, read = gr._s(ref), gr._s(read)
    e1, o1, e2, o2 = (int(x) for x in scores[2:6])
    op, ep = (o1, o2), (e1, e2)
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    mk = lambda v: [[v] * (n + 1) for _ in range(m + 1)]
    H, D = mk(NINF), mk("-")
    E, F = (mk(NINF), mk(NINF)), (mk(NINF), mk(NINF))
    X = (mk(0), mk(0), mk(0), mk(0))                       # XE1, XE2, XF1, XF2
    P = (mk(0), mk(0))                                     # PE, PF
    win = gr.windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    s = gr.score_fn(scores, None)
    H[0][0] = 0
    for j in range(1, win[0][1] + 1):
        H[0][j] = max(o1 + j * e1, o2 + j * e2)
    for i in range(1, m + 1):
        if win[(i - 1) // strip][0] == 1:
            H[i][0] = max(o1 + i * e1, o2 + i * e2)
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    best, best_cells = None, []
    for i, j in gr.order(m, n, strict):
        lo, hi = win[(i - 1) // strip]
        if not lo <= j <= hi:
            continue
        for p in (0, 1):
            ext, opn = E[p][i][j - 1] + ep[p], H[i][j - 1] + op[p] + ep[p]
            E[p][i][j], X[p][i][j] = max(opn, ext), int(ext > opn)
            ext, opn = F[p][i - 1][j] + ep[p], H[i - 1][j] + op[p] + ep[p]
            F[p][i][j], X[2 + p][i][j] = max(opn, ext), int(ext > opn)
        P[0][i][j] = int(E[1][i][j] > E[0][i][j])
        P[1][i][j] = int(F[1][i][j] > F[0][i][j])
        ev, fv = max(E[0][i][j], E[1][i][j]), max(F[0][i][j], F[1][i][j])
        a = H[i - 1][j - 1] + s(ref[j - 1], read[i - 1])
        mx, t = ev, "d"
        if ge(fv, mx):
            mx, t = fv, "i"
        if ge(a, mx):
            mx, t = a, "a"
        assert mx != NINF, (i, j)
        H[i][j], D[i][j] = mx, t
        if extend:
            if best is None or mx > best:
                best, best_cells = mx, [(i, j)]
            elif mx == best:
                best_cells.append((i, j))
    if not extend:
        assert win[-1][0] <= n <= win[-1][1], "(m, n) outside the band"
        best, best_cells = H[m][n], [(m, n)]
    return _finish(ref, read, strict, best, best_cells, D, X, P, cells)


def align_numpy(ref, read, scores, mode=GLOBAL, w=0, extend=False, tie_mode=0, matrix=None, strip=1024, cells=False):
    assert mode == GLOBAL and matrix is None, "two-piece gaps: global and extend runs without a score matrix"
    ref, read = gr._s(ref), gr._s(read)
    e1, o1, e2, o2 = (int(x) for x in scores[2:6])
    op, ep = (o1, o2), (e1, e2)
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    win = gr.windows(m, n, w, strip)
    assert all(lo <= hi for lo, hi in win), "a strip with an empty window"
    T = gr.score_table(scores, None)
    rb = np.frombuffer(ref.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(read.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    rows = np.arange(1, m + 1, dtype=np.int64)
    lo_of = np.repeat(np.array([x[0] for x in win], dtype=np.int64), strip)[:m]
    hi_of = np.repeat(np.array([x[1] for x in win], dtype=np.int64), strip)[:m]
    full = lambda v, dt=np.int64: np.full((m + 1, n + 1), v, dtype=dt)
    H = full(NEG)
    E, F = (full(NEG), full(NEG)), (full(NEG), full(NEG))
    D = full("-", "U1")
    X = tuple(full(0, np.int8) for _ in range(4))
    P = (full(0, np.int8), full(0, np.int8))
    H[0, 0] = 0
    j0 = np.arange(1, win[0][1] + 1, dtype=np.int64)
    i0 = rows[lo_of == 1]
    H[0, j0] = np.maximum(o1 + e1 * j0, o2 + e2 * j0)
    H[i0, 0] = np.maximum(o1 + e1 * i0, o2 + e2 * i0)
    diag = np.arange(m + n + 1)
    first = np.searchsorted(rows + hi_of, diag, "left") + 1
    last = np.searchsorted(rows + lo_of, diag, "right")
    letters = np.array(list("-aid"))
    for d in range(2, m + n + 1):
        i = np.arange(first[d], last[d] + 1)
        if i.size == 0:
            continue
        j = d - i
        for p in (0, 1):
            ext, opn = E[p][i, j - 1] + ep[p], H[i, j - 1] + op[p] + ep[p]
            E[p][i, j] = np.maximum(opn, ext)
            X[p][i, j] = ext > opn
            ext, opn = F[p][i - 1, j] + ep[p], H[i - 1, j] + op[p] + ep[p]
            F[p][i, j] = np.maximum(opn, ext)
            X[2 + p][i, j] = ext > opn
        P[0][i, j] = E[1][i, j] > E[0][i, j]
        P[1][i, j] = F[1][i, j] > F[0][i, j]
        ev, fv = np.maximum(E[0][i, j], E[1][i, j]), np.maximum(F[0][i, j], F[1][i, j])
        a = H[i - 1, j - 1] + T[qb[i - 1], rb[j - 1]]
        h = np.maximum(np.maximum(ev, fv), a)
        if strict:
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
        else:
            dd = np.where(a == h, 1, np.where(fv == h, 2, 3))
        H[i, j], D[i, j] = h, letters[dd]
    if extend:
        cols = np.arange(n + 1)[None, :]
        inb = np.zeros((m + 1, n + 1), dtype=bool)
        inb[1:] = (cols >= lo_of[:, None]) & (cols <= hi_of[:, None])
        best = int(H[inb].max())
        best_cells = [tuple(int(x) for x in c) for c in np.argwhere(inb & (H == best))]
        if strict:
            best_cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    else:
        assert win[-1][0] <= n <= win[-1][1], "(m, n) outside the band"
        best, best_cells = int(H[m, n]), [(m, n)]
    return _finish(ref, read, strict, best, best_cells, D, X, P, cells)
