"""Two independent restatements of the end-to-end alignment contract (DESIGN.md "End-to-end modes") -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  mode: 1 fit (the whole read against any stretch of the reference), 2 global (the
whole read against the whole reference); mode 0 is handed to affine_reference / matrix_reference, the local contract.
scores = (match, mismatch, gap, gap_open); matrix = None or (alphabet, rows) as swmi_set_score_matrix takes them
(row = read symbol, column = reference symbol; a base outside the alphabet keeps the match / mismatch rule).
Both return (score, [(beginning, (refAligned, readAligned)), ...]).  Python ints throughout the scalar form: no bound applies.

  E(i,j) = max(H(i,j-1) + o + e, E(i,j-1) + e)    xE = 1 iff E(i,j-1) + e > H(i,j-1) + o + e
  F(i,j) = max(H(i-1,j) + o + e, F(i-1,j) + e)    xF = 1 iff F(i-1,j) + e > H(i-1,j) + o + e
  H(i,j) = max(E, F, H(i-1,j-1) + s): E 'd', then F 'i', then the diagonal 'a' replace on '>=' (serial) or '>' (strict)
  fit:    H(0,j) = 0, H(i,0) = F(i,0) = o + i*e;            score = max_j H(m,j), cells (m,j) ascending j
  global: H(0,j) = E(0,j) = o + j*e, H(i,0) as fit, H(0,0) = 0; score = H(m,n), the one cell (m,n)
"""
import numpy as np

import affine_reference as _ar
import matrix_reference as _mr

NEG = -(1 << 60)
GAP_CHAR = "_"
LOCAL, FIT, GLOBAL = 0, 1, 2
_s, _upper, _UPPER = _ar._s, _ar._upper, _ar._UPPER


def _score_fn(scores, matrix):
    match, mismatch = scores[0], scores[1]
    if matrix is None:
        return lambda r, q: match if _upper(r) == _upper(q) else mismatch
    alphabet, rows = matrix
    alphabet = _s(alphabet)
    idx = {_upper(c): k for k, c in enumerate(alphabet)}

    def s(r, q):
        cr, cq = idx.get(_upper(r)), idx.get(_upper(q))
        if cr is not None and cq is not None:
            return int(rows[cq][cr])
        return match if _upper(r) == _upper(q) else mismatch
    return s


def _walk(cell, ref, read, D, XE, XF, mode):
    i, j = cell
    st, beginning, stack = "H", j, []
    while i > 0:
        if j == 0:
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


def _finish(ref, read, H, D, XE, XF, mode, strict):
    m, n = len(read), len(ref)
    if mode == GLOBAL:
        score, cells = H[m][n], [(m, n)]
    else:
        score = max(H[m][1:])
        cells = [(m, j) for j in range(1, n + 1) if H[m][j] == score]
    opt = [_walk(c, ref, read, D, XE, XF, mode) for c in cells]
    if strict:
        opt.sort(key=lambda t: t[0])
    return int(score), opt


def _local(ref, read, scores, tie_mode, matrix):
    if matrix is None:
        return _ar.align_numpy(ref, read, scores, tie_mode)
    return _mr.align_numpy(ref, read, scores, matrix, tie_mode)


def align_scalar(ref, read, scores, mode, tie_mode=0, matrix=None, matrices=False):
    ref, read = _s(ref), _s(read)
    if mode == LOCAL:
        return _local(ref, read, scores, tie_mode, matrix)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, []
    s = _score_fn(scores, matrix)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        H[i][0] = F[i][0] = o + i * e
    if mode == GLOBAL:
        for j in range(1, n + 1):
            H[0][j] = E[0][j] = o + j * e
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
            E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
            ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
            F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
            mx, t = E[i][j], "d"
            if ge(F[i][j], mx):
                mx, t = F[i][j], "i"
            a = H[i - 1][j - 1] + s(ref[j - 1], read[i - 1])
            if ge(a, mx):
                mx, t = a, "a"
            H[i][j], D[i][j] = mx, t
    res = _finish(ref, read, H, D, XE, XF, mode, strict)
    if matrices:
        return res + (H, E, F, D, XE, XF)
    return res


def _score_table(ref, read, scores, matrix):
    """s(i, j) for every cell as an (m, n) int64 array"""
    rc = _UPPER[np.frombuffer(ref.encode("latin-1"), dtype=np.uint8)]
    qc = _UPPER[np.frombuffer(read.encode("latin-1"), dtype=np.uint8)]
    S = np.where(qc[:, None] == rc[None, :], np.int64(scores[0]), np.int64(scores[1]))
    if matrix is not None:
        alphabet, rows = matrix
        cls = np.full(256, -1, dtype=np.int64)
        for k, c in enumerate(_s(alphabet)):
            cls[_UPPER[ord(c)]] = k
        M = np.asarray(rows, dtype=np.int64)
        cq, cr = cls[qc], cls[rc]
        both = (cq[:, None] >= 0) & (cr[None, :] >= 0)
        S = np.where(both, M[np.maximum(cq, 0)[:, None], np.maximum(cr, 0)[None, :]], S)
    return S


def align_numpy(ref, read, scores, mode, tie_mode=0, matrix=None):
    ref, read = _s(ref), _s(read)
    if mode == LOCAL:
        return _local(ref, read, scores, tie_mode, matrix)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, []
    S = _score_table(ref, read, scores, matrix)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int8)          # 1 'a', 2 'i', 3 'd'
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    H[1:, 0] = F[1:, 0] = o + e * np.arange(1, m + 1, dtype=np.int64)
    if mode == GLOBAL:
        H[0, 1:] = E[0, 1:] = o + e * np.arange(1, n + 1, dtype=np.int64)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        ext, opn = E[i, j - 1] + e, H[i, j - 1] + o + e
        E[i, j] = np.maximum(opn, ext)
        XE[i, j] = ext > opn
        ext, opn = F[i - 1, j] + e, H[i - 1, j] + o + e
        F[i, j] = np.maximum(opn, ext)
        XF[i, j] = ext > opn
        a = H[i - 1, j - 1] + S[i - 1, j - 1]
        ev, fv = E[i, j], F[i, j]
        h = np.maximum(np.maximum(ev, fv), a)
        if strict:      # '>' chain: the first candidate that reaches the maximum wins (d, then i, then a)
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
        else:           # '>=' chain: the last candidate that reaches the maximum wins (a, then i, then d)
            dd = np.where(a == h, 1, np.where(fv == h, 2, 3))
        H[i, j] = h
        D[i, j] = dd
    Dc = np.array(["-", "a", "i", "d"])[D]
    return _finish(ref, read, H.tolist(), Dc.tolist(), XE.tolist(), XF.tolist(), mode, strict)


def rescore(ref_al, read_al, scores, matrix=None):
    """the score of an alignment given as its two strings: a gap of length k costs gap_open + k * gap"""
    s = _score_fn(scores, matrix)
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
