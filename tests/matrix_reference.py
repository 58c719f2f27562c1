"""Two independent restatements of the score-matrix contract (DESIGN.md "Score matrices") -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Both take scores = (match, mismatch, gap, gap_open) as tests/affine_reference.py
does, and matrix = (alphabet, rows): alphabet a str / bytes of n symbols, rows[i][j] the score of READ base alphabet[i] against
REFERENCE base alphabet[j].  The cell score s(i,j) is the matrix entry when both bases are in the alphabet (after
Character.toUpperCase on ISO-8859-1), else match when the two bases are the same symbol and mismatch otherwise.  Everything else
-- the affine recurrence (gap_open = 0: the linear one), the tie chains, the maximum cells and their order, the walk -- is
the affine contract.  They return what OptAlignments.call returns: (score, [(begin, (refAligned, readAligned)), ...]).

align_scalar looks every cell's score up in a dict inside a plain loop; align_numpy builds a 256 x 256 score table and sweeps
whole anti-diagonals.
"""
import numpy as np

from affine_reference import NEG, _finish, _order, _s, _upper


def _alpha(alphabet):
    return alphabet.decode("latin-1") if isinstance(alphabet, (bytes, bytearray)) else alphabet


def cell_score(ref_char, read_char, scores, matrix):
    """s(i, j) of the contract for one (reference, read) character pair."""
    match, mismatch = scores[0], scores[1]
    r, q = _upper(ref_char), _upper(read_char)
    if matrix is not None:
        idx = {_upper(c): k for k, c in enumerate(_alpha(matrix[0]))}
        if r in idx and q in idx:
            return matrix[1][idx[q]][idx[r]]
    return match if r == q else mismatch


def align_scalar(ref, read, scores, matrix, tie_mode=0, matrices=False):
    ref, read = _s(ref), _s(read)
    match, mismatch, e, o = scores
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    entry = {}
    if matrix is not None:
        alpha = _alpha(matrix[0])
        for a, ca in enumerate(alpha):
            for b, cb in enumerate(alpha):
                entry[(_upper(ca), _upper(cb))] = matrix[1][a][b]          # (read symbol, reference symbol)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [["-"] * (n + 1) for _ in range(m + 1)]
    XE = [[0] * (n + 1) for _ in range(m + 1)]
    XF = [[0] * (n + 1) for _ in range(m + 1)]
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    max_score, cells = 0, []
    for i, j in _order(m, n, strict):
        ext, opn = E[i][j - 1] + e, H[i][j - 1] + o + e
        E[i][j], XE[i][j] = max(opn, ext), int(ext > opn)
        ext, opn = F[i - 1][j] + e, H[i - 1][j] + o + e
        F[i][j], XF[i][j] = max(opn, ext), int(ext > opn)
        q, r = _upper(read[i - 1]), _upper(ref[j - 1])
        s = entry.get((q, r))
        if s is None:
            s = match if q == r else mismatch
        mx, t = 0, "-"
        if ge(E[i][j], mx):
            mx, t = E[i][j], "d"
        if ge(F[i][j], mx):
            mx, t = F[i][j], "i"
        if ge(H[i - 1][j - 1] + s, mx):
            mx, t = H[i - 1][j - 1] + s, "a"
        H[i][j], D[i][j] = mx, t
        if mx > max_score:
            max_score, cells = mx, [(i, j)]
        elif mx == max_score:
            cells.append((i, j))
    res = _finish(ref, read, max_score, cells, H, D, XE, XF, strict)
    if matrices:
        return res + (H, E, F, D, XE, XF)
    return res


def score_table(scores, matrix):
    """256 x 256 int64: [read byte, reference byte] -> s."""
    match, mismatch = scores[0], scores[1]
    up = np.array([ord(_upper(chr(b))) for b in range(256)], dtype=np.int64)   # (0xFF's upper case is outside Latin-1: only itself)
    T = np.where(up[:, None] == up[None, :], match, mismatch).astype(np.int64)
    if matrix is not None:
        alpha = [ord(c) for c in _alpha(matrix[0])]
        cls = np.full(256, -1, dtype=np.int64)
        for k, c in enumerate(alpha):
            cls[up == up[c]] = k
        M = np.asarray(matrix[1], dtype=np.int64)
        inside = (cls[:, None] >= 0) & (cls[None, :] >= 0)
        T = np.where(inside, M[np.maximum(cls, 0)[:, None], np.maximum(cls, 0)[None, :]], T)
    return T


def align_numpy(ref, read, scores, matrix, tie_mode=0):
    ref, read = _s(ref), _s(read)
    _, _, e, o = scores
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, []
    T = score_table(scores, matrix)
    rb = np.frombuffer(ref.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    qb = np.frombuffer(read.encode("latin-1"), dtype=np.uint8).astype(np.int64)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.zeros((m + 1, n + 1), dtype=np.int8)          # 0 '-', 1 'a', 2 'i', 3 'd'
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        ext, opn = E[i, j - 1] + e, H[i, j - 1] + o + e
        E[i, j] = np.maximum(opn, ext)
        XE[i, j] = ext > opn
        ext, opn = F[i - 1, j] + e, H[i - 1, j] + o + e
        F[i, j] = np.maximum(opn, ext)
        XF[i, j] = ext > opn
        a = H[i - 1, j - 1] + T[qb[i - 1], rb[j - 1]]
        ev, fv = E[i, j], F[i, j]
        h = np.maximum(np.maximum(np.maximum(ev, fv), a), 0)
        if strict:
            dd = np.where(h == 0, 0, np.where(ev == h, 3, np.where(fv == h, 2, 1)))
        else:
            dd = np.where(a == h, 1, np.where(fv == h, 2, np.where(ev == h, 3, 0)))
        H[i, j] = h
        D[i, j] = dd
    max_score = int(H.max())
    cells = [tuple(int(x) for x in c) for c in np.argwhere(H == max_score) if c[0] > 0 and c[1] > 0]
    if strict:
        cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    Dc = np.array(["-", "a", "i", "d"])[D]
    return _finish(ref, read, max_score, cells, H.tolist(), Dc.tolist(), XE.tolist(), XF.tolist(), strict)
