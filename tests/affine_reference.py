"""Two independent restatements of the affine-gap contract (DESIGN.md "Affine gaps") -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Both take scores = (match, mismatch, gap, gap_open) -- gap is the per-base
extension e, gap_open the extra cost o of opening a gap, both <= 0 -- and return what OptAlignments.call returns:
(score, [(begin, (refAligned, readAligned)), ...]) in the reference's order (SmithWaterman.java:157-185 row-major;
DistributedSW.java:209-239 per anti-diagonal, ascending j, then the stable sort by begin of :480).

  E(i,j) = max(H(i,j-1) + o + e, E(i,j-1) + e)    xE = 1 iff E(i,j-1) + e > H(i,j-1) + o + e
  F(i,j) = max(H(i-1,j) + o + e, F(i-1,j) + e)    xF = 1 iff F(i-1,j) + e > H(i-1,j) + o + e
  H(i,j) = 0 '-', then E 'd', F 'i', H(i-1,j-1) + s 'a' through a '>=' chain (serial) or a '>' chain (strict)
  row 0 / column 0: H = 0, E = F = -inf

align_scalar is a plain loop over the cells; align_numpy sweeps whole anti-diagonals with numpy.  The walk is the
three-state machine of the contract in both (it is short next to the matrix).
"""
import numpy as np

NEG = -(1 << 60)          # -inf: far below anything a sum of the bounded scores can reach
GAP_CHAR = "_"


def _s(x):
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x


def _upper(c):
    o = ord(c)
    if 0x61 <= o <= 0x7A or (0xE0 <= o <= 0xFE and o != 0xF7):
        return chr(o - 32)
    return c


_UPPER = np.array([_upper(chr(b)).encode("latin-1")[0] if ord(_upper(chr(b))) < 256 else b for b in range(256)], dtype=np.int32)


def _order(m, n, strict):
    if not strict:
        return [(i, j) for i in range(1, m + 1) for j in range(1, n + 1)]
    return [(d - j, j) for d in range(2, m + n + 1) for j in range(max(1, d - m), min(n, d - 1) + 1)]


def _walk(cell, ref, read, H, D, XE, XF):
    """The contract's walk: state H picks M/F/E from dir; M moves diagonally; F and E stay in their gap while x is set."""
    i, j = cell
    st = "H"
    beginning = 0
    stack = []
    while H[i][j] > 0:
        beginning = j
        if st == "H":
            st = {"a": "M", "i": "F", "d": "E"}[D[i][j]]
        if st == "M":
            stack.append((ref[j - 1], read[i - 1]))
            i, j, st = i - 1, j - 1, "H"
        elif st == "F":
            stack.append((GAP_CHAR, read[i - 1]))
            st = "F" if XF[i][j] else "H"
            i -= 1
        else:
            stack.append((ref[j - 1], GAP_CHAR))
            st = "E" if XE[i][j] else "H"
            j -= 1
    stack.reverse()
    return beginning, ("".join(p[0] for p in stack), "".join(p[1] for p in stack))


def _finish(ref, read, max_score, cells, H, D, XE, XF, strict):
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, []
    if max_score == 0:                                    # every cell ties at 0 and yields (0, "", "")
        return 0, [(0, ("", ""))] * (m * n)
    opt = [_walk(c, ref, read, H, D, XE, XF) for c in cells]
    if strict:
        opt.sort(key=lambda t: t[0])
    return max_score, opt


def align_scalar(ref, read, scores, tie_mode=0, matrices=False):
    ref, read = _s(ref), _s(read)
    match, mismatch, e, o = scores
    strict = tie_mode == 1
    m, n = len(read), len(ref)
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
        s = match if _upper(ref[j - 1]) == _upper(read[i - 1]) else mismatch
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


def align_numpy(ref, read, scores, tie_mode=0):
    ref, read = _s(ref), _s(read)
    match, mismatch, e, o = scores
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return 0, []
    rc = _UPPER[np.frombuffer(ref.encode("latin-1"), dtype=np.uint8)]
    qc = _UPPER[np.frombuffer(read.encode("latin-1"), dtype=np.uint8)]
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
        a = H[i - 1, j - 1] + np.where(rc[j - 1] == qc[i - 1], match, mismatch)
        ev, fv = E[i, j], F[i, j]
        h = np.maximum(np.maximum(np.maximum(ev, fv), a), 0)
        if strict:      # '>' chain: the first candidate above 0 that reaches the maximum wins (d, then i, then a)
            dd = np.where(h == 0, 0, np.where(ev == h, 3, np.where(fv == h, 2, 1)))
        else:           # '>=' chain: the last candidate that reaches the maximum wins (a, then i, then d)
            dd = np.where(a == h, 1, np.where(fv == h, 2, np.where(ev == h, 3, 0)))
        H[i, j] = h
        D[i, j] = dd
    max_score = int(H.max())
    cells = [tuple(int(x) for x in c) for c in np.argwhere(H == max_score) if c[0] > 0 and c[1] > 0]
    if strict:
        cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    Dc = np.array(["-", "a", "i", "d"])[D]
    return _finish(ref, read, max_score, cells, H.tolist(), Dc.tolist(), XE.tolist(), XF.tolist(), strict)
