"""The per-read profile contract of DESIGN.md section 8t, restated twice -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  A profile is m rows of n integers over an alphabet of n symbols: the cell score is

    s(i,j) = profile[i-1][class(ref[j-1])]   if the reference byte, upper-cased as Character.toUpperCase does on ISO-8859-1, is in
                                             the alphabet
           = mismatch                        otherwise

and everything else is the contract of tests/gotoh_reference.py (local, fit, global, extend) or tests/overlap_reference.py (overlap)
with this s.  The read's bytes score nothing; they are what the read side of an alignment shows.

align_scalar needs no DP of its own.  The read is encoded as m distinct code points outside Latin-1, one per position, and the
scalar form of the mode's reference is given a score matrix whose alphabet is the profile's alphabet plus those m symbols: the row of
position symbol i is profile[i].  A position symbol never equals a reference byte, so a reference byte outside the alphabet scores
mismatch, which is the contract.  The read strings of the result are mapped back to the real bases.

align_numpy is an anti-diagonal form of its own for the larger shapes (gotoh_reference.align_numpy looks scores up in a 256 x 256
table by the read's BYTE and cannot take such a read); tests/test_profile_cpu.py holds it to the scalar form.

Both take (ref, read, alphabet, profile, scores, mode, extend, overlap, tie_mode, cells) and return what gotoh_reference's functions
return.  scores = (match, mismatch, gap, gap_open); match is not read.  overlap=True needs mode FIT, extend=True mode GLOBAL.
"""
import numpy as np

import gotoh_reference as gr
import overlap_reference as ov
from gotoh_reference import FIT, GLOBAL, LOCAL, NEG

POS0 = 0x4E00                 # the code point of read position 0 in the scalar form


def _classes(alphabet):
    """256 entries: the symbol index of a byte, -1 outside the alphabet"""
    alphabet = gr._s(alphabet)
    up = [ord(gr.upper(chr(b))) for b in range(256)]
    cls = [-1] * 256
    for k, c in enumerate(alphabet):
        for b in range(256):
            if up[b] == up[ord(c)]:
                cls[b] = k
    return cls


def check_profile(read, alphabet, profile):
    n = len(gr._s(alphabet))
    assert len(profile) == len(read) and all(len(r) == n for r in profile), "a profile has one row of n entries per read base"


def cell_score(ref_char, i, alphabet, profile, mismatch):
    """s of the contract for read row i (1-based) against one reference character"""
    c = _classes(alphabet)[ord(ref_char)]
    return int(profile[i - 1][c]) if c >= 0 else int(mismatch)


def rescore(ref_al, read_al, end_i, alphabet, profile, scores):
    """the score of an alignment given as its two strings and the read row it ends on"""
    cls = _classes(alphabet)
    e, o = scores[2], scores[3]
    i = end_i - sum(1 for c in read_al if c != gr.GAP_CHAR)
    total, prev = 0, None
    for r, q in zip(ref_al, read_al):
        if q != gr.GAP_CHAR:
            i += 1
        if r == gr.GAP_CHAR or q == gr.GAP_CHAR:
            kind = "i" if r == gr.GAP_CHAR else "d"
            total += e + (o if kind != prev else 0)
            prev = kind
        else:
            c = cls[ord(r)]
            total += int(profile[i - 1][c]) if c >= 0 else scores[1]
            prev = None
    return total


def align_scalar(ref, read, alphabet, profile, scores, mode=LOCAL, extend=False, overlap=False, tie_mode=0, cells=False):
    ref, read, alphabet = gr._s(ref), gr._s(read), gr._s(alphabet)
    check_profile(read, alphabet, profile)
    m, n = len(read), len(alphabet)
    pos = "".join(chr(POS0 + i) for i in range(m))
    rows = [[0] * (n + m) for _ in range(n)] + [[int(v) for v in profile[i]] + [0] * m for i in range(m)]
    matrix = (alphabet + pos, rows)
    if overlap:
        res = ov.align_scalar(ref, pos, scores, mode=mode, tie_mode=tie_mode, matrix=matrix, cells=cells)
    else:
        res = gr.align_scalar(ref, pos, scores, mode=mode, extend=extend, tie_mode=tie_mode, matrix=matrix, cells=cells)
    back = {ord(c): read[i] for i, c in enumerate(pos)}
    opt = [(b, (ra, qa.translate(back))) for b, (ra, qa) in res[1]]
    return (res[0], opt) + tuple(res[2:])


def score_rows(ref, alphabet, profile, mismatch):
    """(m, n) int64: s(i, j) at [i - 1, j - 1]"""
    cls = np.array(_classes(alphabet), dtype=np.int64)
    rb = np.frombuffer(gr._s(ref).encode("latin-1"), dtype=np.uint8).astype(np.int64)
    P = np.asarray(profile, dtype=np.int64).reshape(len(profile), -1)
    c = cls[rb]
    return np.where(c[None, :] >= 0, P[:, np.maximum(c, 0)], int(mismatch))


def align_numpy(ref, read, alphabet, profile, scores, mode=LOCAL, extend=False, overlap=False, tie_mode=0, cells=False):
    assert mode == GLOBAL or not extend, "extend is an option of global mode"
    assert mode == FIT or not overlap, "overlap is an option of fit mode"
    ref, read = gr._s(ref), gr._s(read)
    check_profile(read, alphabet, profile)
    e, o = int(scores[2]), int(scores[3])
    strict = tie_mode == 1
    m, n = len(read), len(ref)
    if m == 0 or n == 0:
        return (0, [], []) if cells else (0, [])
    S = score_rows(ref, alphabet, profile, scores[1])
    H = np.full((m + 1, n + 1), 0 if mode == LOCAL else NEG, dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    D = np.full((m + 1, n + 1), "-", dtype="U1")
    XE = np.zeros((m + 1, n + 1), dtype=np.int8)
    XF = np.zeros((m + 1, n + 1), dtype=np.int8)
    i0, j0 = np.arange(1, m + 1, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64)
    H[0, 0] = 0
    if mode == GLOBAL:
        H[0, j0] = E[0, j0] = o + e * j0
    else:
        H[0, j0] = 0
    if mode == LOCAL or overlap:
        H[i0, 0] = 0
    else:
        H[i0, 0] = F[i0, 0] = o + e * i0
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
        a = H[i - 1, j - 1] + S[i - 1, j - 1]
        h = np.maximum(np.maximum(ev, fv), a)
        if mode == LOCAL:
            h = np.maximum(h, 0)
        if strict:      # '>' chain: the first candidate (above 0 in local mode) that reaches the maximum wins: d, then i, then a
            dd = np.where(ev == h, 3, np.where(fv == h, 2, 1))
            if mode == LOCAL:
                dd = np.where(h == 0, 0, dd)
        else:           # '>=' chain: the last candidate that reaches the maximum wins: a, then i, then d, then local's 0
            dd = np.where(a == h, 1, np.where(fv == h, 2, np.where(ev == h, 3, 0)))
        E[i, j], F[i, j], H[i, j], D[i, j] = ev, fv, h, letters[dd]
    if overlap:
        best = max(int(H[m, 1:].max()), int(H[1:, n].max()))
        best_cells = [c for c in ov.competing(m, n, strict) if H[c[0], c[1]] == best]
        return ov._finish(ref, read, strict, best, best_cells, D, XE, XF, cells)
    if mode == LOCAL or extend:
        best = int(H[1:, 1:].max())
        best_cells = []
        if cells or not (mode == LOCAL and best == 0):
            best_cells = [(int(c[0]) + 1, int(c[1]) + 1) for c in np.argwhere(H[1:, 1:] == best)]      # row-major
            if strict:
                best_cells.sort(key=lambda c: (c[0] + c[1], c[1]))
    elif mode == FIT:
        best = int(H[m, 1:].max())
        best_cells = [(m, j) for j in range(1, n + 1) if H[m, j] == best]
    else:
        best, best_cells = int(H[m, n]), [(m, n)]
    return gr._finish(ref, read, mode, strict, best, best_cells, m * n, H, D, XE, XF, cells)
