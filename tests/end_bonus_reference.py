"""Option "end_bonus" (DESIGN.md section 8o), restated on tests/gotoh_reference.py -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  An extend run (global mode's cells, the maximum over every existing cell) of a pair
with both sides non-empty, and beside it
  max_score  the extend run's score
  end_score  the maximum of H(m, j) over the existing cells of read row m: the columns of the last strip's window under a band
             (w > 0 and m > strip), else 1 .. n
  end_col    the smallest such column that holds it
The pair is taken to the end iff end_score + b > max_score (b >= 1; Python ints, so the sum is exact).  A pair that is taken has
the score end_score, the one cell (m, end_col) and the one alignment the module's own global walk spells from that cell; a pair
that is not, and every pair under b = 0, is the extend run as it stands.

align_scalar is the specification, over the scalar matrices; align sweeps with the numpy form (the 1,025 .. 2,048 base shapes
of the GPU tests) and keeps the matrices of the last sweeps, so that a test which runs several bonuses on one pair sweeps it
once.  Both return (score, alignments, cells, taken, (max_score, end_score, end_col)); a pair with an empty side gives
(0, [], [], False, (0, 0, 0))."""
import gotoh_reference as gr
import xdrop_reference as xr          # the extend matrices of a pair, scalar and numpy (the numpy ones kept between calls)

EMPTY = (0, [], [], False, (0, 0, 0))


def end_of_row(H, m, n, w=0, strip=1024):
    """(end_score, end_col) of the matrices of an (m, n) pair: row m over the last window, the smallest column on a tie"""
    lo, hi = gr.windows(m, n, w, strip)[-1]
    row = [int(H[m][j]) for j in range(lo, hi + 1)]
    best = max(row)
    return best, lo + row.index(best)


def taken(max_score, end_score, b):
    """the choice: strict, and never under b = 0"""
    return b > 0 and end_score + b > max_score


def _choose(ref, read, b, w, strip, full, H, D, XE, XF):
    m, n = len(read), len(ref)
    end_score, end_col = end_of_row(H, m, n, w, strip)
    ends = (int(full[0]), end_score, end_col)
    if not taken(full[0], end_score, b):
        return full[0], full[1], full[2], False, ends
    cell = (m, end_col)
    return end_score, [gr._walk(cell, ref, read, H, D, XE, XF, gr.GLOBAL)], [cell], True, ends


def align_scalar(ref, read, scores, b, w=0, tie_mode=0, matrix=None, strip=1024):
    ref, read = gr._s(ref), gr._s(read)
    if not ref or not read:
        return EMPTY
    full, H, D, XE, XF = xr._matrices_scalar(ref, read, scores, w, tie_mode, matrix, strip)
    return _choose(ref, read, b, w, strip, full, H, D, XE, XF)


def align(ref, read, scores, b, w=0, tie_mode=0, matrix=None, strip=1024):
    ref, read = gr._s(ref), gr._s(read)
    if not ref or not read:
        return EMPTY
    full, H, D, XE, XF = xr._matrices_numpy(ref, read, scores, w, tie_mode, matrix, strip)
    return _choose(ref, read, b, w, strip, full, H, D, XE, XF)
