"""The pairs of the long-read tests (option "long_reads": reads of more than 1024 bases on the affine kernels, swept in strips
of 1024 rows), shared by tests/test_long_reads_gpu.py and tests/test_long_reads_cpu.py.  Every case is (name, ref, read, scores)
with scores = (match, mismatch, gap, gap_open); rows are 1-based read positions, the seam lies between rows 1024 and 1025."""
import random

STRIP = 1024


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def seam_cases():
    """case 2 of the issue: alignments that cross the seam, and tied maxima on both sides of it"""
    rng = random.Random(8202)
    sc = (5, -3, -2, -6)
    out = []
    ref = rand_seq(rng, 150)
    # (a) a diagonal over rows 985 .. 1064
    out.append(("diagonal", ref, rand_seq(rng, 984, "AT") + ref[30:110] + rand_seq(rng, 30, "AT"), sc))
    # (b) 100 matching bases (rows 910 .. 1009), 40 inserted ones (rows 1010 .. 1049: the F extension bit is read across the
    #     seam), 100 matching bases
    ref_b = rand_seq(rng, 260, "ACG")
    read_b = rand_seq(rng, 909, "T") + ref_b[20:120] + "T" * 40 + ref_b[120:220] + rand_seq(rng, 25, "T")
    out.append(("insertion", ref_b, read_b, (2, -3, -1, -6)))
    # (c) 12 reference bases deleted after read row 1024 (the run lies in row 1024), and after row 1025
    ref_c = rand_seq(rng, 200)
    for name, at in (("deletion_row_1024", 1024), ("deletion_row_1025", 1025)):
        out.append((name, ref_c, rand_seq(rng, at - 60, "AT") + ref_c[20:80] + ref_c[92:160] + rand_seq(rng, 11, "AT"), sc))
    # (d) X + 1100 other bases + X against X: one maximum in strip 0, its tie in strip 1; (e) a mismatch in the first X: the
    #     later strip's maximum is higher and resets the list; (f) in the second X: it is lower and the list stays
    x = rand_seq(rng, 64, "ACG")
    mid = rand_seq(rng, 1100, "T")
    bad = x[:31] + _other(x[31]) + x[32:]
    out.append(("ties_both_strips", x, x + mid + x, sc))
    out.append(("later_strip_higher", x, bad + mid + x, sc))
    out.append(("later_strip_lower", x, x + mid + bad, sc))
    return out


FIT, GLOBAL = 1, 2


def ends_cases():
    """case 4 of the issue: (name, ref, read, scores, mode); the last one hangs the read's head over the reference start
    from row 1100, in strip 1"""
    rng = random.Random(8204)
    sc = (5, -3, -2, -6)
    out = []
    for m in (1025, 2049):
        for n in (300, 700):
            ref = rand_seq(rng, n)
            read = list(rand_seq(rng, m))
            at = m - n // 2 - 40                                 # (half of the reference planted near the read's end)
            read[at:at + n // 2] = ref[n // 4:n // 4 + n // 2]
            out.append(("fit_%d_%d" % (m, n), ref, "".join(read), sc, FIT))
        for n in (300, 2500):
            ref = rand_seq(rng, n)
            read = list(rand_seq(rng, m))
            k = min(m, n) // 2
            read[m - k:] = ref[n - k:]
            out.append(("global_%d_%d" % (m, n), ref, "".join(read), sc, GLOBAL))
    ref = rand_seq(rng, 300, "ACG")
    out.append(("fit_head_overhang", ref, "T" * 1100 + ref[:200], sc, FIT))
    return out
