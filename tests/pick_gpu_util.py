"""What the GPU tests of options "subopt" and "hits" share (test_subopt_gpu, test_hits_gpu, test_pick_gpu) -- TEST INFRASTRUCTURE
ONLY.

Not collected by pytest (no test_ prefix), no fixtures.  Planted inputs (weaken, planted), the expected values of a batch from
tests/subopt_reference.py and tests/hits_reference.py (subopt_expect, hits_expect), the comparison of a batch with them through
the per-pair and the whole-batch accessors (subopt_check; hits_check_pair, hits_check), and a run with the comparison behind it
(subopt_run_and_check, hits_run_and_check)."""
import numpy as np

import sparksmithwaterman_amd as sw

import affine_gpu_util as u
import hits_reference as hr
import subopt_reference as sr

LOCAL = sw.ALIGN_LOCAL


def weaken(read, k, alphabet="ACGT"):
    """the read with k substitutions at evenly spaced places (each base replaced by the next one of the alphabet)"""
    out = list(read)
    for x in range(k):
        p = (2 * x + 1) * len(read) // (2 * k)
        out[p] = alphabet[(alphabet.index(out[p]) + 1) % len(alphabet)]
    return "".join(out)


def planted(rng, read, gaps, loads):
    """random stretches (lengths `gaps`, one more than copies) around copies of the read with `loads` substitutions each; the
    reference and the 1-based end column of every copy"""
    ref, ends = u.rand(rng, gaps[0]), []
    for g, load in zip(gaps[1:], loads):
        ref += weaken(read, load)
        ends.append(len(ref))
        ref += u.rand(rng, g)
    return ref, ends


# ---- option "subopt" ----------------------------------------------------------------------------------------------------------------
def subopt_expect(refs, reads, sc, w, band=0, matrix=None):
    return {(r, q): sr.subopt_numpy(refs[r], reads[q], sc, w, band, matrix) for r in range(len(refs)) for q in range(len(reads))}


def subopt_check(b, refs, reads, exp, what=None):
    """every pair: score, score2 and end2, through the per-pair and the whole-batch accessor"""
    s2, e2 = b.subopts()
    assert len(s2) == len(e2) == len(refs) * len(reads)
    for r in range(len(refs)):
        for q in range(len(reads)):
            pair = r * len(reads) + q
            got = (b.score(pair),) + b.subopt(pair)
            assert got == exp[(r, q)], (what, r, q, len(refs[r]), len(reads[q]), got, exp[(r, q)])
            assert (int(s2[pair]), int(e2[pair])) == got[1:], (what, pair)


def subopt_run_and_check(ctx, refs, reads, sc, w, band=None, matrix=None, tie=0, exp=None, **options):
    exp = exp or subopt_expect(refs, reads, sc, w, band or 0, matrix and (matrix.alphabet, matrix.scores))
    b = u.run(ctx, refs, reads, sc, tie, LOCAL, band, matrix=matrix, subopt=w, **options)
    subopt_check(b, refs, reads, exp, (w, band, tie))
    return b, exp


# ---- option "hits" ------------------------------------------------------------------------------------------------------------------
def hits_expect(refs, reads, sc, w, k, band=0, matrix=None):
    return {(r, q): hr.hits_numpy(refs[r], reads[q], sc, w, k, band, matrix) for r in range(len(refs)) for q in range(len(reads))}


def hits_check_pair(b, pair, want, k, what=None, cells=True):
    got = b.hits(pair)
    assert got == want, (what, pair, got, want)
    s2, e2 = b.subopt(pair)
    if len(got) >= 2:
        assert (got[1][0], got[1][2]) == (s2, e2), (what, pair)
    elif k >= 2:
        assert (s2, e2) == (0, 0), (what, pair)
    if got:
        assert b.score(pair) == got[0][0], (what, pair)
        if cells:
            assert got[0][1:] in [a[-1] for a in b.alignments(pair, with_cell=True)], (what, pair)
    else:
        assert b.score(pair) == 0


def hits_check(b, refs, reads, exp, k, what=None, cells=True):
    """every pair through the per-pair accessor, then the whole batch through the other one"""
    n = len(refs) * len(reads)
    for r in range(len(refs)):
        for q in range(len(reads)):
            hits_check_pair(b, r * len(reads) + q, exp[(r, q)], k, (what, r, q, len(refs[r]), len(reads[q])), cells)
    cnt, sc, ei, ej = b.hits_all()
    assert cnt.shape == (n,) and sc.shape == ei.shape == ej.shape == (n, 16) and sc.dtype == np.int32
    for r in range(len(refs)):
        for q in range(len(reads)):
            pair, want = r * len(reads) + q, exp[(r, q)]
            assert int(cnt[pair]) == len(want)
            assert [(int(sc[pair, x]), int(ei[pair, x]), int(ej[pair, x])) for x in range(16)] == want + [(0, 0, 0)] * (16 - len(want))


def hits_run_and_check(ctx, refs, reads, sc, w, k, band=None, matrix=None, tie=0, exp=None, cells=True, **options):
    exp = exp or hits_expect(refs, reads, sc, w, k, band or 0, matrix and (matrix.alphabet, matrix.scores))
    b = u.run(ctx, refs, reads, sc, tie, LOCAL, band, matrix=matrix, subopt=w, hits=k, **options)
    hits_check(b, refs, reads, exp, k, (w, k, band, tie), cells and not options.get("scores_only"))
    return b, exp
