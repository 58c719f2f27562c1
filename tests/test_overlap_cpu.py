"""Overlap (ends-free) alignment (option "overlap" on a fit run) without a GPU: the two restatements of the
contract in tests/overlap_reference.py against each other, against a brute force over global alignments of spans and against
properties that hold by construction; the recipes of tests/overlap_cases.py, each held to what it is built for, the two restatements
against each other on them and every alignment re-scored; which kernels the launchers give a mode-4 run (the second pair of lists of swmi_affine.hip);
the host mirror's overlap keyword on a fake context and the driver's --overlap argument."""
import ctypes as C
import itertools
import os
import random
import re

import pytest

import affine_grid_cases as gc
import gotoh_reference as gr
import overlap_cases as oc
import overlap_reference as ov
from affine_census import AffRun, dummy_matrix, load
from test_ends_cpu import _FakeContext, _matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAP = 4                                      # AffRun.mode of an overlap run


def _pairs(seed, count, max_len=12):
    rng = random.Random(seed)
    for _ in range(count):
        alpha = rng.choice(["AC", "ACGT", "A"])
        ref = "".join(rng.choice(alpha) for _ in range(rng.randint(1, max_len)))
        read = "".join(rng.choice(alpha) for _ in range(rng.randint(1, max_len)))
        sc = (rng.randint(0, 4), rng.randint(-4, 1), rng.randint(-3, 0), rng.randint(-4, 0))
        yield ref, read, sc


def _check_alignments(ref, read, sc, got, matrix=None):
    """every alignment spells a span that starts in row 0 or column 0 and ends in its cell, and rescores to the pair's score"""
    score, alns, cells = got
    m, n = len(read), len(ref)
    assert len(alns) == len(cells) >= 1 and len(set(cells)) == len(cells)
    for aln, (i, j) in zip(alns, cells):
        assert (i == m and 1 <= j <= n) or (j == n and 1 <= i <= m)
        begin, (ra, qa) = aln
        assert len(ra) == len(qa) >= 1
        assert gr.rescore(ra, qa, sc, matrix) == score, (ref, read, sc, aln)
        first, end_i, b, end_j = ov.span((i, j), aln)
        assert (end_i, end_j, b) == (i, j, begin)
        assert qa.replace("_", "") == read[first - 1:i]
        used = ra.replace("_", "")
        j0 = j - len(used)
        assert used == ref[j0:j] and begin == (j0 + 1 if used else j)
        assert first == 1 or j0 == 0, (ref, read, sc, aln)


@pytest.mark.parametrize("tie", [0, 1])
def test_restatements_agree_and_alignments_rescore(tie):
    for ref, read, sc in _pairs(300 + tie, 500):
        got = ov.align_scalar(ref, read, sc, tie_mode=tie, strip=8, cells=True)
        assert ov.align_numpy(ref, read, sc, tie_mode=tie, strip=8, cells=True) == got, (ref, read, sc)
        assert ov.align_numpy(ref, read, sc, tie_mode=tie, strip=8) == got[:2]
        _check_alignments(ref, read, sc, got)
    assert ov.align_scalar("", "ACG", (1, -1, -1, -1), cells=True) == ov.align_numpy("", "ACG", (1, -1, -1, -1), cells=True) == (0, [], [])
    assert ov.align_scalar("ACG", "", (1, -1, -1, -1)) == ov.align_numpy("ACG", "", (1, -1, -1, -1)) == (0, [])


def test_restatements_agree_with_a_matrix():
    m = _matrix("BLOSUM62")
    rng = random.Random(305)
    for _ in range(80):
        ref = "".join(rng.choice(m[0][:20] + "z") for _ in range(rng.randint(1, 20)))
        read = "".join(rng.choice(m[0][:20] + "z") for _ in range(rng.randint(1, 20)))
        sc = (1, -1, rng.randint(-2, 0), rng.randint(-11, 0))
        for tie in (0, 1):
            got = ov.align_scalar(ref, read, sc, tie_mode=tie, matrix=m, strip=8, cells=True)
            assert ov.align_numpy(ref, read, sc, tie_mode=tie, matrix=m, strip=8, cells=True) == got
            _check_alignments(ref, read, sc, got, m)


# scores under which an alignment that consumes no base of one side never wins (mismatch > gap_open + gap), and scores under which
# it may (tests/gotoh_reference.py scores a pair with an empty side as 0 without an alignment, so such spans are scored by formula)
_BRUTE_SCORES = [((2, -1, -1, -1), False), ((1, -1, 0, -2), False), ((3, -2, -1, 0), True), ((1, -4, -1, 0), True), ((0, -3, -1, -1), True)]


@pytest.mark.parametrize("sc,gap_only", _BRUTE_SCORES)
def test_brute_force_over_global_alignments_of_spans(sc, gap_only):
    """all pairs with m, n <= 3 and a sample of the longer ones over {A, C}: the score is the largest global score of
    ref[j0:j] against read[i0:i] over the starts with i0 == 0 or j0 == 0 and the ends in C, both sides non-empty"""
    rng = random.Random(310 + sum(sc))
    seqs = ["".join(p) for k in range(1, 4) for p in itertools.product("AC", repeat=k)]
    pairs = [(a, b) for a in seqs for b in seqs]
    pairs += [("".join(rng.choice("AC") for _ in range(rng.randint(4, 7))), "".join(rng.choice("AC") for _ in range(rng.randint(1, 7)))) for _ in range(60)]
    pairs += [(b, a) for a, b in pairs[-60:]]
    e, o = sc[2], sc[3]
    won_by_gap = 0
    for ref, read in pairs:
        m, n = len(read), len(ref)
        ends = [(i, n) for i in range(1, m)] + [(m, j) for j in range(1, n + 1)]
        best = None
        for i, j in ends:
            for i0, j0 in [(0, x) for x in range(j)] + [(x, 0) for x in range(1, i)]:
                g = gr.align_scalar(ref[j0:j], read[i0:i], sc, gr.GLOBAL)[0]
                best = g if best is None else max(best, g)
        # the spans with an empty side: read[0:i] inserted at column j, ref[0:j] deleted at row i
        gap_best = max([o + i * e for i, _ in ends] + [o + j * e for _, j in ends])
        for tie in (0, 1):
            got = ov.align_scalar(ref, read, sc, tie_mode=tie, cells=True)
            if gap_only:
                assert got[0] == max(best, gap_best), (ref, read, sc)
                won_by_gap += got[0] > best
            else:
                assert got[0] == best >= gap_best, (ref, read, sc)
            _check_alignments(ref, read, sc, got)
            for aln, (i, j) in zip(got[1], got[2]):             # ... and a best global alignment of its span, where that has two sides
                first, _, begin, _ = ov.span((i, j), aln)
                sub_ref, sub_read = ref[begin - 1:j] if aln[1][0].replace("_", "") else "", read[first - 1:i]
                if sub_ref and sub_read:
                    assert gr.align_scalar(sub_ref, sub_read, sc, gr.GLOBAL)[0] == got[0]
    assert bool(won_by_gap) == gap_only


@pytest.mark.parametrize("tie", [0, 1])
def test_overlap_ge_fit_both_ways(tie):
    for ref, read, sc in _pairs(320 + tie, 400):
        got = ov.align_numpy(ref, read, sc, tie_mode=tie)[0]
        assert got >= gr.align_scalar(ref, read, sc, gr.FIT, tie_mode=tie)[0], (ref, read, sc)
        assert got >= gr.align_scalar(read, ref, sc, gr.FIT, tie_mode=tie)[0], (ref, read, sc)      # the roles swapped
        assert got <= gr.align_numpy(ref, read, sc, gr.LOCAL, tie_mode=tie)[0] or got <= 0


def test_corner_is_listed_once_and_order():
    sc = (1, -3, -2, -2)
    for tie in (0, 1):
        score, alns, cells = ov.align_scalar("ACAC" * 3, "ACAC" * 2, sc, tie_mode=tie, cells=True)
        assert score == 8 and cells.count((8, 12)) == 1 and len(cells) == len(set(cells)) == 3
        assert sorted(cells) == [(8, 8), (8, 10), (8, 12)]
        # row m and column n tie at once: the read's tail against the reference's head, and the reverse
        score, alns, cells = ov.align_scalar("AAAA", "AAAA", sc, tie_mode=tie, cells=True)
        assert score == 4 and cells == [(4, 4)]
        score, alns, cells = ov.align_scalar("AAAA", "AAAA", (0, -3, -2, -2), tie_mode=tie, cells=True)
        assert score == 0 and sorted(cells) == [(1, 4), (2, 4), (3, 4), (4, 1), (4, 2), (4, 3), (4, 4)]
        if tie == 0:
            assert cells == sorted(cells)                                   # row-major
        else:
            assert [c for c in cells] == sorted(cells, key=lambda c: (alns[cells.index(c)][0],))     # stably by begin
    # a non-competing cell that holds the maximum's value is not listed: H(2, 2) = 2 = the score, reached again in column n only
    score, alns, cells = ov.align_scalar("ACGAC", "ACT", (1, -3, -1, 0), cells=True)
    assert (score, cells) == (2, [(2, 5)])
    H = ov.align_scalar("ACGAC", "ACT", (1, -3, -1, 0), matrices=True)[2]
    assert H[2][2] == 2


# ---- the recipes of tests/overlap_cases.py: what each is built for, on the restatements alone ----
def test_tie_sets_restatements_agree_and_hold_their_ties():
    """6 sets x 64 pairs x 2 tie modes: the numpy form is the scalar one on all 768 runs; every set has pairs beyond cell_cap = 8,
    sets 3 and 5 have alignments that start with a gap, set 3 never scores above 0"""
    runs = 0
    for sc, refs, reads in oc.tie_sets():
        assert len(refs) == len(reads) == 8
        for tie in (0, 1):
            for ref in refs:
                for read in reads:
                    got = oc.want(ref, read, sc, tie)
                    assert got == ov.align_scalar(ref, read, sc, tie_mode=tie, cells=True), (sc, ref, read, tie)
                    _check_alignments(ref, read, sc, got)
                    runs += 1
    assert runs == 768
    counts = oc.check_tie_sets()
    assert all(c[0] >= 10 for c in counts) and counts[2][1] >= 20 and counts[4][1] >= 20 and counts[2][2] <= 0, counts


@pytest.mark.parametrize("matrix", [False, True])
def test_walk_pairs_keep_their_runs_with_all_four_ends_free(matrix):
    """the cut walk grid: every pair's overlap alignment is not its fit alignment, keeps both planted runs, ends on row m left of
    the corner and starts at column 0 below row 1; the uncut pair ends at the corner.  Classes R <= 4 against the scalar form."""
    mat = oc.matrix_of(matrix)
    for tie in (0, 1):
        assert oc.check_walk_pairs(matrix, tie) == 16
        for (R, ref, read), (_, whole_ref, whole_read) in zip(oc.walk_pairs(matrix), gc.walk_grid(matrix)):
            for a, b in ((ref, read), (whole_ref, whole_read)):
                got = oc.want(a, b, gc.WALK_SCORES, tie, mat)
                _check_alignments(a, b, gc.WALK_SCORES, got, mat)
                if R <= 4:
                    assert got == ov.align_scalar(a, b, gc.WALK_SCORES, tie_mode=tie, matrix=mat, cells=True), (R, tie)


@pytest.mark.parametrize("tie", [0, 1])
def test_long_read_recipes(tie):
    """the seam cases and the tied maxima over both strips and row m"""
    oc.check_seam_cases(tie)
    for name, ref, read, sc, span in oc.seam_cases():
        _check_alignments(ref, read, sc, oc.want(ref, read, sc, tie))
    oc.check_long_tie_case(tie)
    ref, read = oc.long_tie_case()
    _check_alignments(ref, read, oc.LONG_TIE_SCORES, oc.want(ref, read, oc.LONG_TIE_SCORES, tie))


def test_bound_recipes():
    """every score of the restatement (int64 sums) fits int32, one set ties in more than 64 cells, the two known answers"""
    oc.check_bound_cases()
    for name, ref, read, sc in oc.bound_cases():
        for tie in (0, 1):
            _check_alignments(ref, read, sc, oc.want(ref, read, sc, tie))
    S = oc.LONG_S_OK
    for name, ref, read in oc.long_bound_cases():
        assert len(read) == 2049
        _check_alignments(ref, read, (S, -S, -S, -S), oc.want(ref, read, (S, -S, -S, -S)))


def _listed(macro):
    """the kernel names of the rows of a list of swmi_affine.hip, in order"""
    with open(os.path.join(ROOT, "sparksmithwaterman_amd", "csrc", "swmi_affine.hip")) as f:
        src = f.read()
    body = src[src.index("#define %s(X)" % macro):]
    rows = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*X\((sw_affine_\w+),", line)
        if not m:
            break
        rows.append(m.group(1))
    return rows


def _affrun(mat=0, **kw):
    base = dict(gap_open=-5, gap_open2=0, gap2=0, mode=OVERLAP, band=0, xdrop=0, adapt=0, mat=dummy_matrix() if mat else None,
                nn=5 if mat else 0, cigar=0, subopt=0, hits=0, end_bonus=0)
    base.update(kw)
    return AffRun(**base)


def test_mode_4_gets_the_overlap_kernels():
    """fails on a library without the feature: mode 4 is refused there"""
    lib = load()
    sweeps, walks = [], []
    for mat in (0, 1):
        for long_reads, shape in ((0, 0), (0, 1), (1, 2)):
            r = _affrun(mat)
            assert lib.swmi_affine_run_ok(C.byref(r), long_reads) == 1
            s = lib.swmi_affine_sweep_name(C.byref(r), long_reads, shape)
            t = lib.swmi_affine_traceback_name(C.byref(r), long_reads)
            assert s is not None and t is not None, (mat, long_reads, shape)
            sweeps.append(s.decode())
            walks.append(t.decode())
            want = "sw_affine_sweep_%soverlap%s%s_kernel" % ("long_" if shape == 2 else "", "_matrix" if mat else "", "_wide" if shape == 1 else "")
            assert s.decode() == want and t.decode() == "sw_affine_traceback_%soverlap_kernel" % ("long_" if long_reads else "")
    listed_sweeps, listed_walks = _listed("AFF_OVERLAP_SWEEPS"), _listed("AFF_OVERLAP_TRACEBACKS")
    assert len(listed_sweeps) == 6 and len(listed_walks) == 2
    assert sorted(sweeps) == sorted(listed_sweeps) and set(walks) == set(listed_walks)
    assert not set(listed_sweeps) & set(_listed("AFF_SWEEPS")) and not set(listed_walks) & set(_listed("AFF_TRACEBACKS"))
    # the cigar payload is the walk's, whatever the mode
    for cigar in (1, 2):
        r = _affrun(cigar=cigar)
        assert lib.swmi_affine_run_ok(C.byref(r), 0) == 1 and lib.swmi_affine_traceback_name(C.byref(r), 0).decode() == "sw_affine_traceback_overlap_kernel"


@pytest.mark.parametrize("option", [dict(band=64), dict(xdrop=50), dict(adapt=1), dict(band=64, adapt=1), dict(gap_open2=-6, gap2=-1),
                                    dict(subopt=5), dict(subopt=-1, hits=3), dict(hits=3), dict(end_bonus=7)])
def test_mode_4_takes_no_other_option(option):
    lib = load()
    for mat in (0, 1):
        for long_reads, shape in ((0, 0), (0, 1), (1, 2)):
            r = _affrun(mat, **option)
            assert lib.swmi_affine_run_ok(C.byref(r), long_reads) == 0, (option, mat, long_reads)
            assert lib.swmi_affine_sweep_name(C.byref(r), long_reads, shape) is None
            assert lib.swmi_affine_traceback_name(C.byref(r), long_reads) is None
    r = _affrun(mode=5)
    assert lib.swmi_affine_run_ok(C.byref(r), 0) == 0 and lib.swmi_affine_sweep_name(C.byref(r), 0, 0) is None


def test_mirror_takes_overlap_keyword():
    import inspect
    import sparksmithwaterman_amd as sw
    from sparksmithwaterman_amd import sw as mirror
    for cls in (mirror.SmithWaterman.OptAlignments, mirror.Distribution.MapPartition, mirror.Distribution.MapRef, mirror._FileDriver):
        assert "overlap" in inspect.signature(cls.__init__).parameters, cls
    c = _FakeContext()
    assert sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_FIT, overlap=True).call(["ACGT", "CG"], [5, -3, -4, -6]) == (-4, [])
    assert c.log == [("set_option", "gap_open", -6), ("set_option", "align_mode", 1), ("set_option", "overlap", 1), ("upload",),
                     ("run", (5, -3, -4)), ("free",), ("set_option", "overlap", 0), ("set_option", "align_mode", 0), ("set_option", "gap_open", 0)]
    c = _FakeContext()
    c.options["overlap"] = 1                                    # the context's own setting comes back after the call
    sw.DistributedSW.OptAlignments(c, overlap=False).call(["ACGT", "CG"], [5, -3, -4])
    assert c.log == [("set_option", "overlap", 0), ("upload",), ("run", (5, -3, -4)), ("free",), ("set_option", "overlap", 1)]
    c = _FakeContext()
    sw.Distribution.MapRef(c, align_mode=sw.ALIGN_FIT, overlap=True).call(((">r", "ACGT"), ["CG"], ([2, -1, -1], ["a", "i", "d", "-"])))
    assert c.log[:2] == [("set_option", "align_mode", 1), ("set_option", "overlap", 1)] and c.log[-2:] == [("set_option", "overlap", 0), ("set_option", "align_mode", 0)]
    c = _FakeContext()
    sw.SmithWaterman.OptAlignments(c).call(["ACGT", "CG"], [5, -3, -4])
    assert not any(e[0] == "set_option" for e in c.log)         # no keyword: the context's options are left alone
    for bad in (1, 0, "yes", 2):
        c = _FakeContext()
        with pytest.raises(ValueError):
            sw.SmithWaterman.OptAlignments(c, align_mode=sw.ALIGN_FIT, overlap=bad).call(["ACGT", "CG"], [5, -3, -4])
        assert c.log == []                                       # rejected before anything reaches the library


def test_sharded_files_parser_overlap_needs_fit(capsys):
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "R", "--in-dir", "I", "--out-dir", "O"]
    assert sharded_files._parser().parse_args(base).overlap is False
    args = sharded_files._parser().parse_args(base + ["--align-mode", "fit", "--overlap", "--long-reads", "--scores", "5,-3,-2,-6"])
    assert args.overlap is True and args.align_mode == "fit" and args.long_reads is True
    for mode in ([], ["--align-mode", "local"], ["--align-mode", "global"]):
        with pytest.raises(SystemExit) as e:
            sharded_files._parser().parse_args(base + mode + ["--overlap"])
        assert e.value.code == 2                                  # an argparse error
        assert "--overlap requires --align-mode fit" in capsys.readouterr().err
    for more in (["--band", "64", "--long-reads"], ["--scores", "5,-3,-2,-6,-1,-12"]):
        with pytest.raises(SystemExit):
            sharded_files._parser().parse_args(base + ["--align-mode", "fit", "--overlap"] + more)
        assert "--overlap is not built for --band or two-piece gaps" in capsys.readouterr().err


def test_span_helper_is_bound():
    from sparksmithwaterman_amd.aligner import Batch
    assert callable(Batch.span)
    assert ov.span((5, 9), (7, ("ACG", "A_G"))) == (4, 5, 7, 9)
