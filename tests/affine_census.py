"""The census of the affine kernels (the two lists of swmi_affine.hip) -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  Shared by tests/test_affine_grid_gpu.py::test_census, which launches every listed
kernel and compares all it returns with the restatement that owns it, and by tests/test_affine_grid_cpu.py, which checks without a
GPU that the census is the lists and that the inputs below reach the kernel they are meant for.

  AffRun, load()            the launch descriptor of swmi_launch.h and the three entry points that name a run's kernels
  options_to_affrun         aff_run (swmi_run.cpp) restated: the descriptor of a run from the options a test sets
  census()                  one Entry per sweep kernel: the first admitted point of the option product with the traceback it implies
  inputs(entry)             the smallest run that launches the entry's kernel and makes its special path matter: two pairs
  expected(entry, tie)      what the restatement that owns the entry returns for the two pairs
  properties(entry)         the requirements on the inputs, asserted from the restatements alone

A new row of AFF_SWEEPS or AFF_TRACEBACKS needs an admitted run in PRODUCT and a recipe in inputs(): the CPU census test fails and
names the kernel otherwise."""
import collections
import ctypes as C
import itertools
import random

from sparksmithwaterman_amd import _capi

import adapt_reference as ar
import affine_grid_cases as gc
import end_bonus_reference as er
import gotoh_reference as gr
import hits_reference as hr
import subopt_reference as sr
import twopiece_reference as tr
import xdrop_reference as xr

LOCAL, FIT, GLOBAL, EXTEND = 0, 1, 2, 3          # AffRun.mode: 3 is option "extend" on a global run


class AffRun(C.Structure):
    """AffRun of swmi_launch.h"""
    _fields_ = [("gap_open", C.c_int32), ("gap_open2", C.c_int32), ("gap2", C.c_int32), ("mode", C.c_uint32), ("band", C.c_uint32),
                ("xdrop", C.c_uint32), ("adapt", C.c_uint32), ("mat", C.c_void_p), ("nn", C.c_uint32), ("cigar", C.c_uint32),
                ("subopt", C.c_int32), ("hits", C.c_uint32), ("end_bonus", C.c_uint32)]


_DUMMY = (C.c_uint32 * 1)()                      # a non-null matrix image: never dereferenced
_LIB = []


def load():
    """the library with the prototypes of swmi_affine_run_ok, swmi_affine_sweep_name and swmi_affine_traceback_name; none calls HIP"""
    if not _LIB:
        lib = _capi.load()
        lib.swmi_affine_run_ok.restype = C.c_int
        lib.swmi_affine_run_ok.argtypes = [C.POINTER(AffRun), C.c_uint32]
        lib.swmi_affine_sweep_name.restype = C.c_char_p
        lib.swmi_affine_sweep_name.argtypes = [C.POINTER(AffRun), C.c_uint32, C.c_uint32]
        lib.swmi_affine_traceback_name.restype = C.c_char_p
        lib.swmi_affine_traceback_name.argtypes = [C.POINTER(AffRun), C.c_uint32]
        _LIB.append(lib)
    return _LIB[0]


def dummy_matrix():
    return C.addressof(_DUMMY)


def options_to_affrun(options, matrix):
    """aff_run of swmi_run.cpp from a test's option dict (the names of set_option; what is absent is the context's default) and its
    score matrix, (alphabet, rows) or None"""
    o = options
    mode = o.get("align_mode", LOCAL)
    g2 = o.get("gap_open2", 0)
    return AffRun(gap_open=o.get("gap_open", 0), gap_open2=g2, gap2=o.get("gap2", 0) if g2 else 0,
                  mode=EXTEND if o.get("extend", 0) and mode == GLOBAL else mode,
                  band=o.get("band", 0), xdrop=o.get("xdrop", 0), adapt=o.get("band_adapt", 0),
                  mat=dummy_matrix() if matrix else None, nn=len(matrix[0]) + 1 if matrix else 0, cigar=o.get("cigar", 0),
                  subopt=o.get("subopt", 0), hits=o.get("hits", 0), end_bonus=o.get("end_bonus", 0))


def names(run, long_reads, shape):
    """(sweep, traceback) a launch of that shape gets, None where the launcher refuses"""
    lib = load()
    s, t = lib.swmi_affine_sweep_name(C.byref(run), long_reads, shape), lib.swmi_affine_traceback_name(C.byref(run), long_reads)
    return s and s.decode(), t and t.decode()


# the option product tests/test_affine_kernel_table_cpu.py walks: mode, matrix, band, xdrop, band_adapt, gap_open2, subopt, hits,
# end_bonus, long_reads
FIELDS = ("mode", "mat", "band", "xdrop", "adapt", "gap_open2", "subopt", "hits", "end_bonus", "long_reads")
PRODUCT = ((0, 1, 2, 3), (0, 1), (0, 64), (0, 50), (0, 1), (0, -6), (0, 5, -1), (0, 3), (0, 7), (0, 1))

Entry = collections.namedtuple("Entry", "sweep traceback point shape")     # point: dict over FIELDS; shape: 0 narrow, 1 wide, 2 long


def point_affrun(p):
    return AffRun(gap_open=-5, gap_open2=p["gap_open2"], gap2=-1, mode=p["mode"], band=p["band"], xdrop=p["xdrop"], adapt=p["adapt"],
                  mat=dummy_matrix() if p["mat"] else None, nn=5 if p["mat"] else 0, cigar=0, subopt=p["subopt"], hits=p["hits"],
                  end_bonus=p["end_bonus"])


_CENSUS = []


def census():
    """[Entry]: for every distinct sweep name the launchers give over the product, the first admitted point"""
    if not _CENSUS:
        seen = {}
        for values in itertools.product(*PRODUCT):
            p = dict(zip(FIELDS, values))
            for shape in ((2,) if p["long_reads"] else (0, 1)):
                sweep, traceback = names(point_affrun(p), p["long_reads"], shape)
                if sweep is not None and sweep not in seen:
                    assert traceback is not None, p
                    seen[sweep] = Entry(sweep, traceback, p, shape)
        _CENSUS.extend(seen.values())
    return list(_CENSUS)


# ---- the inputs --------------------------------------------------------------------------------------------------------------
M_OF_SHAPE = (100, 300, 1100)                   # R = 2, R = 5, two strips with 76 rows in the second
BAND = 32
SC = {False: (5, -3, -2, -6), True: (4, -3, -2, -6)}       # by matrix, as the grid's
SC_DROP = (2, -4, -2, -4)                       # xdrop: unrelated stretches lose score (tests/test_xdrop_gpu.py)
SC_TWO = (2, -3, -2, -4, -1, -12)               # two-piece: the pieces tie at a gap of 8 (tests/test_twopiece_gpu.py)
SUBOPT_W, HITS_K, END_BONUS = 10, 3, 5
Inputs = collections.namedtuple("Inputs", "family refs reads scores mode band extend matrix options")


def family(entry):
    p = entry.point
    return ("two" if p["gap_open2"] else "sub" if p["subopt"] else "endb" if p["end_bonus"] else "xdrop" if p["xdrop"] else
            "adapt" if p["adapt"] else "band" if p["band"] else "plain")


def _drifting(rng, read, draw, tail=30):
    """the long shape's reference under a band: a copy of the read without its bases 501 .. 540, so that from row 541 on the read
    meets a column 40 to the left -- at row 1025 a column left of the static window of half-width 32, 993 .."""
    return gc.mutate(rng, read[:500] + read[540:], draw, 0.03, 0.0) + gc.rand_seq(rng, tail, draw)


_INPUTS = {}


def inputs(entry):
    """the run of the entry: 2 pairs (2 references x 1 read, or 1 x 2), the scores, align_mode, band, extend, the matrix and the
    further options, as tests/affine_gpu_util.run takes them.  Deterministic: the seed comes from the kernel's name."""
    if entry.sweep in _INPUTS:
        return _INPUTS[entry.sweep]
    p, fam = entry.point, family(entry)
    lng = entry.shape == 2
    m = M_OF_SHAPE[entry.shape]
    matrix = gc.score_matrix() if p["mat"] else None
    draw = gc.MATRIX_DRAW if p["mat"] and fam != "xdrop" else gc.PLAIN_ALPHABET
    rng = random.Random(7600 + sum(map(ord, entry.sweep)))
    band = BAND if p["band"] else 0
    mode = GLOBAL if p["mode"] == EXTEND else p["mode"]
    options = {"long_reads": 1} if lng else {}
    sc = SC[bool(p["mat"])]
    read = gc.rand_seq(rng, m, draw)
    if fam == "xdrop":
        # one reference, two reads: the first leaves the reference after row 600 for a tail of T against unrelated bases, the
        # second follows it to the end -- past 40 columns the read lacks, so that its rows 1017 .. 1024 meet columns right of strip
        # 0's window (.. 1056) and the seam row's best column is not 1024; X lies between their differences at the first seam
        sc = SC_DROP
        ref = gc.mutate(rng, read[:900], draw, 0.03, 0.0) + gc.rand_seq(rng, 40, draw) + gc.mutate(rng, read[900:], draw, 0.03, 0.0) + "C" * 50
        refs, reads = [ref], [read[:600] + "T" * (m - 600), read]
        (b0, s0), (b1, s1) = (xr.drops(ref, q, sc, band, matrix)[0] for q in reads)
        assert b1 - s1 < b0 - s0 - 1, (entry.sweep, b0 - s0, b1 - s1)
        options["xdrop"] = b0 - s0 - 1
    elif fam == "two":
        # a run of 20 read bases the reference lacks, and a run of 20 (long shape: 60, which leaves strip 0's window) columns the read lacks
        sc = SC_TWO
        k = 60 if band else 20
        tail = gc.rand_seq(rng, 12, draw) if p["mode"] == EXTEND else ""
        refs = [read[:m // 3] + read[m // 3 + 20:] + tail, read[:m - 200 if lng else m // 2] + gc.rand_seq(rng, k, draw) + read[m - 200 if lng else m // 2:] + tail]
        reads = [read]
        options.update(gap_open2=sc[5], gap2=sc[4])
    elif fam == "sub":
        # a weaker copy of a stretch of the read, 30 or more unrelated columns, then a mutated copy of the whole read
        part = read[m // 10:m // 10 + (200 if lng else m // 2)]
        weak = gc.mutate(rng, part, draw, 0.12, 0.0)
        refs = [weak + gc.rand_seq(rng, 50, draw) + gc.mutate(rng, read, draw, 0.03, 0.004) + gc.rand_seq(rng, 20, draw),
                gc.rand_seq(rng, 9, draw) + gc.mutate(rng, read[:m - 11], draw, 0.05, 0.01) + gc.rand_seq(rng, 30, draw) + part]
        reads = [read]
        options["subopt"] = SUBOPT_W
        if p["hits"]:
            options["hits"] = HITS_K
    elif fam == "endb":
        # one reference runs on past the read's end, one ends 30 bases before it: the read's end costs a gap of 30 there
        body = read[:500] + read[540:m - 12] if band else read[:m - 12]          # (under a band: the drifting reference)
        # (its last 12 bases exact but the very last, a substitution that costs less than the bonus: the bonus decides)
        last = min((c for c in "ACGT" if -END_BONUS < gr.cell_score(c, read[-1], sc, matrix) < 0),
                   key=lambda c: gr.cell_score(c, read[-1], sc, matrix))
        refs = [gc.mutate(rng, body, draw, 0.04, 0.0) + read[m - 12:m - 1] + last + gc.rand_seq(rng, 20, draw),
                gc.mutate(rng, read[:m - 30], draw, 0.04, 0.0)]
        reads = [read]
        options["end_bonus"] = END_BONUS
    elif band:
        # (band and adapt) the drifting reference, and one with 60 columns more at its start: the read's last rows of strip 0 meet
        # columns right of its window, .. 1056
        refs = [_drifting(rng, read, draw), gc.rand_seq(rng, 60, draw) + gc.mutate(rng, read, draw, 0.03, 0.0) + gc.rand_seq(rng, 20, draw)]
        reads = [read]
        if p["adapt"]:
            options["band_adapt"] = 1
    else:
        refs = [gc.rand_seq(rng, 11, draw) + gc.mutate(rng, read, draw, 0.05, 0.01) + gc.rand_seq(rng, 20, draw),
                gc.mutate(rng, read[5:m - 20], draw, 0.04, 0.01) + gc.rand_seq(rng, 25, draw)]
        reads = [read]
    if fam == "xdrop" and p["adapt"]:
        options["band_adapt"] = 1
    assert len(refs) * len(reads) == 2 and all(len(q) == m for q in reads)
    _INPUTS[entry.sweep] = Inputs(fam, refs, reads, sc, mode, band, int(p["mode"] == EXTEND), matrix, options)
    return _INPUTS[entry.sweep]


def run_options(inp):
    """every option of the run by its set_option name (what options_to_affrun reads)"""
    return dict(inp.options, gap_open=inp.scores[3], align_mode=inp.mode, band=inp.band, extend=inp.extend)


def launch_of(inp):
    """(long_reads, shape) of the launch the run's pairs go to: all of them to one"""
    got = {(1, 2) if len(q) > 1024 else (0, 0 if gc.rows_per_lane(len(q)) <= 4 else 1) for q in inp.reads}
    assert len(got) == 1 and (inp.options.get("long_reads") or all(len(q) <= 1024 for q in inp.reads))
    return got.pop()


def pairs(inp):
    """[(ref, read)] in the batch's order"""
    return [(ref, read) for ref in inp.refs for read in inp.reads]


# ---- the expected values -----------------------------------------------------------------------------------------------------
# the restatement that owns each kind of run, as (numpy form, plain-loop form)
_TWO = (tr.align_numpy, tr.align_scalar)
_ADAPT = (ar.align, ar.align_scalar)
_XDROP = (xr.align, xr.align_scalar)
_ENDB = (er.align, er.align_scalar)
_ALIGN = (gr.align_numpy, gr.align_scalar)
_SUBOPT = (lambda ref, read, sc, width, w, tie, mat: sr.subopt_numpy(ref, read, sc, width, w, mat), sr.subopt_scalar)
_HITS = (lambda ref, read, sc, width, k, w, tie, mat: hr.hits_numpy(ref, read, sc, width, k, w, mat), hr.hits_scalar)
_EXPECTED = {}


def _pair_values(inp, ref, read, tie, w, adapt, scalar):
    m, n, sc, mat, X = len(read), len(ref), inp.scores, inp.matrix, inp.options.get("xdrop", 0)
    e = {"windows": gr.windows(m, n, w), "rows_swept": m}
    if inp.family == "two":
        e["align"] = _TWO[scalar](ref, read, sc, GLOBAL, w, bool(inp.extend), tie, cells=True)
    elif adapt:
        res = _ADAPT[scalar](ref, read, sc, w, X, tie, mat)
        e.update(align=res[:3], windows=res[3], rows_swept=res[4] if X else m)
    elif inp.family == "xdrop":
        res = _XDROP[scalar](ref, read, sc, X, w, tie, mat)
        e.update(align=res[:3], rows_swept=res[3], windows=e["windows"][:(res[3] + 1023) // 1024])
    elif inp.family == "endb":
        score, alns, cells, took, ends = _ENDB[scalar](ref, read, sc, inp.options["end_bonus"], w, tie, mat)
        e.update(align=(score, alns, cells), taken=took, ends=ends)
    else:
        e["align"] = _ALIGN[scalar](ref, read, sc, inp.mode, w, bool(inp.extend), tie, mat, cells=True)
        if inp.family == "sub":
            e["subopt"] = _SUBOPT[scalar](ref, read, sc, inp.options["subopt"], w, tie, mat)
            assert e["subopt"][0] == e["align"][0]
            if "hits" in inp.options:
                e["hits"] = _HITS[scalar](ref, read, sc, inp.options["subopt"], inp.options["hits"], w, tie, mat)
    return e


def expected(entry, tie, band=None):
    """[one dict per pair]: "align" = (score, alignments, cells), "rows_swept" and "windows" = the column windows of the strips swept
    always, and the option's own values: "subopt" = (score, score2, end2), "hits" = the list, "ends" = (max_score, end_score,
    end_col) with "taken".  band: another half-width than the run's (0: the same run without its band; the run's: the static
    windows in place of the adaptive ones)"""
    key = (entry.sweep, tie, band)
    if key not in _EXPECTED:
        inp = inputs(entry)
        w = inp.band if band is None else band
        adapt = bool(inp.options.get("band_adapt")) and band is None
        _EXPECTED[key] = [_pair_values(inp, ref, read, tie, w, adapt, False) for ref, read in pairs(inp)]
    return _EXPECTED[key]


def expected_scalar(entry, tie, only=None):
    """expected() from the plain-loop forms of the restatements (the CPU test holds a sample of entries to it); only: the index of
    the one pair to compute, None in the place of the other"""
    inp = inputs(entry)
    return [_pair_values(inp, ref, read, tie, inp.band, bool(inp.options.get("band_adapt")), True) if only in (None, x) else None
            for x, (ref, read) in enumerate(pairs(inp))]


# ---- the requirements on the inputs ------------------------------------------------------------------------------------------
def properties(entry):
    """asserts, from the restatements alone, that the entry's inputs make its options matter: the band cuts the result, xdrop stops one pair and
    not the other, band_adapt moves strip 1's window, piece 2 is the cheaper one, a runner-up lies outside the mask, the bonus decides"""
    inp, what = inputs(entry), entry.sweep
    exp = expected(entry, 0)
    if inp.band:
        # band: the banded result differs from the unbanded one
        assert [e["align"] for e in exp] != [e["align"] for e in expected(entry, 0, 0)], what
        assert all(len(e["windows"]) == 2 or e["rows_swept"] == 1024 for e in exp), what
    if "xdrop" in inp.options:
        # xdrop: one pair stops at the first seam, after its tail has diverged around row 600, and one does not stop
        assert [e["rows_swept"] for e in exp] == [1024, len(inp.reads[1])], what
        assert all(i <= 640 for i, _ in exp[0]["align"][2]), what
    if inp.options.get("band_adapt"):
        # band_adapt: strip 1's window differs from the static one
        moved = [e["windows"] for e in exp if len(e["windows"]) == 2]
        static = [e["windows"] for e in expected(entry, 0, inp.band) if len(e["windows"]) == 2 and e["rows_swept"] > 1024]
        assert moved and all(a[0] == s[0] for a, s in zip(moved, static)) and any(a[1] != s[1] for a, s in zip(moved, static)), what
    if inp.family == "two":
        # gap_open2: a gap long enough that piece 2 is the cheaper one, of either kind, and the one-piece result differs
        for e, side in zip(exp, (0, 1)):
            assert all("_" * 20 in al[1][side] for al in e["align"][1]), what
        for (ref, read), e in zip(pairs(inp), exp):
            one = gr.align_numpy(ref, read, inp.scores[:4], GLOBAL, inp.band, bool(inp.extend), 0, None, cells=True)
            assert one[0] < e["align"][0], what
        assert tr.gap_cost(20, inp.scores) == inp.scores[5] + 20 * inp.scores[4] > inp.scores[3] + 20 * inp.scores[2]
    if inp.family == "sub":
        # subopt / hits: a second, weaker copy more than w columns away
        w = inp.options["subopt"]
        for e in exp:
            s, s2, end2 = e["subopt"]
            assert 0 < s2 < s and all(abs(end2 - c[1]) > w for c in e["align"][2]), what
        if "hits" in inp.options:
            assert all(len(e["hits"]) >= 2 and e["hits"][1][0::2] == e["subopt"][1:] for e in exp), what
            assert any(len({h[1] for h in e["hits"]}) >= 2 for e in exp), what
    if inp.family == "endb":
        # end_bonus: one pair taken to the end and one not
        assert [e["taken"] for e in exp] == [True, False] and exp[0]["ends"][1] < exp[0]["ends"][0], what
