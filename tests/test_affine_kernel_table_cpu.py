"""Which affine kernel a run gets (the two lists of swmi_affine.hip and the launchers' tables made from them)
without a GPU.  swmi_affine_sweep_name / swmi_affine_traceback_name return the name of the kernel a launcher would launch, null
where it refuses; swmi_affine_run_ok is aff_run_ok.  None of them calls HIP.

The expectation is a restatement of the selection the launchers made BEFORE the lists existed -- a chain of branches over tables
typed by signature -- written from the kernel-name grammar of the header comment of swmi_affine.hip, not from the lists:

  sweeps      sw_affine_sweep[2]_[long_|band_]<what>[_matrix][_wide]_kernel
              band, xdrop and band_adapt count for the long shape only, band_adapt only under a band; the first that applies of
                gap_open2            sweep2, what = global | extend
                subopt               what = hits (with option hits) | subopt
                end_bonus            what = endb
                band                 what = adapt[_xdrop] (band_adapt) | xdrop | the mode: "" | fit | global | extend
                xdrop                long_xdrop
                otherwise            the mode, and _long in place of a prefix
  tracebacks  an extend run is walked by global mode's kernels; gap_open2: traceback2_[long_|band_]global; under a band
              band_adapt_global (band_adapt) or band + the mode; otherwise [long] + the mode
"""
import ctypes as C
import itertools
import os
import re

import pytest

from affine_census import AffRun, load          # the ctypes struct and the three prototypes, shared with the census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("", "_fit", "_global", "_extend")


def _parent_sweep(r, long_reads, shape):
    band = r.band if long_reads else 0
    xdrop = r.xdrop if long_reads else 0
    adapt = r.adapt if band else 0
    pre = "band_" if band else "long_" if shape == 2 else ""
    matrix = "_matrix" if r.mat else ""
    wide = "_wide" if shape == 1 else ""
    if r.gap_open2:
        return "sw_affine_sweep2_%s%s%s_kernel" % (pre, MODES[r.mode][1:], wide)
    if r.subopt or r.end_bonus:
        what = ("hits" if r.hits else "subopt") if r.subopt else "endb"
        return "sw_affine_sweep_%s%s%s%s_kernel" % (pre, what, matrix, wide)
    if band:
        what = ("_adapt_xdrop" if xdrop else "_adapt") if adapt else "_xdrop" if xdrop else MODES[r.mode]
        return "sw_affine_sweep_band%s%s_kernel" % (what, matrix)
    if xdrop:
        return "sw_affine_sweep_long_xdrop%s_kernel" % matrix
    return "sw_affine_sweep%s%s%s%s_kernel" % ("_long" if shape == 2 else "", MODES[r.mode], matrix, wide)


def _parent_traceback(r, long_reads):
    mode = MODES[2 if r.mode == 3 else r.mode]
    band = long_reads and r.band
    if r.gap_open2:
        return "sw_affine_traceback2_%sglobal_kernel" % ("band_" if band else "long_" if long_reads else "")
    if band:
        return "sw_affine_traceback_band%s_kernel" % ("_adapt_global" if r.adapt else mode)
    return "sw_affine_traceback%s%s_kernel" % ("_long" if long_reads else "", mode)


@pytest.fixture(scope="module")
def lib():
    return load()


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


def test_every_run_gets_the_kernel_the_branch_chain_gave_it(lib):
    dummy = (C.c_uint32 * 1)()                                    # never dereferenced
    sweeps, tracebacks, points = set(), set(), 0
    for mode, mat, band, xdrop, adapt, gap_open2, subopt, hits, end_bonus, long_reads in itertools.product(
            (0, 1, 2, 3), (0, 1), (0, 64), (0, 50), (0, 1), (0, -6), (0, 5, -1), (0, 3), (0, 7), (0, 1)):
        r = AffRun(gap_open=-5, gap_open2=gap_open2, gap2=-1, mode=mode, band=band, xdrop=xdrop, adapt=adapt,
                   mat=C.addressof(dummy) if mat else None, nn=5 if mat else 0, cigar=0, subopt=subopt, hits=hits, end_bonus=end_bonus)
        ok = bool(lib.swmi_affine_run_ok(C.byref(r), long_reads))
        where = (mode, mat, band, xdrop, adapt, gap_open2, subopt, hits, end_bonus, long_reads)
        for shape in ((2,) if long_reads else (0, 1)):            # the shapes a launch can ask for
            name = lib.swmi_affine_sweep_name(C.byref(r), long_reads, shape)
            assert (name is not None) == ok, (where, shape, name)
            if name is not None:
                assert name.decode() == _parent_sweep(r, long_reads, shape), (where, shape)
                sweeps.add(name.decode())
        name = lib.swmi_affine_traceback_name(C.byref(r), long_reads)
        assert (name is not None) == ok, (where, name)
        if name is not None:
            assert name.decode() == _parent_traceback(r, long_reads), where
            tracebacks.add(name.decode())
        points += 1
    assert points == 3072
    # every listed kernel is some run's, no run gets a kernel outside the lists, and no row is there twice
    listed_sweeps, listed_tracebacks = _listed("AFF_SWEEPS"), _listed("AFF_TRACEBACKS")
    assert len(listed_sweeps) == 72 and len(listed_tracebacks) == 13
    assert len(sweeps) == 72 and sweeps == set(listed_sweeps)
    assert len(tracebacks) == 13 and tracebacks == set(listed_tracebacks)
