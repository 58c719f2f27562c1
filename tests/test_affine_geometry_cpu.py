"""How big a mode-3 pair's workspace is (AffGeom and swmi_aff_pair_dir_words / _seam_words / _table_off of swmi_device.h, DESIGN.md
section 8k) without a GPU: the three functions, compiled into a host program of their own, against a Python restatement built on
gotoh_reference.windows, on a grid of (m, n, w) in the five classes -- short reads, long reads unbanded, under a band, under a
band with two-piece gaps, under an adaptive band."""
import os
import subprocess

import gotoh_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 64, 65, 1024, 1025, 2048, 2049, 3000, 4097)
NS = (1, 8, 1000, 1100, 2100, 5000)
WS = (0, 1, 100, 1024, 2000)

PROGRAM = r'''
#include <cstdio>
#include <hip/hip_runtime.h>
#include "swmi_device.h"
int main() {
    unsigned m, n, w, adapt, two;
    while (scanf("%u %u %u %u %u", &m, &n, &w, &adapt, &two) == 5) {
        const AffGeom g{w, adapt != 0, two != 0};
        printf("%llu %llu %llu\n", (unsigned long long)swmi_aff_pair_dir_words(m, n, g), (unsigned long long)swmi_aff_pair_seam_words(m, n, g),
               (unsigned long long)swmi_aff_pair_table_off(m, n, g));
    }
    return 0;
}
'''


def _strip_field(cols):
    """dwords of the field of one strip whose window has `cols` columns: (cols + 70) // 8 blocks of 16 row slots x 64 lanes"""
    return (cols + 70) // 8 * 16 * 64


def _want(m, n, w, adapt, two):
    """(dir_words, seam_words, table_off)"""
    planes = 2 if two else 1
    if m <= 1024:                                                 # one strip: R rows per lane, the lanes that own rows, no seam row
        rows = max(1, (m + 63) // 64)
        lanes = (m + rows - 1) // rows
        field = planes * ((n + lanes - 1 + 7) // 8) * rows * 64
        return field, 0, field
    strips = (m + 1023) // 1024
    seam = (4 if two else 2) * n
    if adapt:                                                     # a fixed stride, and the window table rounded up to 64 dwords
        field = strips * _strip_field(min(n, 1024 + 2 * w))
        return field + (strips + 63) // 64 * 64, seam, field
    field = planes * sum(_strip_field(hi - lo + 1) for lo, hi in gr.windows(m, n, w))
    return field, seam, field


def _cases():
    """[(class, m, n, w, adapt, two)]; a static band with an empty window is left out: the host refuses it"""
    cases = []
    for m in MS:
        for n in NS:
            for w in WS:
                if m <= 1024:
                    cases += [("short", m, n, w, adapt, two) for adapt, two in ((0, 0), (0, 1), (1 if w else 0, 0))]
                elif w == 0:
                    cases += [("unbanded", m, n, 0, 0, 0), ("unbanded", m, n, 0, 0, 1)]
                else:
                    cases.append(("band+adapt", m, n, w, 1, 0))
                    if all(lo <= hi for lo, hi in gr.windows(m, n, w)):
                        cases += [("band", m, n, w, 0, 0), ("band+two", m, n, w, 0, 1)]
    return cases


def test_pair_geometry_matches_its_restatement(tmp_path):
    cases = _cases()
    per_class = {c: sum(1 for x in cases if x[0] == c) for c in ("short", "unbanded", "band", "band+two", "band+adapt")}
    assert per_class["band"] >= 60 and per_class["band+two"] == per_class["band"], per_class
    assert per_class["band+adapt"] == 120 and per_class["unbanded"] == 60 and per_class["short"] == 360, per_class
    src = tmp_path / "aff_geometry.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "aff_geometry"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-std=c++17", "-O1",
                           "-I", os.path.join(ROOT, "sparksmithwaterman_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="".join("%d %d %d %d %d\n" % c[1:] for c in cases), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == _want(*c[1:]), (c, g, _want(*c[1:]))
    # the classes differ where they should: a band shrinks the field, two planes double it, the table is what adapt adds to its fields
    by = {c[1:]: g for c, g in zip(cases, got)}
    assert by[(3000, 5000, 100, 0, 0)][0] < by[(3000, 5000, 0, 0, 0)][0]
    assert by[(3000, 5000, 100, 0, 1)][0] == 2 * by[(3000, 5000, 100, 0, 0)][0]
    assert by[(3000, 5000, 100, 1, 0)][0] - by[(3000, 5000, 100, 1, 0)][2] == 64
