"""Affine gap penalties on the GPU (swmi_affine.hip, swmi_set_option "gap_open" / "affine").

Checked against the oracle at gap_open = 0 (the affine kernels must reduce to the linear results bit for bit) and against the
numpy restatement of the contract in tests/gotoh_reference.py otherwise."""
import os
import random

import numpy as np
import pytest

import sparksmithwaterman_amd as sw
from sparksmithwaterman_amd import _capi
from oracle import sw_oracle as orc

import affine_gpu_util as u
import gotoh_reference as gr
import limit_cases as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5       # swmi_status (include/swmi.h)


def _golden(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture
def ctx():
    c = sw.Context(0)
    yield c
    c.close()


def _expect_linear(refs, reads, scores, tie):
    exp = {}
    for r, ref in enumerate(refs):
        for q, read in enumerate(reads):
            s, al = orc.opt_alignments((ref, read), scores[:3], b"aid-", tie)
            exp[(r, q)] = (s, [(a[0], tuple(a[1])) for a in al])
    return exp


# 1 -- gap_open = 0 on the affine kernels reduces to today's results
@pytest.mark.parametrize("tie", [0, 1])
def test_affine_kernels_at_gap_open_zero_match_the_oracle(ctx, tie):
    ctx.set_option("affine", 1)
    kats = _golden("kat.json")["kats"] + _golden("engineerdata_small.json")["kats"]
    n_checked = 0
    for k in kats:
        if k["scores"][2] > 0 or tuple(k.get("types", "aid-")) != tuple("aid-"):
            continue                        # (a positive gap is outside the affine bounds; alignTypes are the linear path's)
        if k["tie_mode"] != tie:
            continue
        b = u.run(ctx, [k["ref"]], [k["read"]], tuple(k["scores"]) + (0,), tie, mode3=False)
        assert b.pipeline_mode() == 3
        assert b.score(0) == k["score"], k["name"]
        assert [[x[0], x[1][0], x[1][1]] for x in b.alignments(0)] == k["alignments"], k["name"]
        b.free()
        n_checked += 1
    assert n_checked >= 3
    rng = random.Random(11 + tie)
    refs = [u.rand(rng, rng.randint(1, 600), rng.choice(["ACGT", "AC", "ACGTacgtN"])) for _ in range(20)]
    refs[3] = "ACGTTGCA" * 60                           # periodic: a tied maximum per period
    reads = [u.rand(rng, rng.randint(1, 200)) for _ in range(50)]
    reads[7] = "ACGTTGCAAC"
    b = u.run(ctx, refs, reads, (5, -3, -4, 0), tie, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, _expect_linear(refs, reads, (5, -3, -4), tie))
    b.free()


# 2 -- gap_open != 0 against the numpy restatement
def test_affine_read_lengths_and_long_references(ctx):
    rng = random.Random(5)
    reads = [u.rand(rng, m) for m in (1, 63, 64, 65, 128, 150, 256, 257, 512, 1024)]
    refs = [u.rand(rng, 700), u.rand(rng, 1500)]
    for o, tie in ((-1, 0), (-6, 1), (-12, 0)):
        b = u.run(ctx, refs, reads, (5, -3, -2, o), tie, mode3=False)
        assert b.pipeline_mode() == 3
        u.check(b, refs, reads, u.expect(refs, reads, (5, -3, -2, o), tie=tie))
        b.free()
    # a 20 kbp reference with a planted read and a read of 1024
    big = u.rand(rng, 20000)
    reads2 = [big[13000:13150], big[5000:5400] + big[5460:6084], u.rand(rng, 90)]
    b = u.run(ctx, [big], reads2, (2, -3, -1, -6), 0, mode3=False)
    u.check(b, [big], reads2, u.expect([big], reads2, (2, -3, -1, -6)))
    b.free()


@pytest.mark.parametrize("tie", [0, 1])
def test_affine_ties_symbols_and_empty_sides(ctx, tie):
    rng = random.Random(21 + tie)
    # EngineerData-shaped periodic pairs: many tied maxima; non-ACGT bytes and mixed case; empty sequences
    refs = ["CCTGGGTCCTGCCTCG" * 25, "acgtNNacgtRYacgt" * 12, "", u.rand(rng, 300, "ACGTacgt\xe9\xc9x"), "AAAA"]
    reads = ["CCTGGGTCCTGC", "ACGTNNACG", "", u.rand(rng, 80, "ACGTacgt\xe9\xc9"), "TT", "CCTGGGACCTGCCTCGCC"]
    for o in (-1, -6, -12):
        b = u.run(ctx, refs, reads, (5, -3, -4, o), tie, mode3=False)
        u.check(b, refs, reads, u.expect(refs, reads, (5, -3, -4, o), tie=tie))
        b.free()


def test_affine_kats(ctx):
    for k in _golden("affine_kat.json")["kats"]:
        b = u.run(ctx, [k["ref"]], [k["read"]], tuple(k["scores"]), k["tie_mode"], mode3=False)
        assert b.score(0) == k["score"], k["name"]
        assert [[x[0], x[1][0], x[1][1]] for x in b.alignments(0)] == k["alignments"], k["name"]
        b.free()


# 3 -- the options that apply to affine runs give the same results
@pytest.mark.parametrize("opt", [("device_strings", 0), ("zero_copy", 0), ("scores_only", 1), ("cell_cap", 4),
                                 ("max_workspace_bytes", 1 << 20)])
def test_affine_options(ctx, opt):
    rng = random.Random(31)
    refs = ["ACGTTGCA" * 40, u.rand(rng, 900), "GATTACA" * 30 + u.rand(rng, 200), u.rand(rng, 64), u.rand(rng, 2500)]
    reads = ["ACGTTGCAAC", u.rand(rng, 150), "GATTACAGATTACA", u.rand(rng, 300), u.rand(rng, 400)]     # (> 1 MiB of field in all)
    sc = (5, -3, -2, -6)
    ctx.set_option(*opt)
    b = u.run(ctx, refs, reads, sc, 0, mode3=False)
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc), alignments=opt[0] != "scores_only")
    if opt[0] == "cell_cap":
        assert b.timing().rerun_pairs >= 1
    if opt[0] == "max_workspace_bytes":
        assert b.timing().fill_launches >= 2
    b.free()


def test_affine_async_and_one_shot(ctx):
    rng = random.Random(41)
    refs = [u.rand(rng, 500) for _ in range(3)]
    reads = [u.rand(rng, 120) for _ in range(4)]
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    b = ctx.upload(refs, reads).run_async(sw.make_params(sc[:3])).wait()
    assert b.pipeline_mode() == 3
    u.check(b, refs, reads, u.expect(refs, reads, sc))
    b.free()
    score, alns = sw.SmithWaterman.OptAlignments(ctx).call([refs[0], reads[0]], list(sc))
    assert (score, alns) == gr.align_numpy(refs[0], reads[0], sc)


# 4 -- a stream from a FASTA file
def test_affine_stream_from_fasta(ctx, tmp_path):
    rng = random.Random(51)
    refs = [u.rand(rng, rng.randint(200, 800)) for _ in range(40)]
    reads = [u.rand(rng, 150), refs[17][100:250], u.rand(rng, 64)]
    path = tmp_path / "refs.fa"
    with open(path, "w") as f:
        for k, r in enumerate(refs):
            f.write(">gi|ref%d\n" % k)
            for x in range(0, len(r), 70):
                f.write(r[x:x + 70] + "\n")
    sc = (5, -3, -2, -6)
    ctx.set_option("gap_open", sc[3])
    st = ctx.stream(reads, sw.make_params(sc[:3]), slots=2, chunk_bytes=1 << 16)
    st.push_file(path).finish()
    exp = [[gr.align_numpy(r, q, sc) for q in reads] for r in refs]
    totals = st.totals()
    assert [int(t) for t in totals] == [sum(e[0] for e in row) for row in exp]
    for first, c in st.chunks():
        assert c.pipeline_mode() == 3
        for r in range(c.n_refs):
            if (first + r) % 7 == 3 or first + r == 17:
                sites = sorted([a for e in exp[first + r] for a in e[1]], key=lambda t: t[0])
                assert c.ref_match_sites(r) == sites, first + r
    st.close()


# 5 -- out of bounds
def test_affine_bounds(ctx):
    with pytest.raises(_capi.SwmiError) as e:
        ctx.set_option("gap_open", 1)
    assert e.value.code == ERR_INVALID
    with pytest.raises(_capi.SwmiError) as e:
        ctx.set_option("affine", 0)
    assert e.value.code == ERR_INVALID
    ctx.set_option("gap_open", -6)
    b = ctx.upload(["ACGT" * 10], ["A" * 1025])
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()
    b = ctx.upload(["ACGT" * 10], ["ACG"])
    for bad in ((5, -3, 1), ((1 << 20) + 1, -3, -4)):
        with pytest.raises(_capi.SwmiError) as e:
            b.run(sw.make_params(bad))
        assert e.value.code == ERR_UNSUPPORTED
    ctx.set_option("gap_open", -((1 << 20) + 1))
    with pytest.raises(_capi.SwmiError) as e:
        b.run(sw.make_params((5, -3, -4)))
    assert e.value.code == ERR_UNSUPPORTED
    b.free()


# 5b -- local mode AT its bounds, against the restatement in unbounded Python ints (fit and global: tests/test_ends_gpu.py)
@pytest.mark.parametrize("sc", lc.AFFINE_BOUND_SCORES, ids=lc.score_id)
def test_affine_local_bounds_scores_and_read_length(ctx, sc):
    """every score at +-2^20 and the longest read: the local cell takes its x bits from the sign of t1 - t2
    (swmi_affine.hip: "|values| < 2^30 + 2^21, the difference fits"), H reaches 200 * 2^20 on the cut"""
    ref, read = lc.affine_bound_pair(1024, 200, 50)
    assert len(read) == 1024 and len(ref) == 300
    ctx.set_option("affine", 1)                                   # (gap_open = 0 alone would select the linear pipeline)
    for tie in (0, 1):
        b = u.run(ctx, [ref], [read], sc, tie, mode3=False)
        assert b.pipeline_mode() == 3
        assert (b.score(0), b.alignments(0)) == gr.align_scalar(ref, read, sc, tie_mode=tie), (sc, tie)
        b.free()


def test_affine_local_perfect_match_reaches_2_30_and_the_total_wraps(ctx):
    """1024 matches of 2^20: the largest H the bounds allow; three such pairs make MapRef's Java int total wrap on mode 3"""
    L = lc.L
    sc = (L, -L, -L, -L)
    read = lc.rand_seq(random.Random(1410), 1024, "AC")
    b = u.run(ctx, [read], [read] * 3, sc, 0, mode3=False)
    assert b.pipeline_mode() == 3
    want = gr.align_scalar(read, read, sc)
    assert want == (1 << 30, [(1, (read, read))])
    for q in range(3):
        assert b.score(q) == 1 << 30
        assert (b.score(q), b.alignments(q)) == want
    total = int(np.array([1 << 30] * 3, dtype=np.int32).sum(dtype=np.int32))
    assert total == -(1 << 30)
    assert b.ref_total(0) == total and [int(x) for x in b.ref_totals()] == [total]
    assert b.ref_sites_packed() == [(total, 0, want[1] * 3)]
    b.free()
    b = u.run(ctx, [read], [read], sc, 1, mode3=False)
    assert (b.score(0), b.alignments(0)) == gr.align_numpy(read, read, sc, tie_mode=1) == want
    b.free()


def test_affine_local_bound_path_lds(ctx):
    """gap = 0 lifts the cap "the score stays positive" off a local path: path_bound is m + n as in fit and global mode, and
    the traceback's LDS bounds it the same way (tests/test_ends_gpu.py::test_ends_bound_path_lds): 587760 runs, 587761 does not"""
    limit = (160 * 1024 // 4 - 4096 - 128 - 1) * 16
    assert limit == 587760
    rng = random.Random(1420)
    ref = list(u.rand(rng, limit, "ACT"))
    for at in (0, 1, 300000, limit - 2):                          # (the read's only matches: four tied maxima)
        ref[at] = "G"
    ref = "".join(ref)
    sc = (2, -3, 0, -2)
    b = u.run(ctx, [ref[:limit - 1]], ["G"], sc, 0, mode3=False)                # m + n = limit
    assert b.pipeline_mode() == 3
    assert (b.score(0), b.alignments(0)) == gr.align_scalar(ref[:limit - 1], "G", sc)
    assert b.n_alignments(0)[0] == 4
    b.free()
    b = ctx.upload([ref], ["G"])                                  # m + n = limit + 1
    with pytest.raises(_capi.SwmiError) as err:
        b.run(sw.make_params(sc[:3]))
    assert err.value.code == ERR_UNSUPPORTED
    ctx.set_option("gap_open", -2)
    b.run(sw.make_params((2, -3, -1)))                            # gap < 0 caps the path again: the same pair runs
    assert b.score(0) == 2
    b.free()


# 6 -- back to the linear kernels on the same context
def test_gap_open_back_to_zero_runs_mode_1(ctx):
    rng = random.Random(61)
    refs = [u.rand(rng, 400) for _ in range(3)]
    reads = [u.rand(rng, 100) for _ in range(3)]
    b = ctx.upload(refs, reads)
    ctx.set_option("gap_open", -6)
    assert b.run(sw.make_params()).pipeline_mode() == 3
    ctx.set_option("gap_open", 0)
    b.run(sw.make_params())
    assert b.pipeline_mode() == 1
    u.check(b, refs, reads, _expect_linear(refs, reads, (5, -3, -4), 0))
    b.free()


# 7 -- the JNI shim's entry point from plain C99
_SHIM_C = r"""
#include <stdio.h>
#include "swmi.h"
#include "swmi_shim.h"
int main(void) {
    char err[640];
    swmi_ctx *ctx = NULL;
    swmi_batch *b = NULL;
    const signed char types[4] = {'a', 'i', 'd', '-'};
    const char *ref = "%(ref)s", *read = "%(read)s";
    int64_t ro[2], qo[2], n = 0, k;
    int32_t total = 0;
    ro[0] = 0; ro[1] = %(n)d; qo[0] = 0; qo[1] = %(m)d;
    if (swmi_create(0, &ctx) != SWMI_OK) { printf("ERROR %%s\n", swmi_last_error()); return 3; }
    if (swmi_shim_set_gap_open(ctx, 1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR positive gapOpen accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(NULL, -1, err, sizeof err) != SWMI_ERR_INVALID) { printf("ERROR null context accepted\n"); return 4; }
    if (swmi_shim_set_gap_open(ctx, %(o)d, err, sizeof err) != SWMI_OK) { printf("ERROR %%s\n", err); return 5; }
    if (swmi_shim_align_batch(ctx, %(match)d, %(mismatch)d, %(gap)d, %(tie)d, types, 4, ref, %(n)d, ro, 1, read, %(m)d, qo, 1, &b, err, sizeof err) != SWMI_OK) {
        printf("ERROR %%s\n", err); return 6;
    }
    if (swmi_shim_ref_total(b, 0, &total, err, sizeof err) != SWMI_OK) { printf("ERROR %%s\n", err); return 7; }
    if (swmi_shim_ref_site_count(b, 0, &n, err, sizeof err) != SWMI_OK) { printf("ERROR %%s\n", err); return 7; }
    printf("%%d %%ld", (int)total, (long)n);
    for (k = 0; k < n; k++) {
        int32_t begin = 0; const char *ra = NULL, *qa = NULL; uint32_t len = 0;
        if (swmi_shim_ref_site(b, 0, k, &begin, &ra, &qa, &len, err, sizeof err) != SWMI_OK) { printf("ERROR %%s\n", err); return 8; }
        printf(" %%d:%%s/%%s", (int)begin, ra, qa);
    }
    printf("\n");
    swmi_batch_free(ctx, b);
    swmi_destroy(ctx);
    return 0;
}
"""


def test_c99_shim_sets_gap_open(tmp_path):
    k = _golden("affine_kat.json")["kats"][0]
    out = u.run_shim(tmp_path, "shim_affine", _SHIM_C % dict(ref=k["ref"], read=k["read"], n=len(k["ref"]), m=len(k["read"]),
                                                             match=k["scores"][0], mismatch=k["scores"][1], gap=k["scores"][2],
                                                             o=k["scores"][3], tie=k["tie_mode"]))
    sites = sorted(k["alignments"], key=lambda a: a[0])
    assert out.split() == [str(k["score"]), str(len(sites))] + ["%d:%s/%s" % tuple(a) for a in sites]
