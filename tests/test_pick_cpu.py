"""The pick kernels' case set without a GPU (tests/pick_cases.py, tests/pick_model.py; DESIGN.md sections 8n and 8p).

Three things are shown here, so that tests/test_pick_gpu.py needs no GPU time to be believed:

  the model is the rule    pick_model's transcription of the pass equals subopt_reference.reduce_colmax and hits_reference.pick on
                           seeded random rows (lengths 1 .. 1500, maximum densities 0 .. 0.3, every w the issue names) and on the
                           column maxima of every case;
  the claims hold          what each family of pick_cases says about itself, and between them the GPU cases take every branch of
                           pick_model.BRANCHES -- a missing one is named;
  every mutation is caught for every entry of pick_model.MUTATIONS some GPU case's expected value differs from what the mutated
                           model returns.  The one entry of pick_model.EQUIVALENT cannot change a value; that is asserted instead,
                           with 0 and with a stale maximum behind the row.
"""
import random

import pytest

import hits_reference as hr
import pick_cases as pc
import pick_model as pm
import subopt_reference as sr

WIDTHS = (1, 2, 3, 10, 63, 64, 65, 100, 255, 256, 300, 1 << 30)
N_RANDOM = 5000


def rule(cm, rw, s, w, k):
    """(the hits list, (score2, end2)) by the plain definition"""
    return hr.pick([0] + cm, [0] + rw, s, w, k), sr.reduce_colmax([0] + cm, s, w)


def random_row(rng):
    """a row with its maximum s in a chosen share of the columns, few distinct other values (ties), zeros"""
    n = rng.choice((rng.randint(1, 70), rng.randint(1, 330), rng.randint(1, 1500)))
    dens = rng.choice((0.0, 0.0, 0.003, 0.02, 0.1, 0.3))
    s = rng.randint(2, 40)
    low = rng.choice((1, 3, s - 1))
    cm = [s if rng.random() < dens else (rng.randint(0, min(low, s - 1)) if rng.random() < 0.5 else 0) for _ in range(n)]
    for _ in range(rng.randint(1, 3) if dens == 0.0 else 0):
        cm[rng.randrange(n)] = s
    if s not in cm:
        cm[rng.randrange(n)] = s
    return cm, [rng.randint(1, 8) for _ in range(n)], s


def test_model_is_the_rule_on_random_rows():
    rng = random.Random(9510)
    seen = set()
    for x in range(N_RANDOM):
        cm, rw, s = random_row(rng)
        w = rng.choice(WIDTHS)
        # sixteen rounds of the plain rule are slow on a long dense row: K = 16 on the shorter ones
        k = rng.choice((1, 2, 3, 16)) if len(cm) <= 330 else rng.choice((1, 2, 3))
        want, want2 = rule(cm, rw, s, w, k)
        assert pm.subopt(cm, s, w, trace=seen) == want2, (x, len(cm), s, w)
        assert pm.hits(cm, rw, s, w, k, trace=seen) == (want, want2), (x, len(cm), s, w, k)
    assert seen == set(pm.BRANCHES), sorted(set(pm.BRANCHES) - seen)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
_exp = {}


def expected(c):
    """(the K = 16 hits list, (score2, end2)) of a case by the plain definition, once"""
    if c not in _exp:
        s, cm, rw = pc.rows(c)
        _exp[c] = rule(cm, rw, s, pc.width(c), 16) if s > 0 else ([], (0, 0))
    return _exp[c]


def model(c, mut=None, trace=None, pad=None):
    s, cm, rw = pc.rows(c)
    if s == 0:
        return ([], (0, 0)), (0, 0)
    w = pc.width(c)
    return pm.hits(cm, rw, s, w, c.k, mut, trace, pad), pm.subopt(cm, s, w, mut, trace, pad)


def agrees(c, got):
    """what the GPU module compares: the hits list of K entries, SuboptOut of both kernels"""
    full, sub = expected(c)
    return got == ((full[:c.k], sub), sub)


def step_of(col):
    return (col - 1) // pc.WAVE


def test_the_comb_profile():
    """an isolated exact copy leaves PROFILE and nothing else; weak copies reach 31, 22 and 13"""
    for n, e in ((100, 50), (321, 64), (321, 300)):
        s, cm, _ = pc.rows(pc.case("one", pc.comb(n, [e]), 1, 1))
        assert s == 40 and cm[e - 8:e + 11] == pc.PROFILE[:n - e + 8] and sum(cm) == sum(pc.PROFILE), (n, e)
    assert len(set(pc.READ)) == 3 and "T" not in pc.READ
    assert [pc.rows(pc.case("weak", pc.comb(60, [], [(30, k)]), 1, 1))[0] for k in (1, 2, 3)] == [31, 22, 13]
    assert expected(pc.case("one", pc.comb(100, [50]), 1, 1))[1] == (30, 48) and expected(pc.case("one", pc.comb(100, [50]), 2, 1))[1] == (26, 53)


def test_model_is_the_rule_on_every_case():
    for c in pc.all_cases():
        assert agrees(c, model(c)), c.name


def test_slide_claim():
    """every seam has a case with the runner-up in the step before its maximum column's and one with it in the step after"""
    before, after = set(), set()
    for c in pc.slide(1) + pc.slide(2):
        s, cm, _ = pc.rows(c)
        e, (v2, e2) = cm.index(s) + 1, expected(c)[1]
        assert cm.count(s) == 1 and v2 > 0
        if step_of(e2) == step_of(e) - 1:
            before.add(step_of(e))
        if step_of(e2) == step_of(e) + 1:
            after.add(step_of(e2))
    assert before == after == {1, 2, 3, 4, 5}, (before, after)
    assert len(pc.slide(1)) == 34 and len(pc.slide(2)) == 43


def test_row_end_claim():
    """every value of (cols - 1) % 256 // 64 with the last step partial and whole; the maximum column, and end2, in the row's last
    column; end2 = n in lane 0 and in lane 63"""
    classes, lanes = set(), set()
    for c in pc.row_ends():
        n = len(c.ref)
        classes.add(((n - 1) % 256 // 64, n % 64 == 0))
        s, cm, _ = pc.rows(c)
        if c.name.endswith("max-last"):
            assert cm[n - 1] == s == 40 and cm.count(s) == 1
        else:
            assert expected(c)[1] == (31, n), c.name
            lanes.add((n - 1) % 64)
    assert classes == {(q, whole) for q in range(4) for whole in (False, True)}
    assert {0, 63} <= lanes
    assert {193, 255, 256} <= {len(c.ref) for c in pc.row_ends()}            # the guarded fourth load: cols - base in 193 .. 256


def test_lookahead_claim():
    by = {c.name: c for c in pc.lookahead()}
    for name, want in pc.LOOK_CHECKED.items():
        assert expected(by[name])[1] == want
    found = {}
    for c in pc.lookahead():
        t = set()
        model(c, trace=t)
        found[c.name] = t
        if "nothing-eligible" in c.name:
            assert expected(c) == ([(40, 8, 30)], (0, 0))
        elif "checked" not in c.name:
            assert expected(c)[1][0] == 31, c.name                            # the weak copy is what decides
    # the second copy is found in load d - 1 of the first search; d = 5 and 9 skip a quad
    for d, b in ((1, "b0"), (2, "b1"), (3, "b2"), (4, "b3")):
        assert b in found["look-n700-d%d-behind" % d]
    assert "quad_skipped" in found["look-n700-d5-behind"] and "quad_skipped" in found["look-n1100-d9-behind"]
    assert {"row_exhausted", "quad_skipped"} <= found["look-n1100-alone"]
    assert {"nxt_kept", "nxt_searched_again"} <= found["look-n1100-three"]


def test_dense_claim():
    for c in pc.dense():
        s, cm, _ = pc.rows(c)
        w, tops = c.w, [j + 1 for j, v in enumerate(cm) if v == s]
        free = [j for j in range(1, len(cm) + 1) if all(abs(j - t) > w for t in tops)]
        inner = [j for j in free if tops[0] < j < tops[-1]]
        assert s == 40 and len(tops) >= 35
        if "one-out" in c.name:
            assert step_of(inner[0]) == 0 and step_of(inner[-1]) == 1 and inner == list(range(inner[0], inner[-1] + 1))
        elif w == 8:
            assert not inner
        elif w == 7:
            assert len(inner) == len(tops) - 1 and len(expected(c)[0]) == 16     # one per period; sixteen equal entries
            assert len({h[0] for h in expected(c)[0][1:]}) == 1


def test_rounds_claim():
    cases = {c.name: c for c in pc.rounds()}
    full = expected(cases["rounds-k16"])[0]
    ends = pc.rounds_ends()
    assert len(full) == 16 and full[0] == (40, 8, ends[pc.ROUNDS_EXACT])
    want = sorted((40 - 9 * k, e) for e, k in zip(ends, pc.ROUNDS_STRENGTH) if k)
    want.sort(key=lambda t: (-t[0], t[1]))
    assert [(v, j) for v, _, j in full[1:]] == want
    assert {(e - 1) % 64 for e in ends} >= {0, 63} and sorted(step_of(e) for e in ends) == list(range(16))
    near, far = expected(cases["rounds-apart-w15"])[0], expected(cases["rounds-apart-w16"])[0]
    assert [h[2] for h in near[:3]] == [30, 120, 136] and [h[2] for h in far[:2]] == [30, 120] and 136 not in [h[2] for h in far]
    assert step_of(120) != step_of(136)


def test_wide_claim():
    by = {c.name: c for c in pc.wide()}
    for w in (63, 64, 65):
        for d in (64, 65, 66):
            for side in ("right", "left"):
                c = by["wide-w%d-%s%d" % (w, side, d)]
                weak = 100 + d if side == "right" else 100
                assert (expected(c)[1] == (31, weak)) == (d > w), c.name
    assert expected(by["wide-w2^30"]) == ([(40, 8, 200)], (0, 0))
    assert pc.width(by["wide-auto-15"]) == 15
    assert expected(by["wide-auto-16"])[1] == (31, 116) and expected(by["wide-auto-15"])[1][0] < 31


def test_layout_claim():
    refs, reads, w, k = pc.layout_mixed()
    assert refs[2] == "T" * pc.SLIDE_N and refs[4] == "" and pc.rows(pc.case("deg", refs[2], w, k, pc.A8))[0] == 0
    assert (2 * 2 + 1) % 4 == 1                                             # the degenerate pair: second of its workgroup
    assert {len(pc.layout_cut(q, r)) % 4 for q, r in ((2, 1), (3, 2), (1, 3))} == {1, 2, 3}
    # the A8 pairs have many maximum columns
    assert max(pc.rows(c)[1].count(pc.rows(c)[0]) for c in pc.mixed_cases() if c.read == pc.A8) > 30


def test_band_claim():
    for c in pc.band():
        n = pc.cols_of(c)
        s, cm, _ = pc.rows(c)
        free = pc.rows(c._replace(band=0))
        assert n == 2098 and n % 64 != 0 and len(cm) == n
        assert cm[n - 1] == s >= 152                                        # the best alignment ends in the last swept column
        assert free[0] >= 300 > s and free[1].index(free[0]) + 1 > n       # ... and with the band off the copy right of it wins
        assert expected(c)[1][0] > 0
    assert step_of(expected(pc.band()[0])[1][1]) < 16 and step_of(expected(pc.band()[1])[1][1]) == step_of(2098)


def test_the_cases_take_every_branch():
    seen = set()
    for c in pc.all_cases():
        model(c, trace=seen)
    assert seen == set(pm.BRANCHES), "no GPU case takes: %s" % sorted(set(pm.BRANCHES) - seen)


def killers(mut, first=True):
    """the names of the GPU cases whose expected value differs from the mutated model's (first: stop at one)"""
    out = []
    for c in pc.all_cases():
        if not agrees(c, model(c, mut)):
            out.append(c.name)
            if first:
                break
    return out


@pytest.mark.parametrize("mut", sorted(set(pm.MUTATIONS) - set(pm.EQUIVALENT)))
def test_every_mutation_is_caught(mut):
    assert killers(mut), "no GPU case would notice: %s (%s)" % (mut, pm.MUTATIONS[mut])


@pytest.mark.parametrize("mut", sorted(pm.EQUIVALENT))
def test_an_equivalent_mutation_changes_nothing(mut):
    """not an excuse: were the change able to alter a value, this fails and the case that catches it is owed"""
    assert mut in pm.MUTATIONS
    rng = random.Random(9511)
    for x in range(400):
        cm, rw, s = random_row(rng)
        w = rng.choice(WIDTHS)
        for pad in (0, s):
            assert pm.hits(cm, rw, s, w, 3, mut, pad=pad) == pm.hits(cm, rw, s, w, 3), (x, pad)
            assert pm.subopt(cm, s, w, mut, pad=pad) == pm.subopt(cm, s, w), (x, pad)
    for c in pc.all_cases():
        for pad in (0, None):
            assert model(c, mut, pad=pad) == model(c), c.name
