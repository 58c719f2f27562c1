"""Host-side checks of the banded alignment feature (option "band") that need no GPU: the two restatements of
tests/gotoh_reference.py agree on whole staircases at strip = 8, a band that covers everything is no band, a planted alignment is
found inside the band and lost outside the staircase, and the sharded driver's parser knows --band."""
import random

import pytest

import gotoh_reference as gr

SC = (5, -3, -2, -6)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("w", [1, 3, 8])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_scalar_and_numpy_agree_on_a_staircase(mode, w):
    rng = random.Random(9100 + 10 * mode + w)
    done = 0
    for _ in range(60):
        m = rng.randint(9, 40)
        n = max(1, m + rng.choice([-w, -1, 0, 1, w]))
        if gr.refused(m, n, w, mode, strip=8):
            continue
        alphabet = rng.choice(["AC", "ACGT"])
        ref, read = _rand(rng, n, alphabet), _rand(rng, m, alphabet)
        sc = rng.choice([SC, (5, -3, -2, 0), (2, -1, -1, -1)])
        for tie in (0, 1):
            a = gr.align_scalar(ref, read, sc, mode, w, tie_mode=tie, strip=8)
            b = gr.align_numpy(ref, read, sc, mode, w, tie_mode=tie, strip=8)
            assert a == b, (ref, read, sc, tie)
            if mode != 0 or a[0] > 0:                  # every alignment spells the score it claims
                for _, (ra, qa) in a[1]:
                    assert gr.rescore(ra, qa, sc) == a[0], (ref, read, sc, tie)
        done += 1
    assert done >= 30


def test_staircase_geometry():
    assert gr.windows(20, 30, 3, strip=8) == [(1, 11), (6, 19), (14, 27)]
    assert gr.in_band_cells(20, 30, 3, strip=8) == 8 * 11 + 8 * 14 + 4 * 14
    for i in range(1, 21):                            # every cell with |j - i| <= w is in the band
        lo, hi = gr.windows(20, 30, 3, strip=8)[(i - 1) // 8]
        assert lo <= max(1, i - 3) and min(30, i + 3) <= hi
    assert gr.refused(20, 13, 3, 1, strip=8) and not gr.refused(20, 14, 3, 1, strip=8)      # last window starts at 14
    assert gr.refused(20, 28, 3, 2, strip=8) and not gr.refused(20, 27, 3, 2, strip=8)      # (m, n) within 8 * 3 + 3


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_band_over_everything_is_no_band(mode):
    rng = random.Random(9200 + mode)
    for _ in range(12):
        m, n = rng.randint(9, 30), rng.randint(1, 30)
        ref, read = _rand(rng, n, "AC"), _rand(rng, m, "AC")
        w = max(m, n)
        for tie in (0, 1):
            want = gr.align_scalar(ref, read, SC, mode, tie_mode=tie)
            assert gr.align_scalar(ref, read, SC, mode, w, tie_mode=tie, strip=8) == want
            assert gr.align_numpy(ref, read, SC, mode, w, tie_mode=tie, strip=8) == want


def test_short_reads_and_band_0_are_unbanded():
    rng = random.Random(9300)
    ref, read = _rand(rng, 30), _rand(rng, 8)
    assert gr.align_scalar(ref, read, SC, 0, 1, strip=8) == gr.align_scalar(ref, read, SC)      # m = strip: not a long read
    ref, read = _rand(rng, 30), _rand(rng, 20)
    assert gr.align_numpy(ref, read, SC, 1, 0, strip=8) == gr.align_scalar(ref, read, SC, 1)


def test_planted_alignment_inside_and_outside():
    """local mode: a 12-base stretch planted on the diagonal band is found with the unbanded score; planted far off the
    staircase it is not"""
    rng = random.Random(9400)
    plant = "ACGTTGCAGTCA"
    m = n = 40
    w = 2
    read = list(_rand(rng, m, "T"))
    read[20:32] = plant
    read = "".join(read)
    ref_in = list(_rand(rng, n, "C"))
    ref_in[21:33] = plant                              # j - i = 1 <= w
    ref_in = "".join(ref_in)
    full = gr.align_scalar(ref_in, read, SC)
    assert full[0] == 60
    assert gr.align_scalar(ref_in, read, SC, 0, w, strip=8) == full
    ref_out = plant + _rand(rng, n - 12, "C")         # columns 1..12 against rows 21..32: left of every window there
    assert all(lo > 12 for lo, _ in gr.windows(m, n, w, strip=8)[2:4])
    assert gr.align_scalar(ref_out, read, SC)[0] == 60
    assert gr.align_scalar(ref_out, read, SC, 0, w, strip=8)[0] < 60
    assert gr.align_numpy(ref_out, read, SC, 0, w, strip=8) == gr.align_scalar(ref_out, read, SC, 0, w, strip=8)


def test_degenerate_count_is_in_band():
    got = gr.align_scalar("C" * 30, "A" * 20, SC, 0, 3, strip=8)
    assert got == (0, [(0, ("", ""))] * gr.in_band_cells(20, 30, 3, strip=8))
    assert gr.align_numpy("C" * 30, "A" * 20, SC, 0, 3, strip=8) == got


def test_sharded_files_parser_accepts_band():
    from sparksmithwaterman_amd import sharded_files
    base = ["--ref-dir", "R", "--in-dir", "I", "--out-dir", "O"]
    assert sharded_files._parser().parse_args(base).band == 0
    args = sharded_files._parser().parse_args(base + ["--band", "512", "--long-reads", "--align-mode", "global"])
    assert args.band == 512 and args.long_reads is True and args.align_mode == "global"
