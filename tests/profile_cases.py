"""Inputs of the per-read profile tests and their expected values -- TEST INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  tests/test_profile_cpu.py holds every recipe to what it is built for, on the restatements
of tests/profile_reference.py alone; tests/test_profile_gpu.py runs them on the GPU.

The class grid.  One batch per rows-per-lane class R = 1 .. 16 of swmi_affine.hip (R = ceil(m / 64)): five reads of different
lengths in the class -- 64 R - 3 first, 64 (R - 1) + 1 last, for R = 16 also 1024 -- against three references of 70 to 130 bases over
the five-symbol alphabet ACGTN, with bytes outside it and lower-case letters among them.  That is 15 pairs, no multiple of the four
wavefronts of a workgroup, and four different tables in every workgroup.  The entries are random in -6 .. 7.

The grid's tables are small: every launch of it has four wavefronts per workgroup.  wave_grid, mixed_classes, periodic_wide_case,
alphabet_edges and mismatch_case, further down, are built for the workgroup sizes the launcher computes (1, 2 and 3 wavefronts,
partial last workgroups, two sizes over one pair array, a chunk and a re-run with an r_max of their own), for the steps of the
staging loop and for column n of a table; each docstring says for what."""
import functools
import random

import gotoh_reference as gr
import overlap_reference as ov
import profile_reference as pr

ALPHABET = "ACGTN"
SC = (5, -3, -2, -6)                                    # (match, mismatch, gap, gap_open)
RS = tuple(range(1, 17))
# the five runs a profile is built for: gotoh_reference's mode, extend, overlap
MODES = {"local": (gr.LOCAL, False, False), "fit": (gr.FIT, False, False), "global": (gr.GLOBAL, False, False),
         "extend": (gr.GLOBAL, True, False), "overlap": (gr.FIT, False, True)}


def options(name):
    """the context options of a run of MODES[name]"""
    mode, extend, overlap = MODES[name]
    return dict(align_mode=mode, extend=int(extend), overlap=int(overlap))


def random_profile(rng, m, n=len(ALPHABET), lo=-6, hi=7):
    return [[rng.randint(lo, hi) for _ in range(n)] for _ in range(m)]


def random_reference(rng, n):
    """over ACGTN, about one byte in twelve outside the alphabet and one in eight lower-case"""
    out = []
    for _ in range(n):
        c = rng.choice("XZ*") if rng.random() < 0.08 else rng.choice(ALPHABET)
        out.append(c.lower() if rng.random() < 0.12 else c)
    return "".join(out)


def class_lengths(R):
    """five read lengths of class R: 64 R - 3 first, 64 (R - 1) + 1 last, for R = 16 also 1024"""
    lengths = [64 * R - 3, 64 * R - 20, 64 * R - 41, 64 * R if R == 16 else 64 * R - 9, 64 * (R - 1) + 1]
    assert len(set(lengths)) == 5 and all((m + 63) // 64 == R for m in lengths)
    return lengths


@functools.lru_cache(maxsize=None)
def grid(R):
    """(refs, reads, profiles) of class R"""
    rng = random.Random(7700 + R)
    lengths = class_lengths(R)
    reads = ["".join(rng.choice("ACGTacgtN") for _ in range(m)) for m in lengths]
    refs = [random_reference(rng, n) for n in (70, 101, 130)]
    return tuple(refs), tuple(reads), tuple(random_profile(rng, m) for m in lengths)


def want(ref, read, profile, name, tie, sc=SC, alphabet=ALPHABET):
    mode, extend, overlap = MODES[name]
    return pr.align_numpy(ref, read, alphabet, profile, sc, mode, extend, overlap, tie, cells=True)


def plain(ref, read, name, tie, sc=SC):
    """the same pair under match / mismatch"""
    mode, extend, overlap = MODES[name]
    if overlap:
        return ov.align_numpy(ref, read, sc, mode, 0, False, tie, None, cells=True)
    return gr.align_numpy(ref, read, sc, mode, 0, extend, tie, None, cells=True)


@functools.lru_cache(maxsize=None)
def expected(R, name, tie):
    """{(r, q): (score, alignments, cells)} of the class grid"""
    refs, reads, profiles = grid(R)
    return {(r, q): want(refs[r], reads[q], profiles[q], name, tie) for r in range(len(refs)) for q in range(len(reads))}


# ---- matrix parity: 6 x 6 protein pairs of 40 to 300 residues under BLOSUM62 ----
PROTEIN = "ARNDCQEGHILKMFPSTWYV"
SC_PROTEIN = (1, -4, -1, -11)                           # BLOSUM62 with gaps -11 / -1 (match is not read inside the alphabet)


@functools.lru_cache(maxsize=None)
def protein_pairs():
    rng = random.Random(6262)
    base = "".join(rng.choice(PROTEIN) for _ in range(400))
    reads, refs = [], []
    for m in (40, 77, 129, 200, 257, 300):
        at = rng.randrange(0, 400 - m)
        reads.append("".join(rng.choice(PROTEIN) if rng.random() < 0.15 else c for c in base[at:at + m]))
    for n in (40, 90, 150, 210, 260, 300):
        at = rng.randrange(0, 400 - n)
        refs.append("".join(rng.choice(PROTEIN + "BZX") if rng.random() < 0.1 else c for c in base[at:at + n]))
    return tuple(refs), tuple(reads)


# ---- ties beyond cell_cap: a periodic profile against a periodic reference ----
def periodic_case():
    """(ref, read, profile): the read's profile rewards ACGT at rows 0..3 with period 4, the reference is ACGT x 12: a local run ties in
    many cells, far more than cell_cap = 2"""
    read = "ACGT" * 3
    profile = [[4 if c == i % 4 else -3 for c in range(len(ALPHABET))] for i in range(len(read))]
    return "ACGT" * 12, read, profile


# ---- workgroups of one, two and three wavefronts ----
# The profile launcher sizes a workgroup by the launch: waves = min(4, 159 KiB / table), table = 64 r (n + 1) int32 with r the rows
# per lane of the launch's longest read the kernel takes (the narrow sweep: at most 4).  swmi_affine_profile_waves answers without a
# launch; tests/test_profile_cpu.py pins it to the third column.
SYMBOLS31 = "ACGTNBDEFHIKLMPQRSUVWY012345678"               # neither X, Z nor *: the bytes random_reference puts outside
PRINTABLE = "".join(chr(0x21 + k) for k in range(64))       # '!' .. '`': no two of them one symbol (no lower-case letters)
WAVE_CONFIGS = {                                            # name: (n, R, wavefronts per workgroup, shape: 0 narrow, 1 wide)
    "n8_R16": (8, 16, 4, 1),                                # 36 KiB a table: the last size with four
    "n9_R16": (9, 16, 3, 1),                                # 40 KiB: the first size with three
    "n15_R16": (15, 16, 2, 1),                              # 64 KiB
    "n31_R16": (31, 16, 1, 1),                              # 128 KiB: the largest table admitted
    "n64_R7": (64, 7, 1, 1),                                # 448 rows of 65
    "n64_R4": (64, 4, 2, 0),                                # 256 rows of 65, the narrow kernel
    "n64_R3": (64, 3, 3, 0),                                # 192 rows of 65, the narrow kernel
}
N_REFS_OF_WAVES = {4: 3, 3: 2, 2: 3, 1: 1}                  # x 5 reads: 15, 10, 15, 5 pairs -- no multiple of the wavefronts, twice them or more


def alphabet_of(n):
    """n symbols: up to 31 a prefix of ACGTN, the other capital letters but X and Z, and digits; beyond, the printable bytes from '!'
    on, as tests/test_profile_gpu.py::test_bounds_of_the_lds_table builds them"""
    return SYMBOLS31[:n] if n <= len(SYMBOLS31) else PRINTABLE[:n]


def is_outside(c, alphabet):
    return gr.upper(c) not in {gr.upper(s) for s in alphabet}


def extended_reference(rng, length, alphabet):
    """random_reference with about half of its bytes redrawn from the whole alphabet, one in eight of those in lower case; where X, Z
    and * are symbols themselves, the bytes outside are {, | and ~.  Drawn again until it holds a byte outside the alphabet and a
    lower-case letter"""
    while True:
        out = []
        for c in random_reference(rng, length):
            if c in "XZ*xz":
                c = c if is_outside(c, alphabet) else rng.choice("{|~")
            elif rng.random() < 0.5:
                c = rng.choice(alphabet)
                c = c.lower() if rng.random() < 0.12 else c
            out.append(c)
        if any(is_outside(c, alphabet) for c in out) and any(c.islower() for c in out):
            return "".join(out)


def wave_config(name):
    """(alphabet, R): the alphabet of n symbols and the rows-per-lane class of the reads whose tables give a workgroup
    WAVE_CONFIGS[name][2] wavefronts in the kernel of WAVE_CONFIGS[name][3]"""
    n, R = WAVE_CONFIGS[name][:2]
    return alphabet_of(n), R


@functools.lru_cache(maxsize=None)
def wave_grid(name):
    """(alphabet, refs, reads, profiles) of a configuration: the five read lengths of class_lengths(R) against references of 50 to
    70 bases, as many that the pair count is no multiple of the wavefronts of a workgroup and at least twice them -- the last
    workgroup of the launch is partial, and a launcher or a kernel that counts four wavefronts where there are fewer skips pairs"""
    alphabet, R = wave_config(name)
    waves = WAVE_CONFIGS[name][2]
    rng = random.Random(8800 + 17 * len(alphabet) + R)
    lengths = class_lengths(R)
    reads = ["".join(rng.choice("ACGTacgtN") for _ in range(m)) for m in lengths]
    refs = [extended_reference(rng, rng.randint(50, 70), alphabet) for _ in range(N_REFS_OF_WAVES[waves])]
    return alphabet, tuple(refs), tuple(reads), tuple(random_profile(rng, m, len(alphabet)) for m in lengths)


def _expect_all(alphabet, refs, reads, profiles, name, tie, sc=SC):
    return {(r, q): want(refs[r], reads[q], profiles[q], name, tie, sc, alphabet) for r in range(len(refs)) for q in range(len(reads))}


@functools.lru_cache(maxsize=None)
def wave_expected(config, name, tie):
    """{(r, q): (score, alignments, cells)} of wave_grid(config)"""
    return _expect_all(*wave_grid(config), name, tie)


# ---- the narrow and the wide kernel over one pair array, each with its own workgroup size ----
MIXED = {       # variant: (n, read lengths in upload order, reference lengths, wavefronts of the narrow and of the wide kernel)
    "n15": (15, (1, 64, 65, 0, 256, 257, 300, 130, 1000, 1024), (61, 131, 245), (4, 2)),
    "n64": (64, (1, 64, 65, 0, 256, 257, 300, 130, 440, 448), (50, 61, 70), (2, 1)),
}
MIXED_TWIN = 70                                             # the length of the two equal reads
MIXED_TIE = {"local": 0, "fit": 1, "global": 0, "extend": 1, "overlap": 0}       # one tie order per mode, each order used
MIXED_CAP = 1 << 20                                         # max_workspace_bytes of the chunked run (the smallest the option takes)


@functools.lru_cache(maxsize=None)
def mixed_classes(variant="n15"):
    """(alphabet, refs, reads, profiles): ONE batch whose reads are of classes 1 .. 16 (n = 15) or 1 .. 7 (n = 64), so that the narrow
    and the wide kernel walk the same pair array with different workgroup sizes and table sizes -- 4 wavefronts of 256 rows and 2 of
    1024 (n = 15), 2 of 256 and 1 of 448 (n = 64).  The lengths are not monotone in upload order (the image's row offsets are by
    upload order, the pair array by length), an empty read sits in the middle (it has no rows: the next read's offset equals its
    own), and the last two reads are byte-for-byte equal with different profiles (a table keyed by the read's bytes instead of its
    index fails).  Three references with bytes outside the alphabet and lower-case letters; the n = 15 batch's are long enough that
    its fields exceed MIXED_CAP (launches)."""
    n, lengths, ref_lengths = MIXED[variant][:3]
    alphabet = alphabet_of(n)
    rng = random.Random(9900 + n)
    reads = ["".join(rng.choice("ACGTacgtN") for _ in range(m)) for m in lengths]
    reads += ["".join(rng.choice("ACGTacgtN") for _ in range(MIXED_TWIN))] * 2
    refs = [extended_reference(rng, k, alphabet) for k in ref_lengths]
    return alphabet, tuple(refs), tuple(reads), tuple(random_profile(rng, len(q), n) for q in reads)


@functools.lru_cache(maxsize=None)
def mixed_expected(variant, name):
    """{(r, q): (score, alignments, cells)} of mixed_classes(variant) in the mode's tie order, MIXED_TIE"""
    return _expect_all(*mixed_classes(variant), name, MIXED_TIE[name])


def rows_per_lane(m):
    return max(1, (m + 63) // 64)


def dir_words(m, n):
    """swmi_aff_pair_dir_words (swmi_device.h) of a plain pair with a read of at most 1024 bases: the dwords of its direction field"""
    R = rows_per_lane(m)
    lanes = (m + R - 1) // R if m else 1
    return (n + lanes - 1 + 7) // 8 * R * 64


def launches(refs, reads, cap_bytes):
    """[[(r, q)]]: the launches of a cross product under max_workspace_bytes = cap_bytes -- build_schedule and next_launch of
    swmi_run.cpp restated for references of different lengths: the pairs with two non-empty sides, references by descending length,
    under each the reads by descending length (both stable); a launch takes pairs while their fields fit the cap, at least one.
    tests/test_profile_gpu.py::test_mixed_classes_chunked holds the count and the total to what the library reports."""
    assert len({len(r) for r in refs}) == len(refs)
    ro = sorted(range(len(refs)), key=lambda r: -len(refs[r]))
    qo = sorted(range(len(reads)), key=lambda q: -len(reads[q]))
    work = [(r, q) for r in ro if refs[r] for q in qo if reads[q]]
    out, words = [], 0
    for r, q in work:
        w = dir_words(len(reads[q]), len(refs[r]))
        if not out or (words + w) * 4 > cap_bytes:
            out.append([])
            words = 0
        out[-1].append((r, q))
        words += w
    return out


# ---- the exact-size re-run in a wide class ----
@functools.lru_cache(maxsize=None)
def periodic_wide_case():
    """(alphabet, ref, reads, profiles), the periodic pair at reads[2]: periodic_case with a read of 1000 bases (class 16) over the
    n = 15 alphabet -- score 192 in 239 tied cells, far more than cell_cap = 2, so the pair is swept again in a launch of its own,
    whose r_max (16: the wide kernel alone, 2 wavefronts, 1 pair) is not the first launch's doing: that one has r_min = 1.  The four
    other reads are of classes 1 to 3 with random profiles and at most 2 maximum cells each (they are drawn until they are: a random
    profile against a periodic reference may tie at every period)"""
    alphabet = alphabet_of(15)
    ref = "ACGT" * 12
    read = "ACGT" * 250
    profile = [[4 if c == i % 4 else -3 for c in range(len(alphabet))] for i in range(len(read))]
    rng = random.Random(1212)
    reads, profiles = [], []
    for m in (50, 100, 150, 190):
        while True:
            q = "".join(rng.choice("ACGTacgtN") for _ in range(m))
            p = random_profile(rng, m, len(alphabet))
            if len(want(ref, q, p, "local", 0, SC, alphabet)[2]) <= 2:
                break
        reads.append(q)
        profiles.append(p)
    reads.insert(2, read)
    profiles.insert(2, profile)
    return alphabet, ref, tuple(reads), tuple(profiles)


@functools.lru_cache(maxsize=None)
def periodic_wide_expected(tie):
    """[(score, alignments, cells)] of the five pairs of periodic_wide_case in a local run"""
    alphabet, ref, reads, profiles = periodic_wide_case()
    return [want(ref, q, p, "local", tie, SC, alphabet) for q, p in zip(reads, profiles)]


# ---- the staging loop's steps and the canonical form of a byte ----
LATIN1 = "AC\xe9\xff\xf7\xd7"       # e-acute (one symbol with \xc9), y-diaeresis (no Latin-1 upper case), the division and the
                                    # multiplication sign (0xF7 - 32 = 0xD7, and still two symbols)
EDGE_READS = (1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def alphabet_edges():
    """[(alphabet, refs, reads, profiles)]: the row strides n + 1 at which the staging loop of the profile sweeps steps differently
    -- 2 (64 entries are 32 whole rows: the column never moves), 3, 64 (one row a step: the carry never fires), 65 (the step is
    shorter than a row) -- with reads of 1, 63, 64 and 65 rows (one entry, a last step that is partial, none that is, a second row
    per lane); and a six-symbol alphabet above 0x7F against references that hold both cases of e-acute, \xff and \xdf (no upper case
    in Latin-1: \xff is a symbol, \xdf is outside), \xb5 (outside: its upper case is not Latin-1), \xf7 and \xd7 (two symbols)"""
    rng = random.Random(4242)
    cases = []
    for alphabet, extra in (("A", ""), ("AC", ""), (PRINTABLE[:63], ""), (PRINTABLE, ""), (LATIN1, "\xc9\xe9\xff\xdf\xb5\xf7\xd7")):
        reads = ["".join(rng.choice("ACGTacgtN") for _ in range(m)) for m in EDGE_READS]
        refs = []
        for k in (37, 66):
            ref = list(extended_reference(rng, k, alphabet))
            for j, c in enumerate(extra * 2):                                   # every listed byte, twice
                ref[(5 * j + 3) % k] = c
            refs.append("".join(ref))
        assert all(any(is_outside(c, alphabet) for c in ref) for ref in refs)
        cases.append((alphabet, tuple(refs), tuple(reads), tuple(random_profile(rng, m, len(alphabet)) for m in EDGE_READS)))
    return cases


@functools.lru_cache(maxsize=None)
def edges_expected(k, name):
    """{(r, q): (score, alignments, cells)} of alphabet_edges()[k], serial ties"""
    return _expect_all(*alphabet_edges()[k], name, 0)


# ---- column n of a table is the run's mismatch ----
SC_MISMATCH = ((5, -3, -2, -6), (5, -9, -2, -6))


@functools.lru_cache(maxsize=None)
def mismatch_case():
    """(refs, reads, profiles) over ACGTN, for two runs of ONE batch that differ in mismatch alone (SC_MISMATCH): the references hold
    bytes outside the alphabet, and column n of a wavefront's table is filled from the run's parameters, not from the image -- a
    table kept from the first run gives the second the first's scores"""
    rng = random.Random(3939)
    refs = [random_reference(rng, n) for n in (45, 80)]
    reads = ["".join(rng.choice("ACGTacgt") for _ in range(m)) for m in (30, 70, 300)]
    return tuple(refs), tuple(reads), tuple(random_profile(rng, len(q)) for q in reads)


@functools.lru_cache(maxsize=None)
def mismatch_expected(name, k):
    """{(r, q): (score, alignments, cells)} of mismatch_case() under SC_MISMATCH[k], serial ties"""
    return _expect_all(ALPHABET, *mismatch_case(), name, 0, SC_MISMATCH[k])
