"""The pass of sw_subopt_kernel and sw_hits_kernel (swmi_subopt.hip), transcribed into plain Python over a row of ints -- TEST
INFRASTRUCTURE ONLY.

Not collected by pytest (no test_ prefix).  A MODEL FOR CHOOSING CASES, NOT A SECOND REFERENCE: no GPU value is ever compared with
it.  The expected values of every test come from the rule (subopt_reference.reduce_colmax, hits_reference.pick and their numpy
forms).  The model serves two ends, both in tests/test_pick_cpu.py:

  the trace      which branches of the pass a row takes (BRANCHES), so that the cases of tests/pick_cases.py can be shown to reach all
                 of them between them;
  the mutations  named one-line changes of the pass (MUTATIONS): a case set whose expected values differ from what every mutated
                 model returns would notice a kernel that is wrong in that way.

The transcription keeps the kernel's names and order: `step` with its ballot `mk`, the lookahead with `scan` and `nxt`, the lane
masks `ml` / `mr`, the carried `L`, the unrolled loop of four steps with its guarded fourth load, the tail loop, the two
wave_max_i32 reductions, and in a hits round the readlane tests of the earlier entries' columns `pj`.  Wave-uniform values are
Python ints, per-lane values lists of 64.  One liberty: the lane loop of a step visits only the lanes with `valid && v > bv`, the
first and the last term of the kernel's conjunction -- no other lane can change its state.

A shift count is taken modulo 64, as the hardware's 64-bit shifts take it: that is what makes "one lane short" a change at all (lane
0's left mask and lane 63's right mask become the whole ballot, every other lane's loses only its own bit, which the other mask
still holds).
"""
WAVE = 64
FULL = (1 << 64) - 1
FAR = 1 << 40

BRANCHES = (
    "b0", "b1", "b2", "b3",             # the lookahead finds the next maximum column in its first .. fourth in-flight load
    "quad_skipped",                     # ... in none of the four: 256 columns further
    "row_exhausted",                    # ... runs off the row: no maximum column behind this step
    "nxt_kept",                         # a step begins with the column found for an earlier one still ahead
    "nxt_searched_again",               # the pass has moved beyond a found column: the search resumes
    "left_from_ml", "left_from_L",      # a lane's left neighbour is a ballot bit of its own step / the carried L of an earlier step
    "right_from_mr", "right_from_nxt",  # the right one likewise a bit of its own step / the lookahead's column
    "L_decides", "nxt_decides",         # ... and a positive column is masked by L alone / by nxt alone
    "unrolled_quad", "tail_step",       # the two loops
    "fourth_load_guarded_out",          # the unrolled loop's fourth load runs past the row's end in some lane
    "earlier_entry_loop",               # a hits round tests the earlier entries' columns (some lane has a candidate, nprev > 1)
    "earlier_entry_masks",              # ... and one of them masks a candidate
)

# name -> what the kernel would have to get wrong.  `equivalent`: the change cannot alter a value (see test_pick_cpu.py, which
# asserts that instead of a kill)
MUTATIONS = {
    "mask_left_ge": "a column w away from the maximum column on its left counts as outside the mask: j - lcol >= w",
    "mask_right_ge": "likewise on the right: rcol - j >= w",
    "ml_one_lane_short": "ml = mk & (~0 >> (64 - lane))",
    "mr_one_lane_short": "mr = mk & (~0 << (lane + 1))",
    "L_not_carried": "L stays at its start value",
    "nxt_from_end_plus_64": "the lookahead starts one step behind the step's end",
    "scan_not_advanced": "scan += k * WAVE left out after a find in load k: nxt is k steps short",
    "nxt_not_searched_again": "the lookahead runs once per pass",
    "fourth_load_unguarded": "v3 = row[j3] without the guard reads what lies behind the row (0, or a stale maximum)",
    "lookahead_load_unguarded": "u0 .. u3 of the lookahead without their guards read a stale maximum behind the row",
    "earlier_from_q0": "the earlier entries are tested from q = 0: lane 0's pj, which is 0",
    "earlier_from_q2": "... from q = 2: entry 1's column is not masked",
    "earlier_ge": "d >= w || -d >= w around an earlier entry",
    "largest_column": "the largest column among the holders of the maximum",
}
EQUIVALENT = {"fourth_load_unguarded": "`valid` guards both uses of v in step: a lane past the row's end neither sets a ballot bit nor keeps a value"}


def ctz(x):
    return (x & -x).bit_length() - 1


def clz(x):
    return 64 - x.bit_length()


def ballot(flags):
    b = 0
    for lane, f in enumerate(flags):
        if f:
            b |= 1 << lane
    return b


class Pass:
    """one ascending pass over row[0 .. cols - 1]: sw_subopt_kernel's body, and hits_round with pj / nprev"""

    def __init__(self, row, s, w, pj=None, nprev=1, mut=None, trace=None, pad=None):
        self.row, self.cols, self.s, self.w = row, len(row), s, w
        self.pj, self.nprev = pj or [0] * WAVE, nprev
        self.mut, self.trace = mut, trace if trace is not None else set()
        self.pad = s if pad is None else pad                    # what an unguarded load finds behind the row: at worst a stale maximum
        self.L, self.nxt, self.scan = -FAR, -1, 0
        self.bv, self.bc = [0] * WAVE, [0] * WAVE
        self.searched = False

    def load(self, i, guarded=True):
        if i < self.cols:
            return self.row[i]
        return -1 if guarded else self.pad

    def lookahead(self, end):
        row_guard = self.mut != "lookahead_load_unguarded"
        if self.scan < end:
            self.scan = end + (WAVE if self.mut == "nxt_from_end_plus_64" else 0)
        self.nxt = FAR
        while self.scan < self.cols:
            b = []
            for k in range(4):
                b.append(ballot(self.load(self.scan + k * WAVE + lane, row_guard) == self.s for lane in range(WAVE)))
            for k in range(4):
                if b[k]:
                    if self.mut != "scan_not_advanced":
                        self.scan += k * WAVE
                    self.nxt = self.scan + ctz(b[k])
                    self.trace.add("b%d" % k)
                    return
            self.scan += 4 * WAVE
            self.trace.add("quad_skipped")
        self.trace.add("row_exhausted")

    def step(self, base, v):
        s, w, cols, mut, trace = self.s, self.w, self.cols, self.mut, self.trace
        end = base + WAVE
        nvalid = min(WAVE, cols - base) if cols > base else 0
        mk = ballot(lane < nvalid and v[lane] == s for lane in range(WAVE))
        if self.nxt < end:
            if not (mut == "nxt_not_searched_again" and self.searched):
                if self.searched:
                    trace.add("nxt_searched_again")
                self.searched = True
                self.lookahead(end)
        elif self.nxt != FAR:
            trace.add("nxt_kept")
        L, nxt = self.L, self.nxt
        if mk:
            trace.update(("left_from_ml", "right_from_mr"))
        if L != -FAR and (not mk or ctz(mk) > 0):
            trace.add("left_from_L")
        if nxt != FAR and (not mk or 63 - clz(mk) < nvalid - 1):
            trace.add("right_from_nxt")
        cand = [lane for lane in range(nvalid) if v[lane] > self.bv[lane]]
        ok = {}
        for lane in cand:
            j = base + lane
            ml = mk & (FULL >> (63 - lane))
            mr = mk & (FULL << lane) & FULL
            if mut == "ml_one_lane_short":
                ml = mk & (FULL >> ((64 - lane) % 64))
            if mut == "mr_one_lane_short":
                mr = mk & (FULL << ((lane + 1) % 64)) & FULL
            lcol = base + 63 - clz(ml) if ml else L
            rcol = base + ctz(mr) if mr else nxt
            left = j - lcol >= w if mut == "mask_left_ge" else j - lcol > w
            right = rcol - j >= w if mut == "mask_right_ge" else rcol - j > w
            if not ml and not left and right:
                trace.add("L_decides")
            if not mr and not right and left:
                trace.add("nxt_decides")
            ok[lane] = left and right
        # the earlier entries' end columns (one readlane each); only while some lane still has a candidate
        if any(ok.values()):
            first = {"earlier_from_q0": 0, "earlier_from_q2": 2}.get(mut, 1)
            for q in range(first, self.nprev):
                trace.add("earlier_entry_loop")
                for lane in cand:
                    d = base + lane - self.pj[q]
                    far = (d >= w or -d >= w) if mut == "earlier_ge" else (d > w or -d > w)
                    if ok[lane] and not far:
                        trace.add("earlier_entry_masks")
                    ok[lane] = ok[lane] and far
        for lane in cand:
            if ok[lane]:
                self.bv[lane], self.bc[lane] = v[lane], base + lane
        if mk and mut != "L_not_carried":
            self.L = base + 63 - clz(mk)

    def run(self):
        """(smax, col): the largest eligible column maximum (0: none) and the smallest 0-based column that holds it"""
        cols, base = self.cols, 0
        while base + 3 * WAVE < cols:
            self.trace.add("unrolled_quad")
            if base + 4 * WAVE > cols:
                self.trace.add("fourth_load_guarded_out")
            vs = [[self.load(base + k * WAVE + lane, not (k == 3 and self.mut == "fourth_load_unguarded")) for lane in range(WAVE)] for k in range(4)]
            for k in range(4):
                self.step(base + k * WAVE, vs[k])
            base += 4 * WAVE
        while base < cols:
            self.trace.add("tail_step")
            self.step(base, [self.load(base + lane) for lane in range(WAVE)])
            base += WAVE
        smax = max(self.bv)
        if smax <= 0:
            return smax, 0
        holders = [self.bc[lane] for lane in range(WAVE) if self.bv[lane] == smax]
        return smax, max(holders) if self.mut == "largest_column" else min(holders)


def subopt(row, s, w, mut=None, trace=None, pad=None):
    """sw_subopt_kernel on row[0 ..] (colmax of the columns 1 ..), the pair's score s > 0 and the half-width w: (score2, end2)"""
    smax, p = Pass(row, s, w, mut=mut, trace=trace, pad=pad).run()
    return (smax, p + 1) if smax > 0 else (0, 0)


def hits(row, rrow, s, w, K, mut=None, trace=None, pad=None):
    """sw_hits_kernel on the two rows: (the list of (score, end_i, end_j), (score2, end2))"""
    cols = len(row)
    # entry 0: the first maximum column, four loads in flight per lane
    j0, base = None, 0
    while base < cols and j0 is None:
        for k in range(4):
            b = ballot((row[i] if i < cols else -1) == s for i in range(base + k * WAVE, base + (k + 1) * WAVE))
            if b:
                j0 = base + k * WAVE + ctz(b)
                break
        base += 4 * WAVE
    out, res = [], (0, 0)
    if j0 is None:
        return out, res
    out.append((s, rrow[j0], j0 + 1))
    pj = [0] * WAVE                                             # lane q, q >= 1: the 0-based end column of entry q
    for k in range(1, max(K, 2)):
        smax, p = Pass(row, s, w, pj, k, mut, trace, pad).run()
        if smax <= 0:
            break
        if k == 1:
            res = (smax, p + 1)
        if k < K:
            out.append((smax, rrow[p], p + 1))
            pj[k] = p
    return out, res
