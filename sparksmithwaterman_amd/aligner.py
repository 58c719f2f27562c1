"""Context / Batch: thin object wrappers over the C ABI (include/swmi.h)."""
import ctypes as C
import weakref

from . import _capi
from ._capi import Params, Timing, StreamStats, PairSpec, SwmiError, check

DEFAULT_SCORES = (5, -3, -4)              # Distribution.java:36  {match, mismatch, gap}
DEFAULT_TYPES = ("a", "i", "d", "-")      # Distribution.java:37
CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = _capi.CIGAR_M, _capi.CIGAR_I, _capi.CIGAR_D, _capi.CIGAR_EQ, _capi.CIGAR_X


def cigar_string(entries):
    """[(len, op_char), ...] as Batch.cigar returns them -> SAM's text, e.g. "12=1X3I40=" ("" for no entries; SAM writes "*")"""
    return "".join("%d%s" % (int(n), op) for n, op in entries)


def make_params(align_scores=None, align_types=None, tie_mode=_capi.TIE_SERIAL):
    sc = DEFAULT_SCORES if align_scores is None else tuple(int(x) for x in align_scores)
    ty = DEFAULT_TYPES if align_types is None else tuple(align_types)
    if len(sc) != 3 or len(ty) != 4:
        raise ValueError("alignScores needs 3 entries and alignTypes 4")
    p = Params()
    p.match, p.mismatch, p.gap = sc
    p.tie_mode = tie_mode
    p.types = b"".join(_capi.as_bytes(t)[:1] for t in ty)
    return p


def _complement_table():
    """swmi_host.h's complement_table, restated: the IUPAC pairs, S / W / N their own complements, U -> A, lower case alike"""
    t = bytearray(range(256))
    for x, y in zip(b"ATCGRYKMBVDHU", b"TAGCYRMKVBHDA"):
        t[x], t[x | 0x20] = y, y | 0x20
    return bytes(t)


COMPLEMENT = _complement_table()          # 256 bytes: the complement of every byte value (SWMI_SPEC_READ_REVCOMP)


def revcomp(seq):
    """the reverse complement of a sequence (bytes, or str of Latin-1 characters; the same type comes back), by COMPLEMENT"""
    if isinstance(seq, str):
        return seq.encode("latin-1").translate(COMPLEMENT)[::-1].decode("latin-1")
    return bytes(seq).translate(COMPLEMENT)[::-1]


def normalise_pairs(pairs):
    """The pairs of a pair list as 7-tuples (ref, read, ref_start, ref_len, read_start, read_len, reverse), a pair on the minus
    strand as that plus an eighth field "-".  An entry is (ref, read) -- both sources whole --, (ref, read, ref_start, ref_len,
    read_start, read_len), the latter plus `reverse` (true: both segments in reverse byte order, a left extension), or that
    plus the strand, "+" or "-" ("-": the read segment is taken reverse-complemented, SWMI_SPEC_READ_REVCOMP; "+" is dropped).
    A length of None or _capi.SPEC_WHOLE runs to the end of the source.  ValueError for anything else: another number of
    fields, a field that is no integer, a negative value or one past 32 bits, another strand.  Ranges against the sources are
    the library's to check (it knows them)."""
    out = []
    for k, t in enumerate(pairs):
        try:
            t = tuple(t)
        except TypeError:
            raise ValueError("pair %d: not a tuple: %r" % (k, t))
        strand = ()
        if len(t) == 8:
            if not isinstance(t[7], str) or t[7] not in ("+", "-"):
                raise ValueError("pair %d: %d fields, and the eighth is no strand (\"+\" or \"-\"): %r" % (k, len(t), t[7]))
            strand = ("-",) if t[7] == "-" else ()
        elif len(t) not in (2, 6, 7):
            raise ValueError("pair %d: %d fields; (ref, read), (ref, read, ref_start, ref_len, read_start, read_len), the latter "
                             "plus reverse, or that plus the strand" % (k, len(t)))
        rev = False
        if len(t) >= 7:
            if not isinstance(t[6], (bool, int)) or t[6] not in (0, 1):
                raise ValueError("pair %d: reverse must be a bool, got %r" % (k, t[6]))
            rev = bool(t[6])
        f = list(t[:6]) if len(t) >= 6 else [t[0], t[1], 0, None, 0, None]
        for x in (3, 5):
            if f[x] is None:
                f[x] = _capi.SPEC_WHOLE
        for x, v in enumerate(f):
            if isinstance(v, bool) or not hasattr(v, "__index__"):
                raise ValueError("pair %d: field %d is no integer: %r" % (k, x, v))
            v = f[x] = int(v)
            if v < 0 or v > 0xFFFFFFFF:
                raise ValueError("pair %d: field %d = %d is outside 0 .. 2^32 - 1" % (k, x, v))
        out.append(tuple(f) + (rev,) + strand)
    return out


def _is_minus(spec):
    """whether a normalised pair is the 8-tuple of a minus-strand pair"""
    return len(spec) == 8 and spec[7] == "-"


def cut_segments(refs, reads, spec):
    """the two segments of a normalised pair as the library aligns them: cut from the sources, reversed byte-reversed, and on
    the minus strand the read reverse-complemented (so a reversed minus pair has its read complemented in its own order);
    bytes segments, for sources given as bytes"""
    r, q, rs, rl, qs, ql, rev = spec[:7]
    ref, read = refs[r], reads[q]
    a = ref[rs:] if rl == _capi.SPEC_WHOLE else ref[rs:rs + rl]
    b = read[qs:] if ql == _capi.SPEC_WHOLE else read[qs:qs + ql]
    if _is_minus(spec):
        b = revcomp(b)
    return (a[::-1], b[::-1]) if rev else (a, b)


def cell_to_source(spec, seg_lens, i, j):
    """(read byte, reference byte), 0-based in the sources, of cell (i, j) (1-based row and column) of a normalised pair whose
    segments have the lengths seg_lens = (reference, read): start + j - 1 forward, start + len - j reversed (swmi.h); the
    read of a minus-strand pair is reversed when the pair is not, and the other way round"""
    rs, qs, rev = spec[2], spec[4], spec[6]
    n, m = seg_lens
    return (qs + m - i if rev != _is_minus(spec) else qs + i - 1), (rs + n - j if rev else rs + j - 1)


def _spec_array(specs):
    arr = (PairSpec * max(len(specs), 1))()
    for k, sp in enumerate(specs):
        r, q, rs, rl, qs, ql, rev = sp[:7]
        arr[k] = PairSpec(r, q, rs, rl, qs, ql, (_capi.SPEC_REVERSE if rev else 0) | (_capi.SPEC_READ_REVCOMP if _is_minus(sp) else 0), 0)
    return arr


def both_strands(pairs):
    """every pair of a list followed by its minus-strand twin: [p0, p0 on "-", p1, p1 on "-", ...], normalised.  The list to
    upload when the strand of a read is not known; PairBatch.best_strand picks the twin.  ValueError for a pair that is on the
    minus strand already."""
    out = []
    for k, sp in enumerate(normalise_pairs(pairs)):
        if _is_minus(sp):
            raise ValueError("pair %d is on the minus strand already: both_strands takes plus-strand pairs" % k)
        out += [sp, sp + ("-",)]
    return out


class Context:
    """One GPU + one HIP stream (swmi_ctx).  Use one per host thread."""

    def __init__(self, device=0):
        self._lib = _capi.load()
        h = C.c_void_p()
        check(self._lib.swmi_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.options = {}                   # what set_option() last set, by name
        self.score_matrix = None            # what set_score_matrix() last set: (alphabet bytes, row-major scores), or None

    def set_option(self, name, value):
        check(self._lib.swmi_set_option(self._h, name.encode(), int(value)))
        self.options[name] = int(value)

    def set_score_matrix(self, alphabet, scores=None):
        """Substitution scores (swmi_set_score_matrix): alphabet = n symbols (str or bytes, 1..64, distinct ignoring case),
        scores = n x n (rows: read base, columns: reference base), or a sparksmithwaterman_amd.matrix.ScoreMatrix as the only
        argument.  Cells with both bases in the alphabet take the matrix entry, every other cell match / mismatch as before.
        The runs asked for from now on use it (on the affine kernels, swmi_batch_mode 3)."""
        from . import matrix as _matrix
        if isinstance(alphabet, _matrix.ScoreMatrix) and scores is None:
            alphabet, scores = alphabet.alphabet, alphabet.scores
        sym, flat = _matrix.validate(alphabet, scores)
        arr = (C.c_int32 * len(flat))(*flat)
        check(self._lib.swmi_set_score_matrix(self._h, sym, len(sym), arr))
        self.score_matrix = (sym, tuple(flat))

    def clear_score_matrix(self):
        """Back to match / mismatch scoring (the linear or affine pipeline the options select)."""
        check(self._lib.swmi_set_score_matrix(self._h, None, 0, None))
        self.score_matrix = None

    def upload(self, refs, reads):
        """Sequences -> HBM.  refs/reads: lists of str or bytes."""
        return Batch(self, refs, reads)

    def upload_pairs(self, refs, reads, pairs):
        """Sources -> HBM once, and a pair list over them (swmi_batch_upload_pairs): pair k of the PairBatch is pairs[k], see
        normalise_pairs for its forms.  The segments are cut, reversed, on the minus strand complemented, and encoded on the GPU."""
        return PairBatch(self, refs, reads, pairs)

    def stream(self, reads, params=None, slots=0, chunk_bytes=0):
        """A Stream aligning `reads` against references that arrive in chunks (swmi_stream_*)."""
        return Stream(self, reads, params, slots, chunk_bytes)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.swmi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """refs x reads resident on the GPU (swmi_batch); pair index = ref * n_reads + read."""

    _owned = True

    @classmethod
    def _view(cls, lib, handle, n_refs, n_reads, owner):
        """results-only batch owned by a Stream.  The view keeps the Stream alive (swmi_stream_close frees every result
        batch), and Stream.close() sets its handle to None: the library answers a NULL batch with SWMI_ERR_INVALID, so a
        late call raises SwmiError instead of touching freed memory."""
        b = cls.__new__(cls)
        b._ctx, b._lib, b._h, b.n_refs, b.n_reads, b._owned = None, lib, handle, n_refs, n_reads, False
        b._owner = owner
        return b

    def __init__(self, ctx, refs, reads):
        self._ctx = ctx
        self._lib = ctx._lib
        self.n_refs, self.n_reads = len(refs), len(reads)
        rb, ro = _capi.pack(refs)
        qb, qo = _capi.pack(reads)
        h = C.c_void_p()
        check(self._lib.swmi_batch_upload(ctx._h, rb, ro, self.n_refs, qb, qo, self.n_reads, C.byref(h)))
        self._h = h
        self._read_off = qo                 # (the reads' lengths, for set_read_profiles)
        self.read_profiles = None           # what set_read_profiles() last set: (alphabet bytes, number of symbols), or None

    def n_pairs(self):
        return self.n_refs * self.n_reads

    def set_read_profiles(self, alphabet, profiles=None):
        """Per-read score profiles (swmi_batch_set_read_profiles): alphabet = n symbols as for
        Context.set_score_matrix, profiles = one m_q x n integer array per read of the batch, in upload order -- row i scores
        read position i against each symbol of the REFERENCE; a reference byte outside the alphabet scores `mismatch`.
        set_read_profiles(None) clears them.  The old results are dropped: run the batch again."""
        import numpy as np
        from . import matrix as _matrix
        if alphabet is None:
            if profiles is not None:
                raise ValueError("profiles without an alphabet")
            check(self._lib.swmi_batch_set_read_profiles(self._ctx._h, self._h, None, 0, None))
            self.read_profiles = None
            return self
        if profiles is None:
            raise ValueError("an alphabet without profiles (set_read_profiles(None) clears them)")
        sym = _matrix._symbols(alphabet)
        n = len(sym)
        off = getattr(self, "_read_off", None)        # (a pair list has none: the library refuses it)
        lens = None if off is None else [off[q + 1] - off[q] for q in range(self.n_reads)]
        if lens is not None and len(profiles) != len(lens):
            raise ValueError("%d profiles for %d reads" % (len(profiles), len(lens)))
        rows = []
        for q, p in enumerate(profiles):
            a = np.asarray(p)
            if a.size and not np.all(a == np.floor(a)):
                raise ValueError("profile %d has entries that are not integers" % q)
            a = a.astype(np.int64).reshape(-1, n) if a.size else np.zeros((0, n), np.int64)
            if lens is not None and a.shape[0] != lens[q]:
                raise ValueError("profile %d has %d rows of %d entries for a read of %d bases" % (q, a.shape[0], n, lens[q]))
            if a.size and int(np.abs(a).max()) > _matrix.MAX_ABS_SCORE:
                raise ValueError("profile %d: |entries| must be <= 2^20" % q)
            rows.append(a)
        flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, n)), dtype=np.int32)
        ptr = flat.ctypes.data_as(C.POINTER(C.c_int32)) if flat.size else (C.c_int32 * 1)()
        check(self._lib.swmi_batch_set_read_profiles(self._ctx._h, self._h, sym, n, ptr))
        self.read_profiles = (sym, n)
        return self

    def run(self, params=None):
        """Fill + traceback on the GPU for every pair, results to the host.  Synchronous."""
        p = params if params is not None else make_params()
        check(self._lib.swmi_batch_run(self._ctx._h, self._h, C.byref(p)))
        return self

    def run_async(self, params=None):
        """Starts the same run on the context's own host thread and returns at once; wait() completes it."""
        p = params if params is not None else make_params()
        self._async_params = p                     # (copied by the library before the call returns; kept for clarity)
        check(self._lib.swmi_batch_run_async(self._ctx._h, self._h, C.byref(p)))
        return self

    def wait(self):
        """Blocks until the run started by run_async() has finished; raises what it raised."""
        check(self._lib.swmi_batch_wait(self._ctx._h))
        return self

    def timing(self):
        t = Timing()
        check(self._lib.swmi_batch_timing(self._h, C.byref(t)))
        return t

    def pipeline_mode(self):
        v = C.c_int()
        check(self._lib.swmi_batch_mode(self._h, C.byref(v)))
        return v.value

    # ---- per pair -------------------------------------------------------------------
    def score(self, pair):
        v = C.c_int32()
        check(self._lib.swmi_pair_score(self._h, pair, C.byref(v)))
        return v.value

    def n_alignments(self, pair):
        n, f = C.c_uint64(), C.c_uint32()
        check(self._lib.swmi_pair_n_alignments(self._h, pair, C.byref(n), C.byref(f)))
        return n.value, f.value

    def rows_swept(self, pair):
        """the read rows the pair's sweep covered: the read's length, or 1024 * (strips swept) when option "xdrop" stopped it"""
        v = C.c_uint32()
        check(self._lib.swmi_pair_rows_swept(self._h, pair, C.byref(v)))
        return v.value

    def band_window(self, pair, strip):
        """(c_lo, c_hi): the reference columns the pair's sweep used for strip `strip` (rows 1024 * strip + 1 ..) of the read -- (1, n)
        without a band or for a read of at most 1024 bases, the staircase's window under option "band", the window the sweep
        placed under option "band_adapt"; SwmiError (SWMI_ERR_RANGE) for a strip the read does not have or "xdrop" did not sweep"""
        lo, hi = C.c_uint32(), C.c_uint32()
        check(self._lib.swmi_pair_band_window(self._h, pair, strip, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def alignment(self, pair, k, with_cell=False):
        b, ei, ej = C.c_int32(), C.c_int32(), C.c_int32()
        r, q, ln = C.c_char_p(), C.c_char_p(), C.c_uint32()
        check(self._lib.swmi_pair_alignment(self._h, pair, k, C.byref(b), C.byref(ei), C.byref(ej),
                                            C.byref(r), C.byref(q), C.byref(ln)))
        rec = (b.value, (r.value.decode("latin-1"), q.value.decode("latin-1")))
        return rec + ((ei.value, ej.value),) if with_cell else rec

    def alignments(self, pair, with_cell=False):
        n, _ = self.n_alignments(pair)
        return [self.alignment(pair, k, with_cell) for k in range(n)]

    def cigar(self, pair, k):
        """(begin, end_i, end_j, [(len, op_char), ...], nm) of the k-th alignment after a run under option "cigar" (1: M / I / D,
        2: = / X / I / D): entries from the start of the alignment to its end cell, nm = X columns + inserted + deleted bases.
        SwmiError (SWMI_ERR_UNSUPPORTED) after a run with cigar = 0 or scores_only = 1."""
        b, ei, ej = C.c_int32(), C.c_int32(), C.c_int32()
        p, n, nm = C.POINTER(C.c_uint32)(), C.c_uint32(), C.c_uint32()
        check(self._lib.swmi_pair_cigar(self._h, pair, k, C.byref(b), C.byref(ei), C.byref(ej), C.byref(p), C.byref(n), C.byref(nm)))
        ent = [(p[x] >> 4, _capi.CIGAR_CHARS.get(p[x] & 15, "?")) for x in range(n.value)]
        return b.value, ei.value, ej.value, ent, nm.value

    def cigars(self, pair):
        n, _ = self.n_alignments(pair)
        return [self.cigar(pair, k) for k in range(n)]

    def span(self, pair, k):
        """(read_first, end_i, begin, end_j) of the k-th alignment, 1-based and inclusive: it spells read[read_first .. end_i] against
        ref[begin .. end_j].  read_first = end_i - (read bases the alignment consumes) + 1, counted from the CIGAR after a run under
        option "cigar" and else from the read's aligned string.  What the caller of an overlap run (option "overlap") needs to tell
        a dovetail from a containment: the results themselves carry begin, end_i and end_j only."""
        try:
            begin, ei, ej, ent, _ = self.cigar(pair, k)
            used = sum(ln for ln, op in ent if op != "D")
        except SwmiError as e:
            if e.code != _capi.ERR_UNSUPPORTED:
                raise
            begin, (_, read_al), (ei, ej) = self.alignment(pair, k, with_cell=True)
            used = len(read_al) - read_al.count("_")              # (the gap character of the aligned strings)
        return ei - used + 1, ei, begin, ej

    def pair_results(self):
        """(scores int32[n_pairs], n_alignments uint64[n_pairs]) as numpy arrays, one native call."""
        import numpy as np
        n = self.n_pairs()
        sc = np.empty(n, dtype=np.int32)
        na = np.empty(n, dtype=np.uint64)
        check(self._lib.swmi_batch_pair_results(self._h, sc.ctypes.data_as(C.POINTER(C.c_int32)),
                                                na.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return sc, na

    def scores(self):
        """every pair's score as a numpy int32 array (also after a scores_only run, which has no alignment counts)"""
        import numpy as np
        n = self.n_pairs()
        sc = np.empty(n, dtype=np.int32)
        check(self._lib.swmi_batch_pair_results(self._h, sc.ctypes.data_as(C.POINTER(C.c_int32)), None, n))
        return sc

    def subopt(self, pair):
        """(score2, end2) after a run under option "subopt": the pair's second-best local score and the 1-based reference column it
        ends in (on a pair list: of the segment; PairBatch.to_source maps it), (0, 0) when there is none.  Works after a scores_only
        run.  SwmiError (SWMI_ERR_UNSUPPORTED) after a run with subopt = 0."""
        s2, e2 = C.c_int32(), C.c_uint32()
        check(self._lib.swmi_pair_subopt(self._h, pair, C.byref(s2), C.byref(e2)))
        return s2.value, e2.value

    def subopts(self):
        """(scores2 int32[n_pairs], ends2 uint32[n_pairs]) as numpy arrays, one native call."""
        import numpy as np
        n = self.n_pairs()
        s2 = np.empty(n, dtype=np.int32)
        e2 = np.empty(n, dtype=np.uint32)
        check(self._lib.swmi_batch_pair_subopt(self._h, s2.ctypes.data_as(C.POINTER(C.c_int32)),
                                               e2.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return s2, e2

    def hits(self, pair):
        """[(score, end_i, end_j), ...] after a run under options "subopt" and "hits": the pair's best local hits, best first, each
        with the 1-based cell it ends in (read row, reference column; on a pair list: of the segments).  Entry 0 is the primary,
        entry 1 is subopt(pair); an empty list for a degenerate pair or one with an empty side.  Works after a scores_only run.
        SwmiError (SWMI_ERR_UNSUPPORTED) after a run with hits = 0."""
        n = C.c_uint32()
        arr = (_capi.Hit * _capi.HITS_MAX)()
        check(self._lib.swmi_pair_hits(self._h, pair, arr, _capi.HITS_MAX, C.byref(n)))
        return [(arr[k].score, arr[k].end_i, arr[k].end_j) for k in range(n.value)]

    def hits_all(self, k=_capi.HITS_MAX):
        """(counts uint32[n_pairs], scores int32[n_pairs, k], end_i uint32[n_pairs, k], end_j uint32[n_pairs, k]) as numpy arrays, one
        native call; the entries past a pair's count are 0.  k: the columns, at least the run's hits (default: the most there can be)."""
        import numpy as np
        n = self.n_pairs()
        cnt = np.empty(n, dtype=np.uint32)
        raw = np.zeros((n, int(k), 4), dtype=np.uint32)
        check(self._lib.swmi_batch_pair_hits(self._h, raw.ctypes.data_as(C.POINTER(_capi.Hit)), int(k),
                                             cnt.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return cnt, raw[:, :, 0].astype(np.int32), raw[:, :, 1].copy(), raw[:, :, 2].copy()

    def _hit_spec(self, pair, i, j):
        """the reverse-extension spec of a hit (i, j) of the pair: both prefixes that end in the cell, reversed"""
        return (pair // self.n_reads, pair % self.n_reads, 0, j, 0, i, _capi.SPEC_REVERSE)

    def hit_specs(self, pair=None):
        """The pair specs of the REVERSE EXTENSIONS of the hits -- of one pair, or of every pair in pair order: for a hit (i, j) of
        the pair (ref r, read q) the spec (r, q, 0, j, 0, i, SPEC_REVERSE), ready for Context.upload_pairs on the same sources.  An
        extend run over them finds, per hit, where its alignment starts: the extend score equals the hit's score, and the end cell
        of that run, mapped with PairBatch.to_source, is the alignment's first cell."""
        pairs = range(self.n_pairs()) if pair is None else [pair]
        return [self._hit_spec(p, i, j) for p in pairs for _, i, j in self.hits(p)]

    def end_score(self, pair):
        """(max_score, end_score, end_col) after an extend run under option "end_bonus": the pair's best score anywhere (whether or
        not the pair was taken to the end), its best score in the read's last row and the smallest 1-based reference column that holds
        it (on a pair list: of the segment; PairBatch.to_source maps it); (0, 0, 0) for a pair with an empty side.  The flags of
        n_alignments carry PAIR_TO_END for a pair that was taken.  Works after a scores_only run.  SwmiError (SWMI_ERR_UNSUPPORTED)
        after a run with end_bonus = 0."""
        ms, es, ec = C.c_int32(), C.c_int32(), C.c_uint32()
        check(self._lib.swmi_pair_end_score(self._h, pair, C.byref(ms), C.byref(es), C.byref(ec)))
        return ms.value, es.value, ec.value

    def end_scores(self):
        """(max_scores int32[n_pairs], end_scores int32[n_pairs], end_cols uint32[n_pairs]) as numpy arrays, one native call."""
        import numpy as np
        n = self.n_pairs()
        ms = np.empty(n, dtype=np.int32)
        es = np.empty(n, dtype=np.int32)
        ec = np.empty(n, dtype=np.uint32)
        check(self._lib.swmi_batch_pair_end_scores(self._h, ms.ctypes.data_as(C.POINTER(C.c_int32)), es.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   ec.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return ms, es, ec

    def materialise_all(self):
        """Index the records and build every alignment string natively; returns (n_alignments, n_chars)."""
        na, nc = C.c_uint64(), C.c_uint64()
        check(self._lib.swmi_batch_materialise_all(self._h, C.byref(na), C.byref(nc)))
        return na.value, nc.value

    # ---- MapRef view -----------------------------------------------------------------
    def ref_total(self, ref):
        v = C.c_int32()
        check(self._lib.swmi_ref_total(self._h, ref, C.byref(v)))
        return v.value

    def ref_totals(self):
        """numpy int32 array of every reference's total (one native call)."""
        import numpy as np
        out = np.empty(self.n_refs, dtype=np.int32)
        check(self._lib.swmi_ref_totals(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), self.n_refs))
        return out

    def ref_match_sites(self, ref):
        n = C.c_uint64()
        check(self._lib.swmi_ref_n_match_sites(self._h, ref, C.byref(n)))
        out = []
        b, r, q, ln = C.c_int32(), C.c_char_p(), C.c_char_p(), C.c_uint32()
        for k in range(n.value):
            check(self._lib.swmi_ref_match_site(self._h, ref, k, C.byref(b), C.byref(r), C.byref(q), C.byref(ln)))
            out.append((b.value, (r.value.decode("latin-1"), q.value.decode("latin-1"))))
        return out

    def ref_sites_packed(self, ref_lo=0, ref_hi=None):
        """MapRef's output of references ref_lo .. ref_hi-1 in two native calls (sizes, then data): a list of
        (total, n_degenerate, [(begin, (refAligned, readAligned)), ...]) -- what swmi_ref_sites_packed hands a JNI binding."""
        import numpy as np
        ref_hi = self.n_refs if ref_hi is None else ref_hi
        n = ref_hi - ref_lo
        ns, nb = C.c_uint64(), C.c_uint64()
        check(self._lib.swmi_ref_sites_packed(self._h, ref_lo, ref_hi, None, None, None, None, None, None, 0, None, 0,
                                              C.byref(ns), C.byref(nb)))
        totals = np.empty(max(n, 1), dtype=np.int32)
        deg = np.empty(max(n, 1), dtype=np.uint64)
        first = np.empty(n + 1, dtype=np.uint64)
        begins = np.empty(max(ns.value, 1), dtype=np.int32)
        lens = np.empty(max(ns.value, 1), dtype=np.uint32)
        off = np.empty(max(ns.value, 1), dtype=np.uint64)
        blob = np.empty(max(nb.value, 1), dtype=np.uint8)
        P = C.POINTER
        check(self._lib.swmi_ref_sites_packed(
            self._h, ref_lo, ref_hi, totals.ctypes.data_as(P(C.c_int32)), deg.ctypes.data_as(P(C.c_uint64)),
            first.ctypes.data_as(P(C.c_uint64)), begins.ctypes.data_as(P(C.c_int32)), lens.ctypes.data_as(P(C.c_uint32)),
            off.ctypes.data_as(P(C.c_uint64)), ns.value, blob.ctypes.data_as(C.c_void_p), nb.value, C.byref(ns), C.byref(nb)))
        raw = blob.tobytes()
        out = []
        for r in range(n):
            sites = []
            for s in range(int(first[r]), int(first[r + 1])):
                o, ln = int(off[s]), int(lens[s])
                sites.append((int(begins[s]), (raw[o:o + ln].decode("latin-1"), raw[o + ln:o + 2 * ln].decode("latin-1"))))
            out.append((int(totals[r]), int(deg[r]), sites))
        return out

    def free(self):
        if getattr(self, "_h", None) and self._owned:
            self._lib.swmi_batch_free(self._ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PairBatch(Batch):
    """A pair list over sources resident on the GPU (swmi_batch_upload_pairs): pair k is the k-th pair given, coordinates are
    the segments' (to_source maps them back).  The MapRef views (ref_*) need the cross product and raise SwmiError."""

    def __init__(self, ctx, refs, reads, pairs):
        self._ctx = ctx
        self._lib = ctx._lib
        self._refs = [_capi.as_bytes(s) for s in refs]
        self._reads = [_capi.as_bytes(s) for s in reads]
        self.n_refs, self.n_reads = len(self._refs), len(self._reads)      # the SOURCES
        self._specs = normalise_pairs(pairs)
        rb, ro = _capi.pack(self._refs)
        qb, qo = _capi.pack(self._reads)
        h = C.c_void_p()
        check(self._lib.swmi_batch_upload_pairs(ctx._h, rb, ro, self.n_refs, qb, qo, self.n_reads, _spec_array(self._specs),
                                                len(self._specs), C.byref(h)))
        self._h = h

    def n_pairs(self):
        return len(self._specs)

    def set_pairs(self, pairs):
        """another list on the same resident sources (swmi_batch_set_pairs); the results of the old one are dropped.  A list
        the library refuses leaves the batch as it was."""
        specs = normalise_pairs(pairs)
        check(self._lib.swmi_batch_set_pairs(self._ctx._h, self._h, _spec_array(specs), len(specs)))
        self._specs = specs
        return self

    def _hit_spec(self, pair, i, j):
        """... on a pair list with an unreversed spec: offset by the spec's starts.  ValueError for a reversed spec (its cells count
        from the segments' ends: the prefixes that end in the cell are no prefixes of the sources' segments).  On the minus
        strand rows 1 .. i are the LAST i bytes of the read segment: (r, q, rs, j, qs + ql - i, i, True, "-")."""
        r, q, rs, _, qs, ql, rev = self._specs[pair][:7]
        if rev:
            raise ValueError("pair %d has a reversed spec: hit_specs needs unreversed segments" % pair)
        if _is_minus(self._specs[pair]):
            if ql == _capi.SPEC_WHOLE:
                ql = len(self._reads[q]) - qs
            return (r, q, rs, j, qs + ql - i, i, True, "-")
        return (r, q, rs, j, qs, i, _capi.SPEC_REVERSE)

    def spec(self, pair):
        """(ref, read, ref_start, ref_len, read_start, read_len, reverse) of the pair as the library holds it: lengths resolved;
        a minus-strand pair as that plus "-" """
        sp = PairSpec()
        check(self._lib.swmi_batch_pair_spec(self._h, pair, C.byref(sp)))
        strand = ("-",) if sp.flags & _capi.SPEC_READ_REVCOMP else ()
        return (sp.ref, sp.read, sp.ref_start, sp.ref_len, sp.read_start, sp.read_len, bool(sp.flags & _capi.SPEC_REVERSE)) + strand

    def strand(self, pair):
        """"+" or "-": the strand the pair was given"""
        return "-" if _is_minus(self._specs[pair]) else "+"

    def best_strand(self):
        """On a list built by both_strands, after a run: per input pair the index (in this batch) of the twin with the higher
        score; a tie goes to the plus strand.  ValueError on any other list."""
        sp = self._specs
        if len(sp) % 2 or any(_is_minus(sp[k]) or sp[k + 1] != sp[k] + ("-",) for k in range(0, len(sp), 2)):
            raise ValueError("best_strand needs a list built by both_strands: every pair followed by its minus twin")
        sc = self.scores()
        return [k + 1 if sc[k + 1] > sc[k] else k for k in range(0, len(sp), 2)]

    def segments(self, pair):
        """(reference segment, read segment) of the pair as str, cut -- reversed, and on the minus strand complemented -- on the host"""
        a, b = cut_segments(self._refs, self._reads, self._specs[pair])
        return a.decode("latin-1"), b.decode("latin-1")

    def to_source(self, pair, i, j):
        """(read byte, reference byte), 0-based in the sources, of cell (i, j) of the pair (1-based, as end_i / end_j)"""
        a, b = cut_segments(self._refs, self._reads, self._specs[pair])
        return cell_to_source(self._specs[pair], (len(a), len(b)), i, j)


class Stream:
    """Reads resident, references streamed through the GPU in chunks (include/swmi.h: swmi_stream_*)."""

    def __init__(self, ctx, reads, params=None, slots=0, chunk_bytes=0):
        self._ctx, self._lib = ctx, ctx._lib
        self.n_reads = len(reads)
        qb, qo = _capi.pack(reads)
        p = params if params is not None else make_params()
        h = C.c_void_p()
        check(self._lib.swmi_stream_open(ctx._h, C.byref(p), qb, qo, self.n_reads, int(slots), int(chunk_bytes), C.byref(h)))
        self._h = h
        self._views = []                  # weak references to the result views handed out by chunks()

    def push(self, refs):
        rb, ro = _capi.pack(refs)
        check(self._lib.swmi_stream_push(self._h, rb, ro, len(refs)))
        return self

    def push_file(self, path, delimiter=">gi", parse_threads=0):
        import os
        check(self._lib.swmi_stream_push_file(self._h, os.fspath(path).encode(), delimiter.encode("latin-1"), int(parse_threads)))
        return self

    def push_file_shard(self, path, shard, n_shards, delimiter=">gi", parse_threads=0):
        """shard `shard` of `n_shards` of a FASTA file: the records whose metadata line starts in the shard's byte range
        (swmi_stream_push_file_shard); (0, 1) is push_file"""
        import os
        check(self._lib.swmi_stream_push_file_shard(self._h, os.fspath(path).encode(), delimiter.encode("latin-1"),
                                                    int(parse_threads), int(shard), int(n_shards)))
        return self

    def finish(self):
        check(self._lib.swmi_stream_finish(self._h))
        return self

    def n_refs(self):
        return self._lib.swmi_stream_n_refs(self._h)

    def chunks(self):
        """[(first_ref, Batch view), ...] in reference order"""
        out = []
        for k in range(self._lib.swmi_stream_n_chunks(self._h)):
            b, first = C.c_void_p(), C.c_uint64()
            check(self._lib.swmi_stream_chunk(self._h, k, C.byref(b), C.byref(first)))
            n_pairs = self._lib.swmi_batch_n_pairs(b)
            v = Batch._view(self._lib, b, n_pairs // max(self.n_reads, 1), self.n_reads, self)
            self._views.append(weakref.ref(v))
            out.append((first.value, v))
        return out

    def totals(self):
        import numpy as np
        n = self.n_refs()
        out = np.empty(n, dtype=np.int32)
        if n:                                       # (a shard may hold no reference)
            check(self._lib.swmi_stream_totals(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return out

    def ref_pos(self, ref):
        """byte offset of reference `ref`'s metadata line in its file (file sources)"""
        v = C.c_uint64()
        check(self._lib.swmi_stream_ref_pos(self._h, ref, C.byref(v)))
        return v.value

    def ref_sequence(self, ref):
        """reference `ref`'s sequence as bytes (re-read from the mapped file for file sources)"""
        n = C.c_uint64()
        check(self._lib.swmi_stream_ref_sequence(self._h, ref, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        check(self._lib.swmi_stream_ref_sequence(self._h, ref, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def metadata(self, ref):
        cap = 4096
        while True:                                 # (the library truncates to the buffer: grow it until the line fits)
            buf = C.create_string_buffer(cap)
            check(self._lib.swmi_stream_metadata(self._h, ref, buf, cap))
            if len(buf.value) < cap - 1:
                return buf.value.decode("latin-1")
            cap *= 4

    def stats(self):
        st = StreamStats()
        check(self._lib.swmi_stream_get_stats(self._h, C.byref(st)))
        return st

    def close(self):
        if getattr(self, "_h", None):
            for w in getattr(self, "_views", []):      # the native close frees every result batch: no view may outlive it
                v = w()
                if v is not None:
                    v._h = None
            self._views = []
            self._lib.swmi_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
