"""Host-side mirror of the reference's operator interface for the hot path.

Same class names, argument meaning and return shapes as the Java function objects, so a
test written against the reference reads the same here:

  SmithWaterman.OptAlignments().call(seqs, alignScores, alignTypes)
        -> (score, [(begin, (refAligned, readAligned)), ...])      src/sw/SmithWaterman.java:35,62-92
  DistributedSW.OptAlignments().call(...)   same, '>' tie order       src/sw/DistributedSW.java:50,77-104
  Distribution.MapRef().call((ref, reads, (alignScores, alignTypes)))
        -> (total, (ref, matchSites))                               src/sw/Distribution.java:383,403-436
  Distribution.MapPartition().call(iterable of such tuples)        one native call per partition
  Distribution.CombineReadsToRef().call(refs, reads, algoArgs)      src/sw/Distribution.java:702-725
  Distribution.ReduceMax                                           control-path max-with-ties, :600-613, :647-666

All alignment work happens in libswmi.so on the GPU; nothing here computes a score.
"""
import contextlib as _contextlib

from . import _capi
from .aligner import Context, make_params, DEFAULT_SCORES, DEFAULT_TYPES

_default_ctx = {}


def default_context(device=0):
    c = _default_ctx.get(device)
    if c is None:
        c = _default_ctx[device] = Context(device)
    return c


def _algo(align_scores, align_types):
    return (DEFAULT_SCORES if align_scores is None else align_scores,
            DEFAULT_TYPES if align_types is None else align_types)


@_contextlib.contextmanager
def _scores(ctx, align_scores, align_mode=None, long_reads=None, band=None, extend=None, xdrop=None, band_adapt=None, end_bonus=None, overlap=None):
    """alignScores {match, mismatch, gap}, {match, mismatch, gap, gapOpen} or {match, mismatch, gap, gapOpen, gap2, gapOpen2}:
    yields the three entries make_params takes and, for four, sets the context's "gap_open" for the call (affine gaps: a gap of
    length k costs gapOpen + k * gap); for six also "gap2" and "gap_open2" (two-piece gaps on a global or extend run: a gap costs
    max(gapOpen + k * gap, gapOpen2 + k * gap2); gapOpen2 = 0 is a one-piece run).
    align_mode (ALIGN_LOCAL / ALIGN_FIT / ALIGN_GLOBAL, or None: the context's own) is set for the call in the same way;
    long_reads (True / False, or None: the context's own) likewise sets option "long_reads": reads longer than 1024 bases on the
    affine kernels; band (a half-width, 0: none, or None: the context's own) sets option "band"; extend (True / False, or None:
    the context's own) sets option "extend": seed extension, with align_mode ALIGN_GLOBAL only; xdrop (a threshold 0 .. 2^31 - 1, 0:
    off, or None: the context's own) sets option "xdrop": the drop-off rule of an extend run of a read longer than 1024 bases;
    band_adapt (True / False, or None: the context's own) sets option "band_adapt": the band of a banded extend run follows the
    alignment; end_bonus (a bonus 0 .. 2^30, 0: off, or None: the context's own) sets option "end_bonus": an extend run takes a pair to
    the read's end when that scores less than the bonus below its best; overlap (True / False, or None: the context's own) sets option
    "overlap": overlap (ends-free) alignment, with align_mode ALIGN_FIT only.  The options are put back afterwards."""
    sc = tuple(int(x) for x in align_scores)
    if len(sc) in (4, 6) and sc[3] > 0:
        raise ValueError("gapOpen (alignScores[3]) must be <= 0, got %d" % sc[3])
    if len(sc) == 6 and (sc[4] > 0 or sc[5] > 0):
        raise ValueError("gap2 and gapOpen2 (alignScores[4], [5]) must be <= 0, got %d, %d" % (sc[4], sc[5]))
    if align_mode is not None and align_mode not in (_capi.ALIGN_LOCAL, _capi.ALIGN_FIT, _capi.ALIGN_GLOBAL):
        raise ValueError("align_mode must be ALIGN_LOCAL, ALIGN_FIT or ALIGN_GLOBAL, got %r" % (align_mode,))
    if extend is not None and extend is not True and extend is not False:
        raise ValueError("extend must be None, True or False, got %r" % (extend,))
    if xdrop is not None and (isinstance(xdrop, bool) or not isinstance(xdrop, int) or not 0 <= xdrop <= _capi.XDROP_MAX):
        raise ValueError("xdrop must be None or an integer 0 .. 2^31 - 1, got %r" % (xdrop,))
    if band_adapt is not None and band_adapt is not True and band_adapt is not False:
        raise ValueError("band_adapt must be None, True or False, got %r" % (band_adapt,))
    if end_bonus is not None and (isinstance(end_bonus, bool) or not isinstance(end_bonus, int) or not 0 <= end_bonus <= _capi.END_BONUS_MAX):
        raise ValueError("end_bonus must be None or an integer 0 .. 2^30, got %r" % (end_bonus,))
    if overlap is not None and overlap is not True and overlap is not False:
        raise ValueError("overlap must be None, True or False, got %r" % (overlap,))
    restore = []
    try:
        if len(sc) in (4, 6):
            restore.append(("gap_open", ctx.options.get("gap_open", 0)))
            ctx.set_option("gap_open", sc[3])
        if len(sc) == 6:
            restore.append(("gap2", ctx.options.get("gap2", 0)))
            ctx.set_option("gap2", sc[4])
            restore.append(("gap_open2", ctx.options.get("gap_open2", 0)))
            ctx.set_option("gap_open2", sc[5])
        if align_mode is not None:
            restore.append(("align_mode", ctx.options.get("align_mode", _capi.ALIGN_LOCAL)))
            ctx.set_option("align_mode", int(align_mode))
        if long_reads is not None:
            restore.append(("long_reads", ctx.options.get("long_reads", 0)))
            ctx.set_option("long_reads", 1 if long_reads else 0)
        if band is not None:
            restore.append(("band", ctx.options.get("band", 0)))
            ctx.set_option("band", int(band))
        if extend is not None:
            restore.append(("extend", ctx.options.get("extend", 0)))
            ctx.set_option("extend", 1 if extend else 0)
        if xdrop is not None:
            restore.append(("xdrop", ctx.options.get("xdrop", 0)))
            ctx.set_option("xdrop", xdrop)
        if band_adapt is not None:
            restore.append(("band_adapt", ctx.options.get("band_adapt", 0)))
            ctx.set_option("band_adapt", 1 if band_adapt else 0)
        if end_bonus is not None:
            restore.append(("end_bonus", ctx.options.get("end_bonus", 0)))
            ctx.set_option("end_bonus", end_bonus)
        if overlap is not None:
            restore.append(("overlap", ctx.options.get("overlap", 0)))
            ctx.set_option("overlap", 1 if overlap else 0)
        yield sc[:3]
    finally:
        for name, prev in reversed(restore):
            ctx.set_option(name, prev)


class SmithWaterman:
    class OptAlignments:
        """Function3<String[], int[], char[], Tuple2<Integer, ArrayList<Tuple2<Integer,String[]>>>>."""
        tie_mode = _capi.TIE_SERIAL

        def __init__(self, context=None, align_mode=None, long_reads=None, band=None, extend=None, xdrop=None, band_adapt=None, end_bonus=None, overlap=None):
            self._ctx = context
            self._align_mode = align_mode       # ALIGN_FIT / ALIGN_GLOBAL: end-to-end alignment (option "align_mode")
            self._long_reads = long_reads       # True: reads longer than 1024 bases on the affine kernels (option "long_reads")
            self._band = band                   # a half-width: such reads inside the band |j - i| <= band only (option "band")
            self._extend = extend               # True: seed extension, with ALIGN_GLOBAL -- anchored at the start, ends at the best cell (option "extend")
            self._xdrop = xdrop                 # a threshold: an extend run of a long read stops at a strip seam that far below its best (option "xdrop")
            self._band_adapt = band_adapt       # True: the band of an extend run follows the alignment from strip to strip (option "band_adapt")
            self._end_bonus = end_bonus         # a bonus: an extend run takes a pair to the read's end when that scores less than this below its best (option "end_bonus")
            self._overlap = overlap             # True: overlap alignment, with ALIGN_FIT -- all four sequence ends are free (option "overlap")

        def call(self, seqs, alignScores=None, alignTypes=None):
            ctx = self._ctx or default_context()
            sc, ty = _algo(alignScores, alignTypes)
            with _scores(ctx, sc, self._align_mode, self._long_reads, self._band, self._extend, self._xdrop, self._band_adapt, self._end_bonus, self._overlap) as sc3:
                b = ctx.upload([seqs[0]], [seqs[1]])
                try:
                    b.run(make_params(sc3, ty, self.tie_mode))
                    return b.score(0), b.alignments(0)
                finally:
                    b.free()


class DistributedSW:
    class OptAlignments(SmithWaterman.OptAlignments):
        """Same recurrence with DistributedSW's strict '>' tie order and diagonal max-cell order."""
        tie_mode = _capi.TIE_STRICT


class Distribution:
    ALIGN_SCORES = DEFAULT_SCORES
    ALIGN_TYPES = DEFAULT_TYPES

    class CombineReadsToRef:
        def call(self, references, reads, algoArgs):
            return [(ref, reads, algoArgs) for ref in references]

    class MapPartition:
        """mapPartitions variant: every (ref, reads, algoArgs) tuple of a partition in ONE native call.

        Tuples that share the reads list and algoArgs (what CombineReadsToRef builds) are batched
        together; results come back in input order, each exactly what MapRef.call returns.
        """

        def __init__(self, context=None, tie_mode=_capi.TIE_SERIAL, align_mode=None, long_reads=None, band=None, extend=None, xdrop=None, band_adapt=None, end_bonus=None, overlap=None):
            self._ctx = context
            self._band = band
            self._extend = extend
            self._xdrop = xdrop
            self._band_adapt = band_adapt
            self._end_bonus = end_bonus
            self._overlap = overlap
            self._tie = tie_mode
            self._align_mode = align_mode
            self._long_reads = long_reads

        def call(self, tuples):
            tuples = list(tuples)
            out = [None] * len(tuples)
            groups = {}
            for idx, (ref, reads, algo) in enumerate(tuples):
                key = (id(reads), None if algo is None else (tuple(algo[0]), tuple(algo[1])))
                groups.setdefault(key, []).append(idx)
            ctx = self._ctx or default_context()
            for idxs in groups.values():
                _, reads, algo = tuples[idxs[0]]
                sc, ty = _algo(*(algo if algo is not None else (None, None)))
                with _scores(ctx, sc, self._align_mode, self._long_reads, self._band, self._extend, self._xdrop, self._band_adapt, self._end_bonus, self._overlap) as sc3:
                    b = ctx.upload([tuples[i][0][1] for i in idxs], list(reads))
                    try:
                        b.run(make_params(sc3, ty, self._tie))
                        for r, i in enumerate(idxs):
                            out[i] = (b.ref_total(r), (tuples[i][0], b.ref_match_sites(r)))
                    finally:
                        b.free()
            return out

    class MapRef:
        """PairFunction<Tuple3<String[], ArrayList<String>, Tuple2<int[],char[]>>, Integer, Tuple2<...>>."""

        def __init__(self, context=None, tie_mode=_capi.TIE_SERIAL, align_mode=None, long_reads=None, band=None, extend=None, xdrop=None, band_adapt=None, end_bonus=None, overlap=None):
            self._mp = Distribution.MapPartition(context, tie_mode, align_mode, long_reads, band, extend, xdrop, band_adapt, end_bonus, overlap)

        def call(self, tuple3):
            return self._mp.call([tuple3])[0]

    class ReduceMax:
        """Running maximum with ties over MapRef results, then OptSeqsComp order.

        Control-path semantics (NoDistribution, Distribution.java:600-613; sort :621, :647-666).
        DistributeReference's own reduce takes `first()` of an RDD whose sorted copy was discarded
        (Distribution.java:341-342) and so reports the first reference's total, not the maximum;
        the intended (control) behaviour is what is implemented here.
        """

        def __init__(self):
            self.max = 0
            self.opt = []

        def add(self, total, value):
            if total > self.max:
                self.max = total
                self.opt = [value]
            elif total == self.max:
                self.opt.append(value)

        def result(self):
            return self.max, sorted(self.opt, key=lambda v: v[0][0])


# ------------------------------------------------------------------------------------------------
# file-level drivers: same positional ioArgs / algoArgs as the reference
# ------------------------------------------------------------------------------------------------
import time as _time

from . import io as _io


class _FileDriver:
    """Shared body of the two drivers below.  ioArgs = [refDir, inDir, delimiter, outDir, outName, outExt]
    (nulls keep the defaults, Distribution.java:267-281); algoArgs = (alignScores, alignTypes) or None (:284-292)."""

    OUT_FILE, OUT_EXT = "result", ".txt"                              # Distribution.java:40-41
    REF_DIR, IN_DIR = "/home/ubuntu/project/reference", "/home/ubuntu/project/input"   # :43-44
    OUT_DIR = "/home/ubuntu/project/output/reference"                 # :50

    def __init__(self, context=None, tie_mode=_capi.TIE_SERIAL, align_mode=None, long_reads=None, band=None, extend=None, xdrop=None, band_adapt=None, end_bonus=None, overlap=None):
        self._ctx = context
        self._band = band
        self._extend = extend
        self._xdrop = xdrop
        self._band_adapt = band_adapt
        self._end_bonus = end_bonus
        self._overlap = overlap
        self._tie = tie_mode
        self._align_mode = align_mode
        self._long_reads = long_reads

    def call(self, ioArgs=None, algoArgs=None):
        ref_dir, in_dir, delim = self.REF_DIR, self.IN_DIR, _io.DELIMITER
        out_dir, out_name, out_ext = self.OUT_DIR, self.OUT_FILE, self.OUT_EXT
        if ioArgs is not None and len(ioArgs) == 6:
            ref_dir = ioArgs[0] if ioArgs[0] is not None else ref_dir
            in_dir = ioArgs[1] if ioArgs[1] is not None else in_dir
            delim = ioArgs[2] if ioArgs[2] is not None else delim
            out_dir = ioArgs[3] if ioArgs[3] is not None else out_dir
            out_name = ioArgs[4] if ioArgs[4] is not None else out_name
            out_ext = ioArgs[5] if ioArgs[5] is not None else out_ext
        sc, ty = _algo(*(algoArgs if algoArgs is not None else (None, None)))
        ctx = self._ctx or default_context()
        with _scores(ctx, sc, self._align_mode, self._long_reads, self._band, self._extend, self._xdrop, self._band_adapt, self._end_bonus, self._overlap) as sc3:
            return self._run(ctx, make_params(sc3, ty, self._tie), ref_dir, in_dir, delim, out_dir, out_name, out_ext)

    def _run(self, ctx, params, ref_dir, in_dir, delim, out_dir, out_name, out_ext):
        in_crawl = _io.DirectoryCrawler(in_dir)
        input_num = 0
        while in_crawl.hasNext():
            input_num += 1
            reads = _io.InOutOps.GetReads().call(in_crawl.next(), delim)
            num_refs = 0
            t0 = _time.time()
            red = Distribution.ReduceMax()                       # `int max = 0` + ties, Distribution.java:573,600-613
            ref_crawl = _io.DirectoryCrawler(ref_dir)
            while ref_crawl.hasNext():
                rs = _io.read_refs_packed(ref_crawl.next(), delim)
                num_refs += len(rs)
                seqs = rs.sequences()
                b = ctx.upload(seqs, reads).run(params)          # every reference of the file x every read: one batch
                try:
                    for r in range(len(rs)):
                        total = b.ref_total(r)
                        if total >= red.max:                     # match sites are only materialised for candidates
                            red.add(total, ([rs.metadata[r], seqs[r]], b.ref_match_sites(r)))
                finally:
                    b.free()
            exec_ms = int((_time.time() - t0) * 1000)
            mx, opt = red.result()                               # Collections.sort(opt, new OptSeqsComp())  :621
            text = _io.InOutOps.GetOutputStr().call(reads, ((num_refs, len(reads)), mx, exec_ms), opt)
            _io.InOutOps.PrintStrToFile().call("%s/%s%d%s" % (out_dir, out_name, input_num, out_ext), text)
        return None


class _NoDistribution(_FileDriver):
    """Distribution.NoDistribution.call (Distribution.java:482-634), alignments on the GPU."""
    OUT_DIR = "/home/ubuntu/project/output/control"               # :49


class _DistributeReference(_FileDriver):
    """Distribution.DistributeReference.call (Distribution.java:227-373) with the control path's reduce.

    The reference's own reduce (`sortByKey` result discarded, then `first()`, :341-342) reports the FIRST
    reference's total instead of the maximum; the intended semantics (running max with ties, :600-613) are used."""


Distribution.NoDistribution = _NoDistribution
Distribution.DistributeReference = _DistributeReference
