"""MI355X-native Smith-Waterman batch aligner: drop-in for the src/sw hot path of
elizabethfong/SparkSmithWaterman (matrix fill + tied-maximum search + traceback).

The compute path is libswmi.so (hand-written HIP for gfx950, C ABI in include/swmi.h).
Importing this package does not load the library; the first Context does, and fails loudly
if it has not been built.
"""
from ._capi import SwmiError, TIE_SERIAL, TIE_STRICT, ALIGN_LOCAL, ALIGN_FIT, ALIGN_GLOBAL, PAIR_DEGENERATE, PAIR_TO_END, LIB_PATH
from ._capi import CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X, SUBOPT_AUTO, HITS_MAX
from .aligner import Context, Batch, PairBatch, Stream, make_params, normalise_pairs, cigar_string, DEFAULT_SCORES, DEFAULT_TYPES
from .aligner import COMPLEMENT, revcomp, both_strands
from .sw import SmithWaterman, DistributedSW, Distribution, default_context

__all__ = ["SwmiError", "TIE_SERIAL", "TIE_STRICT", "ALIGN_LOCAL", "ALIGN_FIT", "ALIGN_GLOBAL", "PAIR_DEGENERATE", "PAIR_TO_END", "LIB_PATH", "Context", "Batch", "PairBatch", "normalise_pairs", "Stream",
           "make_params", "DEFAULT_SCORES", "DEFAULT_TYPES", "SmithWaterman", "DistributedSW",
           "Distribution", "default_context", "cigar_string", "CIGAR_M", "CIGAR_I", "CIGAR_D", "CIGAR_EQ", "CIGAR_X", "SUBOPT_AUTO", "HITS_MAX",
           "COMPLEMENT", "revcomp", "both_strands"]
