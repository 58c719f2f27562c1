"""ctypes binding of libswmi.so (include/swmi.h).  No torch types cross this boundary.

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C sparksmithwaterman_amd/csrc``.
Loading fails loudly when it is missing: there is no Python or CPU implementation behind it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SWMI_LIB: another build of the same sources, e.g. the -DSWMI_CK_BLOCKS=4u variant of tools/build_variants.sh)
LIB_PATH = os.environ.get("SWMI_LIB") or os.path.join(_HERE, "lib", "libswmi.so")

TIE_SERIAL = 0
TIE_STRICT = 1
ALIGN_LOCAL = 0      # option "align_mode": Smith-Waterman (the default)
ALIGN_FIT = 1        # the whole read against any stretch of the reference
ALIGN_GLOBAL = 2     # the whole read against the whole reference
BAND_MAX = 1 << 20   # option "band": the largest half-width (0: no band)
XDROP_MAX = (1 << 31) - 1   # option "xdrop": the largest threshold (0: off)
CIGAR_M, CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 0, 1, 2, 7, 8     # option "cigar": the op of an entry  len << 4 | op  (BAM's)
CIGAR_CHARS = {CIGAR_M: "M", CIGAR_I: "I", CIGAR_D: "D", CIGAR_EQ: "=", CIGAR_X: "X"}
SUBOPT_AUTO = -1     # option "subopt": the mask half-width per pair, max(m // 2, 15) (0: off; 1 .. 2^30: the half-width)
END_BONUS_MAX = 1 << 30     # option "end_bonus": the largest bonus (0: off)
HITS_MAX = 16        # option "hits": the most entries per pair (0: off; needs option "subopt")
PAIR_DEGENERATE = 0x1
PAIR_TO_END = 0x2           # option "end_bonus": the pair was taken to the read's end (flags of swmi_pair_n_alignments)
SPEC_REVERSE = 0x1          # swmi_pair_spec.flags: both segments in reverse byte order (left extension)
SPEC_READ_REVCOMP = 0x4     # ... the pair is on the minus strand: the read segment reverse-complemented, the reference untouched
SPEC_WHOLE = 0xFFFFFFFF     # as ref_len / read_len: from the start given to the end of the source
ERR_INVALID = -1
ERR_UNSUPPORTED = -5


class SwmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("swmi error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32),
                ("tie_mode", C.c_int32), ("types", C.c_char * 4)]


class Timing(C.Structure):
    _fields_ = [("fill_ms", C.c_float), ("traceback_ms", C.c_float), ("d2h_ms", C.c_float),
                ("total_ms", C.c_float), ("fill_launches", C.c_uint32), ("rerun_pairs", C.c_uint32),
                ("cells", C.c_uint64), ("dir_bytes", C.c_uint64),
                ("strip_fallbacks", C.c_uint32), ("col_chunks", C.c_uint32),
                ("resident_pairs", C.c_uint32), ("tfused_pairs", C.c_uint32)]


class Hit(C.Structure):
    """swmi_hit: one entry of option "hits" -- a local score and the 1-based cell it ends in, 16 bytes"""
    _fields_ = [("score", C.c_int32), ("end_i", C.c_uint32), ("end_j", C.c_uint32), ("reserved", C.c_uint32)]


class PairSpec(C.Structure):
    """swmi_pair_spec: one pair of a pair list (swmi_batch_upload_pairs), 32 bytes"""
    _fields_ = [("ref", C.c_uint32), ("read", C.c_uint32), ("ref_start", C.c_uint32), ("ref_len", C.c_uint32),
                ("read_start", C.c_uint32), ("read_len", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class StreamStats(C.Structure):
    _fields_ = [("push_ms", C.c_double), ("parse_ms", C.c_double), ("upload_ms", C.c_double), ("run_ms", C.c_double),
                ("gpu_sweep_ms", C.c_double), ("gpu_traceback_ms", C.c_double), ("bytes", C.c_uint64), ("cells", C.c_uint64),
                ("chunks", C.c_uint32), ("pad", C.c_uint32)]


# every symbol include/swmi.h declares: (name, restype, argtypes)
_P = C.c_void_p
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
SYMBOLS = [
    ("swmi_abi_version", C.c_int, []),
    ("swmi_last_error", C.c_char_p, []),
    ("swmi_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("swmi_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("swmi_destroy", None, [_P]),
    ("swmi_default_params", None, [C.POINTER(Params)]),
    ("swmi_set_option", C.c_int, [_P, C.c_char_p, C.c_int64]),
    ("swmi_set_score_matrix", C.c_int, [_P, C.c_char_p, C.c_uint32, C.POINTER(C.c_int32)]),
    ("swmi_batch_upload", C.c_int, [_P, C.c_char_p, _u64p, C.c_uint32, C.c_char_p, _u64p, C.c_uint32, C.POINTER(_P)]),
    ("swmi_batch_upload_pairs", C.c_int, [_P, C.c_char_p, _u64p, C.c_uint32, C.c_char_p, _u64p, C.c_uint32, C.POINTER(PairSpec),
                                          C.c_uint64, C.POINTER(_P)]),
    ("swmi_batch_set_pairs", C.c_int, [_P, _P, C.POINTER(PairSpec), C.c_uint64]),
    ("swmi_batch_pair_spec", C.c_int, [_P, C.c_uint64, C.POINTER(PairSpec)]),
    ("swmi_batch_set_read_profiles", C.c_int, [_P, _P, C.c_char_p, C.c_uint32, C.POINTER(C.c_int32)]),
    ("swmi_batch_run", C.c_int, [_P, _P, C.POINTER(Params)]),
    ("swmi_batch_run_async", C.c_int, [_P, _P, C.POINTER(Params)]),
    ("swmi_batch_wait", C.c_int, [_P]),
    ("swmi_batch_free", None, [_P, _P]),
    ("swmi_batch_timing", C.c_int, [_P, C.POINTER(Timing)]),
    ("swmi_batch_mode", C.c_int, [_P, C.POINTER(C.c_int)]),
    ("swmi_batch_n_pairs", C.c_uint64, [_P]),
    ("swmi_pair_score", C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int32)]),
    ("swmi_pair_n_alignments", C.c_int, [_P, C.c_uint64, _u64p, C.POINTER(C.c_uint32)]),
    ("swmi_pair_alignment", C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_uint32)]),
    ("swmi_pair_cigar", C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("swmi_pair_rows_swept", C.c_int, [_P, C.c_uint64, C.POINTER(C.c_uint32)]),
    ("swmi_pair_band_window", C.c_int, [_P, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("swmi_batch_pair_results", C.c_int, [_P, C.POINTER(C.c_int32), _u64p, C.c_uint64]),
    ("swmi_pair_subopt", C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    ("swmi_batch_pair_subopt", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint64]),
    ("swmi_pair_hits", C.c_int, [_P, C.c_uint64, C.POINTER(Hit), C.c_uint32, C.POINTER(C.c_uint32)]),
    ("swmi_batch_pair_hits", C.c_int, [_P, C.POINTER(Hit), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint64]),
    ("swmi_pair_end_score", C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    ("swmi_batch_pair_end_scores", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint64]),
    ("swmi_batch_materialise_all", C.c_int, [_P, _u64p, _u64p]),
    ("swmi_ref_total", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_int32)]),
    ("swmi_ref_totals", C.c_int, [_P, C.POINTER(C.c_int32), C.c_uint32]),
    ("swmi_ref_n_match_sites", C.c_int, [_P, C.c_uint32, _u64p]),
    ("swmi_ref_match_site", C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_char_p), C.POINTER(C.c_uint32)]),
    ("swmi_ref_sites_packed", C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), _u64p, _u64p, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_uint32), _u64p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    ("swmi_stream_open", C.c_int, [_P, C.POINTER(Params), C.c_char_p, _u64p, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(_P)]),
    ("swmi_stream_push", C.c_int, [_P, C.c_char_p, _u64p, C.c_uint32]),
    ("swmi_stream_push_file", C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_uint32]),
    ("swmi_stream_push_file_shard", C.c_int, [_P, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("swmi_stream_finish", C.c_int, [_P]),
    ("swmi_stream_n_refs", C.c_uint64, [_P]),
    ("swmi_stream_n_chunks", C.c_uint32, [_P]),
    ("swmi_stream_chunk", C.c_int, [_P, C.c_uint32, C.POINTER(_P), _u64p]),
    ("swmi_stream_totals", C.c_int, [_P, C.POINTER(C.c_int32), C.c_uint64]),
    ("swmi_stream_metadata", C.c_int, [_P, C.c_uint64, C.c_char_p, C.c_size_t]),
    ("swmi_stream_ref_pos", C.c_int, [_P, C.c_uint64, _u64p]),
    ("swmi_stream_ref_sequence", C.c_int, [_P, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
    ("swmi_stream_get_stats", C.c_int, [_P, C.POINTER(StreamStats)]),
    ("swmi_stream_close", None, [_P]),
    ("swmi_align_batch", C.c_int, [_P, C.POINTER(Params), C.c_char_p, _u64p, C.c_uint32, C.c_char_p, _u64p,
                                   C.c_uint32, C.POINTER(_P)]),
]
# entry points of csrc/swmi_launch.h that answer for a launcher without a launch (no HIP call); include/swmi.h does not declare them.
# Bound where the library has them: a tool that loads an earlier build (SWMI_LIB) goes without.
LAUNCH_SYMBOLS = [
    ("swmi_affine_profile_waves", C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
]

_lib = None


def load():
    """Load libswmi.so and bind every declared symbol.  Raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(lib, name)      # AttributeError if a declared symbol is not exported
            f.restype = res
            f.argtypes = args
        for name, res, args in LAUNCH_SYMBOLS:
            if hasattr(lib, name):
                getattr(lib, name).restype = res
                getattr(lib, name).argtypes = args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise SwmiError(rc, load().swmi_last_error().decode("utf-8", "replace"))


def as_bytes(s):
    return bytes(s) if isinstance(s, (bytes, bytearray, memoryview)) else s.encode("latin-1")


def pack(seqs):
    """list of str/bytes -> (blob, uint64 offsets[len+1])."""
    bs = [as_bytes(s) for s in seqs]
    off = (C.c_uint64 * (len(bs) + 1))()
    t = 0
    for k, b in enumerate(bs):
        off[k] = t
        t += len(b)
    off[len(bs)] = t
    return b"".join(bs), off
