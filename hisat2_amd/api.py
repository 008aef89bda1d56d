"""ctypes mirror of include/h2g.h (libh2g.so) — the host-side view used by tests and bench.py.

There is no fallback: if the HIP library is missing or no GPU is usable, loading / the first call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_TAIL, DEFAULT_ALIGN_MATE = 16, 0     # H2G_DEFAULT_TAIL / H2G_DEFAULT_ALIGN_MATE of csrc/h2g_kernels.hip (what a stream does without H2G_FAST_TAIL / H2G_FAST_AM)
LIB_PATH = os.environ.get("H2G_LIBPATH") or os.path.join(_HERE, "libh2g.so")   # H2G_LIBPATH: development builds (tools/)
MAX = 0xFFFFFFFF
MAX_EDITS = 32
SEED_CAP = 5

u32, u8, i32, u64, i64 = C.c_uint32, C.c_uint8, C.c_int32, C.c_uint64, C.c_int64


class LoadOpts(C.Structure):
    _fields_ = [("device", i32), ("load_local", i32)]


class IndexInfo(C.Structure):
    _fields_ = [("len", u32), ("gbwtLen", u32), ("numNodes", u32), ("lineRate", i32), ("offRate", i32),
                ("ftabChars", i32), ("eftabLen", u32), ("linear", u32), ("sideSz", u32), ("sideGbwtSz", u32),
                ("sideGbwtLen", u32), ("numSides", u32), ("offsLen", u32), ("ftabLen", u32), ("nPat", u32),
                ("nFrag", u32), ("nZ", u32), ("minK", u32), ("nLocal", u32), ("nRefRecs", u32), ("device_bytes", u64)]


class FmQuery(C.Structure):
    _fields_ = [("read", u32), ("offset", u32), ("fw", u8), ("mode", u8), ("pseudogeneStop", u8), ("anchorStop", u8)]


FM_HIT_FIELDS = ("top", "bot", "node_top", "node_bot", "bwoff", "len", "hit_type", "cur", "done", "numPartialSearch",
                 "numUniqueSearch", "pseudogeneStop", "anchorStop", "nrank", "nside")


class FmHit(C.Structure):
    _fields_ = [(n, u32) for n in FM_HIT_FIELDS]


H2G_IEDGE_CAP = 24
H2G_ERR_ARG = -4          # include/h2g.h: bad argument / capacity exceeded


class IEdges(C.Structure):           # h2g_iedges
    _fields_ = [("n", u32), ("e", (u32 * 2) * H2G_IEDGE_CAP)]

    def pairs(self):
        return [(self.e[i][0], self.e[i][1]) for i in range(min(self.n, H2G_IEDGE_CAP))]


class GlfQuery(C.Structure):         # h2g_glf_query
    _fields_ = [("top", u32), ("bot", u32), ("c", C.c_uint8), ("single", C.c_uint8), ("pad", C.c_uint8 * 2)]


class GlfResult(C.Structure):        # h2g_glf_result
    _fields_ = [("ok", u32), ("top", u32), ("bot", u32), ("node_top", u32), ("node_bot", u32)]


class AdjustQuery(C.Structure):      # h2g_adjust_query
    _fields_ = [(n, u32) for n in ("read", "fw", "rdoff", "len", "tidx", "toff", "joinedOff")]


class GsaQuery(C.Structure):         # h2g_gsa_query
    _fields_ = [(n, u32) for n in ("top", "bot", "node_top", "node_bot", "maxelt", "len", "rejectStraddle")]


class SaQuery(C.Structure):
    _fields_ = [("top", u32), ("bot", u32), ("maxelt", u32), ("len", u32), ("rejectStraddle", u32)]


class Coord(C.Structure):
    _fields_ = [("tidx", u32), ("toff", u32), ("joinedOff", u32)]


class SaResult(C.Structure):
    _fields_ = [("ok", u32), ("ncoords", u32), ("straddled", u32), ("nsteps", u32)]


class Edit(C.Structure):
    _fields_ = [("pos", u32), ("chr", u8), ("qchr", u8), ("type", u8), ("pad", u8), ("snp", u32)]


class GHit(C.Structure):
    _fields_ = [("read", u32), ("fw", u32), ("rdoff", u32), ("len", u32), ("trim5", u32), ("trim3", u32),
                ("tidx", u32), ("toff", u32), ("joinedOff", u32), ("score", i64), ("nedits", u32), ("overflow", u32),
                ("edits", Edit * MAX_EDITS)]


class ExtSearchQuery(C.Structure):   # h2g_ext_search_query
    _fields_ = [("read", u32), ("rdoff", u32), ("lidx", u32), ("maxHitLen", u32), ("fw", u8), ("uniqueStop", u8), ("pad", u8 * 2)]


class ExtSearchHit(C.Structure):     # h2g_ext_search_hit
    _fields_ = [("nelt", u32), ("hitlen", u32), ("top", u32), ("bot", u32), ("uniqueStop", u32), ("nrank", u32), ("nside", u32), ("staged", u32)]


class ExtSearchStats(C.Structure):   # h2g_ext_search_stats
    _fields_ = [("n_local", u64), ("n_staged", u64), ("n_buckets", u64), ("n_buckets_staged", u64), ("lds_bytes_staged", u64),
                ("ms_staged", C.c_float), ("ms_hbm", C.c_float)]


class SwQuery(C.Structure):          # h2g_sw_query
    _fields_ = [("read", u32), ("fw", u32), ("tidx", u32), ("refoff", u32), ("minsc", C.c_int32), ("rnd", u32)]


class SwResult(C.Structure):         # h2g_sw_result
    _fields_ = [("found_align", C.c_int32), ("found", C.c_int32), ("best", C.c_int32), ("score", C.c_int32),
                ("off", C.c_int64), ("nedits", u32), ("gaps", u32), ("overflow", u32), ("rnd", u32),
                ("refl", C.c_int64), ("refr", C.c_int64), ("edits", Edit * MAX_EDITS)]


class ExtArgs(C.Structure):
    _fields_ = [("mm", u32), ("max_leftext", u32), ("max_rightext", u32)]


class ExtResult(C.Structure):
    _fields_ = [("extended", u32), ("leftext", u32), ("rightext", u32)]


class SeedExt(C.Structure):
    _fields_ = [("tidx", u32), ("toff", u32), ("joinedOff", u32), ("rdoff", u32), ("len", u32), ("score", i32)]


class SeedResult(C.Structure):
    _fields_ = [("hit", FmHit), ("ncoords", u32), ("straddled", u32), ("nsteps", u32), ("pad", u32),
                ("ext", SeedExt * SEED_CAP)]


class SeedParams(C.Structure):
    _fields_ = [("pseudogeneStop", u32), ("anchorStop", u32), ("khits", u32), ("search_variant", u32)]


class Counters(C.Structure):
    _fields_ = [("n_rank", u64), ("n_side", u64), ("n_sa_steps", u64), ("n_ext", u64), ("n_ref_bytes", u64),
                ("n_queries", u64), ("n_aligned", u64), ("n_overflow", u64), ("ms_search", C.c_float),
                ("ms_resolve_extend", C.c_float), ("ms_rank", C.c_float), ("ms_align", C.c_float), ("ms_align_kernel", C.c_float),
                ("n_second_pass", u64), ("n_fast", u64), ("n_fast_bail", u64), ("ms_fast_kernel", C.c_float), ("pad_", C.c_float), ("n_fast_side", u64), ("n_fast_sa_steps", u64),
                ("ms_drain_kernel", C.c_float), ("pad2_", C.c_float), ("n_drain_side", u64), ("n_drain_sa_steps", u64), ("n_adopted", u64)]


ALN_CAP = 10


class AlnRes(C.Structure):
    _fields_ = [("fw", u32), ("tidx", u32), ("toff", u32), ("len", u32), ("trim5", u32), ("trim3", u32), ("nedits", u32),
                ("pad", u32), ("score", i64), ("edits", Edit * MAX_EDITS)]


class SpliceSite(C.Structure):
    _fields_ = [("tidx", u32), ("left", u32), ("right", u32), ("readid", u32), ("dir", u8), ("fromfile", u8), ("known", u8), ("editdist", u8)]


def splice_site_array(sites, known=True):
    """[(tidx, left, right, '+'|'-'), ...] -> (SpliceSite * n) as --known-splicesite-infile / --novel-splicesite-infile load them"""
    a = (SpliceSite * max(1, len(sites)))()
    for i, (t, l, r, d) in enumerate(sites):
        a[i].tidx, a[i].left, a[i].right, a[i].readid = t, l, r, 0
        a[i].dir, a[i].fromfile, a[i].known = (2 if d == "+" else 3), 1, (1 if known else 0)
    return a


def read_splice_site_file(path, refnames):
    """the reference's splice-site file (SpliceSiteDB::read splice_site.cpp:727): name, left, right, strand per line"""
    idx = {n: i for i, n in reversed(list(enumerate(refnames)))}
    out = []
    toks = open(path).read().split()
    for k in range(0, len(toks) - 3, 4):
        if toks[k] in idx:
            out.append((idx[toks[k]], int(toks[k + 1]), int(toks[k + 2]), toks[k + 3][0]))
    return out


class ReadResult(C.Structure):
    _fields_ = [("nres", u32), ("nselect", u32), ("overflow", u32), ("nrank", u32), ("nsteps", u32), ("depth", u32),
                ("best", C.c_int32), ("secbest", C.c_int32), ("best_h2", u32), ("secbest_h2", u32)]


class AlignParams(C.Structure):
    _fields_ = [("khits", u32), ("kseeds", u32), ("no_spliced_alignment", u32), ("secondary", u32), ("bowtie2_dp", u32),
                ("mm_max", C.c_int32), ("mm_min", C.c_int32), ("n_pen", C.c_int32), ("rdg_const", C.c_int32), ("rdg_linear", C.c_int32),
                ("rfg_const", C.c_int32), ("rfg_linear", C.c_int32), ("sc_max", C.c_int32), ("sc_min", C.c_int32), ("score_min_type", u32),
                ("score_min_const", C.c_double), ("score_min_coeff", C.c_double), ("no_temp_splicesite", u32),
                ("min_intronlen", u32), ("max_intronlen", u32), ("pen_cansplice", C.c_int32), ("pen_noncansplice", C.c_int32),
                ("pen_canintronlen_type", u32), ("pen_noncanintronlen_type", u32), ("first_read_id", u32),
                ("pen_canintronlen_const", C.c_double), ("pen_canintronlen_coeff", C.c_double),
                ("pen_noncanintronlen_const", C.c_double), ("pen_noncanintronlen_coeff", C.c_double),
                ("min_anchor_len", u32), ("min_anchor_len_noncan", u32), ("xs_only", u32), ("use_haplotype", u32), ("max_alts_tried", u32), ("max_frag_len", u32), ("min_frag_len", u32), ("pe_orientation", u32), ("nofw", u32), ("norc", u32),
                ("avoid_pseudogene", u32), ("transcriptome_mapping_only", u32), ("no_anchorstop", u32), ("pen_conflictsplice", C.c_int32),
                ("seed", u32), ("n_ceil_type", u32), ("n_ceil_const", C.c_double), ("n_ceil_coeff", C.c_double)]

    def apply_options(self, opts, linear=None):
        """apply a list of reference command-line options (['-k', '3', '--mp', '4,2', ...]) to this block; returns leftovers.
        Every rule is the library's (h2g_align_params_apply_options, then h2g_align_params_presets: the command line's parser);
        a faulty option raises ValueError with the library's message.  `linear` defaults to what the block's default -k says about
        the index (5 = linear, 10 = graph)."""
        if linear is None:
            linear = self.khits == 5
        L = lib()
        rest, mine, i = [], [], 0
        while i < len(opts):
            o = opts[i]
            arity = L.h2g_align_option_arity(o.encode())
            if arity >= 0:
                mine += opts[i:i + 1 + arity]
            elif o == "--spliced":          # test shorthand: the reference's default mode
                self.no_spliced_alignment = 0
            elif o not in OUTPUT_OPTIONS:
                rest.append(o)
            i += 1 + max(arity, OUTPUT_OPTIONS.get(o, 0))
        pre, err = AlignPresets(), C.create_string_buffer(512)
        argv = (C.c_char_p * max(1, len(mine)))(*[m.encode() for m in mine])
        if L.h2g_align_params_apply_options(C.byref(self), C.byref(pre), argv, len(mine), err, len(err)) != 0:
            raise ValueError(err.value.decode())
        L.h2g_align_params_presets(C.byref(self), int(bool(linear)), C.byref(pre))
        return rest


class AlignPresets(C.Structure):     # h2g_align_presets
    _fields_ = [(n, u32) for n in ("saw_k", "k_arg", "max_seeds_arg", "sensitive", "very_sensitive")]


# options of the command line that change the SAM text only (include/h2g_sam.h), never h2g_align_params: name -> arity
OUTPUT_OPTIONS = {"--rg-id": 1, "--rg": 1, "--rna-strandness": 1, "--novel-splicesite-outfile": 1, "--summary-file": 1, "--no-sq": 0, "--omit-sec-seq": 0,
                  "--new-summary": 0, "--add-chrname": 0, "--remove-chrname": 0, "--no-mixed": 0, "--no-discordant": 0, "--no-templatelen-adjustment": 0}


def parse_n_ceil(arg, cur=(2, 0.0, float(np.float32(0.15)))):
    """--n-ceil <arg> applied to the ceiling `cur` = (type, constant, coefficient) by the library's parser (fields not given keep
    their value).  ValueError carries the reference's message."""
    p = AlignParams()
    p.n_ceil_type, p.n_ceil_const, p.n_ceil_coeff = cur
    p.apply_options(["--n-ceil", arg], linear=True)
    return p.n_ceil_type, p.n_ceil_const, p.n_ceil_coeff


PAIR_RES_CAP = 16
PAIR_CAP = 32
KHITS_MAX = 128              # h2g_align_*run's range: 1 <= khits <= KHITS_MAX, khits <= kseeds <= KSEEDS_MAX (include/h2g.h)
KSEEDS_MAX = 256
PAIR_TRAILER_TAG = 0x52494150   # nedits of the concordant-list trailer behind mate 1's compact records (XL runs)
OVF_PAIR_LIST = 4096         # overflow bit of the slot / dense paired fetches: the pair's list only travels compact


class PairResult(C.Structure):
    _fields_ = [("nres", u32 * 2), ("npairs", u32), ("overflow", u32), ("nrank", u32), ("nsteps", u32), ("depth", u32),
                ("nside", u32), ("rnd_state", u32), ("pad", u32), ("pair_i", u8 * PAIR_CAP), ("pair_j", u8 * PAIR_CAP)]


READ_RESULT_DTYPE = np.dtype([(n, np.uint32) for n in ("nres", "nselect", "overflow", "nrank", "nsteps", "depth")] +
                             [("best", np.int32), ("secbest", np.int32), ("best_h2", np.uint32), ("secbest_h2", np.uint32)])


# numpy views of the result structs (same memory layout)
FM_HIT_DTYPE = np.dtype([(n, np.uint32) for n in FM_HIT_FIELDS])
SEED_EXT_DTYPE = np.dtype([("tidx", np.uint32), ("toff", np.uint32), ("joinedOff", np.uint32), ("rdoff", np.uint32),
                           ("len", np.uint32), ("score", np.int32)])
SEED_RESULT_DTYPE = np.dtype([("hit", FM_HIT_DTYPE), ("ncoords", np.uint32), ("straddled", np.uint32),
                              ("nsteps", np.uint32), ("pad", np.uint32), ("ext", SEED_EXT_DTYPE, (SEED_CAP,))])
assert SEED_RESULT_DTYPE.itemsize == C.sizeof(SeedResult)

class WindowSeg(C.Structure):        # h2g_window_seg
    _fields_ = [("text_start", C.c_uint64), ("name_off0", C.c_uint64), ("rdid0", C.c_uint64), ("n_windows", C.c_uint32), ("prefix_start", C.c_uint32),
                ("prefix_len", C.c_uint32), ("pad", C.c_uint32)]


class WindowPlanInfo(C.Structure):   # h2g_window_plan_info
    _fields_ = [("n_reads", C.c_uint64), ("n_text", C.c_uint64), ("n_segs", C.c_uint64), ("n_prefix_bytes", C.c_uint64), ("next_rdid", C.c_uint64),
                ("len", C.c_uint32), ("step", C.c_uint32)]


class WindowsStats(C.Structure):     # h2g_windows_stats
    _fields_ = [("bytes_uploaded", C.c_uint64), ("bytes_written", C.c_uint64), ("kernel_ms", C.c_float), ("pad", C.c_float)]


class FastqOpts(C.Structure):        # h2g_fastq_opts
    _fields_ = [("trim5", C.c_uint32), ("trim3", C.c_uint32), ("phred64", C.c_uint8), ("final1", C.c_uint8), ("final2", C.c_uint8), ("pad", C.c_uint8), ("max_records", C.c_uint64)]


class FastqResult(C.Structure):      # h2g_fastq_result
    _fields_ = [("n_records", C.c_uint64), ("consumed1", C.c_uint64), ("consumed2", C.c_uint64), ("n_bases1", C.c_uint64), ("n_bases2", C.c_uint64),
                ("n_name_bytes1", C.c_uint64), ("n_name_bytes2", C.c_uint64), ("n_not_plain", C.c_uint64), ("first_not_plain", C.c_uint64),
                ("max_read_len", C.c_uint32), ("pad", C.c_uint32)]


class FastqStats(C.Structure):       # h2g_fastq_stats
    _fields_ = [("bytes_uploaded", C.c_uint64), ("bytes_written", C.c_uint64), ("kernel_ms", C.c_float), ("pad", C.c_float)]


WINDOW_SEG_DTYPE = np.dtype([("text_start", np.uint64), ("name_off0", np.uint64), ("rdid0", np.uint64), ("n_windows", np.uint32), ("prefix_start", np.uint32),
                             ("prefix_len", np.uint32), ("pad", np.uint32)])
assert WINDOW_SEG_DTYPE.itemsize == C.sizeof(WindowSeg)


class SamLine(C.Structure):
    """h2g_sam_line (include/h2g.h): one SAM line as the planner decides it, 64 bytes"""
    _fields_ = [("read", C.c_uint32), ("nh", C.c_uint32), ("rec_off", C.c_uint64), ("orec_off", C.c_uint64), ("tlen", C.c_int64), ("zs", C.c_int32), ("oref_tidx", C.c_int32),
                ("oref_toff", C.c_uint32), ("aux_off", C.c_uint32), ("aux_len", C.c_uint32), ("flag", C.c_uint16), ("cigar_len", C.c_uint16), ("mdz_len", C.c_uint16),
                ("mapq", C.c_uint8), ("mate", C.c_uint8), ("yt", C.c_uint8), ("yf", C.c_uint8), ("bits", C.c_uint16)]


SAM_LINE_DTYPE = np.dtype([("read", np.uint32), ("nh", np.uint32), ("rec_off", np.uint64), ("orec_off", np.uint64), ("tlen", np.int64), ("zs", np.int32), ("oref_tidx", np.int32),
                           ("oref_toff", np.uint32), ("aux_off", np.uint32), ("aux_len", np.uint32), ("flag", np.uint16), ("cigar_len", np.uint16), ("mdz_len", np.uint16),
                           ("mapq", np.uint8), ("mate", np.uint8), ("yt", np.uint8), ("yf", np.uint8), ("bits", np.uint16)])
assert SAM_LINE_DTYPE.itemsize == C.sizeof(SamLine) == 64
SAM_LINE_HAS_ZS, SAM_LINE_HAS_YS, SAM_LINE_HAS_TLEN, SAM_LINE_STAR_SEQ, SAM_LINE_STRIP_MATE_SUFFIX, SAM_LINE_AUX_CIGAR_MDZ, SAM_LINE_WHOLE_LINE, SAM_LINE_SENSE_MATE1 = 1, 2, 4, 8, 16, 32, 64, 128
SAM_NONE = (1 << 64) - 1     # rec_off / orec_off of a line without that record


class SamTextStats(C.Structure):
    _fields_ = [("bytes_uploaded", C.c_uint64), ("bytes_written", C.c_uint64), ("kernel_ms", C.c_float), ("write_kernel_ms", C.c_float)]


class SamPlanStats(C.Structure):
    """h2g_sam_plan_stats: of a stream's last h2g_sam_text_*_planned call"""
    _fields_ = [("device_planned", C.c_uint64), ("host_planned", C.c_uint64), ("n_lines", C.c_uint64), ("bytes_uploaded", C.c_uint64), ("whole_lines", C.c_uint64), ("plan_kernel_ms", C.c_float), ("host_plan_ms", C.c_float)]


# class bytes of the split planner (csrc/h2g_sam_plan.h): 0 = handed on to the host planner
(SAM_CLS_HOST, SAM_CLS_U_UNAL, SAM_CLS_U_UNIQ, SAM_CLS_P_CONC, SAM_CLS_P_DISC, SAM_CLS_P_NONE, SAM_CLS_P_MATE1, SAM_CLS_P_MATE2, SAM_CLS_P_BOTH) = range(9)

EXPORTS = [
    "h2g_load_opts_init", "h2g_index_load", "h2g_index_get_info", "h2g_index_synth_sides", "h2g_index_free", "h2g_index_set_splice_sites", "h2g_index_add_splice_sites",
    "h2g_last_error", "h2g_stream_create", "h2g_stream_free", "h2g_stream_hip", "h2g_stream_sync", "h2g_stream_select_batch", "h2g_set_reads",
    "h2g_rank_bench", "h2g_rank_bench_synth", "h2g_rank_bench_synth_sample", "h2g_fm_search", "h2g_sa_resolve", "h2g_extend",
    "h2g_seed_params_init", "h2g_seed_extend_run", "h2g_seed_extend_fetch", "h2g_get_counters",
    "h2g_device_count", "h2g_ext_search", "h2g_local_index_of", "h2g_align_params_init", "h2g_align_option_arity", "h2g_align_params_apply_options", "h2g_align_params_presets", "h2g_set_read_names", "h2g_align_run", "h2g_align_fetch",
    "h2g_set_mates", "h2g_set_read_seeds", "h2g_set_read_filter", "h2g_set_read_ids", "h2g_sam_set_read_ids", "h2g_sam_set_read_filter", "h2g_sam_set_record_ends", "h2g_sam_set_n_ceil", "h2g_combine_with", "h2g_align_pairs_run", "h2g_align_pairs_fetch", "h2g_align_fetch_dense", "h2g_align_pairs_fetch_dense", "h2g_align_fetch_long_edits",
    "h2g_align_fetch_compact", "h2g_align_pairs_fetch_compact", "h2g_host_alloc", "h2g_host_free",
    "h2g_graph_lf", "h2g_fm_search_graph", "h2g_index_synth_graph_sides", "h2g_sw_align", "h2g_sa_resolve_graph", "h2g_adjust_with_alt",
    "h2g_index_dense_sa_check",
    "h2g_index_dense_lsa_check",
    "h2g_window_plan_create", "h2g_window_plan_add_file", "h2g_window_plan_get_info", "h2g_window_plan_text", "h2g_window_plan_prefixes", "h2g_window_plan_segments",
    "h2g_window_plan_select", "h2g_window_plan_free", "h2g_set_reads_windows", "h2g_get_windows_stats", "h2g_fetch_reads",
    "h2g_set_reads_fastq", "h2g_fetch_read_set", "h2g_get_fastq_stats",
    "h2g_sam_plan_unpaired_compact", "h2g_sam_plan_paired_compact", "h2g_sam_text_unpaired", "h2g_sam_text_paired", "h2g_sam_text_from_plan_host", "h2g_get_sam_text_stats",
    "h2g_sam_text_unpaired_planned", "h2g_sam_text_paired_planned", "h2g_get_sam_plan_stats", "h2g_sam_plan_split_host",
]


class H2GError(RuntimeError):
    pass


_EMPTY = np.zeros(16, np.uint8)      # the address an empty text is handed by


def _ptr(x):
    """address of a numpy array / bytes / ctypes object, None for None"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, bytes):                      # (the caller keeps the object alive through the call)
        return C.cast(C.c_char_p(x), C.c_void_p).value
    if isinstance(x, int):
        return x
    return C.addressof(x)


def _sam_plan(call, n, head, tail):
    """runs a planning call, growing the descriptor array and the pool once when the first sizes were too small (H2G_ERR_ARG with the needed counts)"""
    line_cap, aux_cap = 2 * n + 16, 64 * n + 256
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    for attempt in range(2):
        lines = np.zeros(line_cap, dtype=SAM_LINE_DTYPE)
        aux = np.zeros(max(aux_cap, 1), dtype=np.uint8)
        nl, na = C.c_size_t(0), C.c_size_t(0)
        rc = call(*head, n, *tail, lines.ctypes.data, line_cap, C.byref(nl), aux.ctypes.data, aux_cap, C.byref(na), ends.ctypes.data)
        if rc == 0:
            return lines[:nl.value], aux[:na.value], ends[:n]
        if attempt or rc != H2G_ERR_ARG or (nl.value <= line_cap and na.value <= aux_cap):
            _chk(rc, "h2g_sam_plan")
        line_cap, aux_cap = max(line_cap, nl.value), max(aux_cap, na.value)


def sam_plan_unpaired(sam, codes, offs, quals, name_bytes, name_offs, res, rec, boffs):
    """h2g_sam_plan_unpaired_compact over the arguments of h2g_sam_format_unpaired_compact (sam: the handle of h2g_sam_open) -> (lines [SAM_LINE_DTYPE], pool bytes,
    line_ends [n]); the handle counts what the format call would have counted"""
    n = len(offs) - 1
    keep = (codes, offs, quals, name_bytes, name_offs, res, rec, boffs)
    return _sam_plan(lib().h2g_sam_plan_unpaired_compact, n, [sam] + [_ptr(x) for x in keep[:5]], [_ptr(x) for x in keep[5:]])


def sam_plan_paired(sam, codes1, offs1, quals1, name_bytes1, name_offs1, codes2, offs2, quals2, name_bytes2, name_offs2, res, rec1, boffs1, rec2, boffs2, khits):
    """h2g_sam_plan_paired_compact -> (lines, pool bytes, line_ends [n])"""
    n = len(offs1) - 1
    keep = (codes1, offs1, quals1, name_bytes1, name_offs1, codes2, offs2, quals2, name_bytes2, name_offs2, res, rec1, boffs1, rec2, boffs2)
    return _sam_plan(lib().h2g_sam_plan_paired_compact, n, [sam] + [_ptr(x) for x in keep[:10]], [_ptr(x) for x in keep[10:]] + [khits])


def sam_plan_split_host(sam, set1, set2, res, rec1, boffs1, rec2=None, boffs2=None, khits=0):
    """h2g_sam_plan_split_host: the plain reads planned by the shared planner of csrc/h2g_sam_plan.h, the rest by the host planner, merged in read order (no device).
    set1 / set2 = (codes, offs, quals, name_bytes, name_offs), set2 None for an unpaired run -> (lines, pool bytes, line_ends [n], class bytes [n])"""
    n = len(set1[1]) - 1
    classes = np.zeros(max(n, 1), dtype=np.uint8)
    head = [sam] + [_ptr(x) for x in set1] + ([_ptr(x) for x in set2] if set2 is not None else [None] * 5)
    tail = [_ptr(res), _ptr(rec1), _ptr(boffs1), _ptr(rec2), _ptr(boffs2), khits]
    call = lambda *a: lib().h2g_sam_plan_split_host(*a, classes.ctypes.data)
    lines, aux, ends = _sam_plan(call, n, head, tail)
    return lines, aux, ends, classes[:n]


def _sam_text(call, n_lines, cap=None):
    """runs a text call: first with `cap` (default: sized by a first call that only reports the bytes needed), -> (text bytes, line_offs [n_lines + 1])"""
    used = C.c_size_t(0)
    offs = np.zeros(n_lines + 1, dtype=np.uint64)
    if cap is None:
        rc = call(None, 0, C.byref(used), None)
        if rc not in (0, H2G_ERR_ARG) or (rc == H2G_ERR_ARG and used.value == 0):
            _chk(rc, "h2g_sam_text")
        cap = used.value
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    _chk(call(out.ctypes.data, cap, C.byref(used), offs.ctypes.data), "h2g_sam_text")
    return out[:used.value].tobytes(), offs


def sam_text_from_plan_host(sam, set1, set2, rec1, rec2, lines, aux, cap=None):
    """h2g_sam_text_from_plan_host: the emitter's host instantiation.  set1 / set2 = (codes, offs, quals, name_bytes, name_offs) as given to the planner (set2 None for
    an unpaired plan) -> (text bytes, line_offs)"""
    lines = np.ascontiguousarray(lines, dtype=SAM_LINE_DTYPE)
    aux = np.ascontiguousarray(aux, dtype=np.uint8)
    n = len(set1[1]) - 1
    a = [_ptr(x) for x in set1] + ([_ptr(x) for x in set2] if set2 is not None else [None] * 5)
    nr1 = 0 if rec1 is None else len(rec1)
    nr2 = 0 if rec2 is None else len(rec2)
    keep = (set1, set2, rec1, rec2)
    call = lambda out, cap_, used, offs: lib().h2g_sam_text_from_plan_host(sam, *a, n, _ptr(rec1), nr1, _ptr(rec2), nr2, lines.ctypes.data, len(lines), aux.ctypes.data, len(aux), out, cap_, used, offs)
    r = _sam_text(call, len(lines), cap)
    del keep
    return r


_lib = None


def lib():
    """Load libh2g.so (built by hisat2_amd/csrc/Makefile).  Raises if it is not there: no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    if os.environ.get("H2G_LIB"):          # development: a variant build of the library
        LIB_PATH = os.environ["H2G_LIB"]
    if not os.path.exists(LIB_PATH):
        raise H2GError(f"{LIB_PATH} not built (run __graft_entry__.build()); hisat2_amd has no CPU path")
    L = C.CDLL(LIB_PATH)
    P, vp = C.POINTER, C.c_void_p
    L.h2g_last_error.restype = C.c_char_p
    L.h2g_index_load.argtypes = [C.c_char_p, P(LoadOpts), P(vp)]
    L.h2g_index_get_info.argtypes = [vp, P(IndexInfo)]
    L.h2g_index_synth_sides.argtypes = [u64, u64, C.c_int, P(vp)]
    L.h2g_index_free.argtypes = [vp]
    L.h2g_index_free.restype = None
    L.h2g_index_dense_sa_check.argtypes = [vp, P(u32), P(u64)]
    L.h2g_index_dense_lsa_check.argtypes = [vp, P(u32), P(u64)]
    L.h2g_stream_create.argtypes = [vp, C.c_size_t, C.c_size_t, P(vp)]
    L.h2g_stream_free.argtypes = [vp]
    L.h2g_stream_free.restype = None
    L.h2g_stream_hip.argtypes = [vp]
    L.h2g_stream_hip.restype = vp
    L.h2g_stream_sync.argtypes = [vp]
    L.h2g_stream_select_batch.argtypes = [vp, C.c_uint]
    L.h2g_set_reads.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.h2g_rank_bench.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, P(C.c_float)]
    L.h2g_rank_bench_synth.argtypes = [vp, C.c_size_t, u64, C.c_int, C.c_int, P(C.c_float), P(u64)]
    L.h2g_rank_bench_synth_sample.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.h2g_fm_search.argtypes = [vp, vp, C.c_size_t, u32, vp]
    L.h2g_sa_resolve.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
    L.h2g_sw_align.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, P(C.c_float)]
    L.h2g_adjust_with_alt.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
    L.h2g_sa_resolve_graph.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, vp]
    L.h2g_graph_lf.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
    L.h2g_fm_search_graph.argtypes = [vp, vp, C.c_size_t, u32, u32, vp, vp]
    L.h2g_index_synth_graph_sides.argtypes = [u64, u64, C.c_int, P(vp)]
    L.h2g_extend.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.h2g_seed_params_init.argtypes = [P(SeedParams), vp, C.c_int]
    L.h2g_seed_params_init.restype = None
    L.h2g_seed_extend_run.argtypes = [vp, P(SeedParams)]
    L.h2g_seed_extend_fetch.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.h2g_get_counters.argtypes = [vp, P(Counters)]
    L.h2g_align_params_init.argtypes = [P(AlignParams), vp]
    L.h2g_align_params_init.restype = None
    L.h2g_align_option_arity.argtypes = [C.c_char_p]
    L.h2g_align_params_apply_options.argtypes = [P(AlignParams), P(AlignPresets), P(C.c_char_p), C.c_size_t, C.c_char_p, C.c_size_t]
    L.h2g_align_params_presets.argtypes = [P(AlignParams), C.c_int, P(AlignPresets)]
    L.h2g_align_params_presets.restype = None
    L.h2g_ext_search.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
    L.h2g_local_index_of.argtypes = [vp, u32, u32]
    L.h2g_local_index_of.restype = u32
    L.h2g_set_read_names.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    L.h2g_align_run.argtypes = [vp, P(AlignParams)]
    L.h2g_align_fetch.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t]
    L.h2g_set_mates.argtypes = [vp, vp, vp, vp, C.c_char_p, vp, C.c_size_t]
    L.h2g_set_read_seeds.argtypes = [vp, vp, vp, C.c_size_t]
    L.h2g_set_read_filter.argtypes = [vp, vp, vp]
    L.h2g_set_read_ids.argtypes = [vp, vp]
    L.h2g_window_plan_create.argtypes = [u32, u32, u64, P(vp)]
    L.h2g_window_plan_add_file.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.h2g_window_plan_get_info.argtypes = [vp, P(WindowPlanInfo)]
    L.h2g_window_plan_text.argtypes = [vp]
    L.h2g_window_plan_text.restype = vp
    L.h2g_window_plan_prefixes.argtypes = [vp]
    L.h2g_window_plan_prefixes.restype = vp
    L.h2g_window_plan_segments.argtypes = [vp, u64, u64, vp, C.c_size_t]
    L.h2g_window_plan_segments.restype = C.c_size_t
    L.h2g_window_plan_select.argtypes = [vp, u64, u64, P(u64), P(u64)]
    L.h2g_window_plan_select.restype = None
    L.h2g_window_plan_free.argtypes = [vp]
    L.h2g_window_plan_free.restype = None
    L.h2g_set_reads_windows.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, u32, u32, vp, C.c_size_t]
    L.h2g_get_windows_stats.argtypes = [vp, P(WindowsStats)]
    L.h2g_fetch_reads.argtypes = [vp, P(C.c_size_t), P(C.c_size_t), P(C.c_size_t), P(C.c_int), vp, vp, vp, vp, vp]
    L.h2g_set_reads_fastq.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, P(FastqOpts), P(FastqResult)]
    L.h2g_fetch_read_set.argtypes = [vp, C.c_int, P(C.c_size_t), P(C.c_size_t), P(C.c_size_t), vp, vp, vp, vp, vp]
    L.h2g_get_fastq_stats.argtypes = [vp, P(FastqStats)]
    L.h2g_align_pairs_run.argtypes = [vp, P(AlignParams)]
    sz = C.c_size_t
    L.h2g_sam_plan_unpaired_compact.argtypes = [vp] * 6 + [sz, vp, vp, vp, vp, sz, P(sz), vp, sz, P(sz), vp]
    L.h2g_sam_plan_paired_compact.argtypes = [vp] * 11 + [sz, vp, vp, vp, vp, vp, u32, vp, sz, P(sz), vp, sz, P(sz), vp]
    L.h2g_sam_text_unpaired.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, P(sz), vp]
    L.h2g_sam_text_paired.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, P(sz), vp]
    L.h2g_sam_text_from_plan_host.argtypes = [vp] * 11 + [sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, P(sz), vp]
    L.h2g_get_sam_text_stats.argtypes = [vp, P(SamTextStats)]
    L.h2g_sam_text_unpaired_planned.argtypes = [vp] * 7 + [sz, vp, vp, vp, vp, sz, P(sz), vp, sz, P(sz), vp]
    L.h2g_sam_text_paired_planned.argtypes = [vp] * 12 + [sz, vp, vp, vp, vp, vp, u32, vp, sz, P(sz), vp, sz, P(sz), vp]
    L.h2g_get_sam_plan_stats.argtypes = [vp, P(SamPlanStats), vp, sz]
    L.h2g_sam_plan_split_host.argtypes = [vp] * 11 + [sz, vp, vp, vp, vp, vp, u32, vp, sz, P(sz), vp, sz, P(sz), vp, vp]
    L.h2g_align_pairs_fetch.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t]
    L.h2g_align_fetch_dense.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t]
    L.h2g_align_pairs_fetch_dense.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t]
    _lib = L
    return L


def _chk(rc, what):
    if rc != 0:
        msg = lib().h2g_last_error()
        raise H2GError(f"{what} failed: status {rc} ({msg.decode() if msg else ''})")


def mstreams_policy(units, last_bails, linear, pinned=0, light=2):
    """development hook (h2g_mstreams_policy, a pure host function): the machine streams a run keeps in rotation for a batch of `units` pairs whose
    latest finished fast pass handed on `last_bails`; pinned = H2G_MSTREAMS (0: not set), light = H2G_MSTREAMS_LIGHT"""
    f = lib().h2g_mstreams_policy
    f.argtypes = [C.c_ulonglong, C.c_uint, C.c_int, C.c_uint, C.c_uint]
    f.restype = C.c_uint
    return int(f(int(units), int(last_bails), int(bool(linear)), int(pinned), int(light)))


class WindowPlan:
    """-F <len>,<step>: the planner of include/h2g.h (h2g_window_plan_*; host only).  add_file() takes the bytes of one FASTA file; the id counter
    carries over from file to file.  text / prefixes are copies; segments(first, n) is a WINDOW_SEG_DTYPE array."""
    def __init__(self, length, step, first_rdid=0):
        self.h = C.c_void_p()
        _chk(lib().h2g_window_plan_create(length, step, first_rdid, C.byref(self.h)), "h2g_window_plan_create")
        self.len, self.step = length, step

    def add_file(self, data: bytes):
        _chk(lib().h2g_window_plan_add_file(self.h, data, len(data)), "h2g_window_plan_add_file")

    def info(self):
        i = WindowPlanInfo()
        _chk(lib().h2g_window_plan_get_info(self.h, C.byref(i)), "h2g_window_plan_get_info")
        return i

    @property
    def n_reads(self):
        return int(self.info().n_reads)

    def text(self):
        n = int(self.info().n_text)
        return np.frombuffer(C.string_at(lib().h2g_window_plan_text(self.h), n), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8)

    def prefixes(self):
        n = int(self.info().n_prefix_bytes)
        return C.string_at(lib().h2g_window_plan_prefixes(self.h), n) if n else b""

    def segments(self, first=0, n=None):
        n = self.n_reads - first if n is None else n
        cnt = lib().h2g_window_plan_segments(self.h, first, n, None, 0)
        out = np.zeros(cnt, dtype=WINDOW_SEG_DTYPE)
        if cnt:
            lib().h2g_window_plan_segments(self.h, first, n, out.ctypes.data, cnt)
        return out

    def select(self, rdid_lo, rdid_hi):
        """-> (first_read, n): the reads with rdid_lo <= rdid < rdid_hi (-s / -u)"""
        a, b = C.c_uint64(), C.c_uint64()
        lib().h2g_window_plan_select(self.h, rdid_lo, rdid_hi, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        if self.h:
            lib().h2g_window_plan_free(self.h)
            self.h = C.c_void_p()


def expand_windows(text, segs, length, step, prefixes):
    """The arrays h2g_set_reads_windows leaves on the device, computed on the host with numpy: (codes, offs, name bytes, name offs, ids)."""
    text = np.asarray(text, dtype=np.uint8)
    starts, names, ids = [], [], []
    for s in segs:
        j = np.arange(int(s["n_windows"]), dtype=np.uint64)
        starts.append(np.uint64(s["text_start"]) + j * np.uint64(step))
        pre = prefixes[int(s["prefix_start"]):int(s["prefix_start"]) + int(s["prefix_len"])]
        names += [pre + str(int(s["name_off0"]) + int(k) * step).encode() for k in j]
        ids.append(((np.uint64(s["rdid0"]) + j * np.uint64(step)) & np.uint64(0xffffffff)).astype(np.uint32))
    starts = np.concatenate(starts) if starts else np.zeros(0, np.uint64)
    n = len(starts)
    codes = text[(starts[:, None] + np.arange(length, dtype=np.uint64)[None, :]).astype(np.int64)].reshape(-1)
    offs = (np.arange(n + 1, dtype=np.uint64) * np.uint64(length)).astype(np.uint32)
    noffs = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
    return codes, offs, b"".join(names), noffs, (np.concatenate(ids) if ids else np.zeros(0, np.uint32))


class Index:
    def __init__(self, base=None, device=0, synth_sides=None, seed=20260925, graph=False):
        L = lib()
        self.h = C.c_void_p()
        if synth_sides is not None and graph:
            _chk(L.h2g_index_synth_graph_sides(int(synth_sides), int(seed), int(device), C.byref(self.h)),
                 "h2g_index_synth_graph_sides")
        elif synth_sides is not None:
            _chk(L.h2g_index_synth_sides(int(synth_sides), int(seed), int(device), C.byref(self.h)), "h2g_index_synth_sides")
        else:
            o = LoadOpts(device, 1)
            _chk(L.h2g_index_load(base.encode(), C.byref(o), C.byref(self.h)), "h2g_index_load")
        self.info = IndexInfo()
        _chk(L.h2g_index_get_info(self.h, C.byref(self.info)), "h2g_index_get_info")

    def dense_sa(self, verify=False):
        """Waits for the dense SA table's build (H2G_DENSE_SA).  -> (has_table, rows that differ from the canonical walk or None)"""
        st, nd = u32(0), u64(0)
        _chk(lib().h2g_index_dense_sa_check(self.h, C.byref(st), C.byref(nd) if verify else None), "h2g_index_dense_sa_check")
        return bool(st.value), (int(nd.value) if verify else None)

    def dense_lsa(self, verify=False):
        """Waits for the build of the dense table of local rows (H2G_DENSE_LSA).  -> (has_table, entries that differ from the canonical walk or None)"""
        st, nd = u32(0), u64(0)
        _chk(lib().h2g_index_dense_lsa_check(self.h, C.byref(st), C.byref(nd) if verify else None), "h2g_index_dense_lsa_check")
        return bool(st.value), (int(nd.value) if verify else None)

    def close(self):
        if self.h:
            lib().h2g_index_free(self.h)
            self.h = C.c_void_p()


class PinnedPool:
    """page-locked host buffers by key (h2g_host_alloc), grown on demand, handed out as numpy views: what a caller moving results over PCIe allocates once"""
    def __init__(self):
        L = lib()
        L.h2g_host_alloc.restype = C.c_void_p
        L.h2g_host_alloc.argtypes = [C.c_size_t]
        L.h2g_host_free.argtypes = [C.c_void_p]
        self._b = {}

    def array(self, key, nbytes, dtype=np.uint8):
        p, cap = self._b.get(key, (None, 0))
        if cap < nbytes:
            if p:
                lib().h2g_host_free(p)
            cap = nbytes + nbytes // 4 + 4096
            p = lib().h2g_host_alloc(cap)
            if not p:
                raise H2GError("h2g_host_alloc(%d) failed" % cap)
            self._b[key] = (p, cap)
        raw = (C.c_uint8 * cap).from_address(p)
        return np.frombuffer(raw, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize)

    def close(self):
        for p, _ in self._b.values():
            lib().h2g_host_free(p)
        self._b = {}


class Stream:
    def __init__(self, index: Index, max_reads=0, max_bases=0):
        self.ix = index
        self.h = C.c_void_p()
        _chk(lib().h2g_stream_create(index.h, max_reads, max_bases, C.byref(self.h)), "h2g_stream_create")
        self.n_reads = 0
        self._batch = 0
        self._batch_n = {}

    def select_batch(self, k: int):
        """resident batch k (h2g_stream_select_batch): the set_* calls, runs and fetches that follow are its own; runs over other batches stay in flight"""
        self._batch_n[self._batch] = self.n_reads
        _chk(lib().h2g_stream_select_batch(self.h, k), "h2g_stream_select_batch")
        self._batch = k
        self.n_reads = self._batch_n.get(k, 0)

    def close(self):
        if self.h:
            lib().h2g_stream_free(self.h)
            self.h = C.c_void_p()

    def set_reads(self, codes: np.ndarray, offs: np.ndarray, quals=None):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        n = len(offs) - 1
        q = None
        if quals is not None:
            q = np.ascontiguousarray(quals, dtype=np.uint8).ctypes.data
        _chk(lib().h2g_set_reads(self.h, codes.ctypes.data, offs.ctypes.data, q, n), "h2g_set_reads")
        self.n_reads = n

    def set_reads_windows(self, text, segs, length, step, prefixes=b""):
        """-F windows expanded on the device (h2g_set_reads_windows): for the selected batch what set_reads + set_read_names + set_read_ids do with the
        expanded arrays.  text: codes 0..4; segs: WINDOW_SEG_DTYPE (WindowPlan.segments)"""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        segs = np.ascontiguousarray(segs, dtype=WINDOW_SEG_DTYPE)
        pre = np.frombuffer(bytes(prefixes), dtype=np.uint8)
        _chk(lib().h2g_set_reads_windows(self.h, text.ctypes.data, len(text), segs.ctypes.data, len(segs), length, step, pre.ctypes.data if len(pre) else None, len(pre)),
             "h2g_set_reads_windows")
        self.n_reads = int(segs["n_windows"].sum())

    def windows_stats(self):
        st = WindowsStats()
        _chk(lib().h2g_get_windows_stats(self.h, C.byref(st)), "h2g_get_windows_stats")
        return st

    def fetch_reads(self):
        """the selected batch as the device holds it (h2g_fetch_reads): dict(codes, offs, names (bytes), name_offs, ids (None without explicit ids))"""
        n, nb, nn, hi = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
        _chk(lib().h2g_fetch_reads(self.h, C.byref(n), C.byref(nb), C.byref(nn), C.byref(hi), None, None, None, None, None), "h2g_fetch_reads")
        codes = np.zeros(nb.value, np.uint8); offs = np.zeros(n.value + 1, np.uint32)
        names = np.zeros(nn.value, np.uint8); noffs = np.zeros(n.value + 1, np.uint32)
        ids = np.zeros(n.value, np.uint32) if hi.value else None
        _chk(lib().h2g_fetch_reads(self.h, C.byref(n), C.byref(nb), C.byref(nn), C.byref(hi), codes.ctypes.data, offs.ctypes.data, names.ctypes.data if nn.value else None,
                                   noffs.ctypes.data if nn.value else None, None if ids is None else ids.ctypes.data), "h2g_fetch_reads")
        return {"codes": codes, "offs": offs, "names": names.tobytes(), "name_offs": noffs, "ids": ids}

    def set_reads_fastq(self, text1, text2=None, *, trim5=0, trim3=0, phred64=False, max_records=0, final=True):
        """FASTQ records parsed on the device (h2g_set_reads_fastq): for the selected batch what set_reads + set_read_names (+ set_mates) do with a host parser's
        arrays of the same bytes.  text1 / text2: bytes-like, beginning at a record start; final: the texts end their input (a pair (final1, final2) sets them apart).
        Returns the FastqResult; with n_not_plain > 0 the batch is left empty and the caller parses the bytes itself.  An H2GError carries the result as .result."""
        t1 = np.frombuffer(bytes(text1), dtype=np.uint8)
        t2 = None if text2 is None else np.frombuffer(bytes(text2), dtype=np.uint8)
        f1, f2 = final if isinstance(final, tuple) else (final, final)
        opts = FastqOpts(trim5, trim3, 1 if phred64 else 0, 1 if f1 else 0, 1 if f2 else 0, 0, max_records)
        res = FastqResult()
        # (an unpaired call hands NULL for text2; an empty text still needs an address that is not NULL)
        rc = lib().h2g_set_reads_fastq(self.h, t1.ctypes.data if len(t1) else _EMPTY.ctypes.data, len(t1),
                                       None if t2 is None else (t2.ctypes.data if len(t2) else _EMPTY.ctypes.data), 0 if t2 is None else len(t2), C.byref(opts), C.byref(res))
        self.n_reads = int(res.n_records) if rc == 0 and res.n_not_plain == 0 else 0
        try:
            _chk(rc, "h2g_set_reads_fastq")
        except H2GError as e:
            e.result = res
            raise
        return res

    def fetch_read_set(self, mate=0):
        """one mate of the selected batch as the device holds it (h2g_fetch_read_set): dict(codes, offs, quals (None without qualities), names (bytes), name_offs)"""
        n, nb, nn = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _chk(lib().h2g_fetch_read_set(self.h, mate, C.byref(n), C.byref(nb), C.byref(nn), None, None, None, None, None), "h2g_fetch_read_set")
        codes = np.zeros(nb.value, np.uint8); offs = np.zeros(n.value + 1, np.uint32)
        quals = np.zeros(nb.value, np.uint8)
        names = np.zeros(nn.value, np.uint8); noffs = np.zeros(n.value + 1, np.uint32)
        have_n = n.value and nn.value
        rc = lib().h2g_fetch_read_set(self.h, mate, C.byref(n), C.byref(nb), C.byref(nn), codes.ctypes.data, offs.ctypes.data, quals.ctypes.data,
                                      names.ctypes.data if have_n else None, noffs.ctypes.data if have_n else None)
        if rc == -4:     # H2G_ERR_ARG: a set without qualities (any other status is an error of its own)
            quals = None
            rc = lib().h2g_fetch_read_set(self.h, mate, C.byref(n), C.byref(nb), C.byref(nn), codes.ctypes.data, offs.ctypes.data, None,
                                          names.ctypes.data if have_n else None, noffs.ctypes.data if have_n else None)
        _chk(rc, "h2g_fetch_read_set")
        return {"codes": codes, "offs": offs, "quals": quals, "names": names.tobytes(), "name_offs": noffs}

    def fastq_stats(self):
        st = FastqStats()
        _chk(lib().h2g_get_fastq_stats(self.h, C.byref(st)), "h2g_get_fastq_stats")
        return st

    def rank(self, rows, cs, variant=0, repeats=1):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cs = np.ascontiguousarray(cs, dtype=np.uint8)
        out = np.empty(len(rows), dtype=np.uint32)
        ms = C.c_float(0)
        _chk(lib().h2g_rank_bench(self.h, rows.ctypes.data, cs.ctypes.data, len(rows), out.ctypes.data, variant, 0,
                                  repeats, C.byref(ms)), "h2g_rank_bench")
        return out, ms.value

    def rank_synth(self, n, seed, variant=0, repeats=1):
        ms, ck = C.c_float(0), u64(0)
        _chk(lib().h2g_rank_bench_synth(self.h, n, seed, variant, repeats, C.byref(ms), C.byref(ck)), "h2g_rank_bench_synth")
        return ms.value, ck.value

    def rank_synth_sample(self, stride, nsample):
        """results j * stride (j < nsample) of the last rank_synth run"""
        out = np.empty(nsample, dtype=np.uint32)
        _chk(lib().h2g_rank_bench_synth_sample(self.h, stride, nsample, out.ctypes.data), "h2g_rank_bench_synth_sample")
        return out

    def fm_search(self, queries, khits=5):
        n = len(queries)
        q = (FmQuery * n)(*queries)
        out = (FmHit * n)()
        _chk(lib().h2g_fm_search(self.h, q, n, khits, out), "h2g_fm_search")
        return out

    def ext_search(self, queries, stage_min=8):
        """h2g_ext_search: (hits, stats)"""
        n = len(queries)
        q = (ExtSearchQuery * n)(*queries) if not isinstance(queries, C.Array) else queries
        out = (ExtSearchHit * n)()
        st = ExtSearchStats()
        _chk(lib().h2g_ext_search(self.h, q, n, stage_min, out, C.byref(st)), "h2g_ext_search")
        return out, st

    def sw_align(self, queries, repeats=1):
        """SwAligner call site of hybridSearch (frame + end-to-end DP, 8-bit cells or 16-bit for minsc < -254, + gather + first backtrace) -> (results, kernel ms)"""
        n = len(queries)
        q = (SwQuery * n)(*queries)
        out = (SwResult * n)()
        ms = C.c_float(0)
        _chk(lib().h2g_sw_align(self.h, q, n, out, repeats, C.byref(ms)), "h2g_sw_align")
        return out, ms.value

    def adjust_with_alt(self, queries, cap=8):
        n = len(queries)
        q = (AdjustQuery * n)(*queries)
        hits = (GHit * (n * cap))()
        nh = (u32 * n)()
        _chk(lib().h2g_adjust_with_alt(self.h, q, n, cap, hits, nh), "h2g_adjust_with_alt")
        return hits, nh

    def sa_resolve_graph(self, queries, iedges, cap=24):
        n = len(queries)
        q = (GsaQuery * n)(*queries)
        ie = (IEdges * n)(*iedges)
        co = (Coord * (n * cap))()
        res = (SaResult * n)()
        _chk(lib().h2g_sa_resolve_graph(self.h, q, ie, n, cap, co, res), "h2g_sa_resolve_graph")
        return co, res

    def graph_lf(self, queries, k=10):
        """GFM::mapGLF / mapGLF1 on a graph index -> (results, in-edge lists)"""
        n = len(queries)
        q = (GlfQuery * n)(*queries)
        res = (GlfResult * n)()
        ie = (IEdges * n)()
        _chk(lib().h2g_graph_lf(self.h, q, n, k, res, ie), "h2g_graph_lf")
        return res, ie

    def fm_search_graph(self, queries, khits=10, kseeds=20):
        n = len(queries)
        q = (FmQuery * n)(*queries)
        out = (FmHit * n)()
        ie = (IEdges * n)()
        _chk(lib().h2g_fm_search_graph(self.h, q, n, khits, kseeds, out, ie), "h2g_fm_search_graph")
        return out, ie

    def sa_resolve(self, queries, cap=16):
        n = len(queries)
        q = (SaQuery * n)(*queries)
        co = (Coord * (n * cap))()
        res = (SaResult * n)()
        _chk(lib().h2g_sa_resolve(self.h, q, n, cap, co, res), "h2g_sa_resolve")
        return co, res

    def extend(self, hits, args):
        n = len(hits)
        h = (GHit * n)(*hits)
        a = (ExtArgs * n)(*args)
        res = (ExtResult * n)()
        _chk(lib().h2g_extend(self.h, h, a, n, res), "h2g_extend")
        return h, res

    def seed_params(self, no_spliced=True):
        p = SeedParams()
        lib().h2g_seed_params_init(C.byref(p), self.ix.h, 1 if no_spliced else 0)
        return p

    def seed_extend_run(self, params):
        _chk(lib().h2g_seed_extend_run(self.h, C.byref(params)), "h2g_seed_extend_run")

    def sync(self):
        _chk(lib().h2g_stream_sync(self.h), "h2g_stream_sync")

    def seed_extend_fetch(self, first=0, n=None):
        n = self.n_reads - first if n is None else n
        out = np.zeros(n * 2, dtype=SEED_RESULT_DTYPE)
        _chk(lib().h2g_seed_extend_fetch(self.h, out.ctypes.data, first, n), "h2g_seed_extend_fetch")
        return out

    def counters(self):
        c = Counters()
        _chk(lib().h2g_get_counters(self.h, C.byref(c)), "h2g_get_counters")
        return c

    @staticmethod
    def pack_names(qnames):
        """-> (bytes, uint32 offsets [n + 1]): the form the C ABI takes (a caller that uploads a batch more than once packs once)"""
        return "".join(qnames).encode(), np.concatenate([[0], np.cumsum([len(q) for q in qnames])]).astype(np.uint32)

    def set_read_names(self, qnames):
        nb, offs = qnames if isinstance(qnames, tuple) else self.pack_names(qnames)
        _chk(lib().h2g_set_read_names(self.h, nb, offs.ctypes.data, len(offs) - 1), "h2g_set_read_names")

    def align_params(self):
        p = AlignParams()
        lib().h2g_align_params_init(C.byref(p), self.ix.h)
        return p

    def align_run(self, params=None):
        params = params or self.align_params()
        _chk(lib().h2g_align_run(self.h, C.byref(params)), "h2g_align_run")

    def align_fetch(self, first=0, n=None, with_alignments=True):
        n = self.n_reads - first if n is None else n
        res = np.zeros(n, dtype=READ_RESULT_DTYPE)
        aln = (AlnRes * (n * ALN_CAP))() if with_alignments else None
        _chk(lib().h2g_align_fetch(self.h, res.ctypes.data, aln, first, n), "h2g_align_fetch")
        return res, aln

    def set_read_seeds(self, seeds1, seeds2=None):
        """explicit PRNG seeds of the resident batch's reads (mate 1, and mate 2 for pairs) in place of genRandSeed; None clears them"""
        if seeds1 is None:
            _chk(lib().h2g_set_read_seeds(self.h, None, None, 0), "h2g_set_read_seeds")
            return
        s1 = np.ascontiguousarray(seeds1, dtype=np.uint32)
        s2 = None if seeds2 is None else np.ascontiguousarray(seeds2, dtype=np.uint32)
        _chk(lib().h2g_set_read_seeds(self.h, s1.ctypes.data, None if s2 is None else s2.ctypes.data, len(s1)), "h2g_set_read_seeds")

    def set_read_ids(self, ids):
        """explicit read ids (Read::rdid) of the resident batch's reads in place of first_read_id + index; None clears them"""
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        if a is not None and len(a) != self.n_reads:
            raise ValueError("one id per read of the resident batch")
        _chk(lib().h2g_set_read_ids(self.h, None if a is None else a.ctypes.data), "h2g_set_read_ids")

    def set_read_filter(self, pass1, pass2=None):
        """--qc-filter bytes of the resident batch's reads (mate 1, and mate 2 for pairs): 0 = the read is not aligned; None = that set passes; both None clears them"""
        p1 = None if pass1 is None else np.ascontiguousarray(pass1, dtype=np.uint8)
        p2 = None if pass2 is None else np.ascontiguousarray(pass2, dtype=np.uint8)
        for p in (p1, p2):
            if p is not None and len(p) != self.n_reads:
                raise ValueError("one filter byte per read of the resident batch")
        _chk(lib().h2g_set_read_filter(self.h, None if p1 is None else p1.ctypes.data, None if p2 is None else p2.ctypes.data), "h2g_set_read_filter")

    def set_mates(self, codes2, offs2, qnames2, quals2=None):
        codes2 = np.ascontiguousarray(codes2, dtype=np.uint8)
        offs2 = np.ascontiguousarray(offs2, dtype=np.uint32)
        nb, noffs = qnames2 if isinstance(qnames2, tuple) else self.pack_names(qnames2)
        q = None if quals2 is None else np.ascontiguousarray(quals2, dtype=np.uint8).ctypes.data
        _chk(lib().h2g_set_mates(self.h, codes2.ctypes.data, offs2.ctypes.data, q, nb, noffs.ctypes.data, len(offs2) - 1), "h2g_set_mates")

    def align_fetch_dense(self, first=0, n=None):
        """-> (res, aln, offs): only the printed alignments, read i's records are aln[offs[i]:offs[i+1]]"""
        n = self.n_reads - first if n is None else n
        res = np.zeros(n, dtype=READ_RESULT_DTYPE)
        offs = np.zeros(n + 1, dtype=np.uint64)
        cap = n * 2 + 16
        while True:
            aln = (AlnRes * cap)()
            rc = lib().h2g_align_fetch_dense(self.h, res.ctypes.data, aln, cap, offs.ctypes.data, first, n)
            if rc == 0:
                return res, aln, offs
            if int(offs[n]) <= cap:
                _chk(rc, "h2g_align_fetch_dense")
            cap = int(offs[n])

    def align_pairs_fetch_dense(self, first=0, n=None):
        n = self.n_reads - first if n is None else n
        res = (PairResult * n)()
        o1 = np.zeros(n + 1, dtype=np.uint64)
        o2 = np.zeros(n + 1, dtype=np.uint64)
        c1 = c2 = n * 2 + 16
        while True:
            a1 = (AlnRes * c1)()
            a2 = (AlnRes * c2)()
            rc = lib().h2g_align_pairs_fetch_dense(self.h, res, a1, c1, o1.ctypes.data, a2, c2, o2.ctypes.data, first, n)
            if rc == 0:
                return res, a1, o1, a2, o2
            if int(o1[n]) <= c1 and int(o2[n]) <= c2:
                _chk(rc, "h2g_align_pairs_fetch_dense")
            c1, c2 = max(c1, int(o1[n])), max(c2, int(o2[n]))

    def tune(self, key, value):
        """development / measurement knobs of go_run by name (h2g_stream_tune: "mstreams", "mach_total", "fast_reserve", "pair_slots", "fast",
        "fast_spliced" — 0 (the default): a spliced run on a linear index goes to the general machine whole, 1: through the fast pass's spliced build first —, ...)"""
        f = lib().h2g_stream_tune
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        _chk(f(self.h, key.encode(), int(value)), "h2g_stream_tune " + key)

    def probe(self, key):
        """development hook, read-only (h2g_stream_probe): "mstreams_rotation" (machine streams in rotation for the last run behind a fast pass),
        "mstreams_used" (those that ever entered it), "mstreams_created", "pools" (workspace pools allocated), "lanes" """
        f = lib().h2g_stream_probe
        f.argtypes = [C.c_void_p, C.c_char_p]
        f.restype = C.c_long
        v = int(f(self.h, key.encode()))
        if v < 0:
            raise H2GError("h2g_stream_probe: no such name: " + key)
        return v

    def align_pairs_fetch_compact(self, first=0, n=None, pinned=None):
        """-> (res, rec1, boffs1, rec2, boffs2): compact records (40 bytes + 12 per edit held, 8-aligned) as uint8 arrays, byte offsets [n + 1] per mate.
        pinned: a PinnedPool whose page-locked buffers the results land in (valid until its next use)"""
        n = self.n_reads - first if n is None else n
        f = lib().h2g_align_pairs_fetch_compact
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
        alloc = pinned.array if pinned is not None else (lambda key, nbytes, dtype=np.uint8: np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype))
        res = alloc("res", n * C.sizeof(PairResult))
        o1 = alloc("o1", (n + 1) * 8, np.uint64); o2 = alloc("o2", (n + 1) * 8, np.uint64)
        c1 = c2 = n * 64 + 4096
        for attempt in range(2):           # at most one retry, and only on "buffer too small" (H2G_ERR_ARG with the needed size in boffs[n]: buffers may be uninitialised memory)
            r1 = alloc("r1", c1); r2 = alloc("r2", c2)
            o1[n] = 0; o2[n] = 0
            rc = f(self.h, res.ctypes.data, r1.ctypes.data, r1.size, o1.ctypes.data, r2.ctypes.data, r2.size, o2.ctypes.data, first, n)
            if rc == 0:
                return res, r1, o1, r2, o2
            if attempt or rc != H2G_ERR_ARG or (int(o1[n]) <= r1.size and int(o2[n]) <= r2.size):
                _chk(rc, "h2g_align_pairs_fetch_compact")
            c1, c2 = max(c1, int(o1[n]) + 8), max(c2, int(o2[n]) + 8)

    def align_fetch_compact(self, first=0, n=None):
        n = self.n_reads - first if n is None else n
        f = lib().h2g_align_fetch_compact
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
        res = np.zeros(n, dtype=READ_RESULT_DTYPE)
        offs = np.zeros(n + 1, dtype=np.uint64)
        cap = n * 64 + 4096
        for attempt in range(2):           # (as align_pairs_fetch_compact: one retry, on "buffer too small" only)
            rec = np.empty(cap, dtype=np.uint8)
            offs[n] = 0
            rc = f(self.h, res.ctypes.data, rec.ctypes.data, cap, offs.ctypes.data, first, n)
            if rc == 0:
                return res, rec, offs
            if attempt or rc != H2G_ERR_ARG or int(offs[n]) <= cap:
                _chk(rc, "h2g_align_fetch_compact")
            cap = int(offs[n]) + 8

    sam_plan_unpaired = staticmethod(sam_plan_unpaired)
    sam_plan_paired = staticmethod(sam_plan_paired)
    sam_plan_split_host = staticmethod(sam_plan_split_host)

    def _sam_text_dev(self, f, sam, lines, aux, cap):
        lines = np.ascontiguousarray(lines, dtype=SAM_LINE_DTYPE)
        aux = np.ascontiguousarray(aux, dtype=np.uint8)
        call = lambda out, cap_, used, offs: f(self.h, sam, lines.ctypes.data, len(lines), aux.ctypes.data, len(aux), out, cap_, used, offs)
        return _sam_text(call, len(lines), cap)

    def sam_text_unpaired(self, sam, lines, aux, cap=None):
        """the text of a plan on the device (h2g_sam_text_unpaired), right after align_fetch_compact of the reads the plan was made from -> (text bytes, line_offs)"""
        return self._sam_text_dev(lib().h2g_sam_text_unpaired, sam, lines, aux, cap)

    def sam_text_paired(self, sam, lines, aux, cap=None):
        """... after align_pairs_fetch_compact (h2g_sam_text_paired)"""
        return self._sam_text_dev(lib().h2g_sam_text_paired, sam, lines, aux, cap)

    def _sam_text_planned(self, call, n, cap):
        """-> (text bytes, line_offs [n_lines + 1], line_ends [n]); cap None: sized by a first call that only reports what is needed (and counts nothing)"""
        used, nl = C.c_size_t(0), C.c_size_t(0)
        if cap is None:
            rc = call(None, 0, C.byref(used), None, 0, C.byref(nl), None)
            if rc not in (0, H2G_ERR_ARG) or (rc == H2G_ERR_ARG and used.value == 0):
                _chk(rc, "h2g_sam_text_planned")
            cap = used.value
        else:
            nl.value = 8 * n + 64
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(nl.value + 1, dtype=np.uint64)
        ends = np.zeros(max(n, 1), dtype=np.uint64)
        _chk(call(out.ctypes.data, cap, C.byref(used), offs.ctypes.data, len(offs) - 1, C.byref(nl), ends.ctypes.data), "h2g_sam_text_planned")
        return out[:used.value].tobytes(), offs[:nl.value + 1], ends[:n]

    def sam_text_unpaired_planned(self, sam, codes, offs, quals, name_bytes, name_offs, res, rec, boffs, cap=None):
        """h2g_sam_text_unpaired_planned right after align_fetch_compact: the arguments of sam_plan_unpaired (the host copy of the fetch, for the handed-on reads)"""
        n = len(offs) - 1
        keep = (codes, offs, quals, name_bytes, name_offs, res, rec, boffs)
        a = [_ptr(x) for x in keep]
        return self._sam_text_planned(lambda *t: lib().h2g_sam_text_unpaired_planned(self.h, sam, *a[:5], n, *a[5:], *t), n, cap)

    def sam_text_paired_planned(self, sam, codes1, offs1, quals1, name_bytes1, name_offs1, codes2, offs2, quals2, name_bytes2, name_offs2, res, rec1, boffs1, rec2, boffs2, khits, cap=None):
        """... after align_pairs_fetch_compact (h2g_sam_text_paired_planned)"""
        n = len(offs1) - 1
        keep = (codes1, offs1, quals1, name_bytes1, name_offs1, codes2, offs2, quals2, name_bytes2, name_offs2, res, rec1, boffs1, rec2, boffs2)
        a = [_ptr(x) for x in keep]
        return self._sam_text_planned(lambda *t: lib().h2g_sam_text_paired_planned(self.h, sam, *a[:10], n, *a[10:], khits, *t), n, cap)

    def sam_plan_stats(self, n=0):
        """of the last *_planned call -> (SamPlanStats, class bytes [n] or None)"""
        st = SamPlanStats()
        cls = np.zeros(n, dtype=np.uint8) if n else None
        _chk(lib().h2g_get_sam_plan_stats(self.h, C.byref(st), _ptr(cls), n), "h2g_get_sam_plan_stats")
        return st, cls

    def sam_text_stats(self):
        st = SamTextStats()
        _chk(lib().h2g_get_sam_text_stats(self.h, C.byref(st)), "h2g_get_sam_text_stats")
        return st

    def align_fetch_long_edits(self):
        """the used prefix of the stream's long-edit area (records with nedits > MAX_EDITS: edits[0].pos is their offset in it) -> (Edit array or None, n)"""
        n = C.c_size_t(0)
        f = lib().h2g_align_fetch_long_edits
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        f(self.h, None, 0, C.byref(n))
        if n.value == 0:
            return None, 0
        a = (Edit * n.value)()
        _chk(f(self.h, a, n.value, C.byref(n)), "h2g_align_fetch_long_edits")
        return a, n.value

    def align_pairs_run(self, params=None):
        params = params or self.align_params()
        _chk(lib().h2g_align_pairs_run(self.h, C.byref(params)), "h2g_align_pairs_run")

    def align_pairs_fetch(self, first=0, n=None, with_alignments=True):
        n = self.n_reads - first if n is None else n
        res = (PairResult * n)()
        a1 = (AlnRes * (n * PAIR_RES_CAP))() if with_alignments else None
        a2 = (AlnRes * (n * PAIR_RES_CAP))() if with_alignments else None
        _chk(lib().h2g_align_pairs_fetch(self.h, res, a1, a2, first, n), "h2g_align_pairs_fetch")
        return res, a1, a2

    def hip_stream(self):
        return lib().h2g_stream_hip(self.h)
