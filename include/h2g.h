/*
 * h2g.h — C ABI of the MI355X-native HISAT2 seed-and-extend hot path (libh2g.so).
 *
 * The reference (HISAT2 2.2.3) has no FFI for this path: the hot path is header-template
 * code called from the per-thread worker loop (hisat2.cpp:3276-3644 -> HI_Aligner::go,
 * hi_aligner.h:4048).  This header is the boundary a maintainer binds instead; each entry
 * point names the reference function whose semantics it reproduces bit-exactly.  Conventions
 * follow the reference's only C ABI, hisat2lib/ht2.h:30-150: opaque handles, `int` status
 * (0 = OK, <0 = error), option structs initialised by a function, no exceptions across the
 * boundary, caller-owned buffers with explicit capacities.
 *
 * Plain pointers and sizes only; no torch / C++ types.  All kernels are hand-written HIP for
 * gfx950; there is NO CPU fallback — every entry point returns H2G_ERR_DEVICE without a GPU.
 */
#ifndef H2G_H_
#define H2G_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2G_EXPORT __attribute__((visibility("default")))   /* cf. hisat2lib/ht2_handle.h:23-27 */

typedef struct h2g_index  h2g_index;    /* immutable device-resident .ht2 index; shareable across streams      */
typedef struct h2g_stream h2g_stream;   /* per-host-thread batch context: device scratch + one hipStream_t     */
typedef int h2g_status;

enum {
	H2G_OK = 0,
	H2G_ERR_IO = -1,          /* index file missing / short read                                        */
	H2G_ERR_FORMAT = -2,      /* not a little-endian .ht2 (32-bit offsets) index                         */
	H2G_ERR_DEVICE = -3,      /* no usable HIP device / HIP runtime error (see h2g_last_error)           */
	H2G_ERR_ARG = -4,         /* bad argument / capacity exceeded                                        */
	H2G_ERR_UNSUPPORTED = -5, /* feature of the reference not built yet (e.g. graph index in a kernel)   */
	H2G_ERR_NOMEM = -6
};

#define H2G_MAX 0xffffffffu     /* INDEX_MAX of the 32-bit (-s) binaries, btypes.h:24-46 */

/* ---- index ------------------------------------------------------------------------------------------ */
typedef struct {
	int32_t device;            /* HIP device ordinal */
	int32_t load_local;        /* also upload the local (.5/.6) indexes */
} h2g_load_opts;

/* GFMParams gfm.h:115-199 + hi_aligner.h:3979 (_minK) */
typedef struct {
	uint32_t len, gbwtLen, numNodes;
	int32_t  lineRate, offRate, ftabChars;
	uint32_t eftabLen, linear;
	uint32_t sideSz, sideGbwtSz, sideGbwtLen, numSides, offsLen, ftabLen;
	uint32_t nPat, nFrag, nZ, minK, nLocal, nRefRecs;
	uint64_t device_bytes;     /* bytes resident in HBM */
} h2g_index_info;

H2G_EXPORT void       h2g_load_opts_init(h2g_load_opts*);
/* Parses <base>.1-.6.ht2 exactly like GFM::readIntoMemory (gfm.h:5823-6453), HGFM::readIntoMemory
 * (hgfm.h:2453-2651) and BitPairReference (reference.cpp:30-380) and uploads them to HBM. */
H2G_EXPORT h2g_status h2g_index_load(const char* ht2_base, const h2g_load_opts*, h2g_index** out);
H2G_EXPORT h2g_status h2g_index_get_info(const h2g_index*, h2g_index_info* out);
/* Roofline helper: a device-only index whose sides hold `num_sides` random linear sides with
 * consistent Occ checkpoints (GRCh38 scale = 15.3 M sides ~ 0.98 GB); only rank queries are valid. */
H2G_EXPORT h2g_status h2g_index_synth_sides(uint64_t num_sides, uint64_t seed, int device, h2g_index** out);
H2G_EXPORT void       h2g_index_free(h2g_index*);
/* The dense SA table of a linear index: SA[row] and the LF steps of the walk from `row` for every row of the BWT (5 bytes per row; 1.3 GB
 * for 256 Mbp, 15.5 GB at GRCh38 size), built on the device by h2g_index_load on a stream of its own.  A run queued once the table is complete
 * resolves a row with two loads; a run queued earlier, or an index without a table, walks — the results, work counters included, are the same.
 * Environment H2G_DENSE_SA, read by h2g_index_load: 0 no table; 1 (default) build it behind the load when it takes at most a quarter of the
 * device memory that is free once the index is uploaded; 2 the same, and the load returns when the table is complete.
 * h2g_index_dense_sa_check waits for the build; *state = 1 when the index has a complete table (else 0), and with rows_differ != NULL every
 * row is walked on the device and the rows whose entry differs from the walk are counted (0 = the table is right). */
H2G_EXPORT h2g_status h2g_index_dense_sa_check(h2g_index*, uint32_t* state, uint64_t* rows_differ);
/* The dense table of LOCAL rows of a linear index: the joined offset (low 16 bits) and the LF steps of the walk (high 16 bits) for every row of every
 * local index, 4 bytes per row (about 1.02 rows per base: 1.05 GB for 256 Mbp, 12.6 GB at GRCh38 size), built behind the global table's build on the
 * same stream.  Either table is used from the moment its own build is over; results and work counters are the same with and without it.
 * Environment H2G_DENSE_LSA, read by h2g_index_load: 0 no table; 1 build it behind the load when it takes at most a quarter of the device memory
 * that is free once the global table is allocated; 2 the same, and the load returns when it is complete; unset: whatever H2G_DENSE_SA resolves to.
 * h2g_index_dense_lsa_check is h2g_index_dense_sa_check for this table. */
H2G_EXPORT h2g_status h2g_index_dense_lsa_check(h2g_index*, uint32_t* state, uint64_t* rows_differ);
/* Splice sites for spliced alignment (SpliceSiteDB, splice_site.h:470): what --known-splicesite-infile / --novel-splicesite-infile
 * hand the reference (SpliceSiteDB::read splice_site.cpp:727: text name, left = last base of the upstream exon, right = first
 * base of the downstream exon, both 0-based, strand).  go() joins reads through them (spliced_aligner.h:409-676, 685-811,
 * 1365-1496) and the SAM formatter leaves their introns out of TLEN (aligner_result.h:1669-1689).  Replaces the previous set;
 * n == 0 empties the database.  readid / fromfile: a site with fromfile == 0 is one found by read `readid` and is visible only to
 * reads readid + window and later (the reference's -p window, hisat2.cpp:3687). */
typedef struct { uint32_t tidx, left, right, readid; uint8_t dir /* 2 = '+', 3 = '-' (SPL_FW / SPL_RC) */, fromfile, known, editdist /* out of h2g_sam_take_novel_sites: mismatches + gaps of the line that crossed the site (<= 255); ignored on input */; } h2g_splice_site;
H2G_EXPORT h2g_status h2g_index_set_splice_sites(h2g_index*, const h2g_splice_site* sites, size_t n, uint32_t window);
/* the sites met since (new ones, or known ones whose smallest read id went down) join the database: O(sites + n log n), no re-allocation;
 * the call waits for the device first (a caller with shards of a wave still in flight pays that wait; the command line merges at wave
 * boundaries only).  Without a h2g_index_set_splice_sites call before it the database starts from the index's own splice-site ALTs and
 * the window is 0 (SpliceSiteDB::addSpliceSite, splice_site.cpp:243; the temporary-splice-site waves of the command line).
 * Queued runs: h2g_align(_pairs)_run calls queued without a fetch between them share the result rows; a run whose options differ
 * from the previous one's first waits for everything still in flight (go_run). */
H2G_EXPORT h2g_status h2g_index_add_splice_sites(h2g_index*, const h2g_splice_site* delta, size_t n);

H2G_EXPORT const char* h2g_last_error(void);

/* ---- stream / reads ---------------------------------------------------------------------------------- */
H2G_EXPORT h2g_status h2g_stream_create(h2g_index*, size_t max_reads, size_t max_bases, h2g_stream** out);
H2G_EXPORT void       h2g_stream_free(h2g_stream*);
H2G_EXPORT void*      h2g_stream_hip(h2g_stream*);   /* the hipStream_t every kernel of this context runs on */
H2G_EXPORT h2g_status h2g_stream_sync(h2g_stream*);
/* Resident batches: a stream holds up to 16 read sets, each with result rows of its own.  Batch 0 is selected when the stream is created.  After a selection the
 * h2g_set_* calls fill that batch, h2g_align_*run works on it and the fetches read its rows; runs queued over other batches stay in flight (their machine passes next
 * to this batch's fast pass), which is a streaming caller's steady state — the reference's worker threads likewise hold different reads at any moment
 * (hisat2.cpp:3276-3644).  The call itself never waits. */
H2G_EXPORT h2g_status h2g_stream_select_batch(h2g_stream*, unsigned batch);

/* Reads as the worker loop holds them after parsing (read.h:325, Read::patFw): one byte per base,
 * codes A,C,G,T,N = 0..4; read i = codes[offs[i] .. offs[i+1]).  quals = ASCII (phred+33) or NULL for
 * FASTA input (all 'I', pat.cpp).  Copied to HBM; the reverse complement (patRc) is derived on device. */
H2G_EXPORT h2g_status h2g_set_reads(h2g_stream*, const uint8_t* codes, const uint32_t* offs, const char* quals,
                                    size_t n_reads);

/* ---- primitives (batched; semantics == the reference function named) ---------------------------------- */

/* GFM::mapLF(SideLocus(row), c) -> countBt2Side (gfm.h:3712, :2958): the Occ-rank micro-kernel.
 * variant: 0 = one lane per side, 1 = 4 lanes per side (16 B each + DPP reduce), 2 = 8 lanes per side.
 * On a graph index (128 B sides): 0 = one lane per side (8 x dwordx4), 1 = 8 lanes per side.
 * rows/cs/out are HOST arrays unless device_ptrs != 0.  *kernel_ms = HIP-event time of the kernel. */
H2G_EXPORT h2g_status h2g_rank_bench(h2g_stream*, const uint32_t* rows, const uint8_t* cs, size_t n, uint32_t* out,
                                     int variant, int device_ptrs, int repeats, float* kernel_ms);
/* generates the SURVEY §8(d) query set on device: row ~ U[0,gbwtLen) from splitmix64(seed), c = hash&3 */
H2G_EXPORT h2g_status h2g_rank_bench_synth(h2g_stream*, size_t n, uint64_t seed, int variant, int repeats,
                                           float* kernel_ms, uint64_t* checksum);
/* out[j] = result j * stride of this stream's last h2g_rank_bench_synth run: the sampled comparison with GFM::mapLF on the CPU */
H2G_EXPORT h2g_status h2g_rank_bench_synth_sample(h2g_stream*, size_t stride, size_t nsample, uint32_t* out);

enum { H2G_FM_PARTIAL = 0, H2G_FM_GLOBAL = 1, H2G_FM_LOCAL = 2 };
enum { H2G_CANDIDATE_HIT = 1, H2G_PSEUDOGENE_HIT = 2, H2G_ANCHOR_HIT = 3 };   /* hi_aligner.h:96-100 */

typedef struct {
	uint32_t read;             /* index into the batch set by h2g_set_reads */
	uint32_t offset;           /* ReadBWTHit::_cur: bases already consumed from the 3' end */
	uint8_t  fw;               /* 1: patFw, 0: patRc */
	uint8_t  mode;             /* H2G_FM_* */
	uint8_t  pseudogeneStop;   /* hi_aligner.h:4669 */
	uint8_t  anchorStop;       /* hi_aligner.h:4670 */
} h2g_fm_query;

/* the BWTHit appended by partialSearch (hi_aligner.h:6361-6600) + the ReadBWTHit counters it updates */
typedef struct {
	uint32_t top, bot, node_top, node_bot, bwoff, len, hit_type;
	uint32_t cur, done, numPartialSearch, numUniqueSearch, pseudogeneStop, anchorStop;
	uint32_t nrank;            /* rank calls (HI_Aligner::bwops_) */
	uint32_t nside;            /* unique sides visited = algorithmic bytes / sideSz */
} h2g_fm_hit;

H2G_EXPORT h2g_status h2g_fm_search(h2g_stream*, const h2g_fm_query* q, size_t n, uint32_t khits, h2g_fm_hit* out);

/* ---- the searches of hybridSearch_recur: globalGFMSearch (hi_aligner.h:6606) and localGFMSearch (:6751) -----------------
 * Backward search of the read bases [.., rdoff] of the searched strand (rdoff counted from its 5' end, inclusive) in the global
 * index (lidx == H2G_MAX) or in local index `lidx` (HGFM::getLocalGFM hgfm.h:1713: lidx = h2g_local_index_of(tidx, toff)).
 * Local queries are bucketed by lidx; a bucket with at least `stage_min` queries is served by one workgroup that first copies
 * the local index's sides (16-33 KB) and ftab (8 KB) into LDS — every rank of those queries is an LDS read; the other queries
 * (and graph-index locals) read their sides from HBM.  stage_min == 0 never stages.  Linear and graph indexes. */
typedef struct { uint32_t read, rdoff, lidx, maxHitLen; uint8_t fw, uniqueStop, pad[2]; } h2g_ext_search_query;
typedef struct { uint32_t nelt, hitlen, top, bot, uniqueStop, nrank, nside, staged; } h2g_ext_search_hit;
typedef struct { uint64_t n_local, n_staged, n_buckets, n_buckets_staged, lds_bytes_staged; float ms_staged, ms_hbm; } h2g_ext_search_stats;
H2G_EXPORT h2g_status h2g_ext_search(h2g_stream*, const h2g_ext_search_query* q, size_t n, uint32_t stage_min, h2g_ext_search_hit* out,
                                     h2g_ext_search_stats* stats /* nullable */);
H2G_EXPORT uint32_t   h2g_local_index_of(const h2g_index*, uint32_t tidx, uint32_t toff);   /* H2G_MAX: none */

/* ---- graph (GFM) index primitives: 128 B sides with F/M bit vectors (gfm.h:160-176) ------------------- */
/* BWTHit::_node_iedge_count (hi_aligner.h:199): nodes of a range with more than one incoming edge */
#ifndef H2G_IEDGE_CAP       /* (a per-translation-unit capacity like H2G_GHIT_EDITS: the graph fast pass keeps lists of two entries and sets 4) */
#define H2G_IEDGE_CAP 24
#endif
typedef struct {
	uint32_t n;                        /* true count; only the first H2G_IEDGE_CAP entries are stored */
	uint32_t e[H2G_IEDGE_CAP][2];      /* {node index relative to node_top, extra in-edges} */
} h2g_iedges;
/* single == 0: GFM::mapGLF(tloc(top), bloc(bot), c, &node_range, &node_iedges, k)   (gfm.h:3759-3837)
 * single != 0: GFM::mapGLF1(top, loc(top), c, &node_range)                          (gfm.h:3957-4021) */
typedef struct { uint32_t top, bot; uint8_t c, single, pad[2]; } h2g_glf_query;
typedef struct { uint32_t ok, top, bot, node_top, node_bot; } h2g_glf_result;   /* ok == 0: empty (0,0) */
H2G_EXPORT h2g_status h2g_graph_lf(h2g_stream*, const h2g_glf_query* q, size_t n, uint32_t k, h2g_glf_result* res,
                                   h2g_iedges* iedges /* [n] or NULL */);
/* partialSearch on a graph index (h2g_fm_search forwards here with kseeds = max(5, 2 khits), hisat2.cpp:3177);
 * iedges[n] (or NULL) receives the in-edge list the BWTHit is initialised with (hi_aligner.h:6570-6578) */
H2G_EXPORT h2g_status h2g_fm_search_graph(h2g_stream*, const h2g_fm_query* q, size_t n, uint32_t khits, uint32_t kseeds,
                                          h2g_fm_hit* out, h2g_iedges* iedges);
/* Roofline helper, graph flavour of h2g_index_synth_sides: random 128 B graph sides with consistent Occ
 * checkpoints (F/M bits random, headers zero); only rank queries (h2g_rank_bench*) are valid on it. */
H2G_EXPORT h2g_status h2g_index_synth_graph_sides(uint64_t num_sides, uint64_t seed, int device, h2g_index** out);

/* HI_Aligner::getGenomeCoords (hi_aligner.h:5774-5855): GroupWalk2S::advanceElement + GFM::joinedToTextOff */
typedef struct { uint32_t top, bot, maxelt, len; uint32_t rejectStraddle; } h2g_sa_query;
typedef struct { uint32_t tidx, toff, joinedOff; } h2g_coord;          /* tidx == H2G_MAX: straddles */
typedef struct { uint32_t ok, ncoords, straddled, nsteps; } h2g_sa_result;
H2G_EXPORT h2g_status h2g_sa_resolve(h2g_stream*, const h2g_sa_query* q, size_t n, uint32_t cap_per_query,
                                     h2g_coord* coords /* [n*cap] */, h2g_sa_result* res /* [n] */);
/* getGenomeCoords on a graph index: the node-based group walk (GroupWalk2S / GWState, group_walk.h:464-1545).  Query i
 * walks the nodes [node_top, node_bot) of rows [top, bot) with in-edge list iedges[i] (as h2g_fm_search_graph returns
 * them; NULL = none).  Results as h2g_sa_resolve; res[i].nsteps == H2G_MAX flags a capacity overflow (ok = 0). */
typedef struct { uint32_t top, bot, node_top, node_bot, maxelt, len, rejectStraddle; } h2g_gsa_query;
H2G_EXPORT h2g_status h2g_sa_resolve_graph(h2g_stream*, const h2g_gsa_query* q, const h2g_iedges* iedges, size_t n,
                                           uint32_t cap_per_query, h2g_coord* coords /* [n*cap] */, h2g_sa_result* res /* [n] */);

/* GenomeHit::extend (hi_aligner.h:2031-2232) incl. alignWithALTs (:683) and calculateScore (:3711) */
#define H2G_MAX_EDITS 32
enum { H2G_EDIT_READ_GAP = 1, H2G_EDIT_REF_GAP = 2, H2G_EDIT_MM = 3, H2G_EDIT_SPL = 5 };  /* edit.h:36-42 */
/* An H2G_EDIT_SPL edit (an intron, CIGAR N) keeps Edit::splLen / splDir / knownSpl in the three bytes chr, qchr, pad:
 * splLen = chr | qchr << 8 | (pad & 15) << 16 (introns up to 2^20), splDir = (pad >> 4) & 7 (splice_site.h:37-43: 1 unknown, 2 +, 3 -,
 * 4 semi +, 5 semi -), knownSpl = pad >> 7; `snp` holds the float bits of SpliceSiteDB::probscore(donor_seq, acceptor_seq). */
typedef struct { uint32_t pos; uint8_t chr, qchr, type, pad; uint32_t snp; /* Edit::snpID: index into the ALT list, H2G_MAX = none */ } h2g_edit;   /* Edit, edit.h */
/* h2g_ghit is also the WORKING hit of the go() kernels.  The go() units with the large workspace (the second pass, h2g_go_big.h) are compiled with
 * longer edit lists in it (H2G_GHIT_EDITS, set before this header is read): the reference's lists are unbounded (hi_aligner.h:421), and a deletion of
 * n bases is n edits.  Every entry point of this header sees the default, H2G_MAX_EDITS. */
#ifndef H2G_GHIT_EDITS
#define H2G_GHIT_EDITS H2G_MAX_EDITS
#endif
typedef struct {
	uint32_t read;
	uint32_t fw, rdoff, len, trim5, trim3, tidx, toff, joinedOff;
	uint32_t splicescore;      /* GenomeHit::_splicescore (mean intron length of the short-anchored splices), truncated */
	int64_t  score;
	uint32_t nedits;
	uint32_t overflow;         /* edit list exceeded H2G_MAX_EDITS: caller must take its own path */
	h2g_edit edits[H2G_GHIT_EDITS];
} h2g_ghit;
typedef struct { uint32_t mm, max_leftext, max_rightext; } h2g_ext_args;
typedef struct { uint32_t extended, leftext, rightext; } h2g_ext_result;
H2G_EXPORT h2g_status h2g_extend(h2g_stream*, h2g_ghit* hits /* in/out */, const h2g_ext_args* args, size_t n,
                                 h2g_ext_result* res);

/* static GenomeHit::adjustWithALT (hi_aligner.h:2239-2390) as getAnchorHits calls it on a graph index (:5175): an anchor
 * (read, strand, rdoff, len) placed at (tidx, toff, joinedOff) by the SA walk -> the GenomeHits it yields once offsets are
 * corrected for indel ALTs (findOffDiffs :2545) and known variants are written as edits.  hits[i * cap ...], nhits[i]. */
typedef struct { uint32_t read, fw, rdoff, len, tidx, toff, joinedOff; } h2g_adjust_query;
H2G_EXPORT h2g_status h2g_adjust_with_alt(h2g_stream*, const h2g_adjust_query* q, size_t n, uint32_t cap, h2g_ghit* hits /* [n*cap] */,
                                          uint32_t* nhits /* [n] */);

/* ---- Smith-Waterman extension (opt-in in the reference: --bowtie2-dp / --sensitive) ---------------------------- */
/* One problem = the SwAligner call site of hybridSearch (spliced_aligner.h:209-262) for one seed hit of one read:
 * DynProgFramer::frameSeedExtensionRect (dp_framer.cpp:81) around refoff = hit.refoff - hit.rdoff, SwAligner::initRef
 * (aligner_sw.cpp:137), the end-to-end fill — 8-bit cells, alignNucleotidesEnd2EndSseU8 (aligner_swsse_ee_u8.cpp:791), or for
 * minsc < -254 16-bit cells, alignNucleotidesEnd2EndSseI16 (aligner_swsse_ee_i16.cpp:793): SwAligner::align's rule, aligner_sw.cpp:496 —,
 * gatherCells (:1202), and the first SwAligner::nextAlignment (aligner_sw.cpp:709) with its backtrace (:1309) and PRNG
 * reseeding.  Edits are in the coordinates of the aligned strand (fw: patFw, !fw: patRc), ascending. */
typedef struct {
	uint32_t read;             /* index into the batch set by h2g_set_reads */
	uint32_t fw;               /* 1: align patFw, 0: patRc */
	uint32_t tidx, refoff;     /* reference id; ref offset implied by the seed hit assuming no gaps */
	int32_t  minsc;            /* _minsc[rdi] (scoreMin.f(len), hisat2.cpp:3470) */
	uint32_t rnd;              /* RandomSource::last on entry */
} h2g_sw_query;
typedef struct {
	int32_t  found_align;      /* SwAligner::align(): at least one candidate cell */
	int32_t  found;            /* SwAligner::nextAlignment() */
	int32_t  best;             /* bestCell: best last-row score (lrmax - 0xff) */
	int32_t  score;            /* AlnRes::score().score() */
	int64_t  off;              /* AlnRes::refcoord().off() */
	uint32_t nedits, gaps;
	uint32_t overflow;         /* edit / branch-stack capacity exceeded: caller must take its own path */
	uint32_t rnd;              /* RandomSource::last on exit */
	int64_t  refl, refr;       /* DPRect::refl / refr (inclusive) */
	h2g_edit edits[H2G_MAX_EDITS];
} h2g_sw_result;
/* *kernel_ms (nullable) = HIP-event time of the SW kernel; repeats > 1 re-runs it for timing */
H2G_EXPORT h2g_status h2g_sw_align(h2g_stream*, const h2g_sw_query* q, size_t n, h2g_sw_result* out, int repeats,
                                   float* kernel_ms);

/* ---- fused seed-and-extend stage over the resident read batch ------------------------------------------ */
/* For every read and both strands: partialSearch from offset 0 (nextBWT hi_aligner.h:4644-4760) ->
 * getAnchorHits coordinate resolution (:5007, ranges up to H2G_SEED_CAP rows) -> 0-mismatch extend
 * (hybridSearch spliced_aligner.h:139-163).  Results stay in HBM until h2g_seed_extend_fetch. */
#define H2G_SEED_CAP 5
typedef struct {
	h2g_fm_hit hit;
	uint32_t   ncoords, straddled, nsteps, pad;
	struct { uint32_t tidx, toff, joinedOff, rdoff, len; int32_t score; } ext[H2G_SEED_CAP];
} h2g_seed_result;                         /* one per (read, strand): index 2*read + (fw ? 0 : 1) */

typedef struct {
	uint32_t pseudogeneStop, anchorStop, khits;
	uint32_t search_variant;   /* 0 = lane-per-query search kernel, 1 = cooperative 8-lane kernel */
} h2g_seed_params;

H2G_EXPORT void       h2g_seed_params_init(h2g_seed_params*, const h2g_index*, int no_spliced_alignment);
H2G_EXPORT h2g_status h2g_seed_extend_run(h2g_stream*, const h2g_seed_params*);     /* async on the stream */
H2G_EXPORT h2g_status h2g_seed_extend_fetch(h2g_stream*, h2g_seed_result* out, size_t first_read, size_t n_reads);

/* ---- the coarse entry: HI_Aligner::go for every read of the resident batch ---------------------------------- */
/* Semantics == one iteration of the worker loop body (hisat2.cpp:3380-3640) for an unpaired read that passed the
 * filters: rnd.init(genRandSeed(read)) (pat.h:55), splicedAligner.go(...) (hi_aligner.h:4048), and the selection
 * half of AlnSinkWrap::finishRead (aln_sink.h:1939 -> selectByScore :2680).  Built so far: linear (HFM) and SNP-graph
 * (GFM + ALT database) indexes, --no-spliced-alignment, default scoring, --bowtie2-dp 0/1/2. */
#define H2G_FW_STRAND 1u
#define H2G_FW_TCLASS 2u
#define H2G_FW_TCLASS_SHIFT 2
#define H2G_ALN_CAP 10             /* alignments returned per read (>= -k: 5 on linear, 10 on graph indexes) */
typedef struct {                   /* == the arguments reportHit (hi_aligner.h:6064-6166) passes to AlnRes::init */
	uint32_t fw, tidx, toff, len, trim5, trim3, nedits, splicescore;   /* splicescore: AlnScore::splicescore_ (aligner_result.h:322) */
	/* fw: bit 0 (H2G_FW_STRAND) is the strand, 1 = patFw.  Under avoid_pseudogene / transcriptome_mapping_only bit 1 (H2G_FW_TCLASS) is set
	 * and bits 2-3 hold the transcript class reportHit gave the alignment (0 none, 1 spliced or near splice sites, 2 known transcripts:
	 * AlnScore::calculate_hisat2_score bits 24-27, aligner_result.h:335-337); without those options fw is 0 / 1 and the class follows from
	 * the splice edits (2: every splice a database site, 1: spliced).  Read the strand as (fw & H2G_FW_STRAND). */
	int64_t  score;                /* AS:i */
	h2g_edit edits[H2G_MAX_EDITS]; /* as stored in the AlnRes (aligner_result.cpp:110-118): positions along the original read
	                                * 5'->3', relative to its first aligned (non-soft-clipped) base; entries past nedits are unspecified */
} h2g_alnres;
typedef struct {
	uint32_t nres;                 /* alignments reported to the sink (rs1u_) */
	uint32_t nselect;              /* alignments to print, best first; [0] is the primary */
	uint32_t overflow;             /* !=0: a fixed-capacity list overflowed -> caller runs this read through its own go() */
	uint32_t nrank, nsteps, depth; /* work counters: rank calls, SA-walk steps, deepest recursion frame */
	int32_t  best, secbest;        /* AlnSetSumm over all nres alignments (aligner_result.cpp:1209): best / second-best AS:i, */
	uint32_t best_h2, secbest_h2;  /* and the low 32 bits of their AlnScore::hisat2_score_ (aligner_result.h:322: repeat, transcript,
	                                * splice-score and trimmed-base fields — the AlnScore tie-break); best == INT32_MIN = none.  MAPQ, ZS:i */
} h2g_read_result;
typedef struct {
	uint32_t khits, kseeds;        /* -k, --max-seeds: 1 <= khits <= H2G_KHITS_MAX, khits <= kseeds <= H2G_KSEEDS_MAX */
	uint32_t no_spliced_alignment; /* 1: --no-spliced-alignment; 0: introns are placed by combineWith (needs no_temp_splicesite, linear index) */
	uint32_t secondary;
	uint32_t bowtie2_dp;           /* --bowtie2-dp: 0 off (default), 1 SwAligner when no alignment reached minsc, 2 always
	                                * (spliced_aligner.h:209).  Inside go() the DP is run by the read's own lane over
	                                * ~75 KB of HBM scratch per lane; the batched LDS kernel is h2g_sw_align. */
	/* scoring scheme (Scoring scoring.h:29-87; option -> SeedAlignmentPolicy::parseString aligner_seed_policy.cpp:294-620) */
	int32_t  mm_max, mm_min;       /* --mp MX,MN      6,2  (quality-aware mismatch penalty, COST_MODEL_QUAL) */
	int32_t  n_pen;                /* --np            1 */
	int32_t  rdg_const, rdg_linear;/* --rdg           5,3 */
	int32_t  rfg_const, rfg_linear;/* --rfg           5,3 */
	int32_t  sc_max, sc_min;       /* --sp MX,MN      2,1  (soft-clip penalty); --no-softclip = INT32_MAX,INT32_MAX */
	uint32_t score_min_type;       /* --score-min <type>,<const>,<coeff>: 1 = C, 2 = L, 3 = S (sqrt), 4 = G (log)   (simple_func.h:30-33) */
	double   score_min_const, score_min_coeff;   /* default L,0,-0.2 (hisat2.cpp:440) */
	uint32_t no_temp_splicesite;   /* --no-temp-splicesite: novel splice sites are not shared between reads.  Spliced alignment
	                                * (no_spliced_alignment == 0) is built for this setting on linear indexes: every read is independent */
	/* splice scoring (Scoring::canSpl / noncanSpl scoring.h:473-487, TranscriptomePolicy tp.h; hisat2.cpp:493-499, :1631-1688) */
	uint32_t min_intronlen, max_intronlen;           /* --min-intronlen 20, --max-intronlen 500000 */
	int32_t  pen_cansplice, pen_noncansplice;        /* --pen-cansplice 0, --pen-noncansplice 12 */
	uint32_t pen_canintronlen_type, pen_noncanintronlen_type;   /* --pen-canintronlen / --pen-noncanintronlen <type>,<const>,<coeff>: */
	uint32_t first_read_id;                                     /* type as score_min_type; default G,-8,1.  first_read_id: Read::rdid of
	                                                             * read 0 of the batch — the splice-site window compares read ids */
	double   pen_canintronlen_const, pen_canintronlen_coeff, pen_noncanintronlen_const, pen_noncanintronlen_coeff;
	/* TranscriptomePolicy (hisat2.cpp:4076-4084): anchor minima 7 / 14, with --dta (transcript assemblers) 15 / 20 and
	 * --pen-noncanintronlen G,-8,2; xs_only (--dta-cufflinks): spliced alignments of unknown strand are not reported (hi_aligner.h:6101) */
	uint32_t min_anchor_len, min_anchor_len_noncan, xs_only;
	/* --haplotype (graph indexes): an ALT is only tried when a haplotype of the index carries it together with the ALTs already taken
	 * (GraphPolicy::useHaplotype gp.h:71, alignWithALTs_recur hi_aligner.h:2898-2996, :3251-3331) */
	uint32_t use_haplotype;
	/* --max-altstried (GraphPolicy::maxAltsTried, default 16, at least 8: hisat2.cpp:521, :1745): ALTs one extension may walk through
	 * (hi_aligner.h:2794) and, / 4, the offset combinations adjustWithALT tries (:2313, :2423) */
	uint32_t max_alts_tried;
	/* -X / --maxins (PairedEndPolicy::maxfrag, default 1000 hisat2.cpp:345): the longest fragment of a concordant pair (pe.cpp:38; checked
	 * under --no-spliced-alignment, hi_aligner.h:6018) and half the window alignMate searches the other mate in (:5688) */
	uint32_t max_frag_len;
	/* -I / --minins (PairedEndPolicy::minfrag, default 0); --fr / --rf / --ff as pe_orientation 0 / 1 / 2 (gMate1fw, gMate2fw hisat2.cpp:1166-1168:
	 * the strand pair a concordant pair has, hi_aligner.h:5605, :6003, pe.cpp:59-83); --nofw / --norc: the strand of the READ (of mate 1's
	 * fragment strand for pairs, hisat2.cpp:3449-3452) that is not searched (hi_aligner.h:4875) */
	uint32_t min_frag_len, pe_orientation, nofw, norc;
	/* TranscriptomePolicy (tp.h) in reportHit (hi_aligner.h:6105-6127).  avoid_pseudogene (--avoid-pseudogene, spliced alignment only): an
	 * unspliced alignment with a splice site of the database within 10 kbp of either end ranks as "near splice sites", one inside an exon of the
	 * index (widened by 10) as "known transcripts" (AlnScore bits 24-27: the tie-break between equally scored placements).
	 * transcriptome_mapping_only (--tmo): only alignments spliced through known sites only, or (with avoid_pseudogene) inside an exon, are
	 * reported.  no_anchorstop (--no-anchorstop): anchorStop = false (hisat2.cpp:1710).  pen_conflictsplice (--pen-conflictsplice, >= 0,
	 * default 1000000): Scoring::csp, the penalty of an alignment whose splices disagree in direction. */
	uint32_t avoid_pseudogene, transcriptome_mapping_only, no_anchorstop;
	int32_t  pen_conflictsplice;
	/* --seed (hisat2.cpp:1204, default 0): the global seed of genRandSeed (pat.h:55-91), every read's PRNG seed.  h2g_set_read_seeds replaces the
	 * hashed seeds with explicit ones (--non-deterministic) */
	uint32_t seed;
	/* --n-ceil (SimpleFunc nCeil: Scoring::nFilter scoring.cpp:104, the DP's nceil hisat2.cpp:3453-3459): type as score_min_type, default
	 * L,0,0.15 with the coefficient (double)0.15f (aligner_seed_policy.cpp:294); clamped below at 0.  A mate with more Ns than
	 * f(length) is filtered (YF:Z:NS); a mate without N always passes */
	uint32_t n_ceil_type;
	double   n_ceil_const, n_ceil_coeff;
} h2g_align_params;
/* number of visible HIP devices (0 without a GPU: the library has no CPU path) */
H2G_EXPORT int        h2g_device_count(void);
H2G_EXPORT void       h2g_align_params_init(h2g_align_params*, const h2g_index*);
/* --n-ceil as given to the aligner (n_ceil_type / n_ceil_const / n_ceil_coeff) for a SAM handle of include/h2g_sam.h: which unaligned mates
 * it flags YF:Z:NS (default L,0,(double)0.15f, as h2g_align_params_init) */
struct h2g_sam;
H2G_EXPORT void       h2g_sam_set_n_ceil(struct h2g_sam*, uint32_t type, double constant, double coeff);
/* The reference's alignment options (csrc/h2g_options.cpp: host only, needs no device and no index): every rule by which an option changes
 * a field of h2g_align_params.  The command line and the Python binding both parse through these three calls.
 * h2g_align_option_arity: -1 = not an alignment option, 0 = a flag, 1 = takes one argument (aliases such as --minins, --maxins, --tmo,
 * --pen-intronlen included). */
H2G_EXPORT int        h2g_align_option_arity(const char* name);
/* what the options leave for h2g_align_params_presets, which needs the index type */
typedef struct { uint32_t saw_k, k_arg, max_seeds_arg, sensitive, very_sensitive; } h2g_align_presets;
/* Applies opts[0..n) (names known to h2g_align_option_arity, each followed by its argument when its arity is 1) to *p in command-line order,
 * then what the reference applies after every option was read and that does not depend on the index: --dta's anchor minima and
 * --pen-noncanintronlen G,-8,2; --ignore-quals without --mp.  Fills *pre.  On a faulty option returns H2G_ERR_ARG with the message (the
 * reference's wording, no newline) in err[0..err_cap); *p and *pre are then unspecified. */
H2G_EXPORT h2g_status h2g_align_params_apply_options(h2g_align_params* p, h2g_align_presets* pre, const char* const* opts, size_t n,
                                                     char* err, size_t err_cap);
/* The reference applies its presets after ALL options were read (hisat2.cpp:1882-1909) and lets the index type decide the
 * default -k (:3903-3906): khits = saw_k ? k_arg : 10; --sensitive: bowtie2_dp 0 -> 1, khits < 10 -> 10 (counts as saw_k),
 * --score-min L,0,-0.5; --very-sensitive: bowtie2_dp 2, khits < 30 -> 30, L,0,-1; without saw_k khits = 5 (linear) / 10 (graph);
 * max_seeds_arg 0 -> max(5, 2 khits) (:3174).  linear: h2g_index_info.linear.  Call it last, after h2g_align_params_apply_options. */
H2G_EXPORT void       h2g_align_params_presets(h2g_align_params* p, int linear, const h2g_align_presets* pre);
/* Explicit per-read PRNG seeds for the selected resident batch, in place of genRandSeed (hisat2.cpp:3311-3314, --non-deterministic: Read::seed of
 * mate 1 and mate 2 drawn from a RandomSource).  seeds1 / seeds2: [n] (n = the batch's read count); seeds2 is read by paired runs only, and a paired run
 * with seeds1 but no seeds2 is refused.  A pair's PRNG starts from seeds1[i] ^ seeds2[i] when both mates pass the filters (length, --n-ceil) and from
 * seeds1[i] otherwise (hisat2.cpp:3463-3468); an unpaired read's from seeds1[i].  seeds1 == NULL clears them; h2g_set_reads clears them too. */
H2G_EXPORT h2g_status h2g_set_read_seeds(h2g_stream*, const uint32_t* seeds1, const uint32_t* seeds2, size_t n);
/* --qc-filter (hisat2.cpp:3433-3439) for the selected resident batch: one byte per read, 0 = the read failed its QSEQ filter field and is not aligned
 * (go() is skipped for it as for a read that fails the length or --n-ceil filter; its mate, if it passes, is aligned alone and the pair's PRNG starts
 * from mate 1's seed alone).  pass1 / pass2: mate 1's / mate 2's bytes ([n], n = the batch's read count); NULL = that set passes as a whole; both NULL
 * clears them; h2g_set_reads clears them too.  pass2 is read by paired runs only.  The sink prints YF:Z:QC for such a read (h2g_sam_set_read_filter). */
H2G_EXPORT h2g_status h2g_set_read_filter(h2g_stream*, const uint8_t* pass1, const uint8_t* pass2);
/* Explicit read ids (Read::rdid) for the selected resident batch, in place of first_read_id + index: for a batch whose reads are not consecutive records, such as
 * the pairs of a stretch of records that mixes pairs and unpaired reads.  The splice-site database's visibility window is measured against them (temporary splice
 * sites).  ids: [n]; NULL clears them; h2g_set_reads clears them too. */
H2G_EXPORT h2g_status h2g_set_read_ids(h2g_stream*, const uint32_t* ids);
/* ... and for a SAM handle of include/h2g_sam.h (the list of declarations of that header is pinned by tests/test_abi.py, so they stand here, as h2g_sam_set_n_ceil does).
 * The ids the format calls tag collected junctions with (h2g_sam_collect_novel_sites) and test the database's window against, in place of first_read_id + index
 * (ids: [n_reads] of the caller, not copied; NULL switches back): */
H2G_EXPORT void       h2g_sam_set_read_ids(struct h2g_sam*, const uint64_t* ids);
/* --qc-filter: the bytes given to h2g_set_read_filter for the batch about to be formatted (not copied: they must stay valid through the format call;
 * NULL = that set passes as a whole).  A read with a zero byte is printed unaligned with YF:Z:QC, after YF:Z:LN and YF:Z:NS in precedence
 * (aligner_result.cpp:1266-1279); the summary counts it as aligned 0 times.  pass2 is read by the paired format calls only. */
H2G_EXPORT void       h2g_sam_set_read_filter(struct h2g_sam*, const uint8_t* pass1, const uint8_t* pass2);
/* Where each read's / pair's text ends: the format calls that deliver their text also write, for read (pair) i of the call, the offset in `out` just
 * past its last line into ends[i] (ends: [n_reads] of the caller, not copied: the array is written during the format call, by its threads; NULL switches it off).  A read without a line (--no-unal) ends where
 * the one before it does.  For callers that interleave the text of several calls or sort reads by the flags of their lines. */
H2G_EXPORT void       h2g_sam_set_record_ends(struct h2g_sam*, uint64_t* ends);
/* read names (needed by genRandSeed): name i = bytes[offs[i] .. offs[i+1]) */
H2G_EXPORT h2g_status h2g_set_read_names(h2g_stream*, const char* bytes, const uint32_t* offs, size_t n_reads);
/* ---- -F <len>,<step>: reads sampled from long FASTA sequences (FastaContinuousPatternSource, pat.h:1214-1354) ------------------------------
 * Every <len>-base window, <step> bases apart, of a FASTA record is a read; its name is the record's name up to the first blank, '_', and the
 * decimal offset of the window's first base (bases only are counted); qualities are 'I'.  A window set is len / step times larger than the text
 * it is cut from, so it travels as that text plus a list of segments and is expanded on the device (h2g_set_reads_windows).
 * A segment is a run of windows of one record: window j of it starts at text[text_start + j * step], prints the offset name_off0 + j * step behind
 * the prefix prefixes[prefix_start .. prefix_start + prefix_len) (the record's name and '_'; empty for text before the first '>') and has
 * Read::rdid = rdid0 + j * step. */
typedef struct {
	uint64_t text_start;       /* index of window 0's first base in the text */
	uint64_t name_off0;        /* the offset window 0 prints */
	uint64_t rdid0;            /* Read::rdid of window 0 (the device keeps 32 bits, as h2g_set_read_ids) */
	uint32_t n_windows;
	uint32_t prefix_start, prefix_len;
	uint32_t pad;
} h2g_window_seg;
/* The planner (csrc/h2g_windows.cpp: host only, needs no device): the bytes of FASTA files, in order -> the text (one code 0..4 per counted base:
 * asc2dnacat != 0, IUPAC letters become N = 4, every other character is skipped without advancing the offset), the prefix pool and the
 * segments.  The window state restarts at every '>' and at every file; the id counter (rdid of a record's window 0: it grows by L - len + 1
 * after a record of L >= len bases; a shorter record yields no read) is carried across files, starting at first_rdid (0 for a run).  step == 0:
 * one window per record, at offset 0.  len: 1 .. 1024 (the reference's ring). */
typedef struct h2g_window_plan h2g_window_plan;
typedef struct { uint64_t n_reads, n_text, n_segs, n_prefix_bytes, next_rdid; uint32_t len, step; } h2g_window_plan_info;
H2G_EXPORT h2g_status h2g_window_plan_create(uint32_t len, uint32_t step, uint64_t first_rdid, h2g_window_plan** out);
H2G_EXPORT h2g_status h2g_window_plan_add_file(h2g_window_plan*, const char* bytes, size_t n);
H2G_EXPORT h2g_status h2g_window_plan_get_info(const h2g_window_plan*, h2g_window_plan_info* out);
H2G_EXPORT const uint8_t* h2g_window_plan_text(const h2g_window_plan*);        /* [n_text], valid until the next add_file / free */
H2G_EXPORT const char*    h2g_window_plan_prefixes(const h2g_window_plan*);    /* [n_prefix_bytes] */
/* The segments of the reads [first_read, first_read + n) (read = window, in input order; the range may begin and end inside a record) into
 * out[0..cap): returns how many there are (nothing is written past cap; out may be NULL to count). */
H2G_EXPORT size_t     h2g_window_plan_segments(const h2g_window_plan*, uint64_t first_read, uint64_t n, h2g_window_seg* out, size_t cap);
/* -s / -u act on Read::rdid (hisat2.cpp:3319, :3634): the reads with rdid_lo <= rdid < rdid_hi, up to the first read at or past rdid_hi. */
H2G_EXPORT void       h2g_window_plan_select(const h2g_window_plan*, uint64_t rdid_lo, uint64_t rdid_hi, uint64_t* first_read, uint64_t* n);
H2G_EXPORT void       h2g_window_plan_free(h2g_window_plan*);
/* For the selected resident batch, what h2g_set_reads + h2g_set_read_names + h2g_set_read_ids do with the expanded arrays and no qualities:
 * the reads are the windows of segs[0..n_segs) in order, each `len` bases.  Uploads text[lo, hi) (the range the segments touch), the segment
 * table and the prefixes; kernels write the batch's codes, offsets, names, name offsets and ids.  n_text / n_prefix_bytes bound what the
 * segments may name.  The reads must fit the stream's max_reads / max_bases; the names must fit 32-bit offsets. */
H2G_EXPORT h2g_status h2g_set_reads_windows(h2g_stream*, const uint8_t* text, size_t n_text, const h2g_window_seg* segs, size_t n_segs,
                                            uint32_t len, uint32_t step, const char* prefixes, size_t n_prefix_bytes);
/* bytes uploaded / HIP-event time of the expansion kernels of this stream's last h2g_set_reads_windows (measurement) */
typedef struct { uint64_t bytes_uploaded, bytes_written; float kernel_ms, pad; } h2g_windows_stats;
H2G_EXPORT h2g_status h2g_get_windows_stats(h2g_stream*, h2g_windows_stats* out);
/* Debug read-back of the selected resident batch as the device holds it: codes [offs[n]], offs [n + 1], names [name_offs[n]], name_offs [n + 1],
 * ids [n] (a batch without explicit ids: H2G_ERR_ARG when ids != NULL).  The four counts are always set, so a first call with NULL arrays
 * sizes the second; any pointer may be NULL. */
H2G_EXPORT h2g_status h2g_fetch_reads(h2g_stream*, size_t* n_reads, size_t* n_bases, size_t* n_name_bytes, int* has_ids,
                                      uint8_t* codes, uint32_t* offs, char* names, uint32_t* name_offs, uint32_t* ids);
/* ---- FASTQ records parsed on the device (opt-in) ------------------------------------------------------------------------
 * For the selected resident batch, what h2g_set_reads + h2g_set_read_names (+ h2g_set_mates with text2) do with the arrays a host parser makes of the same bytes
 * (FastqPatternSource, pat.cpp:725-1010): the texts are uploaded into the stream's temporary device memory and kernels write the batch's codes, qualities, names and offsets.
 * text1 (and text2) begin at a record start; records are four lines, cut at every fourth '\n'.  final1 / final2: that text ends its input, so a last line without '\n'
 * is complete (else the record it belongs to stays unconsumed).  n_records = min(records of text1, records of text2, max_records; max_records == 0: no bound) are parsed,
 * and consumed1 / consumed2 are the bytes of each text they occupy.  trim5 / trim3 / phred64: -5 / -3 / --phred64.
 * The device parses PLAIN records only (csrc/h2g_fastq.h states the predicate: a non-empty name, a sequence line of '.' and letters only, a '+' line, Lraw or Lraw + 1
 * qualities without a blank, under phred64 every kept quality in [64, 128)).  When any of the n records is not plain the call returns H2G_OK with n_not_plain > 0 and
 * first_not_plain, and the batch is left EMPTY (n_reads == 0): the caller parses those bytes itself.  With all of them plain first_not_plain == n_records, the batch holds
 * them (qualities, names, mates set; seeds, filter and ids cleared) and h2g_align(_pairs)_run, the fetches and h2g_sam_text_* work on it unchanged.
 * H2G_ERR_ARG (h2g_last_error), with the counts in *out where they are known and the batch empty: a text of 2^32 bytes or more; more records or bases than the stream's
 * max_reads / max_bases; name bytes past 32-bit offsets.  Synchronises as h2g_set_reads does. */
typedef struct { uint32_t trim5, trim3; uint8_t phred64, final1, final2, pad; uint64_t max_records; } h2g_fastq_opts;
typedef struct { uint64_t n_records, consumed1, consumed2, n_bases1, n_bases2, n_name_bytes1, n_name_bytes2, n_not_plain, first_not_plain; uint32_t max_read_len, pad; } h2g_fastq_result;
H2G_EXPORT h2g_status h2g_set_reads_fastq(h2g_stream*, const char* text1, size_t n1, const char* text2 /* NULL: unpaired */, size_t n2, const h2g_fastq_opts*, h2g_fastq_result* out);
/* Read-back of one mate (0: the reads of h2g_set_reads, 1: of h2g_set_mates) of the selected resident batch, qualities included.  The three counts are always set, so a
 * first call with NULL arrays sizes the second; any pointer may be NULL.  H2G_ERR_ARG: mate 1 of a batch without mates, quals of a set without qualities, names of a
 * set without names. */
H2G_EXPORT h2g_status h2g_fetch_read_set(h2g_stream*, int mate, size_t* n_reads, size_t* n_bases, size_t* n_name_bytes, uint8_t* codes, uint32_t* offs, char* quals, char* names,
                                         uint32_t* name_offs);
/* bytes uploaded / written and HIP-event time of the kernels of this stream's last h2g_set_reads_fastq (measurement) */
typedef struct { uint64_t bytes_uploaded, bytes_written; float kernel_ms, pad; } h2g_fastq_stats;
H2G_EXPORT h2g_status h2g_get_fastq_stats(h2g_stream*, h2g_fastq_stats* out);
/* GenomeHit::combineWith (hi_aligner.h:1420-2025) as a primitive of its own: a[i] (the left hit) absorbs b[i] — concatenation, the mismatch rescan of the joint,
 * an insertion or deletion, or (spliced alignment) an intron placed by the donor / acceptor scan — over the resident reads; ok[i] = the function's return value.  `p` carries
 * scoring and splice policy (NULL: h2g_align_params_init's defaults for this index).  Inside go() the same device function runs as OP_COMBINE. */
H2G_EXPORT h2g_status h2g_combine_with(h2g_stream*, const h2g_align_params* p, h2g_ghit* a /* in/out */, const h2g_ghit* b, const int64_t* minsc, size_t n, uint32_t* ok);
H2G_EXPORT h2g_status h2g_align_run(h2g_stream*, const h2g_align_params*);           /* async on the stream */
H2G_EXPORT h2g_status h2g_align_fetch(h2g_stream*, h2g_read_result* res /* [n] */, h2g_alnres* aln /* [n*H2G_ALN_CAP] or NULL */,
                                      size_t first_read, size_t n_reads);

/* Dense variant for callers that move the results over PCIe: only the nselect printed alignments of every read, back to back
 * (gathered on the device); read i's records are aln[aln_offs[i] .. aln_offs[i+1]).  H2G_ERR_ARG if aln_cap is too small
 * (aln_offs[n] then holds the count needed). */
H2G_EXPORT h2g_status h2g_align_fetch_dense(h2g_stream*, h2g_read_result* res /* [n] */, h2g_alnres* aln, size_t aln_cap,
                                            uint64_t* aln_offs /* [n+1] */, size_t first_read, size_t n_reads);

/* ---- paired-end: HI_Aligner::go with both mates (initReads hi_aligner.h:4019; pairReads :5948; alignMate :5579) -- */
/* Mate 2 of every read of the batch (same count as h2g_set_reads); names2 feed genRandSeed of mate 2. */
H2G_EXPORT h2g_status h2g_set_mates(h2g_stream*, const uint8_t* codes2, const uint32_t* offs2, const char* quals2,
                                    const char* name_bytes2, const uint32_t* name_offs2, size_t n_reads);
#define H2G_PAIR_RES_CAP 16       /* unpaired alignments returned per mate */
#define H2G_PAIR_CAP 32           /* concordant pairs returned per read pair (pair_i / pair_j); npairs is the true count */
/* The range of -k / --max-seeds h2g_align_run and h2g_align_pairs_run accept.  A run with khits > 32 or max(khits, kseeds) > 64 runs on the
 * extra-large units, whole (no fast pass, no second pass): a pair there may have more concordant pairings than H2G_PAIR_CAP, or name a record past
 * index 255 of a mate's list.  Such a pair's whole list reaches a caller only through h2g_align_pairs_fetch_compact, as a trailer behind mate 1's
 * records: a record prefix (40 bytes) with nedits == H2G_PAIR_TRAILER_TAG — no record carries it — and tidx = the number of pairs, then one uint32_t
 * per pair in report order, mate-1 index | mate-2 index << 16, the whole rounded up to 8 bytes (H2G_PAIR_TRAILER_BYTES).  It is the last entry of
 * the pair's mate-1 bytes; the list replaces npairs / pair_i / pair_j.  h2g_align_pairs_fetch and h2g_align_pairs_fetch_dense cannot carry such a
 * pair: they return the first H2G_PAIR_CAP pairings truncated to 8 bits and set overflow bit H2G_OVF_PAIR_LIST. */
#define H2G_KHITS_MAX 128
#define H2G_KSEEDS_MAX 256
#define H2G_PAIR_TRAILER_TAG 0x52494150u   /* "PAIR" */
#define H2G_PAIR_TRAILER_BYTES(npairs) ((40u + 4u * (uint32_t)(npairs) + 7u) & ~7u)
#define H2G_OVF_PAIR_LIST 4096u
typedef struct {
	uint32_t nres[2];              /* sink.report(mate) events per mate, in report order (rs1u_/rs2u_) */
	uint32_t npairs;               /* sink.report(r1, r2) events, in report order (rs1_/rs2_) */
	uint32_t overflow, nrank, nsteps, depth, nside;
	uint32_t rnd_state;            /* RandomSource::last after go(): the sink's selectByScore continues from it */
	uint32_t pad;                  /* device-side: != 0 when the pair's records live in the stream's growable area (a mate with more reports than its
	                                * fixed rows); h2g_align_pairs_fetch_dense returns all of them, h2g_align_pairs_fetch sets overflow bit 4 for such a pair */
	uint8_t  pair_i[H2G_PAIR_CAP], pair_j[H2G_PAIR_CAP];   /* indexes into the two per-mate lists */
} h2g_pair_result;
/* The concordant / discordant / unpaired decision, -k selection, MAPQ and SAM stay in the caller's AlnSinkWrap
 * (aln_sink.h:1939): it replays these events through msinkwrap.report() and calls finishRead(). */
H2G_EXPORT h2g_status h2g_align_pairs_run(h2g_stream*, const h2g_align_params*);
H2G_EXPORT h2g_status h2g_align_pairs_fetch(h2g_stream*, h2g_pair_result* res /* [n] */, h2g_alnres* aln1 /* [n*H2G_PAIR_RES_CAP] */,
                                            h2g_alnres* aln2 /* [n*H2G_PAIR_RES_CAP] */, size_t first_read, size_t n_reads);

/* Dense variant: the nres[m] report events of each mate back to back (see h2g_align_fetch_dense) */
H2G_EXPORT h2g_status h2g_align_pairs_fetch_dense(h2g_stream*, h2g_pair_result* res /* [n] */, h2g_alnres* aln1, size_t cap1, uint64_t* aln_offs1 /* [n+1] */,
                                                  h2g_alnres* aln2, size_t cap2, uint64_t* aln_offs2 /* [n+1] */, size_t first_read, size_t n_reads);

/* Compact variants — what a caller on the other side of PCIe wants: sized, scanned and gathered on the device in one go.  A record travels as its 40 bytes
 * of fields + 12 bytes per edit it holds (a record beyond H2G_MAX_EDITS: its one marker entry), rounded up to 8: read i's records lie back to back in
 * rec[boffs[i] .. boffs[i + 1]) (byte offsets).  A compact record is a PREFIX of an h2g_alnres: read it through a `const h2g_alnres*` up to edits[nedits), never
 * copy the struct; the next record starts H2G_COMPACT_BYTES(nedits) further.  H2G_ERR_ARG when a capacity is too small (boffs[n] then holds the bytes needed).
 * include/h2g_sam.h formats this layout directly (h2g_sam_format_*_compact). */
#define H2G_COMPACT_BYTES(nedits) ((40u + 12u * ((nedits) > H2G_MAX_EDITS ? 1u : (uint32_t)(nedits)) + 7u) & ~7u)
H2G_EXPORT h2g_status h2g_align_fetch_compact(h2g_stream*, h2g_read_result* res /* [n] */, uint8_t* rec, size_t cap, uint64_t* boffs /* [n+1] */, size_t first_read, size_t n_reads);
H2G_EXPORT h2g_status h2g_align_pairs_fetch_compact(h2g_stream*, h2g_pair_result* res /* [n] */, uint8_t* rec1, size_t cap1, uint64_t* boffs1 /* [n+1] */,
                                                    uint8_t* rec2, size_t cap2, uint64_t* boffs2 /* [n+1] */, size_t first_read, size_t n_reads);
/* Page-locked host memory for the buffers handed to h2g_set_* / h2g_*_fetch_*: copies from / to it run at the link's rate (pageable memory is staged by the
 * runtime at a fraction of it).  NULL when the allocation fails. */
H2G_EXPORT void*      h2g_host_alloc(size_t bytes);
H2G_EXPORT void       h2g_host_free(void*);

/* Records beyond H2G_MAX_EDITS edits.  The reference's edit lists are unbounded (hi_aligner.h:421, reportHit :6129-6166) and a deletion of n bases
 * is n edits (edit.h).  A record whose list does not fit its H2G_MAX_EDITS inline entries says so with nedits > H2G_MAX_EDITS: its edits live in the
 * stream's long-edit area, at offset edits[0].pos (edits[0].snp == 0x4c4f4e47 marks it; the other inline entries are unspecified).  This call returns
 * the used prefix of that area for the resident batch: *n = edits it spans (0 when the batch has no such record); H2G_ERR_ARG with *n set when cap is
 * smaller.  include/h2g_sam.h: h2g_sam_set_long_edits hands it to the formatter.  Capacity of the working lists: 192 edits per alignment (the units with
 * the large workspace, which the flagged reads of the default units are re-run by); beyond that a read keeps overflow bit 1. */
H2G_EXPORT h2g_status h2g_align_fetch_long_edits(h2g_stream*, h2g_edit* out, size_t cap, size_t* n);

/* ---- SAM text written on the device from a host-made line plan (opt-in) -------------------------------------------------
 * The format calls of include/h2g_sam.h decide what to print (pairing, selection, MAPQ, TLEN, filters) and write the bytes.  Here the two halves are
 * separate calls: h2g_sam_plan_*_compact runs the same decisions over the same arguments and returns one 64-byte descriptor per line instead of text;
 * h2g_sam_text_* turns descriptors into text on the device, from the reads, qualities and names of the selected resident batch and the compact
 * records still lying in the stream's buffers after the fetch.  (These stand here because tests/test_abi.py pins the declaration list of h2g_sam.h.)
 * A descriptor carries what the line takes from the decisions; POS, strand, AS:i, YS:i, RNEXT / PNEXT, trims and edits are read from the records.
 * A line whose record has mismatch edits only, and an unaligned line, needs nothing else: CIGAR and MD:Z follow from trims and mismatch positions.  The CIGAR
 * and the MD:Z value of a line with gaps or introns are written by the host (one copy of the left-alignment) into the `aux` byte pool, and so is a Zs:Z
 * value (it needs the ALT names).  WHOLE_LINE: the pool holds the complete line; only for records beyond H2G_MAX_EDITS, whose edits are not inline. */
enum { H2G_SAM_LINE_HAS_ZS = 1, H2G_SAM_LINE_HAS_YS = 2, H2G_SAM_LINE_HAS_TLEN = 4, H2G_SAM_LINE_STAR_SEQ = 8 /* --omit-sec-seq secondary or empty read */,
       H2G_SAM_LINE_STRIP_MATE_SUFFIX = 16 /* part of a pair: a trailing /1 /2 /3 of the name goes */, H2G_SAM_LINE_AUX_CIGAR_MDZ = 32, H2G_SAM_LINE_WHOLE_LINE = 64,
       H2G_SAM_LINE_SENSE_MATE1 = 128 /* XS:A of a stranded library reads the line as mate 1 */ };
typedef struct {
	uint32_t read, nh;             /* read / pair of the call (relative to `first` of the fetch for the text calls); NH:i */
	uint64_t rec_off, orec_off;    /* byte offset of this line's record in its mate's compact bytes / of the opposite mate's record in the other mate's bytes;
	                                * ~0 = none (unaligned line / no opposite) */
	int64_t  tlen;
	int32_t  zs, oref_tidx;        /* ZS:i value; reference of the aligned mate for an unaligned line, -1 = none */
	uint32_t oref_toff, aux_off, aux_len;
	uint16_t flag, cigar_len, mdz_len;   /* SAM FLAG; aux holds CIGAR, MD:Z value, then the Zs:Z value (aux_len - cigar_len - mdz_len bytes), back to back */
	uint8_t  mapq, mate, yt, yf;         /* mate: 0 = the reads of h2g_set_reads, 1 = of h2g_set_mates; yt: 0 UU 1 CP 2 DP 3 UP; yf: 0 none 1 LN 2 NS 3 QC */
	uint16_t bits;                       /* H2G_SAM_LINE_* */
} h2g_sam_line;
/* The planner (host only).  Arguments as h2g_sam_format_{unpaired,paired}_compact up to `khits`; side effects on the handle exactly those of the format call
 * (summary counters, collected novel sites; first_read_id / read ids / filters / long edits honoured), so a caller can swap one for the other.  lines[0 .. *n_lines)
 * in output order, aux[0 .. *aux_used); line_ends ([n] or NULL): lines emitted up to and including read / pair i (--no-unal lines are not planned).  A capacity that is
 * too small: H2G_ERR_ARG with *n_lines / *aux_used = what is needed, and nothing counted into the handle. */
H2G_EXPORT h2g_status h2g_sam_plan_unpaired_compact(const struct h2g_sam*, const uint8_t* codes, const uint32_t* offs, const char* quals, const char* name_bytes,
                                                    const uint32_t* name_offs, size_t n_reads, const h2g_read_result* res, const uint8_t* rec, const uint64_t* boffs,
                                                    h2g_sam_line* lines, size_t line_cap, size_t* n_lines, char* aux, size_t aux_cap, size_t* aux_used, uint64_t* line_ends);
H2G_EXPORT h2g_status h2g_sam_plan_paired_compact(const struct h2g_sam*, const uint8_t* codes1, const uint32_t* offs1, const char* quals1, const char* name_bytes1,
                                                  const uint32_t* name_offs1, const uint8_t* codes2, const uint32_t* offs2, const char* quals2, const char* name_bytes2,
                                                  const uint32_t* name_offs2, size_t n_reads, const h2g_pair_result* res, const uint8_t* rec1, const uint64_t* boffs1,
                                                  const uint8_t* rec2, const uint64_t* boffs2, uint32_t khits,
                                                  h2g_sam_line* lines, size_t line_cap, size_t* n_lines, char* aux, size_t aux_cap, size_t* aux_used, uint64_t* line_ends);
/* The text of lines[0 .. n_lines) on the device: from the selected resident batch (h2g_set_reads / h2g_set_mates / h2g_set_read_names or h2g_set_reads_windows; a batch
 * without qualities prints 'I') and the compact bytes of this stream's last h2g_align_fetch_compact (unpaired) / h2g_align_pairs_fetch_compact (paired) of (first, n):
 * lines[].read counts from that `first`.  The stream remembers whether its buffers still hold that fetch: any call since that reuses them (another fetch, a primitive),
 * selects another batch or sets reads, mates or names makes the text call return H2G_ERR_ARG (h2g_last_error says so) without launching anything.  Every descriptor is
 * checked before the write kernel runs (H2G_ERR_ARG): read < n, mate against the run kind, offsets 8-aligned and the record with its inline edits inside that mate's
 * bytes, pool ranges inside n_aux, reference indexes.  out[0 .. *used); cap too small: H2G_ERR_ARG with *used = the bytes needed, nothing written.  line_offs
 * ([n_lines + 1] or NULL): where each line starts in out, and *used last. */
H2G_EXPORT h2g_status h2g_sam_text_unpaired(h2g_stream*, const struct h2g_sam*, const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux,
                                            char* out, size_t cap, size_t* used, uint64_t* line_offs);
H2G_EXPORT h2g_status h2g_sam_text_paired(h2g_stream*, const struct h2g_sam*, const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux,
                                          char* out, size_t cap, size_t* used, uint64_t* line_offs);
/* The same emitter instantiated on the host (no device needed): host arrays in place of the stream — the read sets as given to the planner (set 2 NULL for an unpaired
 * plan) and the compact bytes with their byte counts.  Same checks, same results. */
H2G_EXPORT h2g_status h2g_sam_text_from_plan_host(const struct h2g_sam*, const uint8_t* codes1, const uint32_t* offs1, const char* quals1, const char* name_bytes1,
                                                  const uint32_t* name_offs1, const uint8_t* codes2, const uint32_t* offs2, const char* quals2, const char* name_bytes2,
                                                  const uint32_t* name_offs2, size_t n_reads, const uint8_t* rec1, size_t n_rec1, const uint8_t* rec2, size_t n_rec2,
                                                  const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux, char* out, size_t cap, size_t* used, uint64_t* line_offs);
/* HIP-event time of the kernels / bytes written by this stream's last h2g_sam_text_* call (measurement) */
typedef struct { uint64_t bytes_uploaded, bytes_written; float kernel_ms, write_kernel_ms; /* sizes + scan + write; the write kernel alone */ } h2g_sam_text_stats;
H2G_EXPORT h2g_status h2g_get_sam_text_stats(h2g_stream*, h2g_sam_text_stats* out);

/* ---- plain lines planned on the device, the rest by the host planner (opt-in) ---------------------------------------------
 * Most reads are PLAIN: nothing aligned, or one alignment (one concordant pairing of two) whose edits are mismatches only.  Their descriptors are closed-form functions of
 * the result header and one or two records, and the device holds all of that after a compact fetch.  These calls classify every read / pair of the fetch on the device
 * (csrc/h2g_sam_plan.h states the predicate), plan the plain ones there, run the host planner over the HANDED-ON rest only, merge the two in read order on the device and
 * write the text as h2g_sam_text_* does.  The bytes are those of h2g_sam_format_*_compact; the side effects on the handle too (summary counters, collected novel sites),
 * counted once the text is delivered.
 * Arguments: those of h2g_sam_plan_*_compact up to `khits` — the host read sets and the host copy of the fetch, for the handed-on reads — then out / cap / used as the text
 * calls take them; line_offs ([line_cap + 1] or NULL) and *n_lines (NULL allowed without line_offs): where each line starts; line_ends ([n_reads] or NULL): lines emitted
 * up to and including read i.  H2G_ERR_ARG without a launch when the stream's buffers do not hold that fetch any more or the fetch is of the other kind; H2G_ERR_ARG with
 * *used (and *n_lines) = what is needed when cap (line_cap) is too small.  On any refusal nothing is written and nothing is counted into the handle. */
H2G_EXPORT h2g_status h2g_sam_text_unpaired_planned(h2g_stream*, const struct h2g_sam*, const uint8_t* codes, const uint32_t* offs, const char* quals, const char* name_bytes,
                                                    const uint32_t* name_offs, size_t n_reads, const h2g_read_result* res, const uint8_t* rec, const uint64_t* boffs,
                                                    char* out, size_t cap, size_t* used, uint64_t* line_offs, size_t line_cap, size_t* n_lines, uint64_t* line_ends);
H2G_EXPORT h2g_status h2g_sam_text_paired_planned(h2g_stream*, const struct h2g_sam*, const uint8_t* codes1, const uint32_t* offs1, const char* quals1, const char* name_bytes1,
                                                  const uint32_t* name_offs1, const uint8_t* codes2, const uint32_t* offs2, const char* quals2, const char* name_bytes2,
                                                  const uint32_t* name_offs2, size_t n_reads, const h2g_pair_result* res, const uint8_t* rec1, const uint64_t* boffs1,
                                                  const uint8_t* rec2, const uint64_t* boffs2, uint32_t khits,
                                                  char* out, size_t cap, size_t* used, uint64_t* line_offs, size_t line_cap, size_t* n_lines, uint64_t* line_ends);
/* Of this stream's last h2g_sam_text_*_planned call: reads / pairs planned on the device and by the host, lines, bytes uploaded for the merge (descriptors, pool, per-read
 * entries of the handed-on reads), HIP-event time of the planner + merge kernels, wall time of the host planner over its subset.  classes ([cap] or NULL): the class byte
 * of each read of that call, 0 = handed on (csrc/h2g_sam_plan.h); H2G_ERR_ARG when cap is smaller than the call's reads. */
typedef struct { uint64_t device_planned, host_planned, n_lines, bytes_uploaded, whole_lines /* lines that travelled as text: records beyond H2G_MAX_EDITS, all handed on */;
                 float plan_kernel_ms, host_plan_ms; } h2g_sam_plan_stats;
H2G_EXPORT h2g_status h2g_get_sam_plan_stats(h2g_stream*, h2g_sam_plan_stats* out, uint8_t* classes, size_t cap);
/* The same split with host arrays only (no device): classification and the plain planner instantiated on the host, the host planner over the handed-on reads, the merge.
 * Arguments and results as h2g_sam_plan_paired_compact (set 2, rec2 and boffs2 NULL: an unpaired run, res = h2g_read_result[n]; else h2g_pair_result[n]); lines, aux and
 * line_ends equal that call's byte for byte, and so do the side effects on the handle.  classes ([n_reads] or NULL) as above. */
H2G_EXPORT h2g_status h2g_sam_plan_split_host(const struct h2g_sam*, const uint8_t* codes1, const uint32_t* offs1, const char* quals1, const char* name_bytes1,
                                              const uint32_t* name_offs1, const uint8_t* codes2, const uint32_t* offs2, const char* quals2, const char* name_bytes2,
                                              const uint32_t* name_offs2, size_t n_reads, const void* res, const uint8_t* rec1, const uint64_t* boffs1,
                                              const uint8_t* rec2, const uint64_t* boffs2, uint32_t khits,
                                              h2g_sam_line* lines, size_t line_cap, size_t* n_lines, char* aux, size_t aux_cap, size_t* aux_used, uint64_t* line_ends, uint8_t* classes);

/* ---- counters (roofline numerators) ------------------------------------------------- */
typedef struct {
	uint64_t n_rank, n_side, n_sa_steps, n_ext, n_ref_bytes, n_queries, n_aligned, n_overflow;
	float    ms_search, ms_resolve_extend, ms_rank, ms_align;   /* HIP-event durations of the last launches */
	float    ms_align_kernel;                                   /* the main go() pass alone (ms_align includes the second pass) */
	uint64_t n_second_pass;                                     /* reads whose default workspace overflowed and that were re-run with the
	                                                             * large one; n_overflow = reads still flagged after that */
	uint64_t n_fast, n_fast_bail;                               /* reads / pairs completed by the fast pass; handed on to the general machine */
	float    ms_fast_kernel, pad_;                              /* the fast pass alone (ms_align covers every pass) */
	uint64_t n_fast_side, n_fast_sa_steps;                      /* sides / SA-walk steps of the fast pass alone (n_side, n_sa_steps cover every pass) */
	float    ms_drain_kernel, pad2_;                            /* the drain launch of the fast pass: the reads its workgroups still held when the batch was exhausted ... */
	uint64_t n_drain_side, n_drain_sa_steps, n_adopted;         /* ... its sides / SA-walk steps (NOT in n_fast_side / n_fast_sa_steps) and how many reads it took up */
} h2g_counters;
H2G_EXPORT h2g_status h2g_get_counters(h2g_stream*, h2g_counters*);

#ifdef __cplusplus
}
#endif
#endif /* H2G_H_ */
