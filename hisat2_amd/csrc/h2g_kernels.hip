// h2g_kernels.hip — gfx950 kernels and the C ABI of libh2g.so (include/h2g.h).
//
// Integer / byte work bound by random 64 B HBM reads: no MFMA anywhere.  Launch geometry: 256-thread
// workgroups (4 waves of 64), grids of >= 8 blocks per CU x 256 CUs so all 8 XCDs stay busy; sides are
// read with 16 B-per-lane vector loads so one side = one 64 B request.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <memory>
#include <chrono>
#include <algorithm>
#define H2G_EXT_OPTS 0      // likewise -I / --fr --rf --ff / --nofw --norc (h2g_align.h): go() units only
#define H2G_HAPLOTYPE 0     // the primitive kernels of this unit (k_extend_alts, k_adjust_alt) run without haplotype lists; go() units: h2g_graph.h
#include "h2g_core.h"
#include "h2g_dev.h"     // DevBuf / PinnedBuf / DevEvent / DevStream: who holds one owns it
#include "h2g_parts.h"   // PartArea: a device area in equal parts, one per lane
#include "h2g_host_index.h"
#include "h2g_align.h"
#include "h2g_graph.h"
#include "h2g_sw.h"
#include "h2g_graph_staged.h"
#include "h2g_local_pack.h"
#include "h2g_splice_host.h"
#include "h2g_splice_db_host.h"
#include "h2g_windows.h"   // the -F window expansion's per-read arithmetic
#include "h2g_fastq.h"     // the record arithmetic of FASTQ parsing on the device
#include "h2g_sam_line.h"  // the SAM line emitter the text kernels and the host share
#include "h2g_sam_plan.h"  // the planner of plain SAM lines the kernels and the host share
#include <chrono>
#include "h2g_go_args.h"   // GoArgs + the extern "C" face of the go() units (their AlignWS layouts are opaque on this side)

using namespace h2g;

// ------------------------------------------------------------------------------------------ error plumbing
static thread_local char g_err[512] = "";
static int set_err(const char* what, hipError_t e) {
	snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
	return H2G_ERR_DEVICE;
}
#define HIPCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) return set_err(#call, e_); } while(0)

extern "C" const char* h2g_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------ handles
// Ownership (h2g_dev.h): a stream is declared before every buffer and event, so it is destroyed after them; the destructor waits for it first.
struct h2g_index {
	DevStream dense_st;                                    // the dense tables' builds (lowest priority)
	HostIndex host;
	bool synthetic = false;
	int device = 0;
	DGfm dg;
	DRef dr;
	DLocalSet dls;
	DAlts dalts;
	bool has_local = false;
	uint32_t n_local = 0;                                  // local indexes loaded (their per-index host objects are not kept: load_local_pack)
	bool has_splice_alts = false;                         // the ALT list holds splice sites / exons (a _tran index)
	std::vector<h2g_splice_site> alt_sites;               // splice-site ALTs of a --ss index: part of every database (SpliceSiteDB::read(gfm, alts))
	DSpliceDB dssdb;                                       // h2g_index_set_splice_sites (device arrays; freed and replaced on every call)
	DExonTbl dexons;                                       // the exons of a --ss/--exon index (--avoid-pseudogene); n == 0 without
	DevBuf<uint8_t> d_ssdb[4];                             // (they grow by doubling: temporary splice sites arrive wave after wave)
	HostSpliceDB h_ssdb;                                   // the host copy h2g_index_add_splice_sites merges into
	const float* d_spl[3] = {nullptr, nullptr, nullptr};   // SpliceSiteDB::probscore tables (donor, acceptor halves), uploaded with the index
	std::vector<DLocalDesc> h_ldesc;   // host copy of the local-index descriptors (bucketing of h2g_ext_search)
	std::vector<DevBuf<uint8_t>> allocs;                   // every array of the index; dg, dr, dls, dalts, d_spl and the dense tables' pointers below are views of them
	uint64_t device_bytes = 0;
	// the dense SA table of a linear index (h2g_core.h sa_resolve_row): built by k_sa_dense_build on a stream of the index's own behind the uploads.
	// `dg` never carries its pointers: a run takes them through dg_now(), which hands them out once the build is over (dense_ready)
	uint32_t* d_sa_dense = nullptr; uint8_t* d_sa_dist = nullptr;   // (views: `allocs` owns them)
	DevEvent dense_ev;
	std::atomic<bool> dense_ready{false};
	double dense_ms = 0.0;                                 // (H2G_DENSE_SA=2: the build, timed on the host)
	bool dense_synced = false;                             // the uploads are known to be over (one device-wide wait, before the first build is queued)
	// the dense table of the local rows (h2g_align.h lsa_resolve_row): built by k_lsa_dense_build behind the global table's build on dense_st, with an
	// event of its own.  `dls` never carries its pointers: dls_now()
	uint32_t* d_lsa = nullptr; uint64_t* d_lsa_base = nullptr;      // (views: `allocs` owns them)
	uint64_t lsa_rows = 0;
	DevEvent lsa_ev;
	std::atomic<bool> lsa_ready{false};
	double lsa_ms = 0.0;                                   // (H2G_DENSE_LSA=2: the build, timed on the host)
	~h2g_index() { if(dense_st) { (void)hipSetDevice(device); (void)hipStreamSynchronize(dense_st); } }
};
struct IndexFree { void operator()(h2g_index* ix) const { h2g_index_free(ix); } };
typedef std::unique_ptr<h2g_index, IndexFree> IndexPtr;
// the index's DGfm as a run queued now may use it: with the dense SA table from the moment its build is over (polled, never waited for)
static DGfm dg_now(h2g_index* ix) {
	DGfm g = ix->dg;
	if(!ix->d_sa_dist) return g;
	if(!ix->dense_ready.load(std::memory_order_acquire)) {
		if(hipEventQuery(ix->dense_ev) != hipSuccess) { (void)hipGetLastError(); return g; }
		ix->dense_ready.store(true, std::memory_order_release);
	}
	g.sa_dense = ix->d_sa_dense; g.sa_dist = ix->d_sa_dist;
	return g;
}

// ... and its DLocalSet: with the dense table of the local rows from the moment that table's own build is over
static DLocalSet dls_now(h2g_index* ix) {
	DLocalSet l = ix->dls;
	if(!ix->d_lsa) return l;
	if(!ix->lsa_ready.load(std::memory_order_acquire)) {
		if(hipEventQuery(ix->lsa_ev) != hipSuccess) { (void)hipGetLastError(); return l; }
		ix->lsa_ready.store(true, std::memory_order_release);
	}
	l.lsa = ix->d_lsa; l.lsa_base = ix->d_lsa_base;
	return l;
}

// The general machine's pass over run k's hand-ons is a LATENCY CHAIN: its length is its longest reads' (hundreds of dependent trips of
// 60-100 us on a 115 KB workspace), not their number — 30 ms behind a 14.5 ms fast pass on the random GRCh38-size genome, 118 ms behind a 25 ms
// fast pass on repeat-structured sequence (profiles/r04_NOTES.md §4-§6).  The stream therefore keeps such passes in flight next to the fast passes of
// the following runs.  Two numbers describe that, and they are not the same thing (profiles/r08_mstreams.md):
//   LANES (M, H2G_MSTREAMS_MAX unless pinned): run k is lane k % M.  Everything that OUTLIVES a pass rotates by lane — the parts of the pair-overflow,
//     long-edit and XL areas (PartArea) and their cursors, ledits_touched, and the per-run buffer sets (h2g_stream::RunSet: events, hand-on list, counters, argument blocks), M + 1 deep.  This is
//     the caller's contract (fetch a batch before M further runs are queued) and does not follow the load.
//   MACHINE STREAMS IN ROTATION (S <= M): lane m's pass runs on HIP stream mst[m % S] with that stream's workspace pools and overflow list (h2g_stream::MachStream), which a pass
//     only needs while it runs (passes on one HIP stream are in order).  HIP streams share the few hardware queues of a process and serialise there, so S
//     follows the load (mstreams_policy): H2G_MSTREAMS_LIGHT_DEFAULT while a linear index's fast pass hands on little — the passes are short and two in
//     flight cover them — and H2G_MSTREAMS_MAX once it hands on more than 1.5 % of the batch, or on a graph index.
// H2G_MSTREAMS / h2g_stream_tune "mstreams" pins both to one value (M = S); H2G_MSTREAMS_LIGHT / "mstreams_light" sets the light S.  A caller sees no
// difference: results are complete when a fetch / sync returns.
#define H2G_MSTREAMS_MAX 8
#define H2G_MSTREAMS_LIGHT_DEFAULT 2
#define H2G_NBUF (H2G_MSTREAMS_MAX + 1)
// CUs the fast pass's persistent grid leaves free for the machine passes: -1 = as many as M passes may hold; 0 = none — the fast pass asks for every
// CU and the hardware dispatcher places machine workgroups as CUs come free (the fast pass draws its reads from one counter, so a late workgroup costs nothing)
#define H2G_FAST_RESERVE_DEFAULT 0
// the fast pass's two scheduling choices for PAIRED batches on a linear index (measured at GRCh38 size: profiles/r04_NOTES.md §4): reads a
// workgroup hands on at the tail of an exhausted batch, and whether alignMate runs inside the pass (k_go_fast_am) or in the machine's pass
#define H2G_DEFAULT_TAIL 16
// The end of a batch (h2g_k_go_fast.hip, fk_loop): workgroups of a fast launch that can fetch no more and hold at most H2G_ORPHAN_T reads list them and leave; the drain launch
// (H2G_DRAIN_GRID workgroups on the stream's drain stream; the machine's pass waits for it) finishes them next to the following run's fast launch.  Drain launches run one after
// the other, so one has to be shorter than a step: 64 workgroups (lease Q: with 32 and the alignMate pairs in it the drain launch, 10 ms, became the step).  Batches below
// H2G_ORPHAN_MIN_UNITS keep the single launch (h2g_stream_tune "orphan": -1 this policy, 0 off, n the threshold; "drain_grid"; "mate_handover").
#define H2G_ORPHAN_T 512
#define H2G_ORPHAN_MIN_UNITS 200000
#define H2G_DRAIN_GRID 64
#define H2G_FAST_POOLS 3
// The first partial searches of the fast pass in a pre-pass kernel (h2g_k_ps0.hip): 1 = on for the linear non-spliced builds (9.40 -> 8.98 ms per step,
// profiles/ps0_ab.md); H2G_FAST_PS0=0 / h2g_stream_tune "ps0" is the code path of before
#ifndef H2G_DEFAULT_PS0
#define H2G_DEFAULT_PS0 1
#endif
#define H2G_DEFAULT_ALIGN_MATE 0
// the fast pass of SPLICED runs on a linear index (h2g_k_go_fast_spl.hip; env H2G_FAST_SPLICED, h2g_stream_tune "fast_spliced").  OFF by default: 1 M pairs drawn from a spliced transcript
// model (36 % with a junction) take 225 ms per run with it and 70 ms with the machine alone — version 1 hands 44 % of the pairs on, and a machine pass behind a fast pass has at most
// H2G_MACH_MAXGRID workgroups where the machine alone has the chip (profiles/r09_spliced_fast.md §4)
#define H2G_DEFAULT_FAST_SPLICED 0
// (the counter words of one go_run generation, H2G_CNT_BLOCK of them: h2g_go_args.h)
#define H2G_MACH_MAXGRID 48u       // workgroups of ONE machine pass behind a fast pass
#define H2G_MACH_TOTAL 128u        // ... and of all machine passes in flight together ("mach_total": a pass gets at most mach_total / mstreams workgroups)
// Resident batches (round 6): a stream holds up to H2G_MAX_BATCHES read sets WITH their result rows (h2g_stream_select_batch): h2g_stream::batch, of which
// h2g_stream::cur() is the selected one.  A run captures its batch's pointers in its argument block when it is queued, so runs over different batches
// are in flight together — fast passes and up to eight machine passes — each writing its own rows (a streaming caller's steady state: SURVEY §8(d) configs[2] is 10 M pairs, not one
// million ten times).
#define H2G_MAX_BATCHES 16
struct BatchCtx {
	size_t n_reads = 0; uint32_t max_read_len = 0;
	DevBuf<uint8_t> d_codes; DevBuf<uint32_t> d_offs; DevBuf<char> d_quals; bool has_quals = false;
	DevBuf<char> d_names; DevBuf<uint32_t> d_name_offs; bool has_names = false;      // (d_names: the name bytes it holds room for + 64)
	DevBuf<uint8_t> d_codes2; DevBuf<uint32_t> d_offs2; DevBuf<char> d_quals2, d_names2; DevBuf<uint32_t> d_name_offs2; bool has_mates = false, has_quals2 = false;
	// result rows: aln_slots (>= -k) records per read in d_aln, pair_slots (>= H2G_PAIR_RES_CAP) per mate in d_paln
	DevBuf<ReadOut> d_rout; DevBuf<h2g_alnres> d_aln; uint32_t aln_slots = 0;
	DevBuf<PairOut> d_pout; DevBuf<h2g_alnres> d_paln[2]; uint32_t pair_slots = 0;
	// explicit PRNG seeds (h2g_set_read_seeds): mate 1's at [0, max_reads), mate 2's at [max_reads, 2 max_reads); a run reads them when has_seeds
	DevBuf<uint32_t> d_seeds; bool has_seeds = false, has_seeds2 = false;
	// --qc-filter bytes (h2g_set_read_filter), laid out like the seeds: 1 = the read passes; a run reads them when has_qc
	DevBuf<uint8_t> d_qc; bool has_qc = false;
	DevBuf<uint32_t> d_ids; bool has_ids = false;         // explicit read ids (h2g_set_read_ids)
	// the read buffers of a batch's first use (h2g_stream_create for batch 0, h2g_stream_select_batch for the others)
	hipError_t ensure_reads(size_t max_reads, size_t max_bases) {
		hipError_t e = d_codes.ensure(max_bases + 64);
		if(e == hipSuccess) e = d_quals.ensure(max_bases + 64);
		return e != hipSuccess ? e : d_offs.ensure(max_reads + 1);
	}
	// room for nb name bytes (h2g_set_read_names, h2g_set_reads_windows, h2g_set_reads_fastq): when they do not fit, the names and their offsets are both replaced
	hipError_t reserve_names(size_t nb, size_t max_reads) {
		if(d_names.size() >= nb + 64 && d_name_offs) return hipSuccess;
		const hipError_t e = d_names.reset(nb + 64);
		return e != hipSuccess ? e : d_name_offs.reset(max_reads + 1);
	}
	// mate 2's buffers, at a batch's first mates (h2g_set_mates, h2g_set_reads_fastq); its names are allocated for every set (nb2 bytes)
	hipError_t ensure_mates(size_t max_reads, size_t max_bases, size_t nb2) {
		hipError_t e = d_codes2.ensure(max_bases + 64);
		if(e == hipSuccess) e = d_quals2.ensure(max_bases + 64);
		if(e == hipSuccess) e = d_offs2.ensure(max_reads + 1);
		if(e == hipSuccess) e = d_name_offs2.ensure(max_reads + 1);
		return e != hipSuccess ? e : d_names2.reset(nb2 + 64);
	}
};
// a stream's timing events (h2g_stream::tm; the pairs h2g_get_counters and the bench entry points read)
enum Tm {
	TM_PRIM0, TM_PRIM1,                     // around the kernels of one primitive call
	TM_SEED0, TM_SEED_MID, TM_SEED1,        // the seed stage: search | resolve + extend
	TM_RUN0, TM_MAIN1, TM_MAIN0, TM_RUN1,   // a go_run: its start, the main pass (TM_MAIN0 .. TM_MAIN1), the end of its last pass
	TM_EXT1,                                // the extended search's HBM stage ends (it starts at TM_PRIM1)
	TM_FAST1,                               // the fast launch has been queued (TM_RUN0 .. TM_FAST1: pre-pass + fast pass)
	TM_SET0, TM_SET1,                       // around the kernels of h2g_set_reads_windows / h2g_set_reads_fastq
	TM_N
};
// Ownership (h2g_dev.h): every device buffer, event and HIP stream below is a handle, and deleting the context gives them all back.  THE STREAMS ARE DECLARED FIRST, so they
// are destroyed last, after every buffer and event; the destructor waits for them before anything goes.  A member that is a raw pointer owns nothing and says whose memory it views.
struct h2g_stream {
	h2g_index* ix = nullptr;          // (the caller's: an index outlives its streams)
	DevStream st;
	// the general machine's pass over a fast pass's hand-ons runs on one of these, next to the fast passes of the FOLLOWING two batches:
	// its few reads are long latency chains (about a fast pass's duration whatever their number), so two such passes are kept in flight
	DevStream mst[H2G_MSTREAMS_MAX];            // all created with the context (h2g_stream_create: their order matters); mst[0 .. n_mst) have entered the rotation, only those ever held work
	DevStream dst;                              // the drain launches' stream: one after the other, each next to the following run's fast launch
	unsigned n_mst = 0;
	unsigned mstreams = 0;                      // pinned (1 .. H2G_MSTREAMS_MAX): lanes = machine streams in rotation = this; 0: S follows the load
	unsigned mstreams_light = H2G_MSTREAMS_LIGHT_DEFAULT;   // S of the light regime
	unsigned rot = 0;                           // machine streams in rotation for the last run behind a fast pass (0: there was none yet)
	bool st2_busy = false;            // a machine stream may hold work
	unsigned gen = 0;                 // go_run generation: run k takes buffer set k % (M + 1), fast pool k % H2G_FAST_POOLS, lane k % M and machine stream lane % S
	// What a run works on is one record per index space, and a run (GoRun) holds a reference to its record of each: an index of one space never subscripts another's.
	// PER-RUN SET, run[gen % (M + 1)]: the fast pass's hand-on list, its counters and the two launches' argument blocks, M + 1 deep — the machine's pass over
	// run k's hand-ons may still be under way while the fast passes of the following runs run
	struct RunSet {
		DevEvent ev_fast, ev_mach;              // the run's fast pass / machine pass is over
		DevEvent ev_bails;                      // h_bail(set) has arrived
		DevEvent ev_drain;                      // the run's drain launch is over (its machine pass waits for it)
		DevBuf<uint32_t> bail_list;             // read ids the fast pass handed on to the general machine (+ their count behind the list)
		DevBuf<uint32_t> orphans;               // slots a fast launch left in flight (+ their count behind the list)
		DevBuf<FastArgs> fast_args, drain_args; // the argument block of the fast launch and of its drain launch (device copies)
	} run[H2G_NBUF];
	// ... and what belongs to a set but lives in one allocation for all of them: its counter block (h2g_go_args.h), the pinned hand-on count of its fast pass
	// (sizes the machine's share of the CUs) and the pinned staging of its two argument blocks (the upload never makes the host wait for the stream)
	DevBuf<unsigned long long> d_counters;      // H2G_NBUF counter blocks of H2G_CNT_BLOCK words
	PinnedBuf<uint32_t> h_bails;
	PinnedBuf<FastArgs> h_fast_args;            // 2 * H2G_NBUF blocks
	unsigned long long* counters(const RunSet& b) const { return d_counters + (&b - run) * H2G_CNT_BLOCK; }
	uint32_t& h_bail(const RunSet& b) const { return h_bails[&b - run]; }
	FastArgs* h_fast(const RunSet& b) const { return h_fast_args + 2 * (&b - run); }
	FastArgs* h_drain(const RunSet& b) const { return h_fast_args + 2 * (&b - run) + 1; }
	unsigned long long* cnt_cur = nullptr;   // the counter block of the last go_run (a view into d_counters)
	uint32_t last_bails = 0;
	size_t max_reads = 0, max_bases = 0;
	BatchCtx batch[H2G_MAX_BATCHES];  // the resident batches: read sets and their result rows
	unsigned cur_batch = 0;
	BatchCtx& cur() { return batch[cur_batch]; }   // the selected one
	const BatchCtx& cur() const { return batch[cur_batch]; }
	DevBuf<h2g_seed_result> d_seed;
	// per-lane scratch of one pass of the go() kernels
	struct GoPool {
		DevBuf<uint8_t> ws;                               // AlignWS x lanes of the unit last run
		DevBuf<uint8_t> gws;                              // GraphWS x lanes (graph indexes only)
		DevBuf<uint8_t> sw; size_t sw_stride = 0, sw_lanes = 0;   // Smith-Waterman scratch (only with bowtie2_dp != 0): what it is laid out for
		DevBuf<uint8_t> sc;                               // combineWith temp_scores per lane
	};
	// MACHINE STREAM, mach[lane % S] (its HIP stream: mst[] above, stream_of): what a pass only needs while it runs.  mach[0] also serves the passes on the first stream
	struct MachStream {
		DevEvent ev_rot;                    // what the stream holds when the rotation changes
		GoPool main, second;                // the main pass's scratch; the second pass's over overflowed reads (large workspace)
		DevBuf<uint32_t> ovf_list;          // read ids whose workspace overflowed in the main pass (+ their count behind the list)
		bool warmed = false;                // the stream has run both machine kernels once
	} mach[H2G_MSTREAMS_MAX];
	hipStream_t stream_of(const MachStream& m) const { return mst[&m - mach]; }
	const MachStream* ovf_cur = mach;       // the one whose overflow list the last run used
	DevBuf<uint32_t> dbg_buf;         // development hook (H2G_GO_DBG_READ)
	// FAST POOL, fpool[gen % H2G_FAST_POOLS]: the fast pass's reads in flight (h2g_k_go_fast.hip) — the drain launch of run k reads run k's pool while the fast passes of runs k + 1 and k + 2 run
	struct FastPool {
		DevBuf<uint8_t> slots;
		DevBuf<uint32_t> ps0;               // the pre-pass's records of the run on this pool (h2g_k_ps0.hip): read by its fast launch and its drain launch
		DevEvent ev_last;                   // the drain launch that last read the pool is over
	} fpool[H2G_FAST_POOLS];
	size_t orphan_cap = 0;
	DevBuf<uint8_t> d_drain_slots;                                   // the drain launch's own pool
	DevBuf<uint8_t> d_drain_sc;                                      // graph indexes: its combineWith scores per lane
	bool dst_busy = false;
	DevEvent ev_dr[2];                                               // (timed) around the last drain launch
	bool ran_drain = false;
	const uint32_t* orph_cur = nullptr;                              // the orphan count of the last run (a view into a buffer set's orphans)
	DevBuf<uint8_t> d_fast_gws;                                     // graph indexes: GraphWS per lane of the fast kernel (scratch of one primitive)
	DevBuf<uint8_t> d_fast_sc;                                      // ... and combineWith's temp_scores per lane
	bool ran_fast = false;
	// development / measurement knobs: the table g_knobs below names each one, with its default, its h2g_stream_tune key and its H2G_* environment name (read ONCE,
	// when the stream is created, which also sets the defaults).  tail_auto / mach_total_auto: nobody has set the knob, its policy decides
	struct Tune { int fast, blocks_per_cu, pair_slots, no_second_pass; unsigned mach_div, mach_min, mach_total; int mach_total_auto = 1; int fast_reserve; long dbg_read;
	              int tail, tail_auto = 1, align_mate, orphan, drain_grid, mate_handover, ps0, fast_spliced; } tune = {};
	h2g_align_params last_p; int last_paired = -1;   // the option set of the last go_run (a different one waits for the machine streams)
	DevBuf<uint8_t> d_sw_ws;      // h2g_sw_align: H/E/F workspace of one batch of problems
	DevBuf<SwLaneState> d_sw_states;
	// LANE, gen % M: the three areas below are partitioned by lane (PartArea, h2g_parts.h: part m is the lane's, with a cursor of its own)
	// records with more than H2G_MAX_EDITS edits keep their lists here (MachOut::ledits); the cursors: d_ledits_cur[lane]
	PartArea<h2g_edit> ledits; DevBuf<uint32_t> d_ledits_cur;
	unsigned ledits_touched = 0;   // parts a run has written to since the last h2g_set_reads (bit per lane): the span h2g_align_fetch_long_edits reports
	PartArea<h2g_alnres> paln_ovf; // pairs with more records than pair_slots per mate (MachOut::ovf); the cursor is a word of the run's counter block
	// the XL units' concordant lists that PairOut cannot carry (XlPairs): per read of the batch where its list starts, the lists and their cursors, d_xlp_cur[lane].
	// xlp_pout: the result rows of the batch the last XL paired run wrote (a view of that batch's d_pout; nullptr: no list is current)
	DevBuf<uint32_t> d_xlp_at; PartArea<uint32_t> xlp; DevBuf<uint32_t> d_xlp_cur;
	const PairOut* xlp_pout = nullptr;
	DevBuf<uint8_t> d_tmp[4];                   // scratch of one call (tmp_buf): each 256 bytes beyond its largest request
	// SAM text on the device (h2g_sam_text_*): what d_tmp holds is nobody's once another call takes a slot, so every such call (tmp_buf), every batch selection and every call
	// that sets reads, mates or names counts tmp_gen up; a compact fetch notes the count it ended with, and the text call runs only while the two are equal
	uint64_t tmp_gen = 0;
	struct CompactFetch { bool valid = false, paired = false; uint64_t gen = 0; unsigned batch = 0; size_t first = 0, n = 0; const uint8_t* d_rec[2] = {nullptr, nullptr}; uint64_t bytes[2] = {0, 0};
	                      const uint64_t* d_boffs[2] = {nullptr, nullptr}; /* the offset arrays of the fetch (tmp slots 0 / 2), [n + 1] each; d_rec and these are views into d_tmp */ } cfetch;
	DevBuf<uint8_t> d_sam[5];                   // descriptors, pool, line offsets (+ scan tile sums + the check's flag), text, the handle's tables
	uint64_t samtab_uid = 0, samtab_gen = 0; uint32_t samtab_nrefs = 0, samtab_names = 0, samtab_rg = 0, samtab_nalts = 0; int32_t samtab_strand = 0;   // whose tables d_sam[4] holds
	DevEvent ev_sam[4];                         // (created by the first text call)
	h2g_sam_text_stats sam_stats = {};
	// h2g_sam_text_*_planned: two descriptor slots per read, class + filter bytes, line counts (+ scan tile sums, per-read source of the handed-on lines, line ends), the
	// handed-on reads' entries, their descriptors
	DevBuf<uint8_t> d_plan[5];
	DevEvent ev_plan[4];                        // (created by the first planned call)
	h2g_sam_plan_stats plan_stats = {};
	std::vector<uint8_t> plan_classes;
	DevEvent tm[TM_N];
	bool ran_seed = false, ran_align = false;
	h2g_counters last;
	h2g_windows_stats win_stats = {};           // of the last h2g_set_reads_windows
	h2g_fastq_stats fq_stats = {};              // of the last h2g_set_reads_fastq
	DevBuf<unsigned long long> d_warm_cnt;      // counter block of the machine streams' empty first launches (go_warmup); word H2G_CNT_NO_SECOND, which nobody writes, is their list's count
	DevBuf<uint8_t> d_warm_rows;                // ... and the result rows they are given: never the current batch's
	// whatever is queued ends before its buffers, events and streams go (h2g_stream_free's contract; any other path that drops a context gets it too)
	~h2g_stream() {
		if(st) (void)hipStreamSynchronize(st);
		if(dst) (void)hipStreamSynchronize(dst);
		for(unsigned k = 0; k < n_mst; k++) (void)hipStreamSynchronize(mst[k]);
	}
};
struct StreamFree { void operator()(h2g_stream* s) const { h2g_stream_free(s); } };

// Large arrays travel through page-locked staging buffers filled by several threads: a pageable hipMemcpy of a human-size index (4.7 GB) was most of its 1.2 s load (round 6).
// Chunk k of a copy is thread k mod T's: wait for its staging buffer, memcpy (from a host vector or straight from a mapped index file: the page faults spread over the threads
// too), hipMemcpyAsync on the thread's own stream.
struct Stager {
	enum { T = 6, NB = 2 };
	static constexpr size_t CH = (size_t)16 << 20;
	DevStream st[T]; PinnedBuf<uint8_t> buf[T][NB]; DevEvent ev[T][NB];
	int device = 0; bool ok = false;
	bool init(int dev) {
		device = dev; ok = true;
		for(int t = 0; t < T && ok; t++) {
			ok = st[t].create(hipStreamNonBlocking) == hipSuccess;
			for(int b = 0; b < NB && ok; b++) ok = buf[t][b].ensure(CH) == hipSuccess && ev[t][b].create(hipEventDisableTiming) == hipSuccess;
		}
		if(!ok) (void)hipGetLastError();
		return ok;
	}
	bool copy(void* dst, const void* src, size_t bytes) {
		return gather(dst, bytes, [src](uint8_t* out, size_t off, size_t len) { memcpy(out, (const uint8_t*)src + off, len); });
	}
	// the same pipeline with the staging buffers filled by `fill(out, off, len)`: bytes [off, off + len) of an array that exists nowhere on the host in one piece
	template <class F>
	bool gather(void* dst, size_t bytes, F fill) {
		std::atomic<bool> good{true};
		std::thread th[T];
		const size_t nch = (bytes + CH - 1) / CH;
		for(int t = 0; t < T; t++) th[t] = std::thread([&, t]() {
			if(hipSetDevice(device) != hipSuccess) { good = false; return; }
			size_t n = 0;
			for(size_t k = (size_t)t; k < nch; k += T, n++) {
				const int b = (int)(n % NB);
				const size_t off = k * CH, len = bytes - off < CH ? bytes - off : CH;
				if(n >= NB && hipEventSynchronize(ev[t][b]) != hipSuccess) { good = false; return; }
				fill(buf[t][b], off, len);
				if(hipMemcpyAsync((uint8_t*)dst + off, buf[t][b], len, hipMemcpyHostToDevice, st[t]) != hipSuccess || hipEventRecord(ev[t][b], st[t]) != hipSuccess) { good = false; return; }
			}
			if(hipStreamSynchronize(st[t]) != hipSuccess) good = false;
		});
		for(int t = 0; t < T; t++) th[t].join();
		if(!good) (void)hipGetLastError();
		return good;
	}
};
// a device array of the index: allocated into a handle of this scope, which `allocs` takes over; counted in device_bytes
static int index_alloc(h2g_index* ix, size_t bytes, uint8_t** out) {
	DevBuf<uint8_t> b;
	HIPCHK(b.reset(bytes));
	*out = b;
	ix->allocs.push_back(std::move(b));
	ix->device_bytes += bytes;
	return H2G_OK;
}
static int upload_raw(h2g_index* ix, const void* src, size_t n, const void** out, size_t pad, Stager* sg) {
	uint8_t* p = nullptr;
	int rc;
	if((rc = index_alloc(ix, n + pad, &p))) return rc;
	HIPCHK(hipMemset(p + n, 0, pad));                                // (the padding only: the rest is about to be written)
	if(n) {
		if(sg && sg->ok && n >= ((size_t)32 << 20)) { if(!sg->copy(p, src, n)) { snprintf(g_err, sizeof g_err, "index upload through the staging buffers failed"); return H2G_ERR_DEVICE; } }
		else HIPCHK(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
	}
	*out = p;
	return H2G_OK;
}
template <typename T>
static int upload(h2g_index* ix, const std::vector<T>& v, const T** out, size_t pad = 64, Stager* sg = nullptr) {
	const void* p = nullptr;
	const int rc = upload_raw(ix, v.data(), v.size() * sizeof(T), &p, pad ? pad : 64, sg);
	*out = (const T*)p;
	return rc;
}

extern "C" void h2g_load_opts_init(h2g_load_opts* o) { o->device = 0; o->load_local = 1; }

// ------------------------------------------------------------------------------------------ the dense SA table
// Row-parallel: every row runs the canonical walk (sa_dense_build_rows, h2g_core.h).  A wave owns H2G_DENSE_CHUNK consecutive rows, lane l the rows
// l, l + 64, ... of them: its stores stay within the chunk's 20 KB while its walks follow one another without waiting for the wave's longest.
#define H2G_DENSE_CHUNK 4096u
__global__ __launch_bounds__(256) void k_sa_dense_build(DGfm g, uint32_t* sa_dense, uint8_t* sa_dist) {
	const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) / 64u;
	const uint64_t base = wave * H2G_DENSE_CHUNK;
	if(base >= g.gbwtLen) return;
	const uint64_t lim = base + H2G_DENSE_CHUNK < g.gbwtLen ? base + H2G_DENSE_CHUNK : g.gbwtLen;
	sa_dense_build_rows(g, base + (threadIdx.x & 63u), 64u, lim, sa_dense, sa_dist);
}
// rows whose table entry is not what the canonical walk gives (h2g_index_dense_sa_check)
__global__ __launch_bounds__(256) void k_sa_dense_check(DGfm g, const uint32_t* sa_dense, const uint8_t* sa_dist, unsigned long long* ndiff) {
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	unsigned long long bad = 0;
	for(uint64_t row = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; row < g.gbwtLen; row += stride) {
		uint32_t steps = 0;
		const uint32_t off = sa_walk(g, (uint32_t)row, &steps);
		const uint32_t d = steps < H2G_SA_DIST_SAT ? steps : H2G_SA_DIST_SAT;
		if(sa_dist[row] != d || (d != H2G_SA_DIST_SAT && sa_dense[row] != off)) bad++;
	}
	if(bad) atomicAdd(ndiff, bad);
}
// H2G_DENSE_SA: 0 never, 1 (default) build asynchronously when the table fits, 2 build and wait.  Nothing here fails a load: no table = every row walks.
static void dense_sa_start(h2g_index* ix) {
	const char* ev = getenv("H2G_DENSE_SA");
	const int mode = ev && *ev ? atoi(ev) : 1;
	const DGfm& g = ix->dg;
	if(mode <= 0 || !g.linear || g.lineRate != 6 || g.gbwtLen == 0) return;
	const size_t rows = g.gbwtLen, b_dense = rows * 4 + 64, b_dist = rows + 64;
	size_t free_b = 0, total_b = 0;
	// it fits when it takes at most a quarter of the memory that is free now, with the index uploaded: a caller's own pools are not squeezed
	if(hipMemGetInfo(&free_b, &total_b) != hipSuccess || b_dense + b_dist > free_b / 4) { (void)hipGetLastError(); return; }
	// built into handles of this scope, which become the index's once everything is queued: a failure on the way drops them
	DevStream st; DevEvent e;
	DevBuf<uint8_t> pd, pt;
	bool ok = pd.reset(b_dense) == hipSuccess && pt.reset(b_dist) == hipSuccess && e.create(hipEventDisableTiming) == hipSuccess;
	if(ok) {   // at the lowest priority: runs queued while it is under way get their workgroups placed first
		int least = 0, greatest = 0;
		ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && st.create_with_priority(hipStreamNonBlocking, least) == hipSuccess;
	}
	ok = ok && hipDeviceSynchronize() == hipSuccess;                  // the uploads (their padding is set on the null stream) are over
	ix->dense_synced = ok;
	const auto t0 = std::chrono::steady_clock::now();
	if(ok) {
		const uint64_t waves = ((uint64_t)rows + H2G_DENSE_CHUNK - 1) / H2G_DENSE_CHUNK;
		hipLaunchKernelGGL(k_sa_dense_build, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, g, (uint32_t*)pd.get(), pt.get());
		ok = hipGetLastError() == hipSuccess && hipEventRecord(e, st) == hipSuccess;
		if(!ok && st) (void)hipStreamSynchronize(st);
	}
	if(!ok) { (void)hipGetLastError(); return; }
	ix->device_bytes += b_dense + b_dist;
	ix->d_sa_dense = (uint32_t*)pd.get(); ix->d_sa_dist = pt.get();
	ix->allocs.push_back(std::move(pd)); ix->allocs.push_back(std::move(pt));
	ix->dense_st = std::move(st); ix->dense_ev = std::move(e);
	if(mode >= 2) {
		if(hipStreamSynchronize(ix->dense_st) != hipSuccess) { (void)hipGetLastError(); return; }       // (the table stays unused: dense_ready is never set by a failed event)
		ix->dense_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		ix->dense_ready.store(true, std::memory_order_release);
	}
}

// ------------------------------------------------------------------------------------------ the dense table of local rows
// One workgroup per local index, a quarter of its rows per wave, lane l the rows l, l + 64, ... of that quarter (lsa_build_rows, h2g_align.h): the index's
// 16 KB of sides stay in cache under the workgroup and a wave's stores stay within its quarter.  An empty local index (never searched) keeps one unused entry.
__global__ __launch_bounds__(256) void k_lsa_dense_build(DLocalSet ls, const uint64_t* lsa_base, uint32_t* lsa) {
	const uint32_t li = blockIdx.x;
	if(li >= ls.n) return;
	const DLocalDesc* d = &ls.desc[li];
	uint32_t* tab = lsa + lsa_base[li];
	if(d->len == 0) { if(threadIdx.x == 0) tab[0] = H2G_LSA_MISS; return; }
	const uint32_t rows = d->len + 1, per = (rows + 3) / 4, lo = (threadIdx.x >> 6) * per, hi = lo + per < rows ? lo + per : rows;
	LIdxR lx; lx.init(&ls, d);
	lsa_build_rows(lx, (0xffffu << ls.offRate) & 0xffffu, ls.offRate, ls.words + d->offs_off, lo + (threadIdx.x & 63u), 64u, hi, tab);
}
// entries that are not what the canonical walk gives (h2g_index_dense_lsa_check)
__global__ __launch_bounds__(256) void k_lsa_dense_check(DLocalSet ls, const uint64_t* lsa_base, const uint32_t* lsa, unsigned long long* ndiff) {
	unsigned long long bad = 0;
	for(uint32_t li = blockIdx.x; li < ls.n; li += gridDim.x) {
		const DLocalDesc* d = &ls.desc[li];
		const uint32_t* tab = lsa + lsa_base[li];
		if(d->len == 0) { if(threadIdx.x == 0 && tab[0] != H2G_LSA_MISS) bad++; continue; }
		LIdxR lx; lx.init(&ls, d);
		for(uint32_t row = threadIdx.x; row <= d->len; row += blockDim.x) {
			uint32_t steps = 0;
			const uint32_t off = sa_walk_idx(lx, row, (0xffffu << ls.offRate) & 0xffffu, ls.offRate, ls.words + d->offs_off, true, &steps);
			const uint32_t want = steps >= H2G_LSA_DIST_SAT || off > 0xffffu ? H2G_LSA_MISS : off | (steps << 16);
			if(tab[row] != want) bad++;
		}
	}
	if(bad) atomicAdd(ndiff, bad);
}
// H2G_DENSE_LSA: 0 never, 1 build asynchronously when the table fits, 2 build and wait; unset: what H2G_DENSE_SA resolves to.  Queued behind the global
// table's build on the same low-priority stream; the fit rule is that table's, applied to the memory free once it is allocated.  Nothing here fails a load.
static void dense_lsa_start(h2g_index* ix) {
	const char* ev = getenv("H2G_DENSE_LSA");
	if(!ev || !*ev) ev = getenv("H2G_DENSE_SA");
	const int mode = ev && *ev ? atoi(ev) : 1;
	if(mode <= 0 || !ix->dg.linear || !ix->has_local || ix->h_ldesc.empty()) return;
	const size_t n = ix->h_ldesc.size();
	std::vector<uint64_t> base(n + 1, 0);
	for(size_t i = 0; i < n; i++) {
		if(!local_is_linear(ix->h_ldesc[i])) return;
		base[i + 1] = base[i] + (uint64_t)ix->h_ldesc[i].len + 1;
	}
	const size_t rows = base[n], b_tab = rows * 4 + 64, b_base = (n + 1) * 8;
	size_t free_b = 0, total_b = 0;
	if(hipMemGetInfo(&free_b, &total_b) != hipSuccess || b_tab + b_base > free_b / 4) { (void)hipGetLastError(); return; }
	DevStream own_st; DevEvent e;                            // (own_st: only when the global table's build left no stream)
	DevBuf<uint8_t> pt, pb;
	bool ok = pt.reset(b_tab) == hipSuccess && pb.reset(b_base) == hipSuccess && e.create(hipEventDisableTiming) == hipSuccess;
	if(ok && !ix->dense_st) {
		int least = 0, greatest = 0;
		ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && own_st.create_with_priority(hipStreamNonBlocking, least) == hipSuccess;
	}
	const hipStream_t st = ix->dense_st ? ix->dense_st.get() : own_st.get();
	if(ok && !ix->dense_synced) { ok = hipDeviceSynchronize() == hipSuccess; ix->dense_synced = ok; }
	ok = ok && hipMemcpy(pb, base.data(), b_base, hipMemcpyHostToDevice) == hipSuccess;
	const auto t0 = std::chrono::steady_clock::now();
	if(ok) {
		hipLaunchKernelGGL(k_lsa_dense_build, dim3((unsigned)n), dim3(256), 0, st, ix->dls, (const uint64_t*)pb.get(), (uint32_t*)pt.get());
		ok = hipGetLastError() == hipSuccess && hipEventRecord(e, st) == hipSuccess;
		if(!ok && st) (void)hipStreamSynchronize(st);
	}
	if(!ok) { (void)hipGetLastError(); return; }
	ix->device_bytes += b_tab + b_base;
	ix->d_lsa = (uint32_t*)pt.get(); ix->d_lsa_base = (uint64_t*)pb.get(); ix->lsa_rows = rows;
	ix->allocs.push_back(std::move(pt)); ix->allocs.push_back(std::move(pb));
	if(own_st) ix->dense_st = std::move(own_st);
	ix->lsa_ev = std::move(e);
	if(mode >= 2) {
		if(hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return; }
		ix->lsa_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		ix->lsa_ready.store(true, std::memory_order_release);
	}
}

static void fill_dgfm(const HostGfm& g, uint32_t minK, DGfm* d) {
	for(int i = 0; i < 5; i++) d->fchr[i] = g.fchr[i];
	d->len = g.p.len; d->gbwtLen = g.p.gbwtLen; d->ftabLim = g.p.linear ? g.p.len : g.p.gbwtLen;
	d->sideGbwtLen = g.p.sideGbwtLen; d->sideGbwtSz = g.p.sideGbwtSz; d->lineRate = g.p.lineRate;
	d->offRate = g.p.offRate; d->offMask = g.p.offMask; d->ftabChars = g.p.ftabChars;
	d->nFrag = g.nFrag; d->nPat = g.nPat; d->nZ = (uint32_t)g.zOffs.size();
	d->zoff = g.zOffs.empty() ? H2G_MAX : g.zOffs[0];
	d->minK = minK; d->linear = g.p.linear;
}

extern "C" h2g_status h2g_index_load(const char* base, const h2g_load_opts* opts, h2g_index** out) {
	if(!base || !out) return H2G_ERR_ARG;
	h2g_load_opts o;
	h2g_load_opts_init(&o);
	if(opts) o = *opts;
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if(e != hipSuccess || ndev <= 0) { snprintf(g_err, sizeof g_err, "no HIP device (libh2g has no CPU path)"); return H2G_ERR_DEVICE; }
	if(o.device < 0 || o.device >= ndev) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(o.device));
	IndexPtr ixp(new h2g_index());                           // (every early return below frees what the index holds by then)
	h2g_index* const ix = ixp.get();
	ix->device = o.device;
	// the local indexes (.5 / .6: 2.1 GB of a human-size index) are packed on a thread of their own, straight from the files, while the global
	// index is read, parsed and uploaded here
	LocalPack lp;
	LocalPlan lpl;                                           // the local indexes' pieces in the mapped files: streamed to the device below, never assembled on the host
	int lrc = 1;                                             // 1: no local files (an index built without them loads for rank / search only)
	std::thread tlocal;
	if(o.load_local) tlocal = std::thread([&]() { try { lrc = plan_local_pack(base, 0, lp, lpl); if(lrc == -1) lrc = 1; } catch(...) { lrc = -2; } });   // (bad_alloc / length_error on a corrupt file must not escape the thread)
	struct Joiner { std::thread& t; ~Joiner() { if(t.joinable()) t.join(); } } joiner{tlocal};      // (every early return below waits for it)
	int rc;
	const bool ltime = getenv("H2G_LOAD_TIMING") != nullptr;
	const auto tl0 = std::chrono::steady_clock::now();
	auto lsec = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count(); };
	BigViews bv;                                             // sides, SA sample and reference bases stay in the mapped files until they are on the device
	std::unique_ptr<Stager> sgp(new Stager());               // (freed before the dense SA table's build is queued: freeing page-locked memory waits for the device)
	Stager& sg = *sgp;
	sg.init(o.device);
	try { rc = load_host_index(base, false, ix->host, false, &bv); } catch(...) { rc = -2; }
	const double t_parse = lsec();   // a length read from a corrupt file: an allocation failure is a format error, not std::terminate across the C ABI
	if(rc != 0) { snprintf(g_err, sizeof g_err, "cannot read index %s", base); return rc == -1 ? H2G_ERR_IO : H2G_ERR_FORMAT; }
	const HostGfm& g = ix->host.g;
	fill_dgfm(g, ix->host.minK, &ix->dg);
	int s = H2G_OK;
	{
		const void *ds_ = nullptr, *do_ = nullptr;
		if((s = upload_raw(ix, bv.sides, bv.sides_n, &ds_, 256, &sg)) || (s = upload_raw(ix, bv.offs, bv.offs_n, &do_, 64, &sg))) return s;
		ix->dg.sides = (const uint8_t*)ds_; ix->dg.offs = (const uint32_t*)do_;
	}
	if((s = upload(ix, g.ftab, &ix->dg.ftab)) ||
	   (s = upload(ix, g.eftab, &ix->dg.eftab)) ||
	   (s = upload(ix, g.rstarts, &ix->dg.rstarts)) || (s = upload(ix, g.plen, &ix->dg.plen)) ||
	   (s = upload(ix, g.zOffs, &ix->dg.zoffs))) return s;
	const HostRef& r = ix->host.r;
	ix->dr.nrefs = r.nrefs;
	{
		const void* db_ = nullptr;
		if((s = upload_raw(ix, bv.buf, bv.buf_n, &db_, 64, &sg))) return s;
		ix->dr.buf = (const uint8_t*)db_;
	}
	const double t_global = lsec();
	if((s = upload(ix, r.rec_start, &ix->dr.rec_start)) ||
	   (s = upload(ix, r.rec_len, &ix->dr.rec_len)) || (s = upload(ix, r.rec_bufoff, &ix->dr.rec_bufoff)) ||
	   (s = upload(ix, r.refRecOffs, &ix->dr.refRecOffs)) || (s = upload(ix, r.refLens, &ix->dr.refLens))) return s;
	static_assert(sizeof(HostAlt) == sizeof(DAlt), "HostAlt mirrors DAlt");
	ix->dalts.a = nullptr; ix->dalts.n = 0; ix->dalts.maxAltsTried = 16;      // --max-altstried default hisat2.cpp:521
	if(!g.p.linear && !ix->host.alts.empty()) {
		std::vector<uint64_t> packed;                      // the ALTs followed by the haplotype table (pack_alts, h2g_graph.h)
		pack_alts(ix->host.alts, ix->host.hap_left, ix->host.hap_right, ix->host.hap_maxright, ix->host.hap_first, ix->host.hap_ids, packed);
		const uint64_t* da = nullptr;
		if((s = upload(ix, packed, &da))) return s;
		ix->dalts.a = reinterpret_cast<const DAlt*>(da);
		ix->dalts.n = (uint32_t)ix->host.alts.size();
		std::vector<uint32_t> bk;
		alt_buckets(reinterpret_cast<const DAlt*>(ix->host.alts.data()), ix->dalts.n, bk);
		const uint32_t* dbk = nullptr;
		if(!bk.empty()) { if((s = upload(ix, bk, &dbk))) return s; ix->dalts.bucket = dbk; ix->dalts.nbucket = (uint32_t)bk.size(); }
		// a --ss index: its splice-site ALTs are graph edges AND known sites of the database (SpliceSiteDB::read(gfm, alts))
		splice_sites_of_alts(reinterpret_cast<const uint32_t*>(ix->host.alts.data()), ix->host.alts.size(), sizeof(HostAlt) / 4, g.rstarts.data(), g.nFrag, g.p.len, ix->alt_sites);
		for(const HostAlt& a : ix->host.alts) if(a.type == 5) ix->dalts.has_splice = 1;
		// ... and its exons, for --avoid-pseudogene (SpliceSiteDB::insideExon): allocated only when the index has some
		std::vector<DExon> ex;
		exons_of_alts(reinterpret_cast<const uint32_t*>(ix->host.alts.data()), ix->host.alts.size(), sizeof(HostAlt) / 4, g.rstarts.data(), g.nFrag, g.p.len, g.plen.data(), g.nPat, ex);
		if(!ex.empty()) {
			const DExon* de = nullptr;
			if((s = upload(ix, ex, &de))) return s;
			ix->dexons.e = de; ix->dexons.n = (uint32_t)ex.size();
		}
	}
	memset(&ix->dls, 0, sizeof ix->dls);
	if(tlocal.joinable()) tlocal.join();
	const double t_join = lsec();
	if(lrc == -2) { snprintf(g_err, sizeof g_err, "cannot read the local indexes of %s", base); return H2G_ERR_FORMAT; }
	if(o.load_local && lrc == 0 && !lp.desc.empty()) {
		while(lp.first.size() <= g.nPat) lp.first.push_back((uint32_t)lp.desc.size());
		const DLocalDesc* dd; const uint8_t* ds = nullptr; const uint16_t* dw = nullptr; const uint32_t* df; const uint32_t* dz;
		{	// the two packed arrays (sides: 128-byte aligned per index, 256 bytes of padding behind; 16-bit words: 64 entries of padding), gathered chunk by chunk out of the files
			const size_t sb = lpl.nsides_tot + 256, wb = (lpl.nwords_tot + 64) * 2;
			uint8_t *ps = nullptr, *pw = nullptr;
			if((s = index_alloc(ix, sb + 64, &ps)) || (s = index_alloc(ix, wb + 64, &pw))) return s;
			HIPCHK(hipMemset(ps + sb, 0, 64)); HIPCHK(hipMemset(pw + wb, 0, 64));
			bool okc = sg.ok;
			if(okc) okc = sg.gather(ps, sb, [&](uint8_t* out_, size_t off_, size_t len_) { local_fill_sides(lpl, out_, off_, len_); }) &&
			              sg.gather(pw, wb, [&](uint8_t* out_, size_t off_, size_t len_) { local_fill_words(lpl, out_, off_, len_); });
			if(!okc) {   // (no staging buffers: through one host chunk at a time)
				std::vector<uint8_t> tmp((size_t)16 << 20);
				for(size_t off_ = 0; off_ < sb; off_ += tmp.size()) { const size_t len_ = sb - off_ < tmp.size() ? sb - off_ : tmp.size(); local_fill_sides(lpl, tmp.data(), off_, len_); HIPCHK(hipMemcpy((uint8_t*)ps + off_, tmp.data(), len_, hipMemcpyHostToDevice)); }
				for(size_t off_ = 0; off_ < wb; off_ += tmp.size()) { const size_t len_ = wb - off_ < tmp.size() ? wb - off_ : tmp.size(); local_fill_words(lpl, tmp.data(), off_, len_); HIPCHK(hipMemcpy((uint8_t*)pw + off_, tmp.data(), len_, hipMemcpyHostToDevice)); }
			}
			ds = (const uint8_t*)ps; dw = (const uint16_t*)pw;
		}
		if((s = upload(ix, lp.desc, &dd)) || (s = upload(ix, lp.first, &df)) || (s = upload(ix, lp.zoffs, &dz))) return s;
		ix->dls = lp.view(dd, ds, dw, df, dz);
		ix->h_ldesc = lp.desc;
		ix->host.local_first = lp.first;                     // (h2g_local_index_of)
		ix->n_local = (uint32_t)lp.desc.size();
		ix->has_local = true;
		for(const HostAlt& a : ix->host.alts) if(a.type >= 5) ix->has_splice_alts = true;   // ALT_SPLICESITE / ALT_EXON alt.h:38-39
	}
	{   // splice-site probability tables (spliced alignment): 1.4 MB, index-independent
		std::vector<float> d, a1, a2;
		splice_tables(d, a1, a2);
		if((s = upload(ix, d, &ix->d_spl[0])) || (s = upload(ix, a1, &ix->d_spl[1])) || (s = upload(ix, a2, &ix->d_spl[2]))) return s;
	}
	if(!ix->alt_sites.empty()) { const h2g_status rs_ = h2g_index_set_splice_sites(ix, nullptr, 0, 0); if(rs_ != H2G_OK) return rs_; }
	sgp.reset();
	const double t_up = lsec();
	dense_sa_start(ix);
	const double t_sa = lsec();
	dense_lsa_start(ix);
	if(ltime) fprintf(stderr, "index load: parse %.3f s, global arrays on the device %.3f s, local pack joined %.3f s, dense SA table %s (%.3f s here, build %.1f ms), "
	                  "dense local table %s (%.3f s here, build %.1f ms, %.2f GB), all %.3f s (%.2f GB)\n", t_parse, t_global, t_join,
	                  !ix->d_sa_dist ? "none" : ix->dense_ready.load() ? "built" : "queued", t_sa - t_up, ix->dense_ms,
	                  !ix->d_lsa ? "none" : ix->lsa_ready.load() ? "built" : "queued", lsec() - t_sa, ix->lsa_ms, ix->d_lsa ? (ix->lsa_rows * 4 + 64 + (ix->h_ldesc.size() + 1) * 8) / 1e9 : 0.0,
	                  lsec(), ix->device_bytes / 1e9);
	*out = ixp.release();
	return H2G_OK;
}

extern "C" h2g_status h2g_index_get_info(const h2g_index* ix, h2g_index_info* o) {
	if(!ix || !o) return H2G_ERR_ARG;
	const GfmParams& p = ix->host.g.p;
	o->len = p.len; o->gbwtLen = p.gbwtLen; o->numNodes = p.numNodes; o->lineRate = p.lineRate; o->offRate = p.offRate;
	o->ftabChars = p.ftabChars; o->eftabLen = p.eftabLen; o->linear = p.linear; o->sideSz = p.sideSz;
	o->sideGbwtSz = p.sideGbwtSz; o->sideGbwtLen = p.sideGbwtLen; o->numSides = p.numSides; o->offsLen = p.offsLen;
	o->ftabLen = p.ftabLen; o->nPat = ix->host.g.nPat; o->nFrag = ix->host.g.nFrag; o->nZ = (uint32_t)ix->host.g.zOffs.size();
	o->minK = ix->host.minK; o->nLocal = ix->n_local; o->nRefRecs = (uint32_t)ix->host.r.rec_len.size();
	o->device_bytes = ix->device_bytes;
	return H2G_OK;
}

static h2g_status upload_splice_db(h2g_index* ix) {
	const HostSpliceDB& h = ix->h_ssdb;
	const uint32_t window = ix->dssdb.window;
	ix->dssdb = DSpliceDB();
	ix->dssdb.window = window;
	if(h.fw.empty()) return H2G_OK;
	const void* src[4] = {h.fw.data(), h.bw.data(), h.fw_first.data(), h.bw_first.data()};
	const size_t bytes[4] = {h.fw.size() * sizeof(DSpliceSite), h.bw.size() * sizeof(DSpliceSite), h.fw_first.size() * 4, h.bw_first.size() * 4};
	for(int k = 0; k < 4; k++) {
		if(ix->d_ssdb[k].size() < bytes[k]) HIPCHK(ix->d_ssdb[k].reset(bytes[k] * 2 < 4096 ? 4096 : bytes[k] * 2));
		HIPCHK(hipMemcpy(ix->d_ssdb[k], src[k], bytes[k], hipMemcpyHostToDevice));
	}
	ix->dssdb.fw = (const DSpliceSite*)ix->d_ssdb[0].get(); ix->dssdb.bw = (const DSpliceSite*)ix->d_ssdb[1].get();
	ix->dssdb.fw_first = (const uint32_t*)ix->d_ssdb[2].get(); ix->dssdb.bw_first = (const uint32_t*)ix->d_ssdb[3].get();
	ix->dssdb.n = (uint32_t)h.fw.size();
	return H2G_OK;
}

extern "C" h2g_status h2g_index_set_splice_sites(h2g_index* ix, const h2g_splice_site* sites, size_t n, uint32_t window) {
	if(!ix || (n && !sites)) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipDeviceSynchronize());
	ix->dssdb = DSpliceDB();
	ix->dssdb.window = window;
	ix->h_ssdb = HostSpliceDB();
	std::vector<h2g_splice_site> all(ix->alt_sites);      // the index's own sites first: of equal sites the first is kept
	if(n) all.insert(all.end(), sites, sites + n);
	// an intron longer than a splice edit holds (20 bits) can never be placed by the aligner (max_intronlen is capped there): such sites
	// are refused by name instead of being joined with a truncated length
	for(const h2g_splice_site& x : all) if(x.right > x.left && x.right - x.left - 1 > H2G_SPL_MAXLEN) {
		snprintf(g_err, sizeof g_err, "splice site %u:%u-%u: an intron of more than %u bases", x.tidx, x.left, x.right, (unsigned)H2G_SPL_MAXLEN);
		return H2G_ERR_UNSUPPORTED;
	}
	if(all.empty()) return H2G_OK;
	build_splice_db(all.data(), all.size(), ix->host.g.nPat, ix->h_ssdb);
	return upload_splice_db(ix);
}

// The sites met since the last call (or known ones whose smallest read id went down) join the database: a merge into the sorted host
// copy and one upload into buffers that only ever grow — no sort of everything, no free / malloc per wave of reads.  The caller has
// nothing in flight on this index (the waves of the temporary-splice-site scheme are synchronous by construction).
extern "C" h2g_status h2g_index_add_splice_sites(h2g_index* ix, const h2g_splice_site* delta, size_t n) {
	if(!ix || (n && !delta)) return H2G_ERR_ARG;
	if(n == 0) return H2G_OK;
	HIPCHK(hipSetDevice(ix->device));
	for(size_t i = 0; i < n; i++) if(delta[i].right > delta[i].left && delta[i].right - delta[i].left - 1 > H2G_SPL_MAXLEN) {
		snprintf(g_err, sizeof g_err, "splice site %u:%u-%u: an intron of more than %u bases", delta[i].tidx, delta[i].left, delta[i].right, (unsigned)H2G_SPL_MAXLEN);
		return H2G_ERR_UNSUPPORTED;
	}
	HIPCHK(hipDeviceSynchronize());
	// without a database yet (no h2g_index_set_splice_sites before this call) the index's own splice-site ALTs seed it, as they seed every
	// database (SpliceSiteDB::read(gfm, alts), splice_site.cpp:653); the window stays what it was (0 until a set call names one)
	if(ix->h_ssdb.fw.empty() && !ix->alt_sites.empty()) build_splice_db(ix->alt_sites.data(), ix->alt_sites.size(), ix->host.g.nPat, ix->h_ssdb);
	merge_splice_db(ix->h_ssdb, delta, n, ix->host.g.nPat);
	return upload_splice_db(ix);
}

// The dense SA table of the index: *state = 0 none (not a linear index, H2G_DENSE_SA=0, or it did not fit), 1 complete.  Waits for the build, then walks
// every row on the device and counts in *rows_differ the rows whose entry is not what the walk gives (tests; either pointer may be NULL).
extern "C" h2g_status h2g_index_dense_sa_check(h2g_index* ix, uint32_t* state, uint64_t* rows_differ) {
	if(!ix) return H2G_ERR_ARG;
	if(state) *state = 0;
	if(rows_differ) *rows_differ = 0;
	if(!ix->d_sa_dist) return H2G_OK;
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipStreamSynchronize(ix->dense_st));
	const DGfm g = dg_now(ix);
	if(!g.sa_dist) return H2G_OK;
	if(state) *state = 1;
	if(!rows_differ) return H2G_OK;
	DevBuf<unsigned long long> dn;
	HIPCHK(dn.reset(1));
	unsigned long long hn = 0;
	hipError_t e = hipMemsetAsync(dn, 0, sizeof hn, ix->dense_st);
	if(e == hipSuccess) {
		hipLaunchKernelGGL(k_sa_dense_check, dim3(8192), dim3(256), 0, ix->dense_st, ix->dg, (const uint32_t*)g.sa_dense, (const uint8_t*)g.sa_dist, dn.get());
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = hipMemcpyAsync(&hn, dn, sizeof hn, hipMemcpyDeviceToHost, ix->dense_st);
	if(e == hipSuccess) e = hipStreamSynchronize(ix->dense_st);
	if(e != hipSuccess) return (h2g_status)set_err("h2g_index_dense_sa_check", e);
	*rows_differ = hn;
	return H2G_OK;
}

// The dense table of the local rows, as h2g_index_dense_sa_check: *state = 0 none (not a linear index, no local indexes, H2G_DENSE_LSA=0, or it did not fit),
// 1 complete; *rows_differ = entries that are not what the walk gives.
extern "C" h2g_status h2g_index_dense_lsa_check(h2g_index* ix, uint32_t* state, uint64_t* rows_differ) {
	if(!ix) return H2G_ERR_ARG;
	if(state) *state = 0;
	if(rows_differ) *rows_differ = 0;
	if(!ix->d_lsa) return H2G_OK;
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipStreamSynchronize(ix->dense_st));
	const DLocalSet l = dls_now(ix);
	if(!l.lsa) return H2G_OK;
	if(state) *state = 1;
	if(!rows_differ) return H2G_OK;
	DevBuf<unsigned long long> dn;
	HIPCHK(dn.reset(1));
	unsigned long long hn = 0;
	hipError_t e = hipMemsetAsync(dn, 0, sizeof hn, ix->dense_st);
	if(e == hipSuccess) {
		hipLaunchKernelGGL(k_lsa_dense_check, dim3(l.n < 8192u ? l.n : 8192u), dim3(256), 0, ix->dense_st, ix->dls, l.lsa_base, l.lsa, dn.get());
		e = hipGetLastError();
	}
	if(e == hipSuccess) e = hipMemcpyAsync(&hn, dn, sizeof hn, hipMemcpyDeviceToHost, ix->dense_st);
	if(e == hipSuccess) e = hipStreamSynchronize(ix->dense_st);
	if(e != hipSuccess) return (h2g_status)set_err("h2g_index_dense_lsa_check", e);
	*rows_differ = hn;
	return H2G_OK;
}

extern "C" void h2g_index_free(h2g_index* ix) { delete ix; }      // (~h2g_index waits for the dense tables' builds; the handles do the rest)

// ------------------------------------------------------------------------------------------ synthetic sides
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
	x += 0x9E3779B97F4A7C15ull;
	x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
	x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}

// fills payloads with random symbols; per-side symbol counts go to cnt[side*4 + c]
// (sideSz 64: 6 payload words, occ at +48; sideSz 128: 6.5 payload words, random F/M bits, zero headers, occ at +112)
__global__ void k_synth_fill(uint8_t* sides, uint32_t* cnt, uint64_t nsides, uint64_t seed, uint32_t sideSz) {
	uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	if(s >= nsides) return;
	uint64_t* w = reinterpret_cast<uint64_t*>(sides + s * sideSz);
	uint32_t c[4] = {0, 0, 0, 0};
	for(int k = 0; k < 6; k++) {
		uint64_t v = splitmix64(seed + s * 16 + k);
		w[k] = v;
		for(int cc = 0; cc < 4; cc++) c[cc] += count_word(v, cc, 32);
	}
	if(sideSz == 128) {
		for(int k = 6; k < 13; k++) w[k] = splitmix64(seed + s * 16 + k);
		w[13] = 0;
		for(int cc = 0; cc < 4; cc++) c[cc] += count_word(w[6], cc, 16);
	}
	for(int cc = 0; cc < 4; cc++) cnt[s * 4 + cc] = c[cc];
}
// exclusive prefix over sides in three passes: per-chunk sums, scan of the chunk sums, write-back
#define SYNTH_CHUNKS 16384
__global__ void k_synth_chunk_sum(const uint32_t* cnt, uint64_t nsides, uint32_t* chunk) {
	uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	if(t >= SYNTH_CHUNKS) return;
	uint64_t per = (nsides + SYNTH_CHUNKS - 1) / SYNTH_CHUNKS, a = t * per, b = a + per < nsides ? a + per : nsides;
	uint32_t c[4] = {0, 0, 0, 0};
	for(uint64_t s = a; s < b; s++) for(int k = 0; k < 4; k++) c[k] += cnt[s * 4 + k];
	for(int k = 0; k < 4; k++) chunk[t * 4 + k] = c[k];
}
__global__ void k_synth_chunk_scan(uint32_t* chunk, uint32_t* totals) {
	int c = threadIdx.x;
	if(c >= 4) return;
	uint32_t run = 0;
	for(uint32_t t = 0; t < SYNTH_CHUNKS; t++) { uint32_t v = chunk[t * 4 + c]; chunk[t * 4 + c] = run; run += v; }
	totals[c] = run;
}
__global__ void k_synth_write(uint8_t* sides, const uint32_t* cnt, uint64_t nsides, const uint32_t* chunk, uint32_t sideSz) {
	uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	if(t >= SYNTH_CHUNKS) return;
	uint64_t per = (nsides + SYNTH_CHUNKS - 1) / SYNTH_CHUNKS, a = t * per, b = a + per < nsides ? a + per : nsides;
	uint32_t run[4];
	for(int k = 0; k < 4; k++) run[k] = chunk[t * 4 + k];
	for(uint64_t s = a; s < b; s++) {
		uint32_t* occ = reinterpret_cast<uint32_t*>(sides + s * sideSz + sideSz - 16);
		for(int k = 0; k < 4; k++) { occ[k] = run[k]; run[k] += cnt[s * 4 + k]; }
	}
}

static h2g_status synth_sides(uint64_t num_sides, uint64_t seed, int device, uint32_t sideSz, h2g_index** out) {
	const uint32_t syms = sideSz == 64 ? 192u : H2G_GSIDE_SYMS;
	if(!out || num_sides == 0 || num_sides * (uint64_t)syms >= 0xffffffffull) return H2G_ERR_ARG;
	int ndev = 0;
	if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { snprintf(g_err, sizeof g_err, "no HIP device"); return H2G_ERR_DEVICE; }
	HIPCHK(hipSetDevice(device));
	IndexPtr ixp(new h2g_index());
	h2g_index* const ix = ixp.get();
	ix->synthetic = true;
	ix->device = device;
	DevBuf<uint8_t> sbuf;
	DevBuf<uint32_t> cnt, tot, chunk;                        // scratch of this call
	const size_t bytes = num_sides * sideSz + 256;
	{   // measurement knob: H2G_SIDES_MTYPE=uncached|finegrained allocates the side array with that memory type (adopted by the handle: hipFree takes either)
		const char* mt = getenv("H2G_SIDES_MTYPE");
		const bool unc = mt && !strcmp(mt, "uncached");
		if(unc || (mt && !strcmp(mt, "finegrained"))) {
			void* p = nullptr;
			HIPCHK(hipExtMallocWithFlags(&p, bytes, unc ? hipDeviceMallocUncached : hipDeviceMallocFinegrained));
			sbuf = DevBuf<uint8_t>((uint8_t*)p, bytes);
		}
		else HIPCHK(sbuf.reset(bytes));
	}
	uint8_t* const sides = sbuf;
	HIPCHK(cnt.reset(num_sides * 4));
	HIPCHK(tot.reset(4));
	ix->allocs.push_back(std::move(sbuf));
	ix->device_bytes = num_sides * sideSz;
	hipLaunchKernelGGL(k_synth_fill, dim3((unsigned)((num_sides + 255) / 256)), dim3(256), 0, 0, sides, cnt.get(), num_sides, seed, sideSz);
	HIPCHK(chunk.reset(SYNTH_CHUNKS * 4));
	hipLaunchKernelGGL(k_synth_chunk_sum, dim3(SYNTH_CHUNKS / 256), dim3(256), 0, 0, (const uint32_t*)cnt, num_sides, chunk.get());
	hipLaunchKernelGGL(k_synth_chunk_scan, dim3(1), dim3(64), 0, 0, chunk.get(), tot.get());
	hipLaunchKernelGGL(k_synth_write, dim3(SYNTH_CHUNKS / 256), dim3(256), 0, 0, sides, (const uint32_t*)cnt, num_sides, (const uint32_t*)chunk, sideSz);
	uint32_t totals[4];
	HIPCHK(hipMemcpy(totals, tot, 16, hipMemcpyDeviceToHost));      // (waits for the kernels: the scratch goes at the end of the call)
	GfmParams& p = ix->host.g.p;
	uint32_t len = (uint32_t)(num_sides * syms - 1);
	if(sideSz == 64) p.init(len, len + 1, len + 1, 6, 4, 10, 0, 4);
	else p.init(len - 1000, len + 1, len - 500, 7, 4, 10, 0, 4);   // gbwtLen != len + 1 => graph (gfm.h:139)
	p.numSides = (uint32_t)num_sides;
	ix->host.g.fchr[0] = 0;
	for(int c = 0; c < 4; c++) ix->host.g.fchr[c + 1] = ix->host.g.fchr[c] + totals[c];
	fill_dgfm(ix->host.g, 16, &ix->dg);
	ix->dg.sides = sides;
	ix->dg.nZ = 0;
	*out = ixp.release();
	return H2G_OK;
}
extern "C" h2g_status h2g_index_synth_sides(uint64_t num_sides, uint64_t seed, int device, h2g_index** out) {
	return synth_sides(num_sides, seed, device, 64, out);
}
extern "C" h2g_status h2g_index_synth_graph_sides(uint64_t num_sides, uint64_t seed, int device, h2g_index** out) {
	return synth_sides(num_sides, seed, device, 128, out);
}

// ------------------------------------------------------------------------------------------ stream
// The knobs of go_run, for development and measurement: a row is a knob's h2g_stream_tune key, its environment name (read once, by h2g_stream_create), its default
// and how a value is stored in h2g_stream::Tune; is_auto: the flag that says "nobody has set this knob, its policy decides", cleared by whoever sets it.
//   fast 0: every run goes to the machine whole.  blocks_per_cu / pair_slots > 0: override the geometry / the pair rows (tests).  mach_div 0: the policy of fast_policy.
//   dbg_read: a read id whose primitive requests are traced, -1 none.  tail: reads a workgroup hands on at the end of an exhausted batch.  align_mate: alignMate inside
//   the pass.  orphan: -1 the policy, 0 no drain launch, n its threshold.  mate_handover, ps0: -1 the policy, 0 off, 1 on.  fast_spliced 0: spliced runs go to the machine
//   whole.  mach_total: workgroups of all machine passes in flight together.  fast_reserve: CUs the fast pass leaves free, -1 = as many as the machine passes may hold.
struct Knob { const char *key, *env; long def; void (*set)(h2g_stream::Tune&, long); int h2g_stream::Tune::* is_auto; };
#define H2G_KNOB(key, env, def, member, is_auto) {key, env, def, [](h2g_stream::Tune& t, long v) { t.member = (decltype(t.member))v; }, is_auto}
static const Knob g_knobs[] = {
	H2G_KNOB("fast",           "H2G_GO_FAST",            1,                        fast,           nullptr),
	H2G_KNOB("blocks_per_cu",  "H2G_GO_BLOCKS_PER_CU",   0,                        blocks_per_cu,  nullptr),
	H2G_KNOB("pair_slots",     "H2G_PAIR_SLOTS",         0,                        pair_slots,     nullptr),
	H2G_KNOB("no_second_pass", "H2G_GO_NO_SECOND_PASS",  0,                        no_second_pass, nullptr),
	H2G_KNOB("mach_div",       "H2G_MACH_DIV",           0,                        mach_div,       nullptr),
	H2G_KNOB("mach_min",       "H2G_MACH_MIN",           4,                        mach_min,       nullptr),
	H2G_KNOB("dbg_read",       "H2G_GO_DBG_READ",        -1,                       dbg_read,       nullptr),
	H2G_KNOB("tail",           "H2G_FAST_TAIL",          H2G_DEFAULT_TAIL,         tail,           &h2g_stream::Tune::tail_auto),
	H2G_KNOB("align_mate",     "H2G_FAST_AM",            H2G_DEFAULT_ALIGN_MATE,   align_mate,     nullptr),
	H2G_KNOB("orphan",         "H2G_FAST_ORPHAN",        -1,                       orphan,         nullptr),
	H2G_KNOB("drain_grid",     "H2G_DRAIN_GRID",         H2G_DRAIN_GRID,           drain_grid,     nullptr),
	H2G_KNOB("mate_handover",  "H2G_FAST_MATE_HANDOVER", -1,                       mate_handover,  nullptr),
	H2G_KNOB("ps0",            "H2G_FAST_PS0",           -1,                       ps0,            nullptr),
	H2G_KNOB("fast_spliced",   "H2G_FAST_SPLICED",       H2G_DEFAULT_FAST_SPLICED, fast_spliced,   nullptr),
	H2G_KNOB("mach_total",     "H2G_MACH_TOTAL",         H2G_MACH_TOTAL,           mach_total,     &h2g_stream::Tune::mach_total_auto),
	H2G_KNOB("fast_reserve",   "H2G_FAST_RESERVE",       H2G_FAST_RESERVE_DEFAULT, fast_reserve,   nullptr),
};
#undef H2G_KNOB
// ("mstreams" / H2G_MSTREAMS and "mstreams_light" / H2G_MSTREAMS_LIGHT are the stream's own members, both clamped to the HIP streams that exist)
static unsigned clamp_mstreams(long m) { return (unsigned)(m < 1 ? 1 : m > H2G_MSTREAMS_MAX ? H2G_MSTREAMS_MAX : m); }

// A stream of this library USES 2 + S HIP streams (the fast launches', the drain launches', and the S <= H2G_MSTREAMS_MAX machine streams in rotation: 2 while the fast pass hands on little) whose kernels must be able to run side by side.  ROCclr maps HIP streams onto
// GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams that share a queue serialise — measured: four machine passes "in flight" on the
// default 4 queues ran one after the other (repeat-structured leg: 127 ms per step against 78 ms with 16 queues; profiles/r05_NOTES.md), and a machine pass or a drain launch in
// front of a fast launch on a shared queue is idle CUs (profiles/r08_mstreams.md): a context opens no more machine streams than its load needs.  The library
// does not set the variable: the number of hardware queues a process opens is the host's and the caller's choice, and results do not depend on it.

extern "C" h2g_status h2g_stream_create(h2g_index* ix, size_t max_reads, size_t max_bases, h2g_stream** out) {
	if(!ix || !out) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(ix->device));
	std::unique_ptr<h2g_stream, StreamFree> sp(new h2g_stream());      // (every early return below gives back what exists by then)
	h2g_stream* const s = sp.get();
	s->ix = ix; s->max_reads = max_reads; s->max_bases = max_bases;
	// Every HIP stream of the context is created here, in this order, whatever the rotation will be: the runtime places a stream on a hardware queue by its place among the
	// process's streams, and the place decides which launches serialise (profiles/r08_mstreams.md §2: the same two machine streams in rotation, created on first use
	// behind the drain stream, 18.4 ms per step; created here, 10.8).  A stream that never enters the rotation never runs a kernel, holds no pools and costs nothing.
	HIPCHK(s->st.create(hipStreamNonBlocking));
	for(int k = 0; k < H2G_MSTREAMS_MAX; k++) { HIPCHK(s->mst[k].create(hipStreamNonBlocking)); HIPCHK(s->mach[k].ev_rot.create(hipEventDisableTiming)); }
	HIPCHK(s->dst.create(hipStreamNonBlocking));
	HIPCHK(s->h_fast_args.ensure(2 * H2G_NBUF));
	HIPCHK(s->h_bails.ensure(H2G_NBUF)); for(int k = 0; k < H2G_NBUF; k++) s->h_bails[k] = 0;
	for(h2g_stream::RunSet& b : s->run) { HIPCHK(b.ev_fast.create(hipEventDisableTiming)); HIPCHK(b.ev_mach.create(hipEventDisableTiming)); HIPCHK(b.ev_bails.create(hipEventDisableTiming)); HIPCHK(b.ev_drain.create(hipEventDisableTiming)); }
	for(h2g_stream::FastPool& fp : s->fpool) HIPCHK(fp.ev_last.create(hipEventDisableTiming));
	for(int k = 0; k < 2; k++) HIPCHK(s->ev_dr[k].create());
	for(DevEvent& e : s->tm) HIPCHK(e.create());
	HIPCHK(s->d_counters.ensure(H2G_NBUF * H2G_CNT_BLOCK));
	HIPCHK(hipMemset(s->d_counters, 0, s->d_counters.bytes()));
	s->cnt_cur = s->d_counters;
	if(max_reads) {
		HIPCHK(s->batch[0].ensure_reads(max_reads, max_bases));
		HIPCHK(s->d_seed.ensure(max_reads * 2));
		// (a strand without coordinates leaves its `ext` entries as they are: zero, whatever block the allocator hands out — a recycled one made tests/test_gpu_frag.py's
		// seed stage differ from the oracle's zero-filled rows)
		HIPCHK(hipMemset(s->d_seed, 0, s->d_seed.bytes()));
	}
	memset(&s->last, 0, sizeof s->last);
	// the knobs: each one's default, or what its environment name says; a knob set there is no longer its policy's
	for(const Knob& k : g_knobs) {
		const char* const e = getenv(k.env);
		k.set(s->tune, e ? atol(e) : k.def);
		if(e && k.is_auto) s->tune.*k.is_auto = 0;
	}
	if(const char* const e = getenv("H2G_MSTREAMS")) s->mstreams = clamp_mstreams(atol(e));   // pinned
	if(const char* const e = getenv("H2G_MSTREAMS_LIGHT")) s->mstreams_light = clamp_mstreams(atol(e));
	*out = sp.release();
	return H2G_OK;
}

extern "C" void h2g_stream_free(h2g_stream* s) { delete s; }      // (~h2g_stream waits for everything queued; the handles give the rest back)

// the machine streams, when one may hold work (st2_busy): waits for every one of them, then clears the flag
static hipError_t sync_mach(h2g_stream* s) {
	if(!s->st2_busy) return hipSuccess;
	for(unsigned k = 0; k < s->n_mst; k++) { const hipError_t e = hipStreamSynchronize(s->mst[k]); if(e != hipSuccess) return e; }
	s->st2_busy = false;
	return hipSuccess;
}
// every stream of a batch context
static hipError_t sync_all(h2g_stream* s) {
	hipError_t e = hipStreamSynchronize(s->st);
	if(e == hipSuccess && s->dst_busy) { e = hipStreamSynchronize(s->dst); s->dst_busy = false; }
	if(e == hipSuccess && s->st2_busy) { e = sync_mach(s); s->st2_busy = false; }   // (the flag goes even when a wait fails)
	return e;
}
extern "C" void* h2g_stream_hip(h2g_stream* s) { return s ? (void*)s->st : nullptr; }
extern "C" h2g_status h2g_stream_sync(h2g_stream* s) {
	if(!s) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	return H2G_OK;
}

// Selects resident batch k: the h2g_set_* calls that follow fill it, the runs that follow work on it and write its rows, the fetches read them.  Nothing waits: runs queued
// over other batches go on.
extern "C" h2g_status h2g_stream_select_batch(h2g_stream* s, unsigned k) {
	if(!s || k >= H2G_MAX_BATCHES) return H2G_ERR_ARG;
	if(k == s->cur_batch) return H2G_OK;
	HIPCHK(hipSetDevice(s->ix->device));
	const BatchCtx& out = s->cur();
	BatchCtx& in = s->batch[k];
	if(s->max_reads) HIPCHK(in.ensure_reads(s->max_reads, s->max_bases));      // first use: the read buffers h2g_stream_create gives batch 0
	// ... and result rows as large as the rows of the batch that is leaving (the option set a streaming caller runs every batch with): a batch's first run then
	// allocates nothing — an allocation of gigabytes in the middle of a queue of runs waits for all of them.  Every buffer knows what it holds, and each block is entered
	// while its last buffer is missing: a call that failed half way is completed by the next one (or by the batch's first run, go_rows).
	if(!in.d_paln[1] && out.d_pout && out.d_paln[1]) {
		HIPCHK(in.d_pout.ensure(s->max_reads));
		for(int m = 0; m < 2; m++) HIPCHK(in.d_paln[m].reserve(out.d_paln[m].size()));
		in.pair_slots = out.pair_slots;
		// (written once here: the first kernel to store into fresh device memory pays for its mapping — measured in bench.py's loop, lease F: 20 timed steps over 10 batches
		// of which 5 had never been run took 18.5 ms each, 60 steps 12.1)
		HIPCHK(hipMemsetAsync(in.d_pout, 0, in.d_pout.bytes(), s->st));
		for(int m = 0; m < 2; m++) HIPCHK(hipMemsetAsync(in.d_paln[m], 0, in.d_paln[m].bytes(), s->st));
	}
	if(!in.d_aln && out.d_rout && out.d_aln) {
		HIPCHK(in.d_rout.ensure(s->max_reads));
		HIPCHK(in.d_aln.reserve(out.d_aln.size()));
		in.aln_slots = out.aln_slots;
		HIPCHK(hipMemsetAsync(in.d_rout, 0, in.d_rout.bytes(), s->st));
		HIPCHK(hipMemsetAsync(in.d_aln, 0, in.d_aln.bytes(), s->st));
	}
	s->cur_batch = k;
	s->tmp_gen++;
	return H2G_OK;
}

// scratch slot `slot` of the stream with room for `bytes` (and 256 beyond: the largest request so far)
static int tmp_buf(h2g_stream* s, int slot, size_t bytes, void** out) {
	s->tmp_gen++;                                                            // (whatever a compact fetch left here is about to be overwritten)
	const hipError_t e = s->d_tmp[slot].reserve(bytes + 256);
	*out = s->d_tmp[slot];
	return e == hipSuccess ? H2G_OK : set_err("tmp_buf", e);
}

extern "C" h2g_status h2g_set_reads(h2g_stream* s, const uint8_t* codes, const uint32_t* offs, const char* quals, size_t n) {
	if(s) HIPCHK(sync_all(s));        // (a machine pass of the previous batch may still read the buffers this call replaces)
	if(!s || !codes || !offs || n > s->max_reads) return H2G_ERR_ARG;
	s->tmp_gen++;
	BatchCtx& B = s->cur();
	size_t nb = offs[n];
	if(nb > s->max_bases) return H2G_ERR_ARG;
	uint32_t mx = 0;
	for(size_t i = 0; i < n; i++) { const uint32_t l = offs[i + 1] - offs[i]; if(l > mx) mx = l; }
	B.max_read_len = mx;
	HIPCHK(hipMemcpyAsync(B.d_codes, codes, nb, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(B.d_offs, offs, (n + 1) * 4, hipMemcpyHostToDevice, s->st));
	B.has_quals = quals != nullptr;
	if(quals) HIPCHK(hipMemcpyAsync(B.d_quals, quals, nb, hipMemcpyHostToDevice, s->st));
	HIPCHK(sync_all(s));
	B.n_reads = n;
	B.has_names = false;
	B.has_mates = false;
	B.has_seeds = B.has_seeds2 = false;
	B.has_qc = false;
	B.has_ids = false;
	s->ledits_touched = 0;            // (long-edit lists of the batch this one replaces are nobody's any more)
	return H2G_OK;
}

static DReads dreads(const h2g_stream* s) {
	DReads r;
	r.codes = s->cur().d_codes; r.offs = s->cur().d_offs; r.quals = s->cur().has_quals ? s->cur().d_quals : nullptr; r.n = (uint32_t)s->cur().n_reads;
	return r;
}

static unsigned grid_for(size_t n, unsigned block) {
	size_t g = (n + block - 1) / block;
	const size_t cap = 256 * 16;   // >= 8 resident blocks per CU plus slack; grid-stride above that
	return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ------------------------------------------------------------------------------------------ rank kernels
// variant 0: one lane per query, 4 x dwordx4 per side
// The row of a synthetic query: the high word of the hash scaled into [0, gbwtLen) — ONE v_mul_hi.  Through round 6 this was `h % gbwtLen`: a 64-bit modulo, ~45 vector and ~55 scalar
// instructions per query next to the rank's own ~120 — the micro-benchmark was measuring its own generator (issue time 3.3 of its 5.8 ms: that, not the request pattern, was the gap to the
// chain kernel's 3.5 TB/s).  tests/rank_synth_check.py draws the same rows on the host.
__device__ __forceinline__ uint32_t synth_row(uint64_t h, uint32_t n) { return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32); }
__global__ __launch_bounds__(256) void k_rank_v0(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out,
                                                 size_t n, uint64_t seed, int synth)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		uint32_t row; int c;
		if(synth) { uint64_t h = splitmix64(seed + i); row = synth_row(h, g.gbwtLen); c = (int)((h >> 40) & 3); }
		else { row = rows[i]; c = cs[i]; }
		out[i] = rank64(g, row, c);
	}
}

__global__ __launch_bounds__(512) void k_rank_v0_512(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out, size_t n, uint64_t seed, int synth)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		uint32_t row; int c;
		if(synth) { uint64_t h = splitmix64(seed + i); row = synth_row(h, g.gbwtLen); c = (int)((h >> 40) & 3); }
		else { row = rows[i]; c = cs[i]; }
		out[i] = rank64(g, row, c);
	}
}

// variant 10: variant 0 without the OUTPUT STREAM (round 6).  In the aligner a rank feeds the next step of its own chain; the 4 bytes per query the micro-benchmark writes
// are its own artefact (2^28 queries: 1 GB of stores next to 17 GB of side lines).  Here every result goes into the run's checksum (the k_checksum function of the full
// output, so the two variants must agree) and every 256th is stored — the samples the comparison with the CPU's mapLF reads.
__global__ __launch_bounds__(256) void k_rank_v0_sampled(DGfm g, uint32_t* out, size_t n, uint64_t seed, unsigned long long* sum)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	unsigned long long acc = 0;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		const uint64_t h = splitmix64(seed + i);
		const uint32_t r = rank64(g, synth_row(h, g.gbwtLen), (int)((h >> 40) & 3));
		if((i & 255) == 0) out[i] = r;
		acc += (unsigned long long)r * (unsigned long long)((i & 1023) + 1);
	}
	for(int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

// variant 1: four lanes per side — one dwordx4 per lane => one fully coalesced 64 B request per query;
// lanes 0-2 popcount two payload words each, lane 3 holds the four Occ words; 2-step butterfly reduce.
template <int UNROLL>
__global__ __launch_bounds__(256) void k_rank_v1(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out,
                                                 size_t n, uint64_t seed, int synth)
{
	const unsigned lane = threadIdx.x & 63, sub = lane & 3;
	const size_t ngroups = ((size_t)gridDim.x * blockDim.x) >> 2;
	const size_t gid = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 2;
	for(size_t base = gid * UNROLL; base < n; base += ngroups * UNROLL) {
		uint32_t row[UNROLL], sideNum[UNROLL], charOff[UNROLL]; int c[UNROLL]; uint4 v[UNROLL];
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			size_t i = base + u;
			bool ok = i < n;
			if(synth) { uint64_t h = splitmix64(seed + (ok ? i : 0)); row[u] = synth_row(h, g.gbwtLen); c[u] = (int)((h >> 40) & 3); }
			else { row[u] = ok ? rows[i] : 0; c[u] = ok ? cs[i] : 0; }
			sideNum[u] = row[u] / 192u; charOff[u] = row[u] - sideNum[u] * 192u;
			v[u] = reinterpret_cast<const uint4*>(g.sides + (size_t)sideNum[u] * 64)[sub];
		}
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			uint64_t w0 = v[u].x | ((uint64_t)v[u].y << 32), w1 = v[u].z | ((uint64_t)v[u].w << 32);
			int n0 = (int)charOff[u] - 64 * (int)sub;
			uint32_t cnt = sub < 3 ? count_word(w0, c[u], n0) + count_word(w1, c[u], n0 - 32) : 0u;
			uint32_t occsel = c[u] == 0 ? v[u].x : c[u] == 1 ? v[u].y : c[u] == 2 ? v[u].z : v[u].w;
			uint32_t part = sub == 3 ? occsel : cnt;
			part += __shfl_xor(part, 1);
			part += __shfl_xor(part, 2);
			if(c[u] == 0 && g.nZ) {
				uint32_t zs = g.zoff / 192u, zc = g.zoff - zs * 192u;
				if(zs == sideNum[u] && zc < charOff[u]) part--;
			}
			if(sub == 0 && base + u < n) out[base + u] = part + (c[u] == 0 ? g.fchr[0] : c[u] == 1 ? g.fchr[1] : c[u] == 2 ? g.fchr[2] : g.fchr[3]);
		}
	}
}

// variant 2: eight lanes per side, one u64 per lane
template <int UNROLL>
__global__ __launch_bounds__(256) void k_rank_v2(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out,
                                                 size_t n, uint64_t seed, int synth)
{
	const unsigned lane = threadIdx.x & 63, sub = lane & 7;
	const size_t ngroups = ((size_t)gridDim.x * blockDim.x) >> 3;
	const size_t gid = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 3;
	for(size_t base = gid * UNROLL; base < n; base += ngroups * UNROLL) {
		uint32_t row[UNROLL], sideNum[UNROLL], charOff[UNROLL]; int c[UNROLL]; uint64_t w[UNROLL];
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			size_t i = base + u;
			bool ok = i < n;
			if(synth) { uint64_t h = splitmix64(seed + (ok ? i : 0)); row[u] = synth_row(h, g.gbwtLen); c[u] = (int)((h >> 40) & 3); }
			else { row[u] = ok ? rows[i] : 0; c[u] = ok ? cs[i] : 0; }
			sideNum[u] = row[u] / 192u; charOff[u] = row[u] - sideNum[u] * 192u;
			w[u] = reinterpret_cast<const uint64_t*>(g.sides + (size_t)sideNum[u] * 64)[sub];
		}
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			uint32_t cnt = sub < 6 ? count_word(w[u], c[u], (int)charOff[u] - 32 * (int)sub) : 0u;
			uint32_t occ = (sub == 6 + (unsigned)(c[u] >> 1)) ? (uint32_t)(w[u] >> ((c[u] & 1) * 32)) : 0u;
			uint32_t part = cnt + occ;
			part += __shfl_xor(part, 1);
			part += __shfl_xor(part, 2);
			part += __shfl_xor(part, 4);
			if(c[u] == 0 && g.nZ) {
				uint32_t zs = g.zoff / 192u, zc = g.zoff - zs * 192u;
				if(zs == sideNum[u] && zc < charOff[u]) part--;
			}
			if(sub == 0 && base + u < n) out[base + u] = part + (c[u] == 0 ? g.fchr[0] : c[u] == 1 ? g.fchr[1] : c[u] == 2 ? g.fchr[2] : g.fchr[3]);
		}
	}
}

// ---- measurement-only variants (same results as variant 0; they probe the memory system) ----
// 3: also loads the partner half of the 128 B line (is the fetch unit 64 B or 128 B?)
// 4: nontemporal loads (no L2/MALL allocation)       5: two independent queries in flight per lane
template <int MODE>
__global__ __launch_bounds__(256) void k_rank_exp(DGfm g, uint32_t* out, size_t n, uint64_t seed) {
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride * (MODE == 5 ? 2 : 1)) {
		uint64_t h = splitmix64(seed + i);
		uint32_t row = synth_row(h, g.gbwtLen); int c = (int)((h >> 40) & 3);
		if(MODE == 3) {
			uint32_t sideNum = row / 192u;
			const uint4* q = reinterpret_cast<const uint4*>(g.sides + (size_t)(sideNum ^ 1u) * 64);
			uint4 x = q[0];
			asm volatile("" :: "v"(x.x), "v"(x.y), "v"(x.z), "v"(x.w));
			out[i] = rank64(g, row, c);
		} else if(MODE == 4) {
			uint32_t sideNum = row / 192u, charOff = row - sideNum * 192u;
			const uint64_t* q = reinterpret_cast<const uint64_t*>(g.sides + (size_t)sideNum * 64);
			Side64 s;
#pragma unroll
			for(int k = 0; k < 8; k++) s.w[k] = __builtin_nontemporal_load(q + k);
			out[i] = rank_in_side64(g, s, sideNum, charOff, c);
		} else {
			size_t j = i + stride;
			uint64_t h2 = splitmix64(seed + (j < n ? j : i));
			uint32_t row2 = synth_row(h2, g.gbwtLen); int c2 = (int)((h2 >> 40) & 3);
			uint32_t s1 = row / 192u, s2 = row2 / 192u;
			Side64 a = load_side64(g.sides + (size_t)s1 * 64), b = load_side64(g.sides + (size_t)s2 * 64);
			out[i] = rank_in_side64(g, a, s1, row - s1 * 192u, c);
			if(j < n) out[j] = rank_in_side64(g, b, s2, row2 - s2 * 192u, c2);
		}
	}
}

// ---- graph sides (128 B = one L2 line) --------------------------------------------------------------------
// g0: one lane per query, 8 x dwordx4
__global__ __launch_bounds__(256) void k_rank_g0(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out,
                                                 size_t n, uint64_t seed, int synth)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		uint32_t row; int c;
		if(synth) { uint64_t h = splitmix64(seed + i); row = synth_row(h, g.gbwtLen); c = (int)((h >> 40) & 3); }
		else { row = rows[i]; c = cs[i]; }
		out[i] = rank128(g, row, c);
	}
}
// g1: eight lanes per side, one dwordx4 each => one fully coalesced 128 B request per query.  Lanes 0..3 hold
// the symbols (lane 3 only 16 of them), lane 7 the Occ words; 3-step butterfly reduce within the 8-lane group.
template <int UNROLL>
__global__ __launch_bounds__(256) void k_rank_g1(DGfm g, const uint32_t* rows, const uint8_t* cs, uint32_t* out,
                                                 size_t n, uint64_t seed, int synth)
{
	const uint32_t lane = threadIdx.x & 63, sub = lane & 7, grp = lane >> 3;
	const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
	for(size_t base = wave * 8 * UNROLL; base < n; base += nwaves * 8 * UNROLL) {
		uint4 v[UNROLL]; uint32_t off[UNROLL], sn[UNROLL]; int cc[UNROLL]; bool ok[UNROLL];
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			const size_t i = base + (size_t)u * 8 + grp;
			ok[u] = i < n;
			uint32_t row = 0; int c = 0;
			if(ok[u]) {
				if(synth) { uint64_t h = splitmix64(seed + i); row = synth_row(h, g.gbwtLen); c = (int)((h >> 40) & 3); }
				else { row = rows[i]; c = cs[i]; }
			}
			sn[u] = row / H2G_GSIDE_SYMS; off[u] = row - sn[u] * H2G_GSIDE_SYMS; cc[u] = c;
			v[u] = reinterpret_cast<const uint4*>(g.sides + (size_t)sn[u] * 128)[sub];
		}
#pragma unroll
		for(int u = 0; u < UNROLL; u++) {
			const uint64_t w0 = v[u].x | ((uint64_t)v[u].y << 32), w1 = v[u].z | ((uint64_t)v[u].w << 32);
			const int c = cc[u];
			uint32_t cnt = 0;
			if(sub < 3) cnt = count_word(w0, c, (int)off[u] - 64 * (int)sub) + count_word(w1, c, (int)off[u] - 64 * (int)sub - 32);
			else if(sub == 3) cnt = count_word(w0 & 0xffffffffull, c, (int)off[u] - 192 > 16 ? 16 : (int)off[u] - 192);
			else if(sub == 7) {
				const uint64_t ow = (c & 2) ? w1 : w0;
				cnt = (c & 1) ? (uint32_t)(ow >> 32) : (uint32_t)ow;
			}
			cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4);
			if(sub == 0 && ok[u]) {
				if(c == 0 && g.nZ) {
					const uint32_t zs = g.zoff / H2G_GSIDE_SYMS, zc = g.zoff - zs * H2G_GSIDE_SYMS;
					if(zs == sn[u] && zc < off[u]) cnt--;
				}
				const uint32_t fc = c == 0 ? g.fchr[0] : c == 1 ? g.fchr[1] : c == 2 ? g.fchr[2] : g.fchr[3];
				out[base + (size_t)u * 8 + grp] = cnt + fc;
			}
		}
	}
}

__global__ void k_checksum(const uint32_t* v, size_t n, unsigned long long* out) {
	unsigned long long acc = 0;
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride)
		acc += (unsigned long long)v[i] * (unsigned long long)((i & 1023) + 1);
	for(int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

static int launch_rank(h2g_stream* s, const uint32_t* d_rows, const uint8_t* d_cs, uint32_t* d_out, size_t n,
                       uint64_t seed, int synth, int variant, int repeats, float* ms)
{
	const DGfm& g = s->ix->dg;
	const bool graph = !g.linear && g.lineRate == 7;
	if(!graph && (!g.linear || g.lineRate != 6)) { snprintf(g_err, sizeof g_err, "rank kernels: 64 B linear or 128 B graph sides only"); return H2G_ERR_UNSUPPORTED; }
	if(graph && g.nZ > 1 && variant == 1) variant = 0;   // the cooperative kernel handles a single '$' row
	if(repeats < 1) repeats = 1;
	HIPCHK(hipEventRecord(s->tm[TM_PRIM0], s->st));
	for(int r = 0; r < repeats; r++) {
		if(graph) {
			if(variant == 0) hipLaunchKernelGGL(k_rank_g0, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
			else if(variant == 1) hipLaunchKernelGGL(k_rank_g1<4>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
			else return H2G_ERR_ARG;
		} else if(variant == 0) {
			hipLaunchKernelGGL(k_rank_v0, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
		} else if(variant == 1) {
			hipLaunchKernelGGL(k_rank_v1<4>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
		} else if(variant == 2) {
			hipLaunchKernelGGL(k_rank_v2<4>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
		} else if(variant == 3 && synth) {
			hipLaunchKernelGGL(k_rank_exp<3>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_out, n, seed);
		} else if(variant == 4 && synth) {
			hipLaunchKernelGGL(k_rank_exp<4>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_out, n, seed);
		} else if(variant == 5 && synth) {
			hipLaunchKernelGGL(k_rank_exp<5>, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_out, n, seed);
		} else if(variant == 10 && synth) {
			HIPCHK(hipMemsetAsync(s->d_counters + H2G_CNT_BENCH_SUM, 0, 8, s->st));
			hipLaunchKernelGGL(k_rank_v0_sampled, dim3(grid_for(n, 256)), dim3(256), 0, s->st, g, d_out, n, seed, s->d_counters + H2G_CNT_BENCH_SUM);
		} else if(variant == 11 || variant == 12) {
			// variant 0's loop in the chain kernel's geometry: ONE 512-thread workgroup per CU (11), two (12)
			hipLaunchKernelGGL(k_rank_v0_512, dim3(variant == 11 ? 256u : 512u), dim3(512), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
		} else if(variant >= 6 && variant <= 9) {
			// variant 0's kernel at a fraction of the chip's occupancy (measurement: the chain kernel sustains more random 64 B requests per second at one 512-thread
			// workgroup per CU than at full occupancy — profiles/r05_NOTES.md): 6: 16 waves per CU, 7: 8, 8: 4, 9: 2
			const unsigned blocks = variant == 6 ? 1024u : variant == 7 ? 512u : variant == 8 ? 256u : 128u;
			hipLaunchKernelGGL(k_rank_v0, dim3(blocks), dim3(256), 0, s->st, g, d_rows, d_cs, d_out, n, seed, synth);
		} else return H2G_ERR_ARG;
	}
	HIPCHK(hipEventRecord(s->tm[TM_PRIM1], s->st));
	HIPCHK(sync_all(s));
	HIPCHK(hipGetLastError());
	float t = 0;
	HIPCHK(hipEventElapsedTime(&t, s->tm[TM_PRIM0], s->tm[TM_PRIM1]));
	s->last.ms_rank = t / repeats;
	if(ms) *ms = t / repeats;
	return H2G_OK;
}

extern "C" h2g_status h2g_rank_bench(h2g_stream* s, const uint32_t* rows, const uint8_t* cs, size_t n, uint32_t* out,
                                     int variant, int device_ptrs, int repeats, float* kernel_ms)
{
	if(!s || !rows || !cs || !out || n == 0) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	if(device_ptrs) return launch_rank(s, rows, cs, out, n, 0, 0, variant, repeats, kernel_ms);
	void *dr, *dc, *dout;
	int rc;
	if((rc = tmp_buf(s, 0, n * 4, &dr)) || (rc = tmp_buf(s, 1, n, &dc)) || (rc = tmp_buf(s, 2, n * 4, &dout))) return rc;
	HIPCHK(hipMemcpyAsync(dr, rows, n * 4, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(dc, cs, n, hipMemcpyHostToDevice, s->st));
	rc = launch_rank(s, (const uint32_t*)dr, (const uint8_t*)dc, (uint32_t*)dout, n, 0, 0, variant, repeats, kernel_ms);
	if(rc) return rc;
	HIPCHK(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost));
	return H2G_OK;
}

extern "C" h2g_status h2g_rank_bench_synth(h2g_stream* s, size_t n, uint64_t seed, int variant, int repeats,
                                           float* kernel_ms, uint64_t* checksum)
{
	if(!s || n == 0) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	void* dout;
	int rc;
	if((rc = tmp_buf(s, 2, n * 4, &dout))) return rc;
	rc = launch_rank(s, nullptr, nullptr, (uint32_t*)dout, n, seed, 1, variant, repeats, kernel_ms);
	if(rc) return rc;
	if(checksum) {
		HIPCHK(hipMemsetAsync(s->d_counters + H2G_CNT_BENCH_CHECKSUM, 0, 8, s->st));
		if(variant != 10) hipLaunchKernelGGL(k_checksum, dim3(1024), dim3(256), 0, s->st, (const uint32_t*)dout, n, s->d_counters + H2G_CNT_BENCH_CHECKSUM);
		unsigned long long v = 0;
		HIPCHK(hipMemcpyAsync(&v, s->d_counters + (variant == 10 ? H2G_CNT_BENCH_SUM : H2G_CNT_BENCH_CHECKSUM), 8, hipMemcpyDeviceToHost, s->st));   // (variant 10 sums on the fly: the last repeat's)
		HIPCHK(sync_all(s));
		*checksum = v;
	}
	return H2G_OK;
}

// ---- chains of dependent rank queries (measurement only: tools/chain_bench.py) ----------------------------------------
// What the search loops of go() are made of is not a stream of independent rank queries (k_rank_*) but CHAINS: the row of step i + 1 comes out of
// the rank of step i.  This kernel runs C independent chains per lane — chain k of lane t starts at splitmix64(seed + t * C + k) and walks
// row' = splitmix64(rank << 32 | row) % gbwtLen — so that one can measure, at the occupancy of the compact-state pass (512-thread workgroups, one per
// CU: `lds_bytes` of dynamic LDS bound them the same way the pass's staging area does), what several chains in flight per lane are worth against the
// same number of chains spread over more lanes.  The sum of out[] depends only on (seed, number of chains, steps).
template <int C, bool GRAPH>
__global__ __launch_bounds__(512) void k_rank_chain(DGfm g, uint64_t seed, int steps, size_t nlanes, unsigned long long* sum)
{
	extern __shared__ uint32_t chain_pad[];
	const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	unsigned long long acc = 0;
	if(t < nlanes) {
		uint32_t row[C]; int c[C];
#pragma unroll
		for(int k = 0; k < C; k++) { const uint64_t h = splitmix64(seed + t * C + k); row[k] = (uint32_t)(h % g.gbwtLen); c[k] = (int)((h >> 40) & 3); }
		for(int i = 0; i < steps; i++) {
			// every chain's side is requested before any of them is counted (the counting has data-dependent branches: left to itself the compiler
			// finishes chain k before it issues chain k + 1's loads)
			uint32_t r[C], sn[C], co[C];
			if constexpr(GRAPH) {
				Side128 sd[C];
#pragma unroll
				for(int k = 0; k < C; k++) { sn[k] = row[k] / DGfm::SYMS; co[k] = row[k] - sn[k] * DGfm::SYMS; sd[k] = load_side128(g.sides + (size_t)sn[k] * 128); }
#pragma unroll
				for(int k = 0; k < C; k++) r[k] = rank_in_side128(g, sd[k], sn[k], co[k], c[k]);
			} else {
				Side64 sd[C];
#pragma unroll
				for(int k = 0; k < C; k++) { sn[k] = row[k] / 192u; co[k] = row[k] - sn[k] * 192u; sd[k] = load_side64(g.sides + (size_t)sn[k] * 64); }
#pragma unroll
				for(int k = 0; k < C; k++) r[k] = rank_in_side64(g, sd[k], sn[k], co[k], c[k]);
			}
#pragma unroll
			for(int k = 0; k < C; k++) {
				const uint64_t h = splitmix64(((uint64_t)r[k] << 32) | row[k]);
				row[k] = (uint32_t)(h % g.gbwtLen); c[k] = (int)((h >> 40) & 3);
				acc += r[k];
			}
		}
	}
	if(threadIdx.x == 0 && steps < 0) chain_pad[0] = (uint32_t)acc;   // (keeps the dynamic allocation alive; never taken)
	for(int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

// nchains chains of `steps` dependent rank queries, chains_per_lane (1, 2, 4 or 8) of them in each lane, workgroups of `block` threads (64..512) with
// `lds_bytes` of dynamic LDS each.  *checksum = the sum of all rank results (the same for every chains_per_lane at equal seed, nchains and steps).
// out[j] = result j * stride of the LAST h2g_rank_bench_synth run of this stream (its device buffer is still there): what a sampled comparison with the
// CPU's mapLF needs of a 2^28-query run
extern "C" h2g_status h2g_rank_bench_synth_sample(h2g_stream* s, size_t stride, size_t nsample, uint32_t* out) {
	if(!s || !out || stride == 0 || nsample == 0 || s->d_tmp[2].size() < ((nsample - 1) * stride + 1) * 4) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(sync_all(s));
	HIPCHK(hipMemcpy2D(out, 4, s->d_tmp[2], stride * 4, 4, nsample, hipMemcpyDeviceToHost));
	return H2G_OK;
}
extern "C" H2G_EXPORT h2g_status h2g_rank_chain_bench(h2g_stream* s, size_t nchains, int chains_per_lane, int steps, int block, int lds_bytes, uint64_t seed,
                                                      int repeats, float* kernel_ms, uint64_t* checksum)
{
	if(!s || nchains == 0 || steps < 1 || block < 64 || block > 512 || (block & 63) || lds_bytes < 0 || lds_bytes > 160 * 1024) return H2G_ERR_ARG;
	if(chains_per_lane != 1 && chains_per_lane != 2 && chains_per_lane != 4 && chains_per_lane != 8) return H2G_ERR_ARG;
	if(nchains % (size_t)chains_per_lane) return H2G_ERR_ARG;
	const DGfm& g = s->ix->dg;
	const bool graph = !g.linear && g.lineRate == 7;
	if(!graph && (!g.linear || g.lineRate != 6)) { snprintf(g_err, sizeof g_err, "rank kernels: 64 B linear or 128 B graph sides only"); return H2G_ERR_UNSUPPORTED; }
	HIPCHK(hipSetDevice(s->ix->device));
	const size_t nlanes = nchains / (size_t)chains_per_lane;
	const unsigned grid = (unsigned)((nlanes + (size_t)block - 1) / (size_t)block);
	if(repeats < 1) repeats = 1;
	const void* fn = nullptr;
#define H2G_CHAIN_CASE(CC) case CC: fn = graph ? (const void*)k_rank_chain<CC, true> : (const void*)k_rank_chain<CC, false>; break;
	switch(chains_per_lane) { H2G_CHAIN_CASE(1) H2G_CHAIN_CASE(2) H2G_CHAIN_CASE(4) H2G_CHAIN_CASE(8) }
#undef H2G_CHAIN_CASE
	if(lds_bytes > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) (void)hipGetLastError();
	unsigned long long* dsum = s->d_counters + H2G_CNT_BENCH_CHECKSUM;
	HIPCHK(hipEventRecord(s->tm[TM_PRIM0], s->st));
	for(int r = 0; r < repeats; r++) {
		HIPCHK(hipMemsetAsync(dsum, 0, 8, s->st));
		void* args[] = {(void*)&g, (void*)&seed, (void*)&steps, (void*)&nlanes, (void*)&dsum};
		HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3((unsigned)block), args, (size_t)lds_bytes, s->st));
	}
	HIPCHK(hipEventRecord(s->tm[TM_PRIM1], s->st));
	unsigned long long v = 0;
	HIPCHK(hipMemcpyAsync(&v, dsum, 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	HIPCHK(hipGetLastError());
	float t = 0;
	HIPCHK(hipEventElapsedTime(&t, s->tm[TM_PRIM0], s->tm[TM_PRIM1]));
	if(kernel_ms) *kernel_ms = t / repeats;
	if(checksum) *checksum = v;
	return H2G_OK;
}

// The same for whole graph LF steps on a REAL graph index (glf1_top_fused: the step of a coordinate walk — rank, rank_M, select_F: two or three dependent
// 128 B lines): C walks per lane, either one after the other (staged = 0: what a lane of the pass does today, C times) or stage by stage over all C
// (h2g_graph_staged.h: every walk's next line is requested before any of them is consumed).  A walk that runs into a '$' row starts over somewhere else.
template <int C>
__global__ __launch_bounds__(512) void k_glf_chain(DGfm g, uint64_t seed, int steps, size_t nlanes, int staged, unsigned long long* sum)
{
	extern __shared__ uint32_t chain_pad[];
	const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	unsigned long long acc = 0;
	if(t < nlanes) {
		uint32_t row[C];
#pragma unroll
		for(int k = 0; k < C; k++) { uint64_t h = splitmix64(seed + t * C + k); row[k] = (uint32_t)(h % g.gbwtLen); while(is_zoff(g, row[k])) { h = splitmix64(h); row[k] = (uint32_t)(h % g.gbwtLen); } }
		for(int i = 0; i < steps; i++) {
			uint32_t top[C], node[C];
			if(staged) {
				GlfStage st[C];
#pragma unroll
				for(int k = 0; k < C; k++) glf_stage_a(g, row[k], st[k]);
#pragma unroll
				for(int k = 0; k < C; k++) glf_stage_b(g, st[k]);
#pragma unroll
				for(int k = 0; k < C; k++) glf_stage_c(g, st[k]);
#pragma unroll
				for(int k = 0; k < C; k++) glf_stage_d(g, st[k], &top[k], &node[k]);
			} else {
#pragma unroll
				for(int k = 0; k < C; k++) glf1_top_fused(g, row[k], &top[k], &node[k]);
			}
#pragma unroll
			for(int k = 0; k < C; k++) {
				acc += (unsigned long long)top[k] + node[k];
				uint32_t nr = top[k];
				if(nr >= g.gbwtLen || is_zoff(g, nr)) { uint64_t h = splitmix64(((uint64_t)top[k] << 32) | row[k]); nr = (uint32_t)(h % g.gbwtLen); while(is_zoff(g, nr)) { h = splitmix64(h); nr = (uint32_t)(h % g.gbwtLen); } }
				row[k] = nr;
			}
		}
	}
	if(threadIdx.x == 0 && steps < 0) chain_pad[0] = (uint32_t)acc;
	for(int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
	if((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

extern "C" H2G_EXPORT h2g_status h2g_glf_chain_bench(h2g_stream* s, size_t nchains, int chains_per_lane, int steps, int block, int lds_bytes, uint64_t seed,
                                                     int staged, int repeats, float* kernel_ms, uint64_t* checksum)
{
	if(!s || nchains == 0 || steps < 1 || block < 64 || block > 512 || (block & 63) || lds_bytes < 0 || lds_bytes > 160 * 1024) return H2G_ERR_ARG;
	if(chains_per_lane != 1 && chains_per_lane != 2 && chains_per_lane != 4) return H2G_ERR_ARG;
	if(nchains % (size_t)chains_per_lane) return H2G_ERR_ARG;
	if(s->ix->synthetic || s->ix->dg.linear || s->ix->dg.lineRate != 7) { snprintf(g_err, sizeof g_err, "h2g_glf_chain_bench: needs a real graph (GFM, 128 B side) index"); return H2G_ERR_ARG; }
	const DGfm& g = s->ix->dg;
	HIPCHK(hipSetDevice(s->ix->device));
	const size_t nlanes = nchains / (size_t)chains_per_lane;
	const unsigned grid = (unsigned)((nlanes + (size_t)block - 1) / (size_t)block);
	if(repeats < 1) repeats = 1;
	const void* fn = chains_per_lane == 1 ? (const void*)k_glf_chain<1> : chains_per_lane == 2 ? (const void*)k_glf_chain<2> : (const void*)k_glf_chain<4>;
	if(lds_bytes > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) (void)hipGetLastError();
	unsigned long long* dsum = s->d_counters + H2G_CNT_BENCH_CHECKSUM;
	HIPCHK(hipEventRecord(s->tm[TM_PRIM0], s->st));
	for(int r = 0; r < repeats; r++) {
		HIPCHK(hipMemsetAsync(dsum, 0, 8, s->st));
		void* args[] = {(void*)&g, (void*)&seed, (void*)&steps, (void*)&nlanes, (void*)&staged, (void*)&dsum};
		HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3((unsigned)block), args, (size_t)lds_bytes, s->st));
	}
	HIPCHK(hipEventRecord(s->tm[TM_PRIM1], s->st));
	unsigned long long v = 0;
	HIPCHK(hipMemcpyAsync(&v, dsum, 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	HIPCHK(hipGetLastError());
	float t = 0;
	HIPCHK(hipEventElapsedTime(&t, s->tm[TM_PRIM0], s->tm[TM_PRIM1]));
	if(kernel_ms) *kernel_ms = t / repeats;
	if(checksum) *checksum = v;
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ primitive kernels
__global__ __launch_bounds__(256) void k_fm_search(DGfm g, DReads rd, const h2g_fm_query* q, size_t n, uint32_t khits,
                                                   h2g_fm_hit* out)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		h2g_fm_query qq = q[i];
		SeqView sv = seq_view(rd, qq.read, qq.fw != 0);
		partial_search_item(g, sv, qq.offset, qq.pseudogeneStop != 0, qq.anchorStop != 0, khits, &out[i]);
	}
}

__global__ __launch_bounds__(256) void k_sa_resolve(DGfm g, const h2g_sa_query* q, size_t n, uint32_t cap, h2g_coord* coords,
                                                    h2g_sa_result* res)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		h2g_sa_query qq = q[i];
		genome_coords_item(g, qq.top, qq.bot, qq.maxelt, qq.len, qq.rejectStraddle != 0, coords + i * cap, cap, &res[i]);
	}
}

__global__ __launch_bounds__(256) void k_extend(DRef ref, DReads rd, DScoring sc, h2g_ghit* hits, const h2g_ext_args* args,
                                                size_t n, h2g_ext_result* res)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		h2g_ghit* h = &hits[i];
		SeqView sv = seq_view(rd, h->read, h->fw != 0);
		uint32_t le = 0, re = 0;
		bool ext = extend_item(ref, sc, sv, h, args[i].mm, args[i].max_leftext, args[i].max_rightext, &le, &re);
		res[i].extended = ext; res[i].leftext = le; res[i].rightext = re;
	}
}

// graph index: GenomeHit::extend through the ALT database (known SNPs / insertions / deletions)
__global__ __launch_bounds__(256) void k_extend_alts(DRef ref, DAlts alts, DReads rd, DScoring sc, h2g_ghit* hits, const h2g_ext_args* args,
                                                     size_t n, h2g_ext_result* res, AwaWS* scratch)
{
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	AwaWS* W = scratch + tid;
	for(size_t i = tid; i < n; i += stride) {
		h2g_ghit* h = &hits[i];
		SeqView sv = seq_view(rd, h->read, h->fw != 0);
		uint32_t le = 0, re = 0;
		bool ext = extend_item_alts(ref, alts, sc, sv, h, args[i].mm, args[i].max_leftext, args[i].max_rightext, &le, &re, W);
		res[i].extended = ext; res[i].leftext = le; res[i].rightext = re;
	}
}

// GenomeHit::combineWith (hi_aligner.h:1420-2025) per lane: a[i] <- a[i] + b[i] (hit_combine of h2g_align.h, the function OP_COMBINE / FOP_COMBINE run inside go())
__global__ __launch_bounds__(256) void k_combine(DRef ref, DAlts alts, DReads rd, AlnParams P, h2g_ghit* a, const h2g_ghit* b, const int64_t* minsc, size_t n, uint32_t* ok, int64_t* scratch)
{
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	int64_t* const t1 = scratch + tid * (size_t)(2 * H2G_COMBINE_MAXLEN);
	for(size_t i = tid; i < n; i += stride) {
		const SeqView sv = seq_view(rd, a[i].read, a[i].fw != 0);
		ok[i] = hit_combine(ref, P.sc, sv, &a[i], &b[i], minsc[i], P.minIntronLen, P.no_spliced != 0, ScVec{t1, 1}, ScVec{t1 + H2G_COMBINE_MAXLEN, 1}, &alts) ? 1u : 0u;
	}
}

__global__ __launch_bounds__(256) void k_adjust_alt(DGfm g, DRef ref, DAlts alts, DReads rd, const h2g_adjust_query* q, size_t n, uint32_t cap,
                                                    h2g_ghit* hits, uint32_t* nhits, AwaWS* scratch)
{
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	AwaWS* W = scratch + tid;
	for(size_t i = tid; i < n; i += stride) {
		SeqView sv = seq_view(rd, q[i].read, q[i].fw != 0);
		uint32_t nh = 0, ovf = 0;
		adjust_with_alt(g, ref, alts, sv, q[i].rdoff, q[i].len, q[i].tidx, q[i].toff, q[i].joinedOff, hits + i * cap, &nh, cap, W, &ovf);
		nhits[i] = ovf ? H2G_MAX : nh;
		for(uint32_t k = 0; k < nh; k++) hits[i * cap + k].read = q[i].read;
	}
}

__global__ __launch_bounds__(256) void k_graph_lf(DGfm g, const h2g_glf_query* q, size_t n, uint32_t k, h2g_glf_result* res, h2g_iedges* ie)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		GRange r;
		IEdges e;
		e.n = 0;
		bool ok;
		if(q[i].single) ok = map_glf1(g, q[i].top, q[i].c, &r);
		else ok = map_glf(g, q[i].top, q[i].bot, q[i].c, k, &r, &e);
		h2g_glf_result o;
		o.ok = ok; o.top = r.top; o.bot = r.bot; o.node_top = r.node_top; o.node_bot = r.node_bot;
		res[i] = o;
		if(ie) {
			ie[i].n = e.n;
			for(uint32_t j = 0; j < e.n && j < H2G_IEDGE_CAP; j++) { ie[i].e[j][0] = e.e[j][0]; ie[i].e[j][1] = e.e[j][1]; }
		}
	}
}

__global__ __launch_bounds__(256) void k_sa_resolve_graph(DGfm g, const h2g_gsa_query* q, const h2g_iedges* ie, size_t n, uint32_t cap,
                                                          h2g_coord* coords, h2g_sa_result* res, GwCtx* scratch)
{
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	GwCtx* x = scratch + tid;
	for(size_t i = tid; i < n; i += stride)
		genome_coords_graph_item(g, x, q[i].top, q[i].bot, q[i].node_top, q[i].node_bot, ie ? &ie[i] : nullptr, q[i].maxelt, q[i].len,
		                         q[i].rejectStraddle != 0, coords + i * cap, cap, &res[i]);
}

__global__ __launch_bounds__(256) void k_fm_search_graph(DGfm g, DReads rd, const h2g_fm_query* q, size_t n, uint32_t khits,
                                                         uint32_t kseeds, h2g_fm_hit* out, h2g_iedges* ie)
{
	size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		SeqView sv = seq_view(rd, q[i].read, q[i].fw != 0);
		partial_search_graph_item(g, sv, q[i].offset, q[i].pseudogeneStop != 0, q[i].anchorStop != 0, khits, kseeds, &out[i],
		                          ie ? &ie[i] : nullptr);
	}
}

// ------------------------------------------------------------------------------------------ Smith-Waterman
static_assert(sizeof(h2g_sw_result) == sizeof(SwOut), "h2g_sw_result must mirror SwOut");
// Two kernels.  k_sw_fill: one wavefront per problem, register-resident systolic fill (sw_fill_wave), H/E/F streamed to an
// HBM workspace in anti-diagonal-major order (64 contiguous cells per step and matrix; 8-bit cells, 16-bit for a problem with minsc < -254).  k_sw_backtrace: one LANE per
// problem walks the reference's sequential gather/backtrace over that workspace, so 64 backtraces share a wavefront
// instead of 63 lanes idling behind one.
struct SwWs { uint8_t* base; size_t stride, mat_bytes, rf_bytes; };   // per problem: H | E | F (mat_bytes each) | rf (rf_bytes) | mask matrix of the rare second walk (SwMaskTab::direct)
__global__ __launch_bounds__(64) void k_sw_fill(DRef ref, DReads rd, SwParams P, const h2g_sw_query* q, size_t n, SwWs ws)
{
	__shared__ uint8_t s_rf[H2G_SW_MAX_COLS + 8];
	const uint32_t lane = threadIdx.x;
	for(size_t p = blockIdx.x; p < n; p += gridDim.x) {
		const h2g_sw_query qq = q[p];
		SeqView sv = seq_view(rd, qq.read, qq.fw != 0);
		const uint32_t nrow = sv.len;
		const SwRect rect = sw_frame(qq.refoff, nrow, ref.refLens[qq.tidx]);
		const uint32_t ncol = (uint32_t)(rect.refr - rect.refl + 1);
		uint8_t* w = ws.base + p * ws.stride;
		SwMats m;
		m.nrow = nrow; m.ncol = ncol; m.nd = nrow + ncol - 1; m.layout = 1; m.wide = sw_wide_for(qq.minsc);
		m.H = w; m.E = w + ws.mat_bytes; m.F = w + 2 * ws.mat_bytes; m.rf = s_rf;
		{   // reference window: BitPairReference::getStretch semantics (N / outside the sequence = 4)
			RefCursor rc;
			rc.init(&ref, qq.tidx);
			uint8_t* grf = w + 3 * ws.mat_bytes;
			for(uint32_t j = lane; j < ncol; j += 64) { const uint8_t c = (uint8_t)rc.get(rect.refl + (int64_t)j); s_rf[j] = c; grf[j] = c; }
		}
		__syncthreads();
		sw_fill_wave(m, P, sv, lane);
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_sw_backtrace(DRef ref, DReads rd, SwParams P, const h2g_sw_query* q, size_t n, SwWs ws,
                                                      SwLaneState* states, h2g_sw_result* out)
{
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	SwLaneState* ls = states + tid;
	for(size_t p = tid; p < n; p += stride) {
		const h2g_sw_query qq = q[p];
		SeqView sv = seq_view(rd, qq.read, qq.fw != 0);
		const uint32_t nrow = sv.len;
		const SwRect rect = sw_frame(qq.refoff, nrow, ref.refLens[qq.tidx]);
		const uint32_t ncol = (uint32_t)(rect.refr - rect.refl + 1);
		uint8_t* w = ws.base + p * ws.stride;
		SwMats m;
		m.nrow = nrow; m.ncol = ncol; m.nd = nrow + ncol - 1; m.layout = 1; m.wide = sw_wide_for(qq.minsc);
		m.H = w; m.E = w + ws.mat_bytes; m.F = w + 2 * ws.mat_bytes; m.rf = w + 3 * ws.mat_bytes;
		uint32_t rnd = qq.rnd;
		const SwOut* o = sw_finish(m, P, sv, rect, qq.minsc, &rnd, ls, reinterpret_cast<uint16_t*>(w + 3 * ws.mat_bytes + ws.rf_bytes));
		SwOut* dst = reinterpret_cast<SwOut*>(&out[p]);
		dst->found_align = o->found_align; dst->found = o->found; dst->best = o->best; dst->score = o->score; dst->off = o->off;
		dst->nedits = o->nedits; dst->gaps = o->gaps; dst->overflow = o->overflow; dst->rnd = o->rnd; dst->refl = o->refl; dst->refr = o->refr;
		for(uint32_t e = 0; e < o->nedits; e++) dst->edits[e] = o->edits[e];
	}
}

static int need_reads(h2g_stream* s) {
	if(s->cur().n_reads == 0) { snprintf(g_err, sizeof g_err, "no read batch set (h2g_set_reads)"); return H2G_ERR_ARG; }
	return H2G_OK;
}
static int need_graph(h2g_stream* s) {
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	if(s->ix->dg.linear || s->ix->dg.lineRate != 7) { snprintf(g_err, sizeof g_err, "not a graph (GFM, 128 B side) index"); return H2G_ERR_ARG; }
	return H2G_OK;
}
static int need_linear(h2g_stream* s) {
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	if(!s->ix->dg.linear || s->ix->dg.lineRate != 6) { snprintf(g_err, sizeof g_err, "graph (GFM) indexes: not built yet"); return H2G_ERR_UNSUPPORTED; }
	return H2G_OK;
}

extern "C" h2g_status h2g_graph_lf(h2g_stream* s, const h2g_glf_query* q, size_t n, uint32_t k, h2g_glf_result* res, h2g_iedges* iedges) {
	if(!s || !q || !res || n == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_graph(s))) return rc;
	const uint32_t glen = s->ix->dg.gbwtLen;
	for(size_t i = 0; i < n; i++) {
		if(q[i].c > 3 || q[i].top >= glen) return H2G_ERR_ARG;
		if(!q[i].single && (q[i].bot <= q[i].top + 1 || q[i].bot > glen)) return H2G_ERR_ARG;   // bloc.valid(): bot - top > 1
	}
	HIPCHK(hipSetDevice(s->ix->device));
	void *dq, *dres, *die = nullptr;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * sizeof *res, &dres))) return rc;
	if(iedges && (rc = tmp_buf(s, 2, n * sizeof *iedges, &die))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_graph_lf, dim3(grid_for(n, 256)), dim3(256), 0, s->st, s->ix->dg, (const h2g_glf_query*)dq, n, k, (h2g_glf_result*)dres, (h2g_iedges*)die);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(res, dres, n * sizeof *res, hipMemcpyDeviceToHost, s->st));
	if(iedges) HIPCHK(hipMemcpyAsync(iedges, die, n * sizeof *iedges, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_adjust_with_alt(h2g_stream* s, const h2g_adjust_query* q, size_t n, uint32_t cap, h2g_ghit* hits, uint32_t* nhits) {
	if(!s || !q || !hits || !nhits || n == 0 || cap == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s)) || (rc = need_graph(s))) return rc;
	for(size_t i = 0; i < n; i++) if(q[i].read >= s->cur().n_reads || q[i].tidx >= s->ix->dr.nrefs) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	const unsigned grid = grid_for(n, 256) > 128 ? 128 : grid_for(n, 256);
	void *dq, *dh, *dn, *dscr;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * cap * sizeof *hits, &dh)) || (rc = tmp_buf(s, 2, n * 4, &dn)) ||
	   (rc = tmp_buf(s, 3, (size_t)grid * 256 * sizeof(AwaWS), &dscr))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_adjust_alt, dim3(grid), dim3(256), 0, s->st, s->ix->dg, s->ix->dr, s->ix->dalts, dreads(s), (const h2g_adjust_query*)dq, n, cap,
	                   (h2g_ghit*)dh, (uint32_t*)dn, (AwaWS*)dscr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(hits, dh, n * cap * sizeof *hits, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(nhits, dn, n * 4, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_sa_resolve_graph(h2g_stream* s, const h2g_gsa_query* q, const h2g_iedges* iedges, size_t n, uint32_t cap,
                                           h2g_coord* coords, h2g_sa_result* res)
{
	if(!s || !q || !coords || !res || n == 0 || cap == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_graph(s))) return rc;
	const uint32_t glen = s->ix->dg.gbwtLen;
	for(size_t i = 0; i < n; i++)
		if(q[i].top >= q[i].bot || q[i].bot > glen || q[i].node_top >= q[i].node_bot || q[i].node_bot - q[i].node_top > q[i].bot - q[i].top) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	const unsigned grid = grid_for(n, 256) > 128 ? 128 : grid_for(n, 256);   // 32 k lanes x sizeof(GwCtx) of scratch
	void *dq, *dco, *dres, *die = nullptr, *dscr;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * cap * sizeof *coords, &dco)) ||
	   (rc = tmp_buf(s, 2, n * sizeof *res + (iedges ? n * sizeof *iedges : 0), &dres)) ||
	   (rc = tmp_buf(s, 3, (size_t)grid * 256 * sizeof(GwCtx), &dscr))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	if(iedges) {
		die = (char*)dres + n * sizeof *res;
		HIPCHK(hipMemcpyAsync(die, iedges, n * sizeof *iedges, hipMemcpyHostToDevice, s->st));
	}
	hipLaunchKernelGGL(k_sa_resolve_graph, dim3(grid), dim3(256), 0, s->st, s->ix->dg, (const h2g_gsa_query*)dq, (const h2g_iedges*)die, n, cap,
	                   (h2g_coord*)dco, (h2g_sa_result*)dres, (GwCtx*)dscr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(coords, dco, n * cap * sizeof *coords, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(res, dres, n * sizeof *res, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_fm_search_graph(h2g_stream* s, const h2g_fm_query* q, size_t n, uint32_t khits, uint32_t kseeds,
                                          h2g_fm_hit* out, h2g_iedges* iedges)
{
	if(!s || !q || !out || n == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s)) || (rc = need_graph(s))) return rc;
	for(size_t i = 0; i < n; i++) {
		if(q[i].read >= s->cur().n_reads) return H2G_ERR_ARG;
		if(q[i].mode != H2G_FM_PARTIAL) { snprintf(g_err, sizeof g_err, "fm_search: only H2G_FM_PARTIAL built"); return H2G_ERR_UNSUPPORTED; }
	}
	HIPCHK(hipSetDevice(s->ix->device));
	void *dq, *dout, *die = nullptr;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * sizeof *out, &dout))) return rc;
	if(iedges && (rc = tmp_buf(s, 2, n * sizeof *iedges, &die))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_fm_search_graph, dim3(grid_for(n, 256)), dim3(256), 0, s->st, s->ix->dg, dreads(s), (const h2g_fm_query*)dq, n,
	                   khits, kseeds, (h2g_fm_hit*)dout, (h2g_iedges*)die);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, dout, n * sizeof *out, hipMemcpyDeviceToHost, s->st));
	if(iedges) HIPCHK(hipMemcpyAsync(iedges, die, n * sizeof *iedges, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_fm_search(h2g_stream* s, const h2g_fm_query* q, size_t n, uint32_t khits, h2g_fm_hit* out) {
	if(!s || !q || !out || n == 0) return H2G_ERR_ARG;
	int rc;
	if(s->ix && !s->ix->synthetic && !s->ix->dg.linear && s->ix->dg.lineRate == 7)
		return h2g_fm_search_graph(s, q, n, khits, khits * 2 > 5 ? khits * 2 : 5, out, nullptr);
	if((rc = need_reads(s)) || (rc = need_linear(s))) return rc;
	for(size_t i = 0; i < n; i++) {
		if(q[i].read >= s->cur().n_reads) return H2G_ERR_ARG;
		if(q[i].mode != H2G_FM_PARTIAL) { snprintf(g_err, sizeof g_err, "fm_search: only H2G_FM_PARTIAL built"); return H2G_ERR_UNSUPPORTED; }
	}
	HIPCHK(hipSetDevice(s->ix->device));
	void *dq, *dout;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * sizeof *out, &dout))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_fm_search, dim3(grid_for(n, 256)), dim3(256), 0, s->st, s->ix->dg, dreads(s), (const h2g_fm_query*)dq, n, khits, (h2g_fm_hit*)dout);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, dout, n * sizeof *out, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ globalGFMSearch / localGFMSearch
// one query on whichever index this is (the item function of both kernels below; sbase/fbase != nullptr: the local index is in LDS)
template <bool GRAPH>
__device__ __forceinline__ void ext_search_item(const DGfm& g, const DLocalSet& ls, const DReads& rd, const h2g_ext_search_query& qq, uint32_t minK,
                                                uint32_t minK_local, uint32_t kseeds, const uint8_t* sbase, const uint16_t* fbase, h2g_ext_search_hit* o)
{
	const SeqView sv = seq_view(rd, qq.read, qq.fw != 0);
	uint32_t hitlen = 0, top = H2G_MAX, bot = H2G_MAX, nr[2] = {0, 0}, nelt = 0;
	bool us = qq.uniqueStop != 0;
	if(qq.lidx == H2G_MAX) {
		GIdx gx; gx.g = &g;
		if(!GRAPH) nelt = gfm_search(gx, sv, qq.rdoff, &hitlen, &top, &bot, &us, minK, H2G_MAX, kseeds, false, nr);
		else { GRange r; r.top = top; r.bot = bot; r.node_top = r.node_bot = 0; IEdges ie; nelt = gfm_search_graph(g, gx, sv, qq.rdoff, &hitlen, &r, &ie, &us, minK, H2G_MAX, kseeds, false, kseeds, nr); if(nelt > 0) { top = r.top; bot = r.bot; } }
	} else {
		LIdx lx; lx.ls = &ls; lx.d = &ls.desc[qq.lidx]; lx.sbase = sbase; lx.fbase = fbase;
		if(lx.d->len == 0) nelt = 0;
		else if(!GRAPH) nelt = gfm_search(lx, sv, qq.rdoff, &hitlen, &top, &bot, &us, minK_local, qq.maxHitLen, kseeds, true, nr);
		else if(local_is_linear(*lx.d)) {   // a local index without a variant is linear inside a graph index (128 B sides): h2g_align.h LIdxW
			LIdxW lw; lw.ls = &ls; lw.d = lx.d;
			nelt = gfm_search(lw, sv, qq.rdoff, &hitlen, &top, &bot, &us, minK_local, qq.maxHitLen, kseeds, true, nr);
		}
		else { const LGfm x = lgfm_of(ls, *lx.d); GRange r; r.top = top; r.bot = bot; r.node_top = r.node_bot = 0; IEdges ie;
		       nelt = gfm_search_graph(x, lx, sv, qq.rdoff, &hitlen, &r, &ie, &us, minK_local, qq.maxHitLen, kseeds, true, kseeds, nr); top = r.top; bot = r.bot; }
	}
	o->nelt = nelt; o->hitlen = hitlen; o->top = top; o->bot = bot; o->uniqueStop = us ? 1u : 0u; o->nrank = nr[0]; o->nside = nr[1]; o->staged = sbase ? 1u : 0u;
}

// lane per query, sides from HBM: global queries, local queries of thin buckets, graph-index locals
template <bool GRAPH>
__global__ __launch_bounds__(256) void k_ext_search_hbm(DGfm g, DLocalSet ls, DReads rd, const h2g_ext_search_query* q, const uint32_t* order, size_t n,
                                                        uint32_t minK, uint32_t minK_local, uint32_t kseeds, h2g_ext_search_hit* out)
{
	const size_t stride = (size_t)gridDim.x * blockDim.x;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		const uint32_t k = order[i];
		ext_search_item<GRAPH>(g, ls, rd, q[k], minK, minK_local, kseeds, nullptr, nullptr, &out[k]);
	}
}

// one workgroup per bucket of same-local-index queries: the index's sides and ftab are copied into LDS once (coalesced 16 B
// loads), then every Occ-rank of the bucket's queries is an LDS read.  Linear local indexes (64 B sides of 16-bit words).
__global__ __launch_bounds__(256) void k_ext_search_lds(DGfm g, DLocalSet ls, DReads rd, const h2g_ext_search_query* q, const uint32_t* order,
                                                        const uint2* buckets /* {first, count} into order */, uint32_t nbuckets, uint32_t minK, uint32_t minK_local,
                                                        uint32_t kseeds, h2g_ext_search_hit* out)
{
	extern __shared__ uint4 s_stage[];
	for(uint32_t b = blockIdx.x; b < nbuckets; b += gridDim.x) {
		const uint2 bk = buckets[b];
		const uint32_t lidx = q[order[bk.x]].lidx;
		const DLocalDesc& d = ls.desc[lidx];
		const uint32_t nside16 = (d.sides_bytes + 15) / 16, nftab = (1u << (2 * ls.ftabChars)) + 1;
		const uint4* src = reinterpret_cast<const uint4*>(ls.sides + d.sides_off);
		for(uint32_t i = threadIdx.x; i < nside16; i += blockDim.x) s_stage[i] = src[i];
		uint16_t* s_ftab = reinterpret_cast<uint16_t*>(s_stage + nside16);
		for(uint32_t i = threadIdx.x; i < nftab; i += blockDim.x) s_ftab[i] = ls.words[d.ftab_off + i];
		__syncthreads();
		for(uint32_t i = threadIdx.x; i < bk.y; i += blockDim.x) {
			const uint32_t k = order[bk.x + i];
			ext_search_item<false>(g, ls, rd, q[k], minK, minK_local, kseeds, reinterpret_cast<const uint8_t*>(s_stage), s_ftab, &out[k]);
		}
		__syncthreads();
	}
}

extern "C" uint32_t h2g_local_index_of(const h2g_index* ix, uint32_t tidx, uint32_t toff) {
	if(!ix || !ix->has_local || tidx >= ix->host.local_first.size() - 1) return H2G_MAX;
	const uint32_t a = ix->host.local_first[tidx], b = ix->host.local_first[tidx + 1], k = toff / H2G_LOCAL_INTERVAL;
	return a + k >= b ? H2G_MAX : a + k;
}

extern "C" h2g_status h2g_ext_search(h2g_stream* s, const h2g_ext_search_query* q, size_t n, uint32_t stage_min, h2g_ext_search_hit* out,
                                     h2g_ext_search_stats* stats)
{
	if(!s || !q || !out || n == 0 || n > 0xffffffffull) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s))) return rc;
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	const bool graph = !s->ix->dg.linear;
	const uint32_t nlocal = s->ix->dls.n;
	for(size_t i = 0; i < n; i++) {
		if(q[i].read >= s->cur().n_reads) return H2G_ERR_ARG;
		if(q[i].lidx != H2G_MAX && (!s->ix->has_local || q[i].lidx >= nlocal)) return H2G_ERR_ARG;
	}
	HIPCHK(hipSetDevice(s->ix->device));
	// bucket the local queries by index (host: the queries come from the host anyway); thin buckets and global queries go to the HBM kernel
	std::vector<uint32_t> ord(n);
	for(size_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return q[a].lidx < q[b].lidx; });
	std::vector<uint32_t> o_lds, o_hbm;
	std::vector<uint2> buckets;
	h2g_ext_search_stats st;
	memset(&st, 0, sizeof st);
	uint32_t max_stage = 0;
	for(size_t i = 0; i < n;) {
		size_t j = i;
		while(j < n && q[ord[j]].lidx == q[ord[i]].lidx) j++;
		const uint32_t lidx = q[ord[i]].lidx;
		const bool local = lidx != H2G_MAX;
		if(local) { st.n_local += j - i; st.n_buckets++; }
		const DLocalDesc* d = local ? &s->ix->h_ldesc[lidx] : nullptr;
		if(local && !graph && stage_min > 0 && j - i >= stage_min && d->len > 0) {
			// a fat bucket is cut into workgroup-sized pieces (each stages its own copy: 25-40 KB against >= 1 MB of side reads saved)
			const uint32_t bytes = (d->sides_bytes + 15) / 16 * 16 + ((1u << (2 * s->ix->dls.ftabChars)) + 1) * 2 + 16;
			for(size_t c = i; c < j; c += 1024) {
				const size_t ce = c + 1024 < j ? c + 1024 : j;
				buckets.push_back(make_uint2((uint32_t)o_lds.size(), (uint32_t)(ce - c)));
				for(size_t k = c; k < ce; k++) o_lds.push_back(ord[k]);
				st.n_buckets_staged++;
				st.lds_bytes_staged += bytes;
			}
			st.n_staged += j - i;
			if(bytes > max_stage) max_stage = bytes;
		} else for(size_t k = i; k < j; k++) o_hbm.push_back(ord[k]);
		i = j;
	}
	void *dq, *dout, *dord, *dbk;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * sizeof *out, &dout)) || (rc = tmp_buf(s, 2, n * 4 + 64, &dord)) ||
	   (rc = tmp_buf(s, 3, buckets.size() * sizeof(uint2) + 64, &dbk))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	uint32_t* d_olds = (uint32_t*)dord;
	uint32_t* d_ohbm = d_olds + o_lds.size();
	if(!o_lds.empty()) HIPCHK(hipMemcpyAsync(d_olds, o_lds.data(), o_lds.size() * 4, hipMemcpyHostToDevice, s->st));
	if(!o_hbm.empty()) HIPCHK(hipMemcpyAsync(d_ohbm, o_hbm.data(), o_hbm.size() * 4, hipMemcpyHostToDevice, s->st));
	if(!buckets.empty()) HIPCHK(hipMemcpyAsync(dbk, buckets.data(), buckets.size() * sizeof(uint2), hipMemcpyHostToDevice, s->st));
	h2g_align_params ap;
	align_params_defaults(&ap, !graph);
	const AlnParams P = aln_params_from(ap, true, !graph);
	const uint32_t minK = s->ix->dg.minK, minKl = P.minK_local, kseeds = P.kseeds;
	HIPCHK(hipEventRecord(s->tm[TM_PRIM0], s->st));
	if(!buckets.empty()) {
		const unsigned grid = (unsigned)(buckets.size() < 256 * 8 ? buckets.size() : 256 * 8);
		hipLaunchKernelGGL(k_ext_search_lds, dim3(grid), dim3(256), max_stage, s->st, s->ix->dg, dls_now(s->ix), dreads(s), (const h2g_ext_search_query*)dq, d_olds,
		                   (const uint2*)dbk, (uint32_t)buckets.size(), minK, minKl, kseeds, (h2g_ext_search_hit*)dout);
	}
	HIPCHK(hipEventRecord(s->tm[TM_PRIM1], s->st));
	if(!o_hbm.empty()) {
		if(graph) hipLaunchKernelGGL((k_ext_search_hbm<true>), dim3(grid_for(o_hbm.size(), 256)), dim3(256), 0, s->st, s->ix->dg, dls_now(s->ix), dreads(s),
		                             (const h2g_ext_search_query*)dq, d_ohbm, o_hbm.size(), minK, minKl, kseeds, (h2g_ext_search_hit*)dout);
		else hipLaunchKernelGGL((k_ext_search_hbm<false>), dim3(grid_for(o_hbm.size(), 256)), dim3(256), 0, s->st, s->ix->dg, dls_now(s->ix), dreads(s),
		                        (const h2g_ext_search_query*)dq, d_ohbm, o_hbm.size(), minK, minKl, kseeds, (h2g_ext_search_hit*)dout);
	}
	HIPCHK(hipEventRecord(s->tm[TM_EXT1], s->st));
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, dout, n * sizeof *out, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	float t = 0;
	if(hipEventElapsedTime(&t, s->tm[TM_PRIM0], s->tm[TM_PRIM1]) == hipSuccess) st.ms_staged = t;
	if(hipEventElapsedTime(&t, s->tm[TM_PRIM1], s->tm[TM_EXT1]) == hipSuccess) st.ms_hbm = t;
	if(stats) *stats = st;
	return H2G_OK;
}

extern "C" h2g_status h2g_sw_align(h2g_stream* s, const h2g_sw_query* q, size_t n, h2g_sw_result* out, int repeats, float* kernel_ms) {
	if(!s || !q || !out || n == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s))) return rc;
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	for(size_t i = 0; i < n; i++) if(q[i].read >= s->cur().n_reads || q[i].tidx >= s->ix->dr.nrefs) return H2G_ERR_ARG;
	const uint32_t maxlen = s->cur().max_read_len;   // longest read of the resident batch: sizes the per-problem workspace
	if(maxlen == 0 || maxlen > H2G_SW_MAX_ROWS) { snprintf(g_err, sizeof g_err, "h2g_sw_align: read length %u outside 1..%d", maxlen, H2G_SW_MAX_ROWS); return H2G_ERR_ARG; }
	HIPCHK(hipSetDevice(s->ix->device));
	const size_t ncolmax = maxlen + 4 * H2G_SW_MAXGAP, ndmax = maxlen + ncolmax - 1;
	SwWs ws;
	bool any_wide = false;                                        // 16-bit cells for the problems with minsc < -254 (aligner_sw.cpp:496)
	for(size_t i = 0; i < n && !any_wide; i++) any_wide = sw_wide_for(q[i].minsc);
	ws.mat_bytes = ((size_t)((maxlen + 63) / 64) * ndmax * 64) << (any_wide ? 1 : 0);
	ws.rf_bytes = (ncolmax + 255) & ~(size_t)255;
	ws.stride = 3 * ws.mat_bytes + ws.rf_bytes + (((size_t)maxlen * ncolmax * 2 + 255) & ~(size_t)255);
	// the batch is sized by BYTES, not by a problem count: a problem's stride runs from ~135 KB (101 rows, 8-bit cells: three H/E/F matrices + the
	// second walk's mask matrix) to ~1 MB (256 rows, 16-bit cells), and the workspace sits next to a human-size index
	const size_t ws_budget = (size_t)6 << 30;
	size_t batch = ws_budget / ws.stride;
	if(batch > 32768) batch = 32768;
	if(batch < 256) batch = 256;
	if(batch > n) batch = n;
	const size_t bt_threads = ((batch + 255) / 256) * 256;
	HIPCHK(s->d_sw_ws.reserve(batch * ws.stride));
	if(s->d_sw_states.size() < bt_threads) {
		HIPCHK(s->d_sw_states.reserve(bt_threads));
		HIPCHK(hipMemset(s->d_sw_states, 0, s->d_sw_states.bytes()));   // mask-table generations start at 0
	}
	ws.base = s->d_sw_ws;
	void *dq, *dout;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * sizeof *out, &dout))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	SwParams P;
	if(repeats < 1) repeats = 1;
	HIPCHK(hipEventRecord(s->tm[TM_PRIM0], s->st));
	for(int r = 0; r < repeats; r++) {
		for(size_t first = 0; first < n; first += batch) {
			const size_t nb = n - first < batch ? n - first : batch;
			hipLaunchKernelGGL(k_sw_fill, dim3((unsigned)nb), dim3(64), 0, s->st, s->ix->dr, dreads(s), P, (const h2g_sw_query*)dq + first, nb, ws);
			hipLaunchKernelGGL(k_sw_backtrace, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s->st, s->ix->dr, dreads(s), P,
			                   (const h2g_sw_query*)dq + first, nb, ws, s->d_sw_states, (h2g_sw_result*)dout + first);
		}
	}
	HIPCHK(hipEventRecord(s->tm[TM_PRIM1], s->st));
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, dout, n * sizeof *out, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	float t = 0;
	HIPCHK(hipEventElapsedTime(&t, s->tm[TM_PRIM0], s->tm[TM_PRIM1]));
	if(kernel_ms) *kernel_ms = t / repeats;
	return H2G_OK;
}

extern "C" h2g_status h2g_sa_resolve(h2g_stream* s, const h2g_sa_query* q, size_t n, uint32_t cap, h2g_coord* coords,
                                     h2g_sa_result* res)
{
	if(!s || !q || !coords || !res || n == 0 || cap == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_linear(s))) return rc;
	const uint32_t glen = s->ix->dg.gbwtLen;
	for(size_t i = 0; i < n; i++) if(q[i].top >= q[i].bot || q[i].bot > glen) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	void *dq, *dco, *dres;
	if((rc = tmp_buf(s, 0, n * sizeof *q, &dq)) || (rc = tmp_buf(s, 1, n * cap * sizeof *coords, &dco)) ||
	   (rc = tmp_buf(s, 2, n * sizeof *res, &dres))) return rc;
	HIPCHK(hipMemcpyAsync(dq, q, n * sizeof *q, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemsetAsync(dco, 0xff, n * cap * sizeof *coords, s->st));
	hipLaunchKernelGGL(k_sa_resolve, dim3(grid_for(n, 256)), dim3(256), 0, s->st, dg_now(s->ix), (const h2g_sa_query*)dq, n, cap, (h2g_coord*)dco, (h2g_sa_result*)dres);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(coords, dco, n * cap * sizeof *coords, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(res, dres, n * sizeof *res, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_extend(h2g_stream* s, h2g_ghit* hits, const h2g_ext_args* args, size_t n, h2g_ext_result* res) {
	if(!s || !hits || !args || !res || n == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s))) return rc;
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	const bool graph = !s->ix->dg.linear;
	for(size_t i = 0; i < n; i++) {
		if(hits[i].read >= s->cur().n_reads || hits[i].tidx >= s->ix->dr.nrefs || hits[i].nedits > H2G_MAX_EDITS) return H2G_ERR_ARG;
	}
	HIPCHK(hipSetDevice(s->ix->device));
	void *dh, *da, *dres;
	if((rc = tmp_buf(s, 0, n * sizeof *hits, &dh)) || (rc = tmp_buf(s, 1, n * sizeof *args, &da)) ||
	   (rc = tmp_buf(s, 2, n * sizeof *res, &dres))) return rc;
	HIPCHK(hipMemcpyAsync(dh, hits, n * sizeof *hits, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(da, args, n * sizeof *args, hipMemcpyHostToDevice, s->st));
	DScoring sc;
	if(graph) {
		const unsigned grid = grid_for(n, 256) > 256 ? 256 : grid_for(n, 256);
		void* dscr;
		if((rc = tmp_buf(s, 3, (size_t)grid * 256 * sizeof(AwaWS), &dscr))) return rc;
		hipLaunchKernelGGL(k_extend_alts, dim3(grid), dim3(256), 0, s->st, s->ix->dr, s->ix->dalts, dreads(s), sc, (h2g_ghit*)dh,
		                   (const h2g_ext_args*)da, n, (h2g_ext_result*)dres, (AwaWS*)dscr);
	} else
	hipLaunchKernelGGL(k_extend, dim3(grid_for(n, 256)), dim3(256), 0, s->st, s->ix->dr, dreads(s), sc, (h2g_ghit*)dh, (const h2g_ext_args*)da, n, (h2g_ext_result*)dres);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(hits, dh, n * sizeof *hits, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(res, dres, n * sizeof *res, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ fused seed stage

// K1: every (read, strand) runs partialSearch from offset 0 (one lane per item)
__global__ __launch_bounds__(256) void k_seed_search(DGfm g, DReads rd, h2g_seed_params p, h2g_seed_result* out,
                                                     unsigned long long* counters)
{
	const size_t n = (size_t)rd.n * 2;
	size_t stride = (size_t)gridDim.x * blockDim.x;
	unsigned long long nrank = 0, nside = 0;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		SeqView sv = seq_view(rd, (uint32_t)(i >> 1), (i & 1) == 0);
		h2g_fm_hit h;
		partial_search_item(g, sv, 0, p.pseudogeneStop != 0, p.anchorStop != 0, p.khits, &h);
		out[i].hit = h;
		nrank += h.nrank; nside += h.nside;
	}
	wave_add(counters + H2G_CNT_RANK, nrank);
	wave_add(counters + H2G_CNT_SIDE, nside);
}

// K2: coordinates + 0-mismatch extension for every partial hit
__global__ __launch_bounds__(256) void k_seed_resolve_extend(DGfm g, DRef ref, DReads rd, DScoring sc, h2g_seed_result* out,
                                                             unsigned long long* counters)
{
	const size_t n = (size_t)rd.n * 2;
	size_t stride = (size_t)gridDim.x * blockDim.x;
	unsigned long long nsteps = 0, next = 0;
	h2g_ghit scratch;
	for(size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
		SeqView sv = seq_view(rd, (uint32_t)(i >> 1), (i & 1) == 0);
		resolve_extend_item(g, ref, sc, sv, &out[i], &scratch);
		nsteps += out[i].nsteps; next += out[i].ncoords;
	}
	wave_add(counters + H2G_CNT_STEPS, nsteps);
	wave_add(counters + H2G_CNT_EXT, next);
}

extern "C" void h2g_seed_params_init(h2g_seed_params* p, const h2g_index* ix, int no_spliced) {
	// nextBWT hi_aligner.h:4669-4670: pseudogeneStop = linearFM && !no_spliced_alignment; anchorStop = !repeat index
	p->pseudogeneStop = (ix && ix->dg.linear && !no_spliced) ? 1 : 0;
	p->anchorStop = 1;
	p->khits = (ix && !ix->dg.linear) ? 10 : 5;   // -k default hisat2.cpp:3903-3906
	p->search_variant = 0;
}

extern "C" h2g_status h2g_seed_extend_run(h2g_stream* s, const h2g_seed_params* p) {
	if(!s || !p) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s)) || (rc = need_linear(s))) return rc;
	HIPCHK(hipSetDevice(s->ix->device));
	const size_t n = s->cur().n_reads * 2;
	HIPCHK(hipMemsetAsync(s->d_counters, 0, 4 * sizeof(unsigned long long), s->st));
	DScoring sc;
	HIPCHK(hipEventRecord(s->tm[TM_SEED0], s->st));
	hipLaunchKernelGGL(k_seed_search, dim3(grid_for(n, 256)), dim3(256), 0, s->st, s->ix->dg, dreads(s), *p, s->d_seed, s->d_counters);
	HIPCHK(hipEventRecord(s->tm[TM_SEED_MID], s->st));
	hipLaunchKernelGGL(k_seed_resolve_extend, dim3(grid_for(n, 256)), dim3(256), 0, s->st, dg_now(s->ix), s->ix->dr, dreads(s), sc, s->d_seed, s->d_counters);
	HIPCHK(hipEventRecord(s->tm[TM_SEED1], s->st));
	HIPCHK(hipGetLastError());
	s->ran_seed = true;
	return H2G_OK;
}

extern "C" h2g_status h2g_seed_extend_fetch(h2g_stream* s, h2g_seed_result* out, size_t first_read, size_t n_reads) {
	if(!s || !out || first_read + n_reads > s->cur().n_reads) return H2G_ERR_ARG;
	HIPCHK(hipMemcpyAsync(out, s->d_seed + first_read * 2, n_reads * 2 * sizeof *out, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ go() for the batch
static_assert(sizeof(h2g_alnres) == sizeof(AlnRec), "h2g_alnres must mirror AlnRec");
static_assert(sizeof(h2g_read_result) == 40, "h2g_read_result layout");
static_assert(sizeof(h2g_pair_result) == sizeof(PairOut), "h2g_pair_result must mirror PairOut");
static_assert(H2G_PAIR_CAP == AL_MAX_PAIRS, "pair capacity");

extern "C" int h2g_device_count(void) { int n = 0; if(hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }

extern "C" void h2g_align_params_init(h2g_align_params* p, const h2g_index* ix) { align_params_defaults(p, !ix || ix->dg.linear); }

extern "C" h2g_status h2g_set_read_names(h2g_stream* s, const char* bytes, const uint32_t* offs, size_t n) {
	if(s) HIPCHK(sync_all(s));        // (a machine pass of the previous batch may still read the buffers this call replaces)
	if(!s || !bytes || !offs || n != s->cur().n_reads || n == 0) return H2G_ERR_ARG;
	s->tmp_gen++;
	HIPCHK(hipSetDevice(s->ix->device));
	BatchCtx& B = s->cur();
	size_t nb = offs[n];
	HIPCHK(B.reserve_names(nb, s->max_reads));
	HIPCHK(hipMemcpyAsync(B.d_names, bytes, nb, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(B.d_name_offs, offs, (n + 1) * 4, hipMemcpyHostToDevice, s->st));
	HIPCHK(sync_all(s));
	B.has_names = true;
	return H2G_OK;
}

extern "C" h2g_status h2g_set_mates(h2g_stream* s, const uint8_t* codes2, const uint32_t* offs2, const char* quals2,
                                    const char* nb2, const uint32_t* noffs2, size_t n)
{
	if(s) HIPCHK(sync_all(s));
	if(!s || !codes2 || !offs2 || !nb2 || !noffs2 || n != s->cur().n_reads || n == 0) return H2G_ERR_ARG;
	if(offs2[n] > s->max_bases) return H2G_ERR_ARG;
	s->tmp_gen++;
	BatchCtx& B = s->cur();
	for(size_t i = 0; i < n; i++) { const uint32_t l = offs2[i + 1] - offs2[i]; if(l > B.max_read_len) B.max_read_len = l; }
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(B.ensure_mates(s->max_reads, s->max_bases, noffs2[n]));
	HIPCHK(hipMemcpyAsync(B.d_codes2, codes2, offs2[n], hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(B.d_offs2, offs2, (n + 1) * 4, hipMemcpyHostToDevice, s->st));
	B.has_quals2 = quals2 != nullptr;
	if(quals2) HIPCHK(hipMemcpyAsync(B.d_quals2, quals2, offs2[n], hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(B.d_names2, nb2, noffs2[n], hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(B.d_name_offs2, noffs2, (n + 1) * 4, hipMemcpyHostToDevice, s->st));
	HIPCHK(sync_all(s));
	B.has_mates = true;
	return H2G_OK;
}

extern "C" h2g_status h2g_set_read_seeds(h2g_stream* s, const uint32_t* seeds1, const uint32_t* seeds2, size_t n) {
	if(s) HIPCHK(sync_all(s));        // (a run of the previous seeds may still read the buffer)
	if(!s) return H2G_ERR_ARG;
	BatchCtx& B = s->cur();
	if(!seeds1) { B.has_seeds = B.has_seeds2 = false; return H2G_OK; }
	if(n != B.n_reads || n == 0) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(B.d_seeds.ensure(2 * s->max_reads));
	HIPCHK(hipMemcpyAsync(B.d_seeds, seeds1, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
	if(seeds2) HIPCHK(hipMemcpyAsync(B.d_seeds + s->max_reads, seeds2, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
	HIPCHK(sync_all(s));
	B.has_seeds = true; B.has_seeds2 = seeds2 != nullptr;
	return H2G_OK;
}

extern "C" h2g_status h2g_set_read_ids(h2g_stream* s, const uint32_t* ids) {
	if(s) HIPCHK(sync_all(s));        // (a run of the previous ids may still read the buffer)
	if(!s) return H2G_ERR_ARG;
	BatchCtx& B = s->cur();
	if(!ids) { B.has_ids = false; return H2G_OK; }
	const size_t n = B.n_reads;
	if(n == 0 || n > s->max_reads) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(B.d_ids.ensure(s->max_reads));
	HIPCHK(hipMemcpyAsync(B.d_ids, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->st));
	HIPCHK(sync_all(s));
	B.has_ids = true;
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ -F windows: the read set expanded on the device
// The code array of a window batch is one run of n * len bytes.  A lane owns 16 consecutive OUTPUT bytes and stores them as one dwordx4: a wave writes 1 KB
// contiguous whatever len and step are.  The sources are gathered byte by byte from the text; neighbouring windows overlap (len / step fold), so the text is read
// from L2 and the kernel's traffic is its stores.  The per-read arithmetic is h2g_windows.h's.
__global__ __launch_bounds__(256) void k_win_codes(const uint8_t* __restrict__ text, const h2g_win::DSeg* __restrict__ segs, uint32_t n_segs, uint32_t len, uint32_t step,
                                                   uint64_t n_bytes, uint8_t* __restrict__ codes)
{
	const uint64_t chunks = (n_bytes + 15) / 16;
	for(uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t b0 = c * 16;
		const uint32_t m = n_bytes - b0 < 16 ? (uint32_t)(n_bytes - b0) : 16u;      // (the bytes past the end of the last chunk are written as 0: the buffer has 64 spare)
		h2g_win::CodeCursor cur;
		cur.seek(segs, n_segs, len, step, b0);
		uint32_t w[4] = {0, 0, 0, 0};
		for(uint32_t k = 0; k < m; k++) w[k >> 2] |= (uint32_t)text[cur.next()] << (8 * (k & 3));
		*(uint4*)(codes + b0) = make_uint4(w[0], w[1], w[2], w[3]);
	}
}
// one lane per read: its offset, id, name offset and the bytes of its name; lane n the closing offsets
__global__ __launch_bounds__(256) void k_win_meta(const h2g_win::DSeg* __restrict__ segs, uint32_t n_segs, uint32_t len, uint32_t step, uint32_t n, const char* __restrict__ prefixes,
                                                  uint32_t* __restrict__ offs, uint32_t* __restrict__ ids, uint32_t* __restrict__ name_offs, char* __restrict__ names)
{
	for(uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += gridDim.x * blockDim.x) {
		offs[r] = r * len;
		if(r == n) { name_offs[r] = segs[n_segs].name_first; break; }
		const h2g_win::DSeg s = segs[h2g_win::seg_of(segs, n_segs, r)];
		const uint32_t j = r - s.first_read;
		ids[r] = s.rdid0 + j * step;
		const uint32_t at = h2g_win::name_start(s, step, j);
		name_offs[r] = at;
		h2g_win::write_name(s, step, j, prefixes, names + at);
	}
}

extern "C" h2g_status h2g_set_reads_windows(h2g_stream* s, const uint8_t* text, size_t n_text, const h2g_window_seg* segs, size_t n_segs, uint32_t len, uint32_t step,
                                            const char* prefixes, size_t n_prefix_bytes)
{
	if(s) HIPCHK(sync_all(s));        // (a machine pass of the previous batch may still read the buffers this call replaces)
	if(!s || !text || !segs || n_segs == 0 || n_segs >= 0xffffffffull || len == 0 || (!prefixes && n_prefix_bytes)) return H2G_ERR_ARG;
	s->tmp_gen++;
	BatchCtx& B = s->cur();
	// the kernels' table: the per-segment first read and first name byte, the text range the segments touch
	std::vector<h2g_win::DSeg> ds(n_segs + 1);
	uint64_t n = 0, nb = 0, lo = UINT64_MAX, hi = 0;
	for(size_t k = 0; k < n_segs; k++) {
		const h2g_window_seg& x = segs[k];
		const uint64_t last = x.text_start + (uint64_t)(x.n_windows ? x.n_windows - 1 : 0) * step;
		if(x.n_windows == 0 || last + len > n_text || last < x.text_start || (uint64_t)x.prefix_start + x.prefix_len > n_prefix_bytes) {
			snprintf(g_err, sizeof g_err, "h2g_set_reads_windows: segment %zu names text or prefix bytes that were not given", k); return H2G_ERR_ARG;
		}
		if(x.text_start < lo) lo = x.text_start;
		if(last + len > hi) hi = last + len;
		h2g_win::DSeg& d = ds[k];
		d.name_off0 = x.name_off0; d.rdid0 = (uint32_t)x.rdid0; d.first_read = (uint32_t)n; d.name_first = (uint32_t)nb;
		d.prefix_start = x.prefix_start; d.prefix_len = x.prefix_len;
		n += x.n_windows;
		nb += (uint64_t)x.n_windows * x.prefix_len + h2g_win::width_sum(x.name_off0, step, x.n_windows);
		if(n > s->max_reads || n * len > s->max_bases || n * len > 0xffffffffull || nb > 0xffffffffull) {      // (read and name offsets are 32 bits)
			snprintf(g_err, sizeof g_err, "h2g_set_reads_windows: the windows exceed the stream's %zu reads / %zu bases, or their names 4 GB", s->max_reads, s->max_bases); return H2G_ERR_ARG;
		}
	}
	if(hi - lo > 0xffffffffull) { snprintf(g_err, sizeof g_err, "h2g_set_reads_windows: the segments span more than 4 G bases of text"); return H2G_ERR_ARG; }
	for(size_t k = 0; k < n_segs; k++) ds[k].text_start = (uint32_t)(segs[k].text_start - lo);
	memset(&ds[n_segs], 0, sizeof ds[n_segs]);
	ds[n_segs].first_read = (uint32_t)n; ds[n_segs].name_first = (uint32_t)nb;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(B.reserve_names(nb, s->max_reads));
	HIPCHK(B.d_ids.ensure(s->max_reads));
	void *d_text, *d_segs, *d_pre;
	int rc;
	if((rc = tmp_buf(s, 0, hi - lo, &d_text)) || (rc = tmp_buf(s, 1, ds.size() * sizeof(h2g_win::DSeg), &d_segs)) || (rc = tmp_buf(s, 2, n_prefix_bytes, &d_pre))) return (h2g_status)rc;
	HIPCHK(hipMemcpyAsync(d_text, text + lo, hi - lo, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(d_segs, ds.data(), ds.size() * sizeof(h2g_win::DSeg), hipMemcpyHostToDevice, s->st));
	if(n_prefix_bytes) HIPCHK(hipMemcpyAsync(d_pre, prefixes, n_prefix_bytes, hipMemcpyHostToDevice, s->st));
	const uint64_t n_bytes = n * len;
	HIPCHK(hipEventRecord(s->tm[TM_SET0], s->st));
	k_win_codes<<<grid_for((n_bytes + 15) / 16, 256), 256, 0, s->st>>>((const uint8_t*)d_text, (const h2g_win::DSeg*)d_segs, (uint32_t)n_segs, len, step, n_bytes, B.d_codes);
	k_win_meta<<<grid_for(n + 1, 256), 256, 0, s->st>>>((const h2g_win::DSeg*)d_segs, (uint32_t)n_segs, len, step, (uint32_t)n, (const char*)d_pre, B.d_offs, B.d_ids, B.d_name_offs, B.d_names);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->tm[TM_SET1], s->st));
	HIPCHK(sync_all(s));
	s->win_stats.bytes_uploaded = (hi - lo) + ds.size() * sizeof(h2g_win::DSeg) + n_prefix_bytes;
	s->win_stats.bytes_written = n_bytes + (n + 1) * 8 + n * 4 + nb;
	HIPCHK(hipEventElapsedTime(&s->win_stats.kernel_ms, s->tm[TM_SET0], s->tm[TM_SET1]));
	B.n_reads = n;
	B.max_read_len = len;
	B.has_quals = false;
	B.has_names = true;
	B.has_mates = false;
	B.has_seeds = B.has_seeds2 = false;
	B.has_qc = false;
	B.has_ids = true;
	s->ledits_touched = 0;
	return H2G_OK;
}
extern "C" h2g_status h2g_get_windows_stats(h2g_stream* s, h2g_windows_stats* out) {
	if(!s || !out) return H2G_ERR_ARG;
	*out = s->win_stats;
	return H2G_OK;
}

extern "C" h2g_status h2g_fetch_reads(h2g_stream* s, size_t* n_reads, size_t* n_bases, size_t* n_name_bytes, int* has_ids, uint8_t* codes, uint32_t* offs, char* names,
                                      uint32_t* name_offs, uint32_t* ids)
{
	if(!s) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	const BatchCtx& B = s->cur();
	const size_t n = B.n_reads;
	uint32_t nb = 0, nn = 0;
	HIPCHK(hipSetDevice(s->ix->device));
	if(n) HIPCHK(hipMemcpy(&nb, B.d_offs + n, 4, hipMemcpyDeviceToHost));
	if(n && B.has_names) HIPCHK(hipMemcpy(&nn, B.d_name_offs + n, 4, hipMemcpyDeviceToHost));
	if(n_reads) *n_reads = n;
	if(n_bases) *n_bases = nb;
	if(n_name_bytes) *n_name_bytes = nn;
	if(has_ids) *has_ids = B.has_ids ? 1 : 0;
	if(n == 0) return H2G_OK;
	if((ids && !B.has_ids) || ((names || name_offs) && !B.has_names)) return H2G_ERR_ARG;
	if(codes && nb) HIPCHK(hipMemcpy(codes, B.d_codes, nb, hipMemcpyDeviceToHost));
	if(offs) HIPCHK(hipMemcpy(offs, B.d_offs, (n + 1) * 4, hipMemcpyDeviceToHost));
	if(names && nn) HIPCHK(hipMemcpy(names, B.d_names, nn, hipMemcpyDeviceToHost));
	if(name_offs) HIPCHK(hipMemcpy(name_offs, B.d_name_offs, (n + 1) * 4, hipMemcpyDeviceToHost));
	if(ids) HIPCHK(hipMemcpy(ids, B.d_ids, n * 4, hipMemcpyDeviceToHost));
	return H2G_OK;
}

extern "C" h2g_status h2g_set_read_filter(h2g_stream* s, const uint8_t* pass1, const uint8_t* pass2) {
	if(s) HIPCHK(sync_all(s));        // (a run of the previous bytes may still read the buffer)
	if(!s) return H2G_ERR_ARG;
	BatchCtx& B = s->cur();
	if(!pass1 && !pass2) { B.has_qc = false; return H2G_OK; }
	const size_t n = B.n_reads;
	if(n == 0 || n > s->max_reads) return H2G_ERR_ARG;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(B.d_qc.ensure(2 * s->max_reads));
	// a set without bytes passes as a whole
	if(pass1) HIPCHK(hipMemcpyAsync(B.d_qc, pass1, n, hipMemcpyHostToDevice, s->st)); else HIPCHK(hipMemsetAsync(B.d_qc, 1, n, s->st));
	if(pass2) HIPCHK(hipMemcpyAsync(B.d_qc + s->max_reads, pass2, n, hipMemcpyHostToDevice, s->st)); else HIPCHK(hipMemsetAsync(B.d_qc + s->max_reads, 1, n, s->st));
	HIPCHK(sync_all(s));
	B.has_qc = true;
	return H2G_OK;
}

// go() on a graph index: the index must be a SNP graph (ALT database present)
// GenomeHit::combineWith as a primitive of its own: a[i] becomes the combination of a[i] (the left hit) and b[i] on the resident reads, ok[i] the
// function's return value.  Scoring and splice policy: `p` (nullptr: the defaults of the index).
extern "C" h2g_status h2g_combine_with(h2g_stream* s, const h2g_align_params* p, h2g_ghit* a, const h2g_ghit* b, const int64_t* minsc, size_t n, uint32_t* ok) {
	if(!s || !a || !b || !minsc || !ok || n == 0) return H2G_ERR_ARG;
	int rc;
	if((rc = need_reads(s))) return rc;
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	const bool linear = s->ix->dg.linear != 0;
	for(size_t i = 0; i < n; i++) {
		if(a[i].read >= s->cur().n_reads || b[i].read != a[i].read || a[i].tidx >= s->ix->dr.nrefs || b[i].tidx >= s->ix->dr.nrefs || a[i].nedits > H2G_MAX_EDITS || b[i].nedits > H2G_MAX_EDITS) return H2G_ERR_ARG;
	}
	if(s->cur().max_read_len > H2G_COMBINE_MAXLEN) return H2G_ERR_ARG;      // (the joint's prefix / suffix score arrays)
	h2g_align_params hp;
	if(p) hp = *p; else align_params_defaults(&hp, linear);
	AlnParams P = aln_params_from(hp, hp.no_spliced_alignment != 0, linear);
	if(!hp.no_spliced_alignment) { P.sc.donor_sum = s->ix->d_spl[0]; P.sc.acc_sum1 = s->ix->d_spl[1]; P.sc.acc_sum2 = s->ix->d_spl[2]; }
	HIPCHK(hipSetDevice(s->ix->device));
	unsigned grid = grid_for(n, 256);
	if(grid > 64) grid = 64;
	void *da, *db, *dm, *dscr;
	const size_t ab = n * sizeof(h2g_ghit);
	if((rc = tmp_buf(s, 0, 2 * ab, &da)) || (rc = tmp_buf(s, 1, n * 8, &dm)) || (rc = tmp_buf(s, 2, n * 4, &db)) ||
	   (rc = tmp_buf(s, 3, (size_t)grid * 256 * 2 * H2G_COMBINE_MAXLEN * sizeof(int64_t), &dscr))) return rc;
	h2g_ghit* const d_a = (h2g_ghit*)da; h2g_ghit* const d_b = d_a + n;
	HIPCHK(hipMemcpyAsync(d_a, a, ab, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(d_b, b, ab, hipMemcpyHostToDevice, s->st));
	HIPCHK(hipMemcpyAsync(dm, minsc, n * 8, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_combine, dim3(grid), dim3(256), 0, s->st, s->ix->dr, s->ix->dalts, dreads(s), P, d_a, (const h2g_ghit*)d_b, (const int64_t*)dm, n, (uint32_t*)db, (int64_t*)dscr);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(a, d_a, ab, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(ok, db, n * 4, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

static int need_alignable(h2g_stream* s) {
	if(s->ix->synthetic) { snprintf(g_err, sizeof g_err, "synthetic index: rank only"); return H2G_ERR_ARG; }
	const DGfm& g = s->ix->dg;
	if(g.linear && g.lineRate == 6) return H2G_OK;
	if(!g.linear && g.lineRate == 7) return H2G_OK;
	snprintf(g_err, sizeof g_err, "unsupported side geometry (lineRate %u)", g.lineRate);
	return H2G_ERR_UNSUPPORTED;
}

// the go() units (GoUnitDesc, h2g_go_args.h): [spliced?][linear?][tier: default, big, extra-large].  Spliced: the units whose machine carries the splice-site database joins
static const GoUnitDesc& go_unit(bool linear, bool big, bool spliced = false, bool xl = false) {
	static const GoUnitDesc* (*const u[2][2][3])() = {
		{{h2g_go_unit_graph, h2g_go_unit_graph_big, h2g_go_unit_graph_xl}, {h2g_go_unit_linear, h2g_go_unit_linear_big, h2g_go_unit_linear_xl}},
		{{h2g_go_unit_graph_spl, h2g_go_unit_graph_spl_big, h2g_go_unit_graph_spl_xl}, {h2g_go_unit_linear_spl, h2g_go_unit_linear_spl_big, h2g_go_unit_linear_spl_xl}}};
	return *u[spliced ? 1 : 0][linear ? 1 : 0][xl ? 2 : big ? 1 : 0]();
}
// the builds of the fast pass (FastUnitDesc): graph indexes; on a linear index spliced runs, alignMate in the pass, or neither
static const FastUnitDesc& fast_unit(bool linear, bool spliced, bool align_mate) {
	return *(!linear ? h2g_go_fast_graph_unit : spliced ? h2g_go_fast_spl_unit : align_mate ? h2g_go_fast_am_unit : h2g_go_fast_unit)();
}

// sizes the per-lane scratch of one pass and fills the pool fields of `a`
static int go_pool_for(h2g_stream* s, h2g_stream::GoPool& pl, const GoUnitDesc& u, size_t slots, size_t lanes, uint32_t bowtie2_dp, GoArgs* a) {
	const size_t wsb = u.ws_bytes, gwb = u.gws_bytes;
	HIPCHK(pl.ws.reserve(slots * wsb));
	a->pool = pl.ws; a->ws_stride = wsb; a->slot_off = u.slot_off; a->gsl_off = u.gsl_off;
	a->gws_base = nullptr; a->gws_stride = gwb;
	if(gwb) {
		HIPCHK(pl.gws.reserve(lanes * gwb));
		a->gws_base = pl.gws;
	}
	HIPCHK(pl.sc.reserve(lanes * (size_t)(2 * H2G_COMBINE_MAXLEN * sizeof(int64_t))));
	a->sc_base = pl.sc;
	a->sw_base = nullptr; a->sw_stride = 0;
	if(bowtie2_dp) {
		const uint32_t swlen = s->cur().max_read_len > H2G_SW_MAX_ROWS ? (uint32_t)H2G_SW_MAX_ROWS : s->cur().max_read_len;
		bool wide = false;                                        // some read length of the batch may put minsc below -254: 16-bit cells
		for(uint32_t l = 1; l <= swlen && !wide; l++) wide = sw_wide_for(min_score_for(a->P, l));
		const size_t stride = (u.sw_bytes(swlen, wide ? 1 : 0) + 255) & ~(size_t)255;   // the unit's own SwLaneState (the large-workspace units hold 192-edit records)
		if(pl.sw_stride < stride || pl.sw_lanes < lanes) {      // (either one short: the pool is allocated again)
			pl.sw_stride = 0; pl.sw_lanes = 0;
			HIPCHK(pl.sw.reset(stride * lanes));
			HIPCHK(hipMemset(pl.sw, 0, stride * lanes));   // SwLaneState: mask-table generations start at 0
			pl.sw_stride = stride; pl.sw_lanes = lanes;
		}
		a->sw_base = pl.sw; a->sw_stride = pl.sw_stride;
	}
	return H2G_OK;
}

// (the reads whose main-pass workspace overflowed are listed by the pass itself — MachOut::defer_list — and their rows left alone until the second pass writes them)

// ---- go_run, phase by phase.  The option checks: no device calls
static int go_check(h2g_stream* s, const h2g_align_params* p, bool paired) {
	int rc;
	if((rc = need_reads(s)) || (rc = need_alignable(s))) return rc;
	if(!s->ix->has_local) { snprintf(g_err, sizeof g_err, "align: index loaded without local (.5/.6) indexes"); return H2G_ERR_ARG; }
	if(!s->cur().has_names || (paired && !s->cur().has_mates)) { snprintf(g_err, sizeof g_err, "align: read names (h2g_set_read_names)%s not set", paired ? " / mates (h2g_set_mates)" : ""); return H2G_ERR_ARG; }
	if(paired && s->cur().has_seeds && !s->cur().has_seeds2) { snprintf(g_err, sizeof g_err, "align: explicit seeds without mate 2's (h2g_set_read_seeds seeds2)"); return H2G_ERR_ARG; }
	if(p->n_ceil_type < 1 || p->n_ceil_type > 4) { snprintf(g_err, sizeof g_err, "align: n_ceil_type %u (1 C, 2 L, 3 S, 4 G)", p->n_ceil_type); return H2G_ERR_ARG; }
	// the scoring fields go() divides by (sc_min: the trimming bound; mm_max: maxmm and the pair bound) or counts down with (max_gaps: a gap
	// extension below 1 never ends it).  A division by zero does not trap on the device: the run would go on with an undefined quotient
	if(p->sc_min < 1) { snprintf(g_err, sizeof g_err, "align: sc_min %d (--sp): the soft-clipping penalty must be at least 1", p->sc_min); return H2G_ERR_ARG; }
	if(p->mm_max < 1) { snprintf(g_err, sizeof g_err, "align: mm_max %d (--mp): the maximum mismatch penalty must be at least 1", p->mm_max); return H2G_ERR_ARG; }
	if(p->mm_max < p->mm_min) { snprintf(g_err, sizeof g_err, "align: mm_max %d is less than mm_min %d (--mp)", p->mm_max, p->mm_min); return H2G_ERR_ARG; }
	if(p->rdg_linear < 1 || p->rfg_linear < 1) { snprintf(g_err, sizeof g_err, "align: rdg_linear %d / rfg_linear %d (--rdg, --rfg): a gap extension penalty must be at least 1", p->rdg_linear, p->rfg_linear); return H2G_ERR_ARG; }
	if(!p->no_spliced_alignment) {
		// spliced alignment: combineWith places introns (hi_aligner.h:1588-1739) and every read is independent when novel splice
		// sites are not shared (--no-temp-splicesite); the shared SpliceSiteDB of the default mode and graph indexes are not built
		// no_temp_splicesite == 0 (the reference's default) is the CALLER's wave protocol: batches of <= window reads, the junctions of
		// each batch's output merged into the database (h2g_index_set_splice_sites) before the next one; first_read_id carries the ids
		if(p->pen_canintronlen_type < 1 || p->pen_canintronlen_type > 4 || p->pen_noncanintronlen_type < 1 || p->pen_noncanintronlen_type > 4 ||
		   p->min_intronlen < 20 || p->max_intronlen < p->min_intronlen || p->pen_cansplice < 0 || p->pen_noncansplice < 0 ||
		   p->min_anchor_len < 1 || p->min_anchor_len_noncan < 1) {
			snprintf(g_err, sizeof g_err, "align: splice scoring outside its range (intron-length function type 1..4, 20 <= min_intronlen <= max_intronlen, penalties >= 0)");
			return H2G_ERR_ARG;
		}
		// a splice edit keeps its intron length in 20 bits (include/h2g.h): longer introns are refused by name, never truncated
		if(p->max_intronlen > H2G_SPL_MAXLEN) {
			snprintf(g_err, sizeof g_err, "align: --max-intronlen %u is beyond the %u bases a splice edit holds", p->max_intronlen, (unsigned)H2G_SPL_MAXLEN);
			return H2G_ERR_UNSUPPORTED;
		}
	}
	if(p->khits == 0 || p->khits > H2G_KHITS_MAX || p->kseeds < p->khits || p->kseeds > H2G_KSEEDS_MAX) {
		snprintf(g_err, sizeof g_err, "align: -k %u / --max-seeds %u outside the built range (1 <= -k <= %u, -k <= --max-seeds <= %u)", p->khits, p->kseeds, (unsigned)H2G_KHITS_MAX, (unsigned)H2G_KSEEDS_MAX);
		return H2G_ERR_ARG;
	}
	if(p->bowtie2_dp > 2 || p->pe_orientation > 2 || p->min_frag_len >= (1u << 24)) return H2G_ERR_ARG;
	if(p->pen_conflictsplice < 0) { snprintf(g_err, sizeof g_err, "align: --pen-conflictsplice arg must be at least 0"); return H2G_ERR_ARG; }
	if(p->max_alts_tried && p->max_alts_tried < 8) { snprintf(g_err, sizeof g_err, "align: --max-altstried arg must be at least 8"); return H2G_ERR_ARG; }
	// (a read longer than H2G_SW_MAX_ROWS is flagged by the kernel — overflow bit 256 — instead of run through the DP)
	if(p->bowtie2_dp && s->cur().max_read_len == 0) return H2G_ERR_ARG;
	return H2G_OK;
}

// what a run does, from its options, the batch and the stream's knobs: no device calls, no side effects
struct GoPlan {
	bool linear, spl, xl, big_main, fast, second;
	bool fast_spl;                 // the fast pass is the build for spliced runs (h2g_k_go_fast_spl.hip): its hand-ons go to the spliced machine units
	const GoUnitDesc *U, *L;       // the main pass's unit; the large-workspace unit (the second pass, the machine streams' warm-up)
	unsigned grid, M, bgrid;       // workgroups of the main pass; lanes (per-run buffers: M + 1 deep; area parts: M); workgroups of a second pass
	unsigned S;                    // machine streams in rotation: lane m's pass runs on mst[m % S]
	unsigned mach_cap, pool_cap;   // workgroups of one machine pass behind a fast pass, and what its pools are sized for
	size_t units;                  // batch units: pairs, or two unpaired reads
};
// Machine streams in rotation, from the load (no device calls, no state): a pinned value as it is; a graph index, and a linear one whose latest finished
// fast pass handed on more than 1.5 % of the batch (the regime of mach_total below: the machine's passes are the step), every lane its own stream; otherwise `light`.
static unsigned mstreams_policy(size_t units, uint32_t last_bails, bool linear, unsigned pinned, unsigned light) {
	if(pinned) return pinned > H2G_MSTREAMS_MAX ? H2G_MSTREAMS_MAX : pinned;
	if(!linear || (size_t)last_bails * 1000 > units * 15) return H2G_MSTREAMS_MAX;
	return light < 1 ? 1u : light > H2G_MSTREAMS_MAX ? (unsigned)H2G_MSTREAMS_MAX : light;
}
// development hook (tests): the policy above, as it is
extern "C" __attribute__((visibility("default"))) unsigned h2g_mstreams_policy(unsigned long long units, unsigned last_bails, int linear, unsigned pinned, unsigned light) {
	return mstreams_policy((size_t)units, last_bails, linear != 0, pinned, light);
}
static GoPlan go_plan(const h2g_stream* s, const h2g_align_params* p, bool paired) {
	GoPlan plan, *g = &plan;
	const size_t n_reads = s->cur().n_reads;
	g->linear = s->ix->dg.linear != 0;
	// --haplotype is compiled into the units that also carry the splice-site database (H2G_HAPLOTYPE, h2g_graph.h); they run either mode
	// ... and so are -I, --rf / --ff, --nofw / --norc (H2G_EXT_OPTS, h2g_align.h)
	// ... and --avoid-pseudogene / --tmo (al_report's transcriptome policy; --tmo also under --no-spliced-alignment)
	const bool ext_opts = pe_flags_from(*p) != H2G_PE_DEFAULT || p->min_frag_len != 0 || p->transcriptome_mapping_only || (p->avoid_pseudogene && !p->no_spliced_alignment);
	g->spl = !p->no_spliced_alignment || (p->use_haplotype && !g->linear) || ext_opts;
	const uint32_t maxsz = p->khits > p->kseeds ? p->khits : p->kseeds;
	g->L = &go_unit(g->linear, true, g->spl);
	const uint32_t* const caps = go_unit(g->linear, false, g->spl).caps, * const bcaps = g->L->caps;   // ([0]: AL_MAX_GHITS)
	// a run beyond what the large units hold (more alignments selected than H2G_SELECT_CAP, or a list beyond their AL_MAX_GHITS) runs on the
	// extra-large units (h2g_go_xl.h), whole: no fast pass, no second pass
	g->xl = p->khits > H2G_SELECT_CAP || maxsz > bcaps[0];
	g->big_main = maxsz > caps[0];                  // (every XL run is one: khits > 32 or maxsz > 64 exceeds the default units' lists)
	g->U = &go_unit(g->linear, g->big_main, g->spl, g->xl);
	// (graph indexes: h2g_k_go_fast_graph.hip, the same pass over the graph form of the compact state; --haplotype and the pair-policy options are `spl`)
	g->fast = s->tune.fast && !g->spl && !g->big_main && p->no_spliced_alignment && !p->secondary && !p->bowtie2_dp;
	// spliced alignment on a linear index (the reference's default run): the build of the pass under the spliced rules takes the reads whose whole trace stays
	// unspliced and hands every other read on to the spliced units (h2g_stream_tune "fast_spliced")
	g->fast_spl = s->tune.fast && s->tune.fast_spliced && g->linear && !p->no_spliced_alignment && !ext_opts && !g->big_main && !p->secondary && !p->bowtie2_dp;
	if(g->fast_spl) g->fast = true;
	g->second = !g->big_main && !s->tune.no_second_pass;     // (no_second_pass: a measurement / debugging knob)
	// geometry of the unit: workgroups of `threads` threads own `slots` reads in flight; resident workgroups per CU = what the
	// unit's waves per SIMD and the LDS (rings + one packed-read region per mate) allow
	size_t per_cu = (size_t)g->U->waves * 256 / g->U->threads;
	const size_t lds_blocks = (160u * 1024u) / (g->U->lds_ring_bytes + (paired ? 2u : 1u) * g->U->lds_pack_bytes);
	if(per_cu > lds_blocks) per_cu = lds_blocks;
	if(per_cu < 1) per_cu = 1;
	if(s->tune.blocks_per_cu > 0) per_cu = (size_t)s->tune.blocks_per_cu;
	const size_t want = (n_reads + g->U->slots - 1) / g->U->slots;
	size_t maxblocks = 256 * per_cu;
	if(g->big_main && maxblocks > 32) maxblocks = 32;        // ~1.3 MB of workspace per read in flight
	if(g->xl && maxblocks > 12) maxblocks = 12;              // XL: 18.7 MB per read in flight, 12 x 128 of them (h2g_go_xl.h)
	g->grid = (unsigned)(want < 1 ? 1 : (want > maxblocks ? maxblocks : want));
	g->M = s->mstreams ? s->mstreams : H2G_MSTREAMS_MAX;
	// workgroups of one machine pass behind a fast pass: mach_total / M (the lanes, whatever S: a pass is the same pass on any stream).  The default policy follows the batch: when the fast pass hands on more than 1.5 % of a linear index's
	// batch (repeat-structured sequence: the machine's passes, not the fast pass, are the step) the passes get 192 workgroups in all instead of 128 — measured on the repeat-structured
	// leg 44.7 -> 40.3 ms per step, while the fast-pass-bound legs (0.8 % handed on) lose 3 % with it (profiles/r05_NOTES.md §6).  The pools are sized for the larger share from the start.
	const bool mt_auto = s->tune.mach_total_auto != 0 && g->linear;
	g->units = paired ? n_reads : (n_reads + 1) / 2;
	const unsigned mach_total_now = mt_auto && (size_t)s->last_bails * 1000 > g->units * 15 ? 192u : s->tune.mach_total;
	g->S = mstreams_policy(g->units, s->last_bails, g->linear, s->mstreams, s->mstreams_light);
	g->mach_cap = mach_total_now / g->M;
	if(g->mach_cap > H2G_MACH_MAXGRID) g->mach_cap = H2G_MACH_MAXGRID;
	if(g->mach_cap < 1) g->mach_cap = 1;
	g->pool_cap = (mt_auto ? 192u : s->tune.mach_total) / g->M;      // what the pools are sized for
	if(g->pool_cap > H2G_MACH_MAXGRID) g->pool_cap = H2G_MACH_MAXGRID;
	if(g->pool_cap < g->mach_cap) g->pool_cap = g->mach_cap;
	g->bgrid = g->fast ? 2u : 4u;                                    // (large workspace: ~5 MB per read in flight)
	return plan;
}

// the fast pass's share of a run (h2g_fast.h), decided by fast_policy
struct FastPlan {
	bool use_am, mate_ho;          // alignMate in the pass; pairs that need it parked for the drain launch (its alignMate build)
	bool ps0;                      // the first partial searches run in a pre-pass in front of the fast launch (h2g_k_ps0.hip)
	const FastUnitDesc *FU, *DU;   // the fast launch's build of the pass and the drain launch's
	unsigned fgrid, mgrid, dgrid;  // workgroups of the fast launch, of the machine pass behind it, of the drain launch
	uint32_t orphan_T;             // > 0: the end of the batch goes to a drain launch
	h2g_stream::FastPool* pool;    // the slot pool of the fast launch (gen % H2G_FAST_POOLS with a drain launch, the first without) ...
	size_t slot_bytes;             // ... and its size
};
// what a run queued now carries through to the end of go_run: its record of each index space (h2g_stream)
struct GoRun {
	GoArgs A; DExonTbl X; XlPairs XP;   // the main pass's arguments (X: --avoid-pseudogene's exons, an argument of their own)
	h2g_stream::RunSet* set;       // the per-run buffer set, gen % (M + 1) ...
	unsigned long long* cblk;      // ... and its counter block (h2g_go_args.h)
	unsigned lane;                 // the run's parts of the three areas: gen % M behind a fast pass, 0 otherwise
	h2g_stream::MachStream* mach;  // the machine stream of the lane, lane % S: its pools and overflow list are the main pass's ...
	hipStream_t ms;                // ... which runs on its HIP stream behind a fast pass, on the first stream otherwise ...
	unsigned mach_grid;            // ... on this many workgroups
	FastPlan f;
	uint32_t* ovl;                 // the main pass's overflow list (+ its count behind it)
};

// the main pass's argument block, less its pools, result rows and counters
static void go_args(const h2g_stream* s, const h2g_align_params* p, bool paired, const GoPlan& g, GoRun* r) {
	const BatchCtx& b = s->cur();
	GoArgs& A = r->A;
	memset(&A, 0, sizeof A);
	A.g = dg_now(s->ix); A.ref = s->ix->dr; A.ls = dls_now(s->ix); A.alts = s->ix->dalts;
	if(p->max_alts_tried) A.alts.maxAltsTried = p->max_alts_tried;          // --max-altstried
	if(p->use_haplotype && !g.linear && A.alts.n) A.alts.has_splice |= 2u;   // --haplotype: the table behind the ALTs is read (h2g_graph.h haps_of)
	A.rd1 = dreads(s); A.rd2 = A.rd1;
	if(paired) { A.rd2.codes = b.d_codes2; A.rd2.offs = b.d_offs2; A.rd2.quals = b.has_quals2 ? b.d_quals2 : nullptr; }
	if(b.has_seeds) { A.rd1.seeds = b.d_seeds; A.rd2.seeds = paired ? b.d_seeds + s->max_reads : b.d_seeds; }   // every launch of the run copies rd1 / rd2
	if(b.has_ids) { A.rd1.ids = b.d_ids; A.rd2.ids = b.d_ids; }
	if(b.has_qc) { A.rd1.qc = b.d_qc; A.rd2.qc = paired ? b.d_qc + s->max_reads : b.d_qc; }
	A.P = aln_params_from(*p, p->no_spliced_alignment != 0, g.linear);
	if(!p->no_spliced_alignment) { A.ssdb = s->ix->dssdb; A.rdid_base = p->first_read_id; }
	r->X = p->no_spliced_alignment ? DExonTbl() : s->ix->dexons;
	if(!p->no_spliced_alignment) { A.P.sc.donor_sum = s->ix->d_spl[0]; A.P.sc.acc_sum1 = s->ix->d_spl[1]; A.P.sc.acc_sum2 = s->ix->d_spl[2]; }
	A.names1 = b.d_names; A.noffs1 = b.d_name_offs; A.names2 = b.d_names2; A.noffs2 = b.d_name_offs2;
	A.paired = paired ? 1u : 0u;
}

// the run's record of each index space (h2g_stream).  A run that is not behind a fast pass is lane 0 on the first stream, with machine stream 0's pools and overflow list
static void go_select(h2g_stream* s, const GoPlan& g, GoRun* r) {
	r->set = &s->run[s->gen % (g.M + 1)];
	r->cblk = s->counters(*r->set);
	r->lane = g.fast ? s->gen % g.M : 0u;
	r->mach = &s->mach[r->lane % g.S];
}

// The machine streams in rotation for a run behind a fast pass: mst[0 .. S); n_mst counts those that ever entered (the others hold nothing to wait for).  When S changes, lane m moves from stream
// m % S' to m % S: what it shares with its earlier passes (its parts' cursors, the rows of a batch) was ordered by the stream, so every stream of the new
// rotation waits for everything queued on the streams in use — on the device: the host never waits here.
static int go_rotation(h2g_stream* s, const GoPlan& g) {
	if(s->n_mst < g.S) s->n_mst = g.S;
	if(s->rot && s->rot != g.S && s->st2_busy) {
		for(unsigned j = 0; j < s->rot; j++) HIPCHK(hipEventRecord(s->mach[j].ev_rot, s->mst[j]));
		for(unsigned k = 0; k < g.S; k++) for(unsigned j = 0; j < s->rot; j++) if(j != k) HIPCHK(hipStreamWaitEvent(s->mst[k], s->mach[j].ev_rot, 0));
	}
	s->rot = g.S;
	return H2G_OK;
}

// the main pass's per-lane scratch: behind a fast pass the machine works on the lane's machine stream with that stream's pools, on at most mach_cap workgroups
static int go_pools(h2g_stream* s, const h2g_align_params* p, const GoPlan& g, GoRun* r) {
	const size_t pgrid = g.fast && g.grid > g.pool_cap ? (size_t)g.pool_cap : (size_t)g.grid;
	int rc;
	if(g.fast && s->cur().n_reads >= 200000) {
		// large batches (a streaming caller's): the pools of every machine stream in rotation exist before the first pass that could need them — an allocation
		// in the middle of a queue of runs (gigabytes, synchronous) would stall all of them.  The stream's SECOND run pays for it, once (round 6: a caller with one
		// batch — a command line over a million pairs — never needs streams 1 .. S - 1: their 30 GB of pools were a second of its three); a stream that enters the
		// rotation later (the regime turns heavy) gets its pools then.
		// (Small batches keep allocating a machine stream's pools when it is first used.)
		GoArgs scratch = r->A;
		for(unsigned k = 0; k < g.S && s->gen >= 1; k++) {
			h2g_stream::MachStream& m = s->mach[k];
			if((rc = go_pool_for(s, m.main, *g.U, pgrid * g.U->slots, pgrid * g.U->threads, p->bowtie2_dp, &scratch))) return rc;
			if(g.second && (rc = go_pool_for(s, m.second, *g.L, (size_t)g.bgrid * g.L->slots, (size_t)g.bgrid * g.L->threads, p->bowtie2_dp, &scratch))) return rc;
			// ... and its overflow list
			if(!m.ovf_list) { HIPCHK(m.ovf_list.ensure(s->max_reads + 4)); HIPCHK(hipMemsetAsync(m.ovf_list + s->max_reads, 0, 16, s->stream_of(m))); }
		}
		for(unsigned k = 0; k < g.M + 1; k++) {      // the per-run buffers of every generation
			h2g_stream::RunSet& b = s->run[k];
			HIPCHK(b.bail_list.ensure(s->max_reads + 4));
			HIPCHK(b.fast_args.ensure(1));
			HIPCHK(b.drain_args.ensure(1));
		}
	}
	return go_pool_for(s, r->mach->main, *g.U, pgrid * g.U->slots, pgrid * g.U->threads, p->bowtie2_dp, &r->A);
}

// the batch's result rows (grown to this run's -k), the pairs' overflow area and the XL units' side area
static int go_rows(h2g_stream* s, const h2g_align_params* p, bool paired, const GoPlan& g, GoRun* r) {
	BatchCtx& b = s->cur();
	GoArgs& A = r->A;
	memset(&A.O, 0, sizeof A.O);
	if(!paired) {
		HIPCHK(b.d_rout.ensure(s->max_reads));
		const uint32_t slots = p->khits;
		HIPCHK(b.d_aln.reserve(s->max_reads * (size_t)slots));
		b.aln_slots = slots;
		A.O.rout = b.d_rout; A.O.aln = b.d_aln; A.O.aln_slots = slots;
	} else {
		HIPCHK(b.d_pout.ensure(s->max_reads));
		// a mate can report more alignments than -k before the pair is settled: 2 k + 4 slots, at least H2G_PAIR_RES_CAP
		uint32_t pslots = p->khits * 2 + 4;
		if(pslots < H2G_PAIR_RES_CAP) pslots = H2G_PAIR_RES_CAP;
		if(s->tune.pair_slots > 0) pslots = (uint32_t)s->tune.pair_slots;   // test knob: tiny rows push pairs through the overflow area (dense fetch only)
		for(int m = 0; m < 2; m++) HIPCHK(b.d_paln[m].reserve(s->max_reads * (size_t)pslots));
		b.pair_slots = pslots;
		A.O.pout = b.d_pout; A.O.paln[0] = b.d_paln[0]; A.O.paln[1] = b.d_paln[1]; A.O.pair_slots = pslots;
		// One part per lane: the machine passes of M queued runs may be in flight together and each takes its blocks
		// from its own cursor.  Block offsets (PairOut::pad) are relative to the whole area, so whichever pass wrote a pair last, its block is found.
		const size_t ovf_cap = s->max_reads / 4 > 65536 ? s->max_reads / 4 : 65536;   // records per part
		if(!s->paln_ovf.fits(g.M, ovf_cap)) {
			HIPCHK(sync_mach(s));
			HIPCHK(hipStreamSynchronize(s->st));
			HIPCHK(s->paln_ovf.reset(g.M, ovf_cap));
		}
		A.O.ovf = s->paln_ovf;
	}
	memset(&r->XP, 0, sizeof r->XP);
	if(paired && g.xl) {
		// the XL units' side area: a word per read, and per lane a part of lists with a cursor (an XL run is never behind a fast pass: it
		// runs on the first stream and uses part 0, but the area is partitioned the way the overflow area is)
		const size_t xcap = s->max_reads * 64 > ((size_t)1 << 20) ? s->max_reads * 64 : ((size_t)1 << 20);      // words per part
		if(s->d_xlp_at.size() < s->max_reads || !s->xlp.fits(g.M, xcap) || !s->d_xlp_cur) {
			HIPCHK(hipStreamSynchronize(s->st));
			HIPCHK(s->d_xlp_at.reset(s->max_reads));
			HIPCHK(s->xlp.reset(g.M, xcap));
			HIPCHK(s->d_xlp_cur.ensure(H2G_MSTREAMS_MAX));
		}
		HIPCHK(hipMemsetAsync(s->d_xlp_at, 0, b.n_reads * 4, s->st));
		HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(s->d_xlp_cur + r->lane), (int)s->xlp.lo(r->lane), 1, s->st));
		r->XP.at = s->d_xlp_at; r->XP.list = s->xlp; r->XP.cursor = s->d_xlp_cur + r->lane; r->XP.cap = (uint32_t)s->xlp.hi(r->lane);
	}
	if(paired) s->xlp_pout = g.xl ? b.d_pout : (s->xlp_pout == b.d_pout ? nullptr : s->xlp_pout);
	return H2G_OK;
}

// the run's counter block (its buffer set's: h2g_stream::RunSet) and cursors
static int go_counters(h2g_stream* s, bool paired, const GoPlan& g, GoRun* r) {
	GoArgs& A = r->A;
	HIPCHK(hipStreamWaitEvent(s->st, r->set->ev_mach, 0));          // run k - NB's machine pass: done with this set of buffers
	HIPCHK(hipMemsetAsync(r->cblk, 0, H2G_CNT_BLOCK * sizeof(unsigned long long), s->st));
	A.counters = r->cblk;
	A.work = reinterpret_cast<uint32_t*>(r->cblk + H2G_CNT_WORK_MAIN);
	if(paired) {   // the cursor starts at this lane's part of the area
		A.O.ovf_cursor = reinterpret_cast<uint32_t*>(r->cblk + H2G_CNT_OVF_CURSOR);
		A.O.ovf_cap = (uint32_t)s->paln_ovf.hi(r->lane);
		if(r->lane) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)A.O.ovf_cursor, (int)s->paln_ovf.lo(r->lane), 1, s->st));
	}
	A.list = nullptr; A.nlist = nullptr;
	if(s->tune.dbg_read >= 0) {
		HIPCHK(s->dbg_buf.ensure(1u << 20));      // (the stream's own: a device's memory, not the process's)
		HIPCHK(hipMemsetAsync(s->dbg_buf, 0, (1u << 20) * 4, s->st));
		A.dbg_buf = s->dbg_buf; A.dbg_read = (uint32_t)s->tune.dbg_read;
	}
	A.defer_overflow = g.second ? 1u : 0u;
	return H2G_OK;
}

// ---- the fast pass (h2g_fast.h): the dominant traces with the per-read state on chip.  What it completes is final; the reads
// it hands on (a device-side list, no host sync) are the general machine's batch.  Built for unspliced alignment (linear and graph
// indexes) and for spliced alignment on a linear index (GoPlan::fast_spl), with the default pair policy; every other option set goes to the machine whole.
// Its policy: geometry, the CUs it takes, the machine pass's share, whether a drain launch finishes the batch
static void fast_policy(h2g_stream* s, bool paired, const GoPlan& g, FastPlan* f) {
	const size_t n_reads = s->cur().n_reads;
	const bool linear = g.linear;
	*f = FastPlan();
	f->use_am = linear && paired && s->tune.align_mate != 0 && !g.fast_spl;      // (alignMate differs in spliced mode: such pairs are the machine's)
	f->FU = &fast_unit(linear, g.fast_spl, f->use_am);
	// CUs: one persistent fast workgroup each (LDS-bound), minus the few the machine pass of the PREVIOUS run may still hold
	// (the machine takes ~150 hand-ons per workgroup in half the time of a fast pass; the count is the last finished fast pass's)
	const unsigned NB = g.M + 1;
	for(unsigned back = 1; back < NB && back <= s->gen; back++) {                           // the latest fast pass that is over
		const h2g_stream::RunSet& b = s->run[(s->gen - back) % NB];
		if(hipEventQuery(b.ev_bails) == hipSuccess) { s->last_bails = s->h_bail(b); break; }
	}
	(void)hipGetLastError();
	// hand-ons per machine workgroup (latency chains, two passes in flight).  Linear index: 400 — the fast pass is short and the machine's pass bounds the
	// step.  Graph index: the fast pass bounds the step and every machine workgroup costs it two of its 256 (one per CU), while the machine's pass only
	// has to end within two steps — so large batches give the machine less: 400 per workgroup up to 500 k batch units (pairs, or two unpaired reads), rising
	// to 1600 at 1 M and beyond.  Measured steady steps, SNP graphs over 8-256 Mbp (profiles/r04_graph_scale.jsonl, r04_graph_scale2.jsonl):
	//   500 k pairs: machine alone 55.3 ms | 400: 51.0 | 800: 55.2 | 1600: 70.6        1 M pairs (32 Mbp): alone 103.1 | 200: 110.0 | 400: 106.1 | 1600: 94.7 | 3200: 129.4
	//   2 M pairs: alone 194.6 | 1600: 171.1 | 3200: 176.4                               1 M pairs, 128 / 256 Mbp: alone 110.6 / 119.6 | 400: 113.7 / 122.7 | 1600: 101.5 / 109.2
	unsigned mach_div = s->tune.mach_div;
	if(mach_div == 0) {
		mach_div = 400;
		if(!linear) {
			const size_t units = paired ? n_reads : n_reads / 2;
			if(units >= 1000000) mach_div = 1600;
			else if(units > 500000) mach_div = 400 + (unsigned)((units - 500000) * 1200 / 500000);
		}
	}
	f->mgrid = (unsigned)((s->last_bails + mach_div - 1) / (mach_div ? mach_div : 1u));
	if(f->mgrid < s->tune.mach_min) f->mgrid = s->tune.mach_min;
	if(f->mgrid > g.mach_cap) f->mgrid = g.mach_cap;
	// (Tried on repeat-rich sequence, 27 000 hand-ons: a share that follows the measured work of the two passes, m = 128 M / (F + M) — the machine's
	// pass stayed a latency chain, 78 -> 66 ms on twice the workgroups, while the fast pass went 14.5 -> 49 ms on what was left; and the second pass
	// on a stream of its own — the extra queues cost the common case 13 -> 20 ms per run.  Neither ships: profiles/r04_NOTES.md §6.)
	const size_t fwant = (n_reads + 127) / 128;                                                // small batches spread over the chip
	unsigned reserve = s->tune.fast_reserve >= 0 ? (unsigned)s->tune.fast_reserve : g.S * f->mgrid;  // (S machine passes may run side by side)
	if(reserve > 192) reserve = 192;
	const unsigned fmax = 256 - reserve;
	f->fgrid = (unsigned)(fwant < 1 ? 1 : (fwant > fmax ? fmax : fwant));
	f->slot_bytes = (size_t)256 * f->FU->slots * f->FU->slot_bytes;
	// the end of the batch goes to a drain launch (h2g_k_go_fast.hip) when the batch is large enough to have one
	f->orphan_T = s->tune.orphan >= 0 ? (uint32_t)s->tune.orphan : (g.units >= H2G_ORPHAN_MIN_UNITS ? (uint32_t)H2G_ORPHAN_T : 0u);
	if(f->orphan_T > f->FU->slots) f->orphan_T = f->FU->slots;
	if(f->FU->gws_bytes != 0) f->orphan_T = 0;                          // (a graph unit with GraphWS in global memory: its scratch is sized for one launch)
	f->dgrid = (unsigned)(s->tune.drain_grid < 1 ? 1 : s->tune.drain_grid);
	// pairs that need alignMate (hi_aligner.h:5579): with a drain launch there, the fast launch parks them and the drain launch is the alignMate build of the pass (k_go_fast_am_drain)
	// — the hot loop keeps the lighter build, the machine sees neither them nor the tail (h2g_stream_tune "mate_handover": -1 this policy, 0 off, 1 on)
	f->mate_ho = f->orphan_T != 0 && linear && paired && !f->use_am && !g.fast_spl && s->tune.mate_handover != 0;
	f->DU = &fast_unit(linear, g.fast_spl, f->use_am || f->mate_ho);
	f->pool = &s->fpool[f->orphan_T ? s->gen % H2G_FAST_POOLS : 0u];
	// the first partial searches in front of the loop: the linear non-spliced builds (h2g_stream_tune "ps0": -1 this policy, 0 off, 1 on)
	f->ps0 = linear && !g.fast_spl && (s->tune.ps0 < 0 ? H2G_DEFAULT_PS0 != 0 : s->tune.ps0 != 0);
}

// every buffer of the two launches exists (and has been written once: fresh device memory costs its first writer the mapping) before the first run that could need it
static int fast_buffers(h2g_stream* s, const GoPlan& g, const FastPlan& f) {
	const size_t ocap = (size_t)256 * f.FU->slots, dbytes = (size_t)f.dgrid * f.DU->slots * f.DU->slot_bytes;
	const size_t dsc = g.linear ? 0 : (size_t)f.dgrid * f.FU->threads * (size_t)(2 * H2G_COMBINE_MAXLEN * sizeof(int64_t));
	// the pools a run may meet: with a drain launch all of them (the following runs' go round), without one its own
	h2g_stream::FastPool* const pools = f.orphan_T ? s->fpool : f.pool;
	const unsigned npools = f.orphan_T ? (unsigned)H2G_FAST_POOLS : 1u;
	bool need = f.pool->slots.size() < f.slot_bytes;
	if(f.orphan_T) {
		for(unsigned q = 0; q < npools; q++) need = need || pools[q].slots.size() < f.slot_bytes;
		need = need || s->d_drain_slots.size() < dbytes || s->d_drain_sc.size() < dsc;
		for(unsigned b = 0; b < g.M + 1; b++) need = need || !s->run[b].orphans || !s->run[b].drain_args;
		need = need || s->orphan_cap < ocap;
	}
	const size_t pswords = (size_t)s->max_reads * 4 * FG_PS0_WORDS;     // one record per (unit, mate, strand)
	if(f.ps0) for(unsigned q = 0; q < npools; q++) need = need || pools[q].ps0.size() < pswords;
	if(!need) return H2G_OK;
	// (every stream, whatever st2_busy and dst_busy say: the pools about to be freed may be any launch's)
	HIPCHK(hipStreamSynchronize(s->st)); HIPCHK(hipStreamSynchronize(s->dst)); for(unsigned k = 0; k < s->n_mst; k++) HIPCHK(hipStreamSynchronize(s->mst[k]));
	// (fresh memory is written once, on the first stream)
	for(unsigned q = 0; q < npools; q++) {
		DevBuf<uint8_t>& fs = pools[q].slots;
		if(fs.size() < f.slot_bytes) { HIPCHK(fs.reserve(f.slot_bytes)); HIPCHK(hipMemsetAsync(fs, 0, f.slot_bytes, s->st)); }
		DevBuf<uint32_t>& ps = pools[q].ps0;
		if(f.ps0 && ps.size() < pswords) { HIPCHK(ps.reserve(pswords)); HIPCHK(hipMemsetAsync(ps, 0xff, pswords * 4, s->st)); }
	}
	if(f.orphan_T) {
		if(s->orphan_cap < ocap) { for(h2g_stream::RunSet& b : s->run) b.orphans = DevBuf<uint32_t>(); s->orphan_cap = ocap; }
		for(unsigned k = 0; k < g.M + 1; k++) {
			h2g_stream::RunSet& b = s->run[k];
			if(!b.orphans) { HIPCHK(b.orphans.ensure(s->orphan_cap + 4)); HIPCHK(hipMemsetAsync(b.orphans, 0, (s->orphan_cap + 4) * 4, s->st)); }
			HIPCHK(b.drain_args.ensure(1));
		}
		if(s->d_drain_slots.size() < dbytes) { HIPCHK(s->d_drain_slots.reserve(dbytes)); HIPCHK(hipMemsetAsync(s->d_drain_slots, 0, dbytes, s->st)); }
		if(s->d_drain_sc.size() < dsc) { HIPCHK(s->d_drain_sc.reserve(dsc)); HIPCHK(hipMemsetAsync(s->d_drain_sc, 0, dsc, s->st)); }
	}
	HIPCHK(hipStreamSynchronize(s->st));
	return H2G_OK;
}

// the fast launch (and the drain launch's argument block) on the first stream; the main pass then takes the hand-on list
static int fast_launch(h2g_stream* s, bool paired, const GoPlan& g, GoRun* r) {
	const FastPlan& f = r->f;
	const GoArgs& A = r->A;
	h2g_stream::RunSet& set = *r->set;
	// run k - 3's drain launch is done with this pool — and a run WITHOUT a drain launch (a small resident batch queued behind a large one) uses pool 0, which the drain launch
	// of an earlier run may still be reading: every fast launch waits for the last reader of its pool
	HIPCHK(hipStreamWaitEvent(s->st, f.pool->ev_last, 0));
	HIPCHK(set.bail_list.ensure(s->max_reads + 4));
	uint32_t* const bl = set.bail_list;
	HIPCHK(hipMemsetAsync(bl + s->max_reads, 0, 16, s->st));
	FastArgs F;
	memset(&F, 0, sizeof F);
	F.g = A.g; F.ref = A.ref; F.ls = A.ls; F.rd1 = A.rd1; F.rd2 = A.rd2; F.P = A.P;
	F.names1 = A.names1; F.noffs1 = A.noffs1; F.names2 = A.names2; F.noffs2 = A.noffs2;
	F.slots = (uint32_t*)f.pool->slots.get();
	F.O.rout = A.O.rout; F.O.aln = A.O.aln; F.O.aln_slots = A.O.aln_slots; F.O.pout = A.O.pout; F.O.paln[0] = A.O.paln[0]; F.O.paln[1] = A.O.paln[1]; F.O.pair_slots = A.O.pair_slots;
	F.counters = r->cblk; F.work = reinterpret_cast<uint32_t*>(r->cblk + H2G_CNT_WORK_FAST);
	F.bail_list = bl; F.bail_count = bl + s->max_reads;
	F.total = (uint32_t)s->cur().n_reads; F.paired = paired ? 1u : 0u;
	F.alts = A.alts; F.gws_base = nullptr; F.gws_stride = 0; F.sc_base = nullptr;
	F.dbg_read = A.dbg_read; F.dbg_buf = A.dbg_buf;
	F.ps0 = f.ps0 ? f.pool->ps0.get() : nullptr;                        // (the drain launch reads run k's table beside run k + 1: D = F below)
	F.ssdb = A.ssdb; F.rdid_base = A.rdid_base;                          // (spliced runs: the database of this run — a wave of the temporary-splice-site mode brings its own)
	// (single-end batches and graph indexes: there the machine's pass is the longer of the two already — NOTES §1, §3: 47 -> 53 ms per 500 k graph pairs with it)
	F.tail = g.linear && paired && s->tune.tail > 0 ? (uint32_t)s->tune.tail : 0u;
	if(!g.linear) {   // per-lane scratch of the graph primitives (every CU may hold a workgroup)
		const size_t lanes = (size_t)256 * f.FU->threads;
		HIPCHK(s->d_fast_gws.reserve(lanes * f.FU->gws_bytes));
		HIPCHK(s->d_fast_sc.reserve(lanes * (size_t)(2 * H2G_COMBINE_MAXLEN * sizeof(int64_t))));
		F.gws_base = s->d_fast_gws; F.gws_stride = f.FU->gws_bytes; F.sc_base = s->d_fast_sc;
	}
	HIPCHK(set.fast_args.ensure(1));
	FastArgs D = F;
	if(f.orphan_T) {
		uint32_t* const ol = set.orphans;
		HIPCHK(hipMemsetAsync(ol + s->orphan_cap, 0, 16, s->st));
		F.orphan_T = f.orphan_T; F.orphan_list = ol; F.orphan_count = ol + s->orphan_cap; F.mate_handover = f.mate_ho ? 1u : 0u;
		D.adopt_slot_words = f.FU->slot_bytes / 4;
		// The drain launch's own tail (the last reads of each of its workgroups go to the machine).  With few hand-ons the machine's passes are short and the tail is a third of
		// what they get: the drain launch finishes its reads itself (lease ZE, random genome: 11.48 -> 11.16 ms per step, hand-ons 2 830 -> 1 880); where the machine's passes are
		// the step (more than 1.5 % handed on: the policy of mach_total) they absorb the tail for nothing and a drain launch that runs to its last read would be the longer one
		// (repeat-structured: 37.8 -> 39.0 ms with it): the tail stays.  A caller's own setting (H2G_FAST_TAIL, "tail") is kept as it is.
		if(s->tune.tail_auto) D.tail = g.linear && paired && (size_t)s->last_bails * 1000 > g.units * 15 ? (uint32_t)H2G_DEFAULT_TAIL : 0u;
		D.slots = (uint32_t*)s->d_drain_slots.get();
		D.adopt_list = ol; D.adopt_count = ol + s->orphan_cap; D.adopt_slots = F.slots;
		D.work = reinterpret_cast<uint32_t*>(r->cblk + H2G_CNT_WORK_DRAIN);
		D.cnt_off = H2G_CNT_DRAIN_OFF;                               // its own rank / side / step / aligned counters
		D.total = 0;
		if(!g.linear) D.sc_base = s->d_drain_sc;
		s->orph_cur = ol + s->orphan_cap;
	}
	// through pinned memory: a pageable source would make this call wait for everything queued on the stream (the previous run's fast
	// pass), and the chip would idle while the host queues this run.  The staging block of this buffer set was last read by the upload
	// of run k - H2G_NBUF, which is over once that run's fast pass is
	if(s->gen >= g.M + 1 && hipEventQuery(set.ev_fast) != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipEventSynchronize(set.ev_fast)); }
	FastArgs* const hF = s->h_fast(set);
	*hF = F;
	HIPCHK(hipMemcpyAsync(set.fast_args, hF, sizeof F, hipMemcpyHostToDevice, s->st));
	if(f.orphan_T) {
		FastArgs* const hD = s->h_drain(set);
		*hD = D;
		HIPCHK(hipMemcpyAsync(set.drain_args, hD, sizeof D, hipMemcpyHostToDevice, s->st));
	}
	// the pre-pass: behind whatever produced the reads and behind the last reader of its table (stream order, the pool's ev_last above), in front of the loop that reads it
	if(f.ps0 && h2g_ps0_launch(set.fast_args, F.total, paired, s->st) != 0) return set_err("go() first-search pre-pass launch", hipGetLastError());
	if(f.FU->launch(set.fast_args, f.fgrid, s->st) != 0) return set_err("go() fast pass launch", hipGetLastError());
	r->A.list = bl; r->A.nlist = bl + s->max_reads;
	return H2G_OK;
}

// the stream hand-off behind a fast pass: the machine works on the lane's machine stream (a short list on few workgroups: the next run's fast pass does not wait for it),
// after the drain launch when there is one
static int fast_handoff(h2g_stream* s, bool paired, const GoPlan& g, GoRun* r) {
	const FastPlan& f = r->f;
	h2g_stream::RunSet& set = *r->set;
	HIPCHK(hipEventRecord(set.ev_fast, s->st));
	r->ms = s->stream_of(*r->mach); s->st2_busy = true;
	if(f.mgrid < r->mach_grid) r->mach_grid = f.mgrid;
	if(f.orphan_T) {
		// the drain launch: the reads the fast launch's workgroups left in flight, on the drain stream next to the following run's fast launch; the machine's pass needs its hand-ons too
		HIPCHK(hipStreamWaitEvent(s->dst, set.ev_fast, 0));
		HIPCHK(hipEventRecord(s->ev_dr[0], s->dst));
		if(f.DU->launch_drain(set.drain_args, f.dgrid, s->dst) != 0) return set_err("go() drain launch", hipGetLastError());
		HIPCHK(hipEventRecord(s->ev_dr[1], s->dst));
		HIPCHK(hipEventRecord(f.pool->ev_last, s->dst));
		HIPCHK(hipMemcpyAsync(&s->h_bail(set), set.bail_list + s->max_reads, 4, hipMemcpyDeviceToHost, s->dst));
		HIPCHK(hipEventRecord(set.ev_drain, s->dst));
		HIPCHK(hipEventRecord(set.ev_bails, s->dst));
		HIPCHK(hipStreamWaitEvent(r->ms, set.ev_drain, 0));
		s->ran_drain = true; s->dst_busy = true;
	} else {
		HIPCHK(hipMemcpyAsync(&s->h_bail(set), set.bail_list + s->max_reads, 4, hipMemcpyDeviceToHost, s->st));
		HIPCHK(hipEventRecord(set.ev_bails, s->st));
		HIPCHK(hipStreamWaitEvent(r->ms, set.ev_fast, 0));
	}
	return H2G_OK;
}

// the machine stream's overflow list and the lane's part of the long-edit area
static int go_mach_lists(h2g_stream* s, const GoPlan& g, GoRun* r) {
	GoArgs& A = r->A;
	const unsigned lane = r->lane;
	s->ovf_cur = r->mach;
	HIPCHK(r->mach->ovf_list.ensure(s->max_reads + 4));
	r->ovl = r->mach->ovf_list;
	HIPCHK(hipMemsetAsync(r->ovl + s->max_reads, 0, 16, r->ms));
	// the long-edit area: this lane's part and its cursor (the pass that used them last is over: it ran on the same stream, or go_rotation made this stream wait for it)
	const size_t lcap = s->max_reads > (1u << 20) ? s->max_reads : (size_t)(1u << 20);
	if(!s->ledits.fits(g.M, lcap) || !s->d_ledits_cur) {
		// (the flag stays: this run's own fast pass, already queued, has set it)
		if(s->st2_busy) for(unsigned k = 0; k < s->n_mst; k++) HIPCHK(hipStreamSynchronize(s->mst[k]));
		HIPCHK(hipStreamSynchronize(s->st));
		HIPCHK(s->ledits.reset(g.M, lcap));
		HIPCHK(s->d_ledits_cur.ensure(H2G_MSTREAMS_MAX));
		for(unsigned m = 0; m < H2G_MSTREAMS_MAX; m++) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(s->d_ledits_cur + m), (int)(m < g.M ? s->ledits.lo(m) : 0), 1, s->st));
		HIPCHK(hipStreamSynchronize(s->st));
	}
	A.O.ledits = s->ledits; A.O.ledits_cursor = s->d_ledits_cur + lane; A.O.ledits_cap = (uint32_t)s->ledits.hi(lane);
	HIPCHK(hipMemsetD32Async((hipDeviceptr_t)A.O.ledits_cursor, (int)s->ledits.lo(lane), 1, r->ms));
	s->ledits_touched |= 1u << lane;
	if(g.second) { A.O.defer_list = r->ovl; A.O.defer_count = r->ovl + s->max_reads; }     // overflowed reads: listed for the second pass, their rows untouched
	return H2G_OK;
}

// A machine stream's FIRST kernels cost it ~64 ms on top of their own time (lease I of round 6, `profiles/r06_i_batches_first.jsonl`: runs 1-7 of a stream 94 ms, every
// later one 30; the kernels' own events read 10 + 20 ms throughout — the queue's scratch memory and code objects are set up when a queue first needs them).  A streaming
// caller's SECOND run therefore runs both machine kernels once on every other machine stream in rotation that has not run them yet (the first run may be the only one), over an
// empty list: with the pools, lists and per-run buffers above this is everything a stream does for the first time (a bench that warms up for 5 steps then timed the first use
// of streams 5-7: 18.5 ms per step where the steady state is 12-13).  A stream that enters the rotation later is warmed by the run that brings it in.
// The launches own everything they could write: a list whose count is a word no kernel writes (a machine stream's overflow list may hold the deferred count of an
// earlier run) and which every warmed stream zeroes itself in front of its launches, rows and cursors of their own.
static bool go_cold(const h2g_stream* s, const GoPlan& g, const GoRun& r) {      // a machine stream in rotation, other than the run's, that has not been warmed
	for(unsigned k = 0; k < g.S; k++) if(&s->mach[k] != r.mach && !s->mach[k].warmed) return true;
	return false;
}
static int go_warmup(h2g_stream* s, const h2g_align_params* p, const GoPlan& g, const GoRun& r) {
	int rc;
	const size_t warm_rows = (size_t)1 << 16;
	if(!s->d_warm_cnt) { HIPCHK(s->d_warm_cnt.ensure(H2G_CNT_BLOCK)); HIPCHK(hipMemset(s->d_warm_cnt, 0, H2G_CNT_BLOCK * sizeof(unsigned long long))); }
	if(!s->d_warm_rows) { HIPCHK(s->d_warm_rows.ensure(warm_rows)); HIPCHK(hipMemset(s->d_warm_rows, 0, warm_rows)); }
	for(unsigned k = 0; k < g.S; k++) {
		h2g_stream::MachStream& m = s->mach[k];
		const hipStream_t ms = s->stream_of(m);
		if(&m == r.mach || m.warmed || !m.ovf_list) continue;
		GoArgs W1 = r.A;
		if((rc = go_pool_for(s, m.main, *g.U, (size_t)g.U->slots, (size_t)g.U->threads, p->bowtie2_dp, &W1))) return rc;      // (the stream's pools exist: nothing is allocated here)
		W1.counters = s->d_warm_cnt; W1.work = reinterpret_cast<uint32_t*>(s->d_warm_cnt + H2G_CNT_WORK_MAIN);
		W1.list = reinterpret_cast<uint32_t*>(s->d_warm_rows.get()); W1.nlist = reinterpret_cast<uint32_t*>(s->d_warm_cnt + H2G_CNT_NO_SECOND);   // a count of zero
		memset(&W1.O, 0, sizeof W1.O);
		W1.O.rout = reinterpret_cast<ReadOut*>(s->d_warm_rows.get()); W1.O.aln = reinterpret_cast<h2g_alnres*>(s->d_warm_rows.get()); W1.O.aln_slots = r.A.O.aln_slots;
		W1.O.pout = reinterpret_cast<PairOut*>(s->d_warm_rows.get()); W1.O.paln[0] = W1.O.paln[1] = reinterpret_cast<h2g_alnres*>(s->d_warm_rows.get()); W1.O.pair_slots = r.A.O.pair_slots;
		W1.O.ovf = reinterpret_cast<h2g_alnres*>(s->d_warm_rows.get()); W1.O.ledits = reinterpret_cast<h2g_edit*>(s->d_warm_rows.get());      // (both areas with a capacity of zero)
		W1.O.ovf_cursor = reinterpret_cast<uint32_t*>(s->d_warm_cnt + H2G_CNT_OVF_CURSOR); W1.O.ledits_cursor = reinterpret_cast<uint32_t*>(s->d_warm_cnt + H2G_CNT_LEDITS_CURSOR);
		W1.defer_overflow = 0;
		// The count is zero ON THIS STREAM before its kernels read it: the hipMemset above runs on the null stream, which the (non-blocking) machine streams do not wait
		// for, and the host does not have to either — a launch that went out first read whatever the fresh block held as its count and the row block as read ids.
		HIPCHK(hipMemsetAsync(s->d_warm_cnt + H2G_CNT_NO_SECOND, 0, 8 * sizeof(unsigned long long), ms));
		if(g.U->launch(&W1, &r.X, nullptr, 1, ms) != 0) return set_err("go() warm-up launch", hipGetLastError());
		if(g.second) {
			GoArgs W2 = W1;
			if((rc = go_pool_for(s, m.second, *g.L, (size_t)g.L->slots, (size_t)g.L->threads, p->bowtie2_dp, &W2))) return rc;
			W2.work = reinterpret_cast<uint32_t*>(s->d_warm_cnt + H2G_CNT_WORK_SECOND);
			if(g.L->launch(&W2, &r.X, nullptr, 1, ms) != 0) return set_err("go() warm-up launch", hipGetLastError());
		}
		m.warmed = true;
	}
	s->st2_busy = true;
	return H2G_OK;
}

// the main pass, then the second pass over the reads it flagged (large workspace), whose results replace theirs
static int go_mach(h2g_stream* s, const h2g_align_params* p, const GoPlan& g, GoRun* r) {
	HIPCHK(hipEventRecord(s->tm[TM_MAIN0], r->ms));
	if(g.U->launch(&r->A, &r->X, &r->XP, r->mach_grid, r->ms) != 0) return set_err("go() launch", hipGetLastError());
	HIPCHK(hipEventRecord(s->tm[TM_MAIN1], r->ms));
	if(g.second) {
		GoArgs A2 = r->A;
		int rc;
		if((rc = go_pool_for(s, r->mach->second, *g.L, (size_t)g.bgrid * g.L->slots, (size_t)g.bgrid * g.L->threads, p->bowtie2_dp, &A2))) return rc;
		A2.counters = r->cblk + H2G_CNT_SECOND;           // (a region of its own: in H2G_GO_PROF builds a pass writes up to 96 words behind its counters)
		A2.work = reinterpret_cast<uint32_t*>(r->cblk + H2G_CNT_WORK_SECOND);
		A2.list = r->ovl; A2.nlist = r->ovl + s->max_reads;   // (the count is filled by the main pass itself: MachOut::defer_list)
		A2.defer_overflow = 0; A2.O.defer_list = nullptr; A2.O.defer_count = nullptr;
		if(g.L->launch(&A2, &r->X, nullptr, g.bgrid, r->ms) != 0) return set_err("go() second pass launch", hipGetLastError());
	}
	HIPCHK(hipEventRecord(s->tm[TM_RUN1], r->ms));
	if(g.fast) { HIPCHK(hipEventRecord(r->set->ev_mach, r->ms)); r->mach->warmed = true; }
	return H2G_OK;
}

// HI_Aligner::go for every read (pair) of the resident batch.  Two passes, both asynchronous on the stream: the main pass
// with the default workspace, then the reads it flagged (a list overflowed) once more through the large-workspace unit,
// whose results replace theirs.  Reads still flagged after that keep `overflow` set (n_overflow counts them).
static h2g_status go_run(h2g_stream* s, const h2g_align_params* p, bool paired) {
	if(!s || !p) return H2G_ERR_ARG;
	int rc;
	if((rc = go_check(s, p, paired))) return rc;
	const GoPlan g = go_plan(s, p, paired);
	HIPCHK(hipSetDevice(s->ix->device));
	// Runs queued back to back share the result arrays (rows per read, record stride): a machine pass still in flight may only meet a
	// run over the same reads with the same options.  Anything else waits for the machine streams first.
	if(s->st2_busy && (s->last_paired != (paired ? 1 : 0) || memcmp(&s->last_p, p, sizeof *p) != 0)) HIPCHK(sync_mach(s));
	s->last_p = *p; s->last_paired = paired ? 1 : 0;
	GoRun r = {};
	go_args(s, p, paired, g, &r);
	go_select(s, g, &r);
	if(!g.fast) HIPCHK(sync_mach(s));   // (the machine streams' pools are about to be used on the first stream)
	else if((rc = go_rotation(s, g))) return rc;
	if((rc = go_pools(s, p, g, &r)) || (rc = go_rows(s, p, paired, g, &r))) return rc;
	(void)hipGetLastError();
	if((rc = go_counters(s, paired, g, &r))) return rc;
	HIPCHK(hipEventRecord(s->tm[TM_RUN0], s->st));
	s->ran_fast = g.fast;
	if(g.fast) {
		fast_policy(s, paired, g, &r.f);
		if((rc = fast_buffers(s, g, r.f)) || (rc = fast_launch(s, paired, g, &r))) return rc;
	}
	HIPCHK(hipEventRecord(s->tm[TM_FAST1], s->st));
	r.ms = s->st; r.mach_grid = g.grid;
	s->ran_drain = false;
	if(g.fast && (rc = fast_handoff(s, paired, g, &r))) return rc;
	if((rc = go_mach_lists(s, g, &r))) return rc;
	if(g.fast && s->cur().n_reads >= 200000 && s->gen >= 1 && go_cold(s, g, r) && (rc = go_warmup(s, p, g, r))) return rc;
	if((rc = go_mach(s, p, g, &r))) return rc;
	s->cnt_cur = r.cblk; s->gen++;
	HIPCHK(hipGetLastError());
	s->ran_align = true;
	return H2G_OK;
}

extern "C" h2g_status h2g_align_run(h2g_stream* s, const h2g_align_params* p) { return go_run(s, p, false); }
extern "C" h2g_status h2g_align_pairs_run(h2g_stream* s, const h2g_align_params* p) { return go_run(s, p, true); }

extern "C" h2g_status h2g_align_fetch(h2g_stream* s, h2g_read_result* res, h2g_alnres* aln, size_t first, size_t n) {
	if(s) HIPCHK(sync_mach(s));   // (results of the machine pass on the second stream)
	if(!s || !res || first + n > s->cur().n_reads || !s->cur().d_rout) return H2G_ERR_ARG;
	std::vector<ReadOut> tmp(n);
	HIPCHK(hipMemcpyAsync(tmp.data(), s->cur().d_rout + first, n * sizeof(ReadOut), hipMemcpyDeviceToHost, s->st));
	if(aln && n) {   // device rows hold aln_slots (= -k of the run) records, the caller's rows H2G_ALN_CAP: copy what fits in both
		const uint32_t w = s->cur().aln_slots < H2G_ALN_CAP ? s->cur().aln_slots : H2G_ALN_CAP;
		HIPCHK(hipMemcpy2DAsync(aln, (size_t)H2G_ALN_CAP * sizeof(h2g_alnres), s->cur().d_aln + first * s->cur().aln_slots, (size_t)s->cur().aln_slots * sizeof(h2g_alnres),
		                        (size_t)w * sizeof(h2g_alnres), n, hipMemcpyDeviceToHost, s->st));
	}
	HIPCHK(sync_all(s));
	for(size_t i = 0; i < n; i++) {
		res[i].nres = tmp[i].nres; res[i].nselect = tmp[i].nselect; res[i].overflow = tmp[i].overflow;
		res[i].nrank = tmp[i].nrank; res[i].nsteps = tmp[i].nsteps; res[i].depth = tmp[i].depth;
		res[i].best = tmp[i].best; res[i].secbest = tmp[i].secbest; res[i].best_h2 = tmp[i].best_h2; res[i].secbest_h2 = tmp[i].secbest_h2;
	}
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ paired go(): fetch
// An XL run's pair whose concordant list PairOut cannot carry (more than H2G_PAIR_CAP pairs, or an index past 255) only reaches a caller through the
// compact fetch (its trailer): the slot and dense fetches flag it with H2G_OVF_PAIR_LIST instead
static h2g_status xlp_flag(h2g_stream* s, h2g_pair_result* res, size_t first, size_t n) {
	if(!s->xlp_pout || s->xlp_pout != s->cur().d_pout || n == 0) return H2G_OK;
	std::vector<uint32_t> at(n);
	HIPCHK(hipMemcpy(at.data(), s->d_xlp_at + first, n * 4, hipMemcpyDeviceToHost));
	for(size_t i = 0; i < n; i++) if(at[i]) res[i].overflow |= H2G_OVF_PAIR_LIST;
	return H2G_OK;
}
static h2g_status pairs_fetch_rows(h2g_stream* s, h2g_pair_result* res, h2g_alnres* aln1, h2g_alnres* aln2, size_t first, size_t n, bool callers_view) {
	if(s) HIPCHK(sync_mach(s));   // (results of the machine pass on the second stream)
	if(!s || !res || first + n > s->cur().n_reads || !s->cur().d_pout) return H2G_ERR_ARG;
	if((aln1 || aln2) && s->cur().pair_slots < H2G_PAIR_RES_CAP) return H2G_ERR_ARG;
	HIPCHK(hipMemcpyAsync(res, s->cur().d_pout + first, n * sizeof(PairOut), hipMemcpyDeviceToHost, s->st));
	// device rows hold pair_slots records, the caller's rows H2G_PAIR_RES_CAP (the dense variant returns all of them)
	for(int m = 0; m < 2 && n; m++) {
		h2g_alnres* dst = m == 0 ? aln1 : aln2;
		if(dst) HIPCHK(hipMemcpy2DAsync(dst, (size_t)H2G_PAIR_RES_CAP * sizeof(h2g_alnres), s->cur().d_paln[m] + first * s->cur().pair_slots, (size_t)s->cur().pair_slots * sizeof(h2g_alnres),
		                                (size_t)H2G_PAIR_RES_CAP * sizeof(h2g_alnres), n, hipMemcpyDeviceToHost, s->st));
	}
	HIPCHK(sync_all(s));
	// a pair kept in the overflow area has more records than these fixed rows return: flagged in the returned copy (the dense variant
	// returns every record)
	if(callers_view) for(size_t i = 0; i < n; i++) if(res[i].pad) { res[i].overflow |= 4; res[i].pad = 0; }      // (the block offset itself is the device's business: allocation order, i.e. timing)
	return xlp_flag(s, res, first, n);
}
extern "C" h2g_status h2g_align_pairs_fetch(h2g_stream* s, h2g_pair_result* res, h2g_alnres* aln1, h2g_alnres* aln2, size_t first, size_t n) { return pairs_fetch_rows(s, res, aln1, aln2, first, n, true); }

// ------------------------------------------------------------------------------------------ dense result fetch
// The slot layout of h2g_align_fetch moves H2G_ALN_CAP x 424 B per read over PCIe whatever was found; these variants gather
// only the records that exist into one dense array on the device (one lane per read) and copy that.
__global__ __launch_bounds__(256) void k_gather_aln(const h2g_alnres* src, uint32_t slots, const uint32_t* cnt, uint32_t cnt_stride,
                                                    const unsigned long long* offs, size_t n, h2g_alnres* dst,
                                                    const PairOut* pout = nullptr, const h2g_alnres* ovf = nullptr, int mate = 0)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i >= n) return;
	uint32_t c = cnt[i * cnt_stride];
	const h2g_alnres* a = src + i * slots;
	if(pout && pout[i].pad) a = ovf + (pout[i].pad - 1u) + (mate ? pout[i].nres[0] : 0u);      // every record of the pair lives in its overflow block
	else if(c > slots) c = slots;
	h2g_alnres* d = dst + offs[i];
	for(uint32_t k = 0; k < c; k++) {
		d[k].fw = a[k].fw; d[k].tidx = a[k].tidx; d[k].toff = a[k].toff; d[k].len = a[k].len; d[k].trim5 = a[k].trim5; d[k].trim3 = a[k].trim3;
		d[k].nedits = a[k].nedits; d[k].splicescore = a[k].splicescore; d[k].score = a[k].score;
		for(uint32_t e = 0; e < a[k].nedits && e < H2G_MAX_EDITS; e++) d[k].edits[e] = a[k].edits[e];
	}
}
// dense offsets of [first, first+n) of a slot array from the per-read record counts already on the host
static uint64_t dense_offsets(const uint32_t* h_cnt, uint32_t h_stride, uint32_t slots, size_t n, uint64_t* offs, const uint32_t* h_pad = nullptr) {
	uint64_t tot = 0;
	for(size_t i = 0; i < n; i++) { offs[i] = tot; const uint32_t c = h_cnt[i * h_stride]; tot += (c < slots || (h_pad && h_pad[i * h_stride])) ? c : slots; }
	offs[n] = tot;
	return tot;
}
// gathers the records into `out` (host) at the offsets computed by dense_offsets
static int gather_dense(h2g_stream* s, const h2g_alnres* d_src, uint32_t slots, const uint32_t* d_cnt, uint32_t cnt_stride, size_t n, h2g_alnres* out,
                        const uint64_t* offs, int tmp_slot, const PairOut* d_pout = nullptr, int mate = 0)
{
	const uint64_t tot = offs[n];
	if(tot == 0) return H2G_OK;
	void *d_offs = nullptr, *d_dense = nullptr;
	int rc;
	if((rc = tmp_buf(s, tmp_slot, (n + 1) * 8, &d_offs)) || (rc = tmp_buf(s, tmp_slot + 1, tot * sizeof(h2g_alnres), &d_dense))) return rc;
	HIPCHK(hipMemcpyAsync(d_offs, offs, (n + 1) * 8, hipMemcpyHostToDevice, s->st));
	hipLaunchKernelGGL(k_gather_aln, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, d_src, slots, d_cnt, cnt_stride,
	                   (const unsigned long long*)d_offs, n, (h2g_alnres*)d_dense, d_pout, (const h2g_alnres*)s->paln_ovf, mate);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_dense, tot * sizeof(h2g_alnres), hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	return H2G_OK;
}

extern "C" h2g_status h2g_align_fetch_dense(h2g_stream* s, h2g_read_result* res, h2g_alnres* aln, size_t aln_cap, uint64_t* aln_offs, size_t first, size_t n) {
	if(s) HIPCHK(sync_mach(s));   // (results of the machine pass on the second stream)
	if(!s || !res || !aln || !aln_offs || first + n > s->cur().n_reads || !s->cur().d_rout) return H2G_ERR_ARG;
	const h2g_status rc = h2g_align_fetch(s, res, nullptr, first, n);
	if(rc != H2G_OK) return rc;
	static_assert(offsetof(ReadOut, nselect) == 4, "ReadOut layout");
	if(dense_offsets(&res[0].nselect, sizeof(h2g_read_result) / 4, s->cur().aln_slots, n, aln_offs) > aln_cap) return H2G_ERR_ARG;
	return gather_dense(s, s->cur().d_aln + first * s->cur().aln_slots, s->cur().aln_slots, reinterpret_cast<const uint32_t*>(s->cur().d_rout + first) + 1, sizeof(ReadOut) / 4,
	                    n, aln, aln_offs, 0);
}

extern "C" h2g_status h2g_align_pairs_fetch_dense(h2g_stream* s, h2g_pair_result* res, h2g_alnres* aln1, size_t cap1, uint64_t* offs1,
                                                  h2g_alnres* aln2, size_t cap2, uint64_t* offs2, size_t first, size_t n)
{
	if(s) HIPCHK(sync_mach(s));   // (results of the machine pass on the second stream)
	if(!s || !res || !aln1 || !aln2 || !offs1 || !offs2 || first + n > s->cur().n_reads || !s->cur().d_pout) return H2G_ERR_ARG;
	const h2g_status rc = pairs_fetch_rows(s, res, nullptr, nullptr, first, n, false);       // (the headers as the device holds them: `pad` says where a pair's records are)
	if(rc != H2G_OK) return rc;
	static_assert(offsetof(PairOut, nres) == 0, "PairOut layout");
	// both totals are known before either capacity is judged, so a caller that has to grow its buffers learns both needs at once
	static_assert(offsetof(h2g_pair_result, pad) == offsetof(PairOut, pad) && sizeof(h2g_pair_result) == sizeof(PairOut), "PairOut layout");
	const uint64_t t1 = dense_offsets(&res[0].nres[0], sizeof(h2g_pair_result) / 4, s->cur().pair_slots, n, offs1, &res[0].pad);
	const uint64_t t2 = dense_offsets(&res[0].nres[1], sizeof(h2g_pair_result) / 4, s->cur().pair_slots, n, offs2, &res[0].pad);
	if(t1 > cap1 || t2 > cap2) return H2G_ERR_ARG;
	int r;
	if((r = gather_dense(s, s->cur().d_paln[0] + first * s->cur().pair_slots, s->cur().pair_slots, reinterpret_cast<const uint32_t*>(s->cur().d_pout + first), sizeof(PairOut) / 4,
	                     n, aln1, offs1, 0, s->cur().d_pout + first, 0))) return r;
	r = gather_dense(s, s->cur().d_paln[1] + first * s->cur().pair_slots, s->cur().pair_slots, reinterpret_cast<const uint32_t*>(s->cur().d_pout + first) + 1, sizeof(PairOut) / 4,
	                 n, aln2, offs2, 2, s->cur().d_pout + first, 1);
	// `pad` is where the device kept the pair's records (a block offset in the overflow area: allocation order, i.e. timing) — nothing a caller may see
	for(size_t i = 0; i < n; i++) res[i].pad = 0;
	if(r == H2G_OK) r = xlp_flag(s, res, first, n);
	return r;
}

// ------------------------------------------------------------------------------------------ compact result fetch
// The dense fetch still moves 424 B per record (40 B of fields + 32 edit entries of which an alignment of a 101 bp read uses one or two) and needs the
// result headers on the host before it can size anything (two round trips).  The compact fetch sizes, scans and gathers on the device: a record travels as its
// 40 B of fields + 12 B per edit it holds (a long record: its marker entry), 8-byte aligned — a tenth of the bytes — and the host gets byte offsets per read.
// A compact record is a PREFIX of an h2g_alnres: read it through a `const h2g_alnres*`, never copy the struct.
__device__ __forceinline__ uint32_t compact_rec_bytes(uint32_t nedits) { const uint32_t e = nedits > H2G_MAX_EDITS ? 1u : nedits; return (40u + 12u * e + 7u) & ~7u; }
__device__ __forceinline__ const h2g_alnres* compact_src(const h2g_alnres* src, uint32_t slots, size_t i, uint32_t* c, const PairOut* pout, const h2g_alnres* ovf, int mate) {
	const h2g_alnres* a = src + i * slots;
	if(pout && pout[i].pad) a = ovf + (pout[i].pad - 1u) + (mate ? pout[i].nres[0] : 0u);      // every record of the pair lives in its overflow block
	else if(*c > slots) *c = slots;
	return a;
}
// The concordant list of an XL pair that PairOut cannot carry (XlPairs) travels as a trailer behind mate 1's records (include/h2g.h H2G_PAIR_TRAILER_TAG):
// `xat` / `xlist` are passed for mate 1 of an XL run only, nullptr otherwise
__device__ __forceinline__ uint32_t compact_trailer_bytes(uint32_t npairs) { return (40u + 4u * npairs + 7u) & ~7u; }
__global__ __launch_bounds__(256) void k_compact_sizes(const h2g_alnres* src, uint32_t slots, const uint32_t* cnt, uint32_t cnt_stride, size_t n, unsigned long long* sizes,
                                                       const PairOut* pout, const h2g_alnres* ovf, int mate, const uint32_t* xat = nullptr, const uint32_t* xlist = nullptr)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i > n) return;
	if(i == n) { sizes[n] = 0; return; }
	uint32_t c = cnt[i * cnt_stride];
	const h2g_alnres* a = compact_src(src, slots, i, &c, pout, ovf, mate);
	unsigned long long b = 0;
	for(uint32_t k = 0; k < c; k++) b += compact_rec_bytes(a[k].nedits);
	if(xat && xat[i]) b += compact_trailer_bytes(xlist[xat[i] - 1u]);
	sizes[i] = b;
}
// exclusive prefix sum of v[0 .. n1) in place, three launches: tiles of 2048 entries scanned by a workgroup each (8 consecutive entries per thread), their sums scanned by
// one workgroup, then added back.  (The first version — one workgroup walking 1 M entries with a stride per thread — took 3 ms of a 48 ms round trip.)
#define H2G_SCAN_TILE 2048u
__global__ __launch_bounds__(256) void k_scan_tiles(unsigned long long* v, size_t n1, unsigned long long* tile_sum) {
	__shared__ unsigned long long part[256];
	const size_t base = (size_t)blockIdx.x * H2G_SCAN_TILE + (size_t)threadIdx.x * 8;
	unsigned long long x[8], sum = 0;
#pragma unroll
	for(int k = 0; k < 8; k++) { x[k] = base + k < n1 ? v[base + k] : 0; sum += x[k]; }
	part[threadIdx.x] = sum;
	__syncthreads();
	for(unsigned d = 1; d < 256; d <<= 1) {
		const unsigned long long t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
		__syncthreads();
		part[threadIdx.x] += t;
		__syncthreads();
	}
	unsigned long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
#pragma unroll
	for(int k = 0; k < 8; k++) { if(base + k < n1) v[base + k] = run; run += x[k]; }
	if(threadIdx.x == 255) tile_sum[blockIdx.x] = part[255];
}
__global__ __launch_bounds__(1024) void k_scan_tile_sums(unsigned long long* tile_sum, size_t ntiles) {      // in place, exclusive; one workgroup
	__shared__ unsigned long long part[1024];
	const size_t per = (ntiles + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < ntiles ? lo + per : ntiles;
	unsigned long long sum = 0;
	for(size_t k = lo; k < hi; k++) sum += tile_sum[k];
	part[threadIdx.x] = sum;
	__syncthreads();
	for(unsigned d = 1; d < 1024; d <<= 1) {
		const unsigned long long t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
		__syncthreads();
		part[threadIdx.x] += t;
		__syncthreads();
	}
	unsigned long long run = threadIdx.x ? part[threadIdx.x - 1] : 0;
	for(size_t k = lo; k < hi; k++) { const unsigned long long x = tile_sum[k]; tile_sum[k] = run; run += x; }
}
__global__ __launch_bounds__(256) void k_scan_add(unsigned long long* v, size_t n1, const unsigned long long* tile_sum) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n1) v[i] += tile_sum[i / H2G_SCAN_TILE];
}
__global__ __launch_bounds__(256) void k_compact_gather(const h2g_alnres* src, uint32_t slots, const uint32_t* cnt, uint32_t cnt_stride, const unsigned long long* offs, size_t n,
                                                        uint8_t* dst, const PairOut* pout, const h2g_alnres* ovf, int mate, const uint32_t* xat = nullptr, const uint32_t* xlist = nullptr)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i >= n) return;
	uint32_t c = cnt[i * cnt_stride];
	const h2g_alnres* a = compact_src(src, slots, i, &c, pout, ovf, mate);
	uint8_t* d = dst + offs[i];
	for(uint32_t k = 0; k < c; k++) {
		const uint32_t ne = a[k].nedits, e = ne > H2G_MAX_EDITS ? 1u : ne, bytes = compact_rec_bytes(ne);
		const unsigned long long* sw = reinterpret_cast<const unsigned long long*>(&a[k]);
		unsigned long long* dw = reinterpret_cast<unsigned long long*>(d);
		for(uint32_t w = 0; w < 5; w++) dw[w] = sw[w];                       // fw .. score: 40 bytes
		const uint32_t* se = reinterpret_cast<const uint32_t*>(a[k].edits);
		uint32_t* de = reinterpret_cast<uint32_t*>(d + 40);
		for(uint32_t w = 0; w < 3 * e; w++) de[w] = se[w];
		if(e & 1u) de[3 * e] = 0;                                            // the alignment pad: never stale bytes
		d += bytes;
	}
	if(xat && xat[i]) {      // the trailer: a record prefix whose nedits no record carries, npairs in tidx, then the pairs
		const uint32_t* l = xlist + (xat[i] - 1u);
		const uint32_t np = l[0];
		uint32_t* dw = reinterpret_cast<uint32_t*>(d);
		for(uint32_t w = 0; w < 10; w++) dw[w] = 0;
		dw[1] = np; dw[6] = H2G_PAIR_TRAILER_TAG;                         // tidx, nedits
		for(uint32_t k = 0; k < np; k++) dw[10 + k] = l[1 + k];
		if(np & 1u) dw[10 + np] = 0;
	}
}
static_assert(offsetof(h2g_alnres, edits) == 40 && sizeof(h2g_edit) == 12, "compact records are prefixes of h2g_alnres");
static_assert(offsetof(h2g_alnres, tidx) == 4 && offsetof(h2g_alnres, nedits) == 24, "the pair trailer's fields");

// sizes + scan for one mate into tmp slot `slot` (-> device offsets [n + 1], exclusive, in bytes)
static int compact_offsets(h2g_stream* s, const h2g_alnres* d_src, uint32_t slots, const uint32_t* d_cnt, uint32_t cnt_stride, size_t n, int slot, const PairOut* d_pout, int mate, void** d_offs,
                           const uint32_t* xat = nullptr) {
	int rc;
	if((rc = tmp_buf(s, slot, (n + 1) * 8 + ((n + 1) / H2G_SCAN_TILE + 2) * 8, d_offs))) return rc;      // offsets [n + 1], then the scan's tile sums
	hipLaunchKernelGGL(k_compact_sizes, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s->st, d_src, slots, d_cnt, cnt_stride, n, (unsigned long long*)*d_offs, d_pout, (const h2g_alnres*)s->paln_ovf, mate,
	                   xat, xat ? (const uint32_t*)s->xlp : (const uint32_t*)nullptr);
	{	// exclusive scan of the n + 1 sizes (the last one is 0: its slot becomes the total); the tile sums live behind the offsets
		const size_t n1 = n + 1, ntiles = (n1 + H2G_SCAN_TILE - 1) / H2G_SCAN_TILE;
		unsigned long long* v = (unsigned long long*)*d_offs;
		unsigned long long* ts = v + n1;
		hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, s->st, v, n1, ts);
		hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, s->st, ts, ntiles);
		hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s->st, v, n1, (const unsigned long long*)ts);
	}
	HIPCHK(hipGetLastError());
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ FASTQ records parsed on the device
// The text of one mate -> the batch's codes, qualities, names and their offsets.  The record arithmetic (what a plain record is, its outputs in closed form, the cursor over
// output bytes) is h2g_fastq.h's; the kernels are the loads, the scans and the stores around it.
// 1. newlines: a lane loads 16 consecutive bytes (one dwordx4, 1 KB contiguous per wave) and counts its '\n'; a workgroup (4 KB of text) leaves one count
__global__ __launch_bounds__(256) void k_fq_count(const uint8_t* __restrict__ text, uint32_t n_text, unsigned long long* __restrict__ blk) {
	__shared__ uint32_t part[4];
	const uint64_t b0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
	uint32_t c = 0;
	if(b0 < n_text) {
		const uint4 v = *(const uint4*)(text + b0);
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
		c = h2g_fq::popc16(h2g_fq::nl_mask16(w, n_text - b0 < 16 ? (uint32_t)(n_text - b0) : 16u));
	}
	for(int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
	if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
	__syncthreads();
	if(threadIdx.x == 0) blk[blockIdx.x] = (unsigned long long)part[0] + part[1] + part[2] + part[3];
}
// ... and, once the workgroups' counts are scanned (k_scan_*), every newline's index follows from a scan across the wave and the workgroup: nlpos[j] = position of newline j, j < cap
__global__ __launch_bounds__(256) void k_fq_lines(const uint8_t* __restrict__ text, uint32_t n_text, const unsigned long long* __restrict__ blk, uint32_t* __restrict__ nlpos, uint64_t cap) {
	__shared__ uint32_t part[4];
	const uint64_t b0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t mask = 0;
	if(b0 < n_text) {
		const uint4 v = *(const uint4*)(text + b0);
		const uint32_t w[4] = {v.x, v.y, v.z, v.w};
		mask = h2g_fq::nl_mask16(w, n_text - b0 < 16 ? (uint32_t)(n_text - b0) : 16u);
	}
	const uint32_t c = h2g_fq::popc16(mask);
	uint32_t incl = c;
	for(uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if(lane >= d) incl += t; }
	if(lane == 63) part[wave] = incl;
	__syncthreads();
	uint64_t idx = blk[blockIdx.x] + (incl - c);
	for(uint32_t k = 0; k < wave; k++) idx += part[k];
	for(uint32_t m = mask; m; m &= m - 1, idx++) if(idx < cap) nlpos[idx] = (uint32_t)b0 + (uint32_t)(__ffs(m) - 1);
}
// 2. one lane per record: its four lines, the predicate, its lengths, sources and plain bit; lane n closes the two size arrays.  res: {not plain, first not plain, longest L}
__global__ __launch_bounds__(256) void k_fq_table(const char* __restrict__ text, uint32_t n_text, const uint32_t* __restrict__ nlpos, uint64_t n_nl_known, uint32_t n, h2g_fq::Opts o,
                                                  unsigned long long* __restrict__ lsz, unsigned long long* __restrict__ nsz, uint32_t* __restrict__ src, uint8_t* __restrict__ bits,
                                                  const uint8_t* __restrict__ prev /* mate 1's bits when this is mate 2: a record is counted once */, uint32_t* __restrict__ res)
{
	__shared__ uint32_t sbad, sfirst, smax;
	if(threadIdx.x == 0) { sbad = 0; sfirst = 0xffffffffu; smax = 0; }
	__syncthreads();
	const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if(r < n) {
		const h2g_fq::Rec x = h2g_fq::eval_record(text, h2g_fq::record_lines(nlpos, n_nl_known, n_text, r), o);
		lsz[r] = x.L; nsz[r] = x.name_len;
		src[r] = x.name_src; src[(uint64_t)n + r] = x.seq_src; src[2ull * n + r] = x.qual_src;
		bits[r] = (uint8_t)x.plain;
		if(!x.plain) { if(!prev || prev[r]) atomicAdd(&sbad, 1u); atomicMin(&sfirst, (uint32_t)r); }
		else atomicMax(&smax, x.L);
	} else if(r == n) { lsz[r] = 0; nsz[r] = 0; }
	__syncthreads();
	if(threadIdx.x == 0) {
		if(sbad) atomicAdd(&res[0], sbad);
		if(sfirst != 0xffffffffu) atomicMin(&res[1], sfirst);
		if(smax) atomicMax(&res[2], smax);
	}
}
// 3. (k_scan_* over both size arrays) the batch's 32-bit offsets
__global__ __launch_bounds__(256) void k_fq_offs(const unsigned long long* __restrict__ lsz, const unsigned long long* __restrict__ nsz, uint32_t n, uint32_t* __restrict__ offs, uint32_t* __restrict__ name_offs) {
	const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if(r <= n) { offs[r] = (uint32_t)lsz[r]; name_offs[r] = (uint32_t)nsz[r]; }
}
// 4. a lane owns 16 consecutive OUTPUT bytes and stores them as one dwordx4 (k_win_codes' scheme): its record by binary search over the scanned lengths, then the cursor walks across
// records.  SEQ: codes and qualities share their offsets, so one pass writes both; else the names, by the same cursor over their own offsets.  The sources are byte gathers from the text.
template<bool SEQ> __global__ __launch_bounds__(256) void k_fq_write(const uint8_t* __restrict__ text, const unsigned long long* __restrict__ offs, const uint32_t* __restrict__ src_a,
                                                                     const uint32_t* __restrict__ src_b, uint32_t n, uint64_t n_bytes, uint32_t phred64, uint8_t* __restrict__ out_a, uint8_t* __restrict__ out_b)
{
	const uint64_t chunks = (n_bytes + 15) / 16;
	for(uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t b0 = c * 16;
		const uint32_t m = n_bytes - b0 < 16 ? (uint32_t)(n_bytes - b0) : 16u;      // (the bytes past the end of the last chunk are written as 0: the buffers have 64 spare)
		h2g_fq::Cursor cur;
		cur.seek(offs, src_a, n, b0);
		uint32_t wa[4] = {0, 0, 0, 0}, wb[4] = {0, 0, 0, 0};
		uint32_t last = 0xffffffffu, delta = 0;
#pragma unroll
		for(uint32_t k = 0; k < 16; k++) if(k < m) {
			if(SEQ && cur.r != last) { last = cur.r; delta = src_b[last] - src_a[last]; }
			const uint32_t at = cur.next();
			if(SEQ) {
				wa[k >> 2] |= (uint32_t)h2g_fq::fq_code(text[at]) << (8 * (k & 3));
				wb[k >> 2] |= (uint32_t)(uint8_t)h2g_fq::fq_qual(text[at + delta], phred64) << (8 * (k & 3));
			} else wa[k >> 2] |= (uint32_t)text[at] << (8 * (k & 3));
		}
		*(uint4*)(out_a + b0) = make_uint4(wa[0], wa[1], wa[2], wa[3]);
		if(SEQ) *(uint4*)(out_b + b0) = make_uint4(wb[0], wb[1], wb[2], wb[3]);
	}
}

static void scan64(h2g_stream* s, unsigned long long* v, size_t n1) {      // exclusive, in place; the tile sums live behind v[0 .. n1)
	const size_t ntiles = (n1 + H2G_SCAN_TILE - 1) / H2G_SCAN_TILE;
	unsigned long long* ts = v + n1;
	hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, s->st, v, n1, ts);
	hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, s->st, ts, ntiles);
	hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s->st, v, n1, (const unsigned long long*)ts);
}
static size_t scan64_bytes(size_t n1) { return (n1 + n1 / H2G_SCAN_TILE + 2) * 8; }
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

extern "C" h2g_status h2g_set_reads_fastq(h2g_stream* s, const char* text1, size_t n1, const char* text2, size_t n2, const h2g_fastq_opts* opts, h2g_fastq_result* out) {
	if(s) HIPCHK(sync_all(s));        // (a machine pass of the previous batch may still read the buffers this call replaces)
	if(!s || !opts || !out || (!text1 && n1) || (!text2 && n2)) return H2G_ERR_ARG;
	memset(out, 0, sizeof *out);
	s->tmp_gen++;
	BatchCtx& B = s->cur();
	// whatever happens below, the batch holds no read of its former set
	B.n_reads = 0; B.max_read_len = 0;
	B.has_quals = B.has_quals2 = B.has_names = B.has_mates = false;
	B.has_seeds = B.has_seeds2 = false; B.has_qc = false; B.has_ids = false;
	s->ledits_touched = 0;
	s->fq_stats = h2g_fastq_stats{};
	const int M = text2 ? 2 : 1;
	const char* text[2] = {text1, text2};
	const size_t nt[2] = {n1, n2};
	const bool fin[2] = {opts->final1 != 0, opts->final2 != 0};
	if(n1 >= (1ull << 32) || n2 >= (1ull << 32)) { snprintf(g_err, sizeof g_err, "h2g_set_reads_fastq: a text of 4 GB or more (offsets into it are 32 bits)"); return H2G_ERR_ARG; }
	HIPCHK(hipSetDevice(s->ix->device));
	float ms = 0, ms_total = 0;
	// ---- phase A: the texts, their newlines per 4 KB, the scan -> how many records there are
	uint8_t* d_text[2] = {nullptr, nullptr};
	size_t nblk[2] = {0, 0}, cnt_at[2] = {0, 0};
	for(int m = 0; m < M; m++) { nblk[m] = (nt[m] + 4095) / 4096; cnt_at[m] = m ? up16(scan64_bytes(nblk[0] + 1)) : 0; }
	void* d_cnt;
	int rc;
	for(int m = 0; m < M; m++) { void* p; if((rc = tmp_buf(s, m, nt[m] + 16, &p))) return (h2g_status)rc; d_text[m] = (uint8_t*)p; }
	if((rc = tmp_buf(s, 2, cnt_at[M - 1] + scan64_bytes(nblk[M - 1] + 1), &d_cnt))) return (h2g_status)rc;
	for(int m = 0; m < M; m++) if(nt[m]) HIPCHK(hipMemcpyAsync(d_text[m], text[m], nt[m], hipMemcpyHostToDevice, s->st));
	unsigned long long nl[2] = {0, 0};
	HIPCHK(hipEventRecord(s->tm[TM_SET0], s->st));
	for(int m = 0; m < M; m++) {
		unsigned long long* v = (unsigned long long*)((uint8_t*)d_cnt + cnt_at[m]);
		HIPCHK(hipMemsetAsync(v + nblk[m], 0, 8, s->st));
		if(nblk[m]) hipLaunchKernelGGL(k_fq_count, dim3((unsigned)nblk[m]), dim3(256), 0, s->st, (const uint8_t*)d_text[m], (uint32_t)nt[m], v);
		scan64(s, v, nblk[m] + 1);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->tm[TM_SET1], s->st));
	for(int m = 0; m < M; m++) HIPCHK(hipMemcpyAsync(&nl[m], (unsigned long long*)((uint8_t*)d_cnt + cnt_at[m]) + nblk[m], 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(sync_all(s));
	HIPCHK(hipEventElapsedTime(&ms, s->tm[TM_SET0], s->tm[TM_SET1])); ms_total += ms;
	// whole records, and the one a text that ends the input may still hold behind them (h2g_fastq.h)
	uint64_t n = opts->max_records ? opts->max_records : UINT64_MAX;
	for(int m = 0; m < M; m++) {
		const bool rest = nl[m] % 4 != 0 || (nt[m] && text[m][nt[m] - 1] != '\n');
		n = std::min<uint64_t>(n, h2g_fq::whole_records(nl[m]) + (fin[m] && rest ? 1 : 0));
	}
	out->n_records = n;
	out->first_not_plain = UINT64_MAX;
	s->fq_stats.bytes_uploaded = n1 + n2;
	if(n == 0) { out->first_not_plain = 0; s->fq_stats.kernel_ms = ms_total; return H2G_OK; }
	// ---- phase B: line starts, the per-record table, the scans of the lengths
	struct Lay { size_t nlpos, lsz, nsz, src, bits, res; } lay[2];
	size_t at = 0;
	for(int m = 0; m < M; m++) {
		Lay& l = lay[m];
		l.nlpos = at; at = up16(at + (4 * n + 1) * 4);
		l.lsz = at;   at = up16(at + scan64_bytes(n + 1));
		l.nsz = at;   at = up16(at + scan64_bytes(n + 1));
		l.src = at;   at = up16(at + 3 * n * 4);
		l.bits = at;  at = up16(at + n);
		l.res = at;   at = up16(at + 16);
	}
	void* d_tab;
	if((rc = tmp_buf(s, 3, at, &d_tab))) return (h2g_status)rc;
	uint8_t* T = (uint8_t*)d_tab;
	const h2g_fq::Opts fo = {opts->trim5, opts->trim3, opts->phred64 ? 1u : 0u};
	static const uint32_t res0[4] = {0, 0xffffffffu, 0, 0};
	uint32_t hres[2][4];
	unsigned long long tot_l[2] = {0, 0}, tot_n[2] = {0, 0};
	uint32_t last_nl[2] = {0, 0};
	uint64_t known[2];
	HIPCHK(hipEventRecord(s->tm[TM_SET0], s->st));
	for(int m = 0; m < M; m++) {
		const Lay& l = lay[m];
		known[m] = std::min<uint64_t>(nl[m], 4 * n);
		HIPCHK(hipMemcpyAsync(T + l.res, res0, 16, hipMemcpyHostToDevice, s->st));
		const unsigned long long* v = (const unsigned long long*)((uint8_t*)d_cnt + cnt_at[m]);
		hipLaunchKernelGGL(k_fq_lines, dim3((unsigned)nblk[m]), dim3(256), 0, s->st, (const uint8_t*)d_text[m], (uint32_t)nt[m], v, (uint32_t*)(T + l.nlpos), known[m]);
		hipLaunchKernelGGL(k_fq_table, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s->st, (const char*)d_text[m], (uint32_t)nt[m], (const uint32_t*)(T + l.nlpos), known[m], (uint32_t)n, fo,
		                   (unsigned long long*)(T + l.lsz), (unsigned long long*)(T + l.nsz), (uint32_t*)(T + l.src), T + l.bits,
		                   m ? (const uint8_t*)(T + lay[0].bits) : (const uint8_t*)nullptr, (uint32_t*)(T + l.res));
		scan64(s, (unsigned long long*)(T + l.lsz), n + 1);
		scan64(s, (unsigned long long*)(T + l.nsz), n + 1);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->tm[TM_SET1], s->st));
	for(int m = 0; m < M; m++) {
		const Lay& l = lay[m];
		HIPCHK(hipMemcpyAsync(hres[m], T + l.res, 16, hipMemcpyDeviceToHost, s->st));
		HIPCHK(hipMemcpyAsync(&tot_l[m], (unsigned long long*)(T + l.lsz) + n, 8, hipMemcpyDeviceToHost, s->st));
		HIPCHK(hipMemcpyAsync(&tot_n[m], (unsigned long long*)(T + l.nsz) + n, 8, hipMemcpyDeviceToHost, s->st));
		if(known[m] == 4 * n) HIPCHK(hipMemcpyAsync(&last_nl[m], (uint32_t*)(T + l.nlpos) + (4 * n - 1), 4, hipMemcpyDeviceToHost, s->st));
	}
	HIPCHK(sync_all(s));
	HIPCHK(hipEventElapsedTime(&ms, s->tm[TM_SET0], s->tm[TM_SET1])); ms_total += ms;
	s->fq_stats.kernel_ms = ms_total;
	const uint64_t consumed[2] = {known[0] == 4 * n ? (uint64_t)last_nl[0] + 1 : n1, M == 2 ? (known[1] == 4 * n ? (uint64_t)last_nl[1] + 1 : n2) : 0};
	out->consumed1 = consumed[0]; out->consumed2 = consumed[1];
	out->n_bases1 = tot_l[0]; out->n_bases2 = tot_l[1];
	out->n_name_bytes1 = tot_n[0]; out->n_name_bytes2 = tot_n[1];
	out->n_not_plain = (uint64_t)hres[0][0] + (M == 2 ? hres[1][0] : 0u);      // (mate 2's count leaves out the records mate 1 counted)
	out->max_read_len = std::max(hres[0][2], M == 2 ? hres[1][2] : 0u);
	if(out->n_not_plain) { out->first_not_plain = std::min(hres[0][1], M == 2 ? hres[1][1] : 0xffffffffu); return H2G_OK; }
	out->first_not_plain = n;
	if(n > s->max_reads || tot_l[0] > s->max_bases || tot_l[1] > s->max_bases || tot_n[0] > 0xffffffffull || tot_n[1] > 0xffffffffull) {
		snprintf(g_err, sizeof g_err, "h2g_set_reads_fastq: %llu records of %llu / %llu bases exceed the stream's %zu reads / %zu bases, or their names 4 GB", (unsigned long long)n,
		         tot_l[0], tot_l[1], s->max_reads, s->max_bases);
		return H2G_ERR_ARG;
	}
	// ---- phase C: the batch's arrays
	HIPCHK(B.reserve_names(tot_n[0], s->max_reads));
	if(M == 2) HIPCHK(B.ensure_mates(s->max_reads, s->max_bases, tot_n[1]));
	HIPCHK(hipEventRecord(s->tm[TM_SET0], s->st));
	for(int m = 0; m < M; m++) {
		const Lay& l = lay[m];
		const unsigned long long* lsz = (const unsigned long long*)(T + l.lsz);
		const unsigned long long* nsz = (const unsigned long long*)(T + l.nsz);
		const uint32_t* src = (const uint32_t*)(T + l.src);
		uint8_t* codes = m ? B.d_codes2 : B.d_codes;
		uint8_t* quals = (uint8_t*)(m ? B.d_quals2 : B.d_quals).get();
		uint8_t* names = (uint8_t*)(m ? B.d_names2 : B.d_names).get();
		hipLaunchKernelGGL(k_fq_offs, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s->st, lsz, nsz, (uint32_t)n, m ? B.d_offs2 : B.d_offs, m ? B.d_name_offs2 : B.d_name_offs);
		if(tot_l[m]) hipLaunchKernelGGL(k_fq_write<true>, dim3(grid_for((tot_l[m] + 15) / 16, 256)), dim3(256), 0, s->st, (const uint8_t*)d_text[m], lsz, src + n, src + 2 * n, (uint32_t)n, (uint64_t)tot_l[m],
		                                fo.phred64, codes, quals);
		if(tot_n[m]) hipLaunchKernelGGL(k_fq_write<false>, dim3(grid_for((tot_n[m] + 15) / 16, 256)), dim3(256), 0, s->st, (const uint8_t*)d_text[m], nsz, src, (const uint32_t*)nullptr, (uint32_t)n,
		                                (uint64_t)tot_n[m], 0u, names, (uint8_t*)nullptr);
		s->fq_stats.bytes_written += 2 * tot_l[m] + tot_n[m] + 2 * (n + 1) * 4;
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->tm[TM_SET1], s->st));
	HIPCHK(sync_all(s));
	HIPCHK(hipEventElapsedTime(&ms, s->tm[TM_SET0], s->tm[TM_SET1])); ms_total += ms;
	s->fq_stats.kernel_ms = ms_total;
	B.n_reads = n;
	B.max_read_len = out->max_read_len;
	B.has_quals = true;
	B.has_names = true;
	B.has_mates = M == 2;
	B.has_quals2 = M == 2;
	return H2G_OK;
}
extern "C" h2g_status h2g_get_fastq_stats(h2g_stream* s, h2g_fastq_stats* out) {
	if(!s || !out) return H2G_ERR_ARG;
	*out = s->fq_stats;
	return H2G_OK;
}

extern "C" h2g_status h2g_fetch_read_set(h2g_stream* s, int mate, size_t* n_reads, size_t* n_bases, size_t* n_name_bytes, uint8_t* codes, uint32_t* offs, char* quals, char* names,
                                         uint32_t* name_offs)
{
	if(!s || mate < 0 || mate > 1) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	const BatchCtx& B = s->cur();
	const size_t n = B.n_reads;
	if(n_reads) *n_reads = n;
	if(n_bases) *n_bases = 0;
	if(n_name_bytes) *n_name_bytes = 0;
	if(n == 0) return H2G_OK;
	if(mate == 1 && !B.has_mates) return H2G_ERR_ARG;
	const uint8_t* dc = mate ? B.d_codes2 : B.d_codes;
	const uint32_t* dof = mate ? B.d_offs2 : B.d_offs;
	const char* dq = mate ? B.d_quals2 : B.d_quals;
	const char* dn = mate ? B.d_names2 : B.d_names;
	const uint32_t* dno = mate ? B.d_name_offs2 : B.d_name_offs;
	const bool hq = mate ? B.has_quals2 : B.has_quals, hn = mate ? true : B.has_names;
	uint32_t nb = 0, nn = 0;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(hipMemcpyAsync(&nb, dof + n, 4, hipMemcpyDeviceToHost, s->st));
	if(hn) HIPCHK(hipMemcpyAsync(&nn, dno + n, 4, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	if(n_bases) *n_bases = nb;
	if(n_name_bytes) *n_name_bytes = nn;
	if((quals && !hq) || ((names || name_offs) && !hn)) return H2G_ERR_ARG;
	if(codes && nb) HIPCHK(hipMemcpyAsync(codes, dc, nb, hipMemcpyDeviceToHost, s->st));
	if(offs) HIPCHK(hipMemcpyAsync(offs, dof, (n + 1) * 4, hipMemcpyDeviceToHost, s->st));
	if(quals && nb) HIPCHK(hipMemcpyAsync(quals, dq, nb, hipMemcpyDeviceToHost, s->st));
	if(names && nn) HIPCHK(hipMemcpyAsync(names, dn, nn, hipMemcpyDeviceToHost, s->st));
	if(name_offs) HIPCHK(hipMemcpyAsync(name_offs, dno, (n + 1) * 4, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	return H2G_OK;
}

extern "C" h2g_status h2g_align_pairs_fetch_compact(h2g_stream* s, h2g_pair_result* res, uint8_t* rec1, size_t cap1, uint64_t* boffs1, uint8_t* rec2, size_t cap2, uint64_t* boffs2,
                                                    size_t first, size_t n)
{
	if(s) HIPCHK(sync_mach(s));
	if(!s || !res || !rec1 || !rec2 || !boffs1 || !boffs2 || first + n > s->cur().n_reads || !s->cur().d_pout) return H2G_ERR_ARG;
	if(n == 0) { boffs1[0] = boffs2[0] = 0; return H2G_OK; }
	HIPCHK(hipSetDevice(s->ix->device));
	static_assert(offsetof(PairOut, nres) == 0 && sizeof(h2g_pair_result) == sizeof(PairOut), "PairOut layout");
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(s->cur().d_pout + first);
	// the XL run's lists that PairOut cannot carry: a trailer behind mate 1's records (nullptr for every other run: the kernels take their former path)
	const uint32_t* xat = s->xlp_pout && s->xlp_pout == s->cur().d_pout ? s->d_xlp_at + first : nullptr;
	void *d_o1 = nullptr, *d_o2 = nullptr, *d_b1 = nullptr, *d_b2 = nullptr;
	int rc;
	if((rc = compact_offsets(s, s->cur().d_paln[0] + first * s->cur().pair_slots, s->cur().pair_slots, cnt, sizeof(PairOut) / 4, n, 0, s->cur().d_pout + first, 0, &d_o1, xat)) ||
	   (rc = compact_offsets(s, s->cur().d_paln[1] + first * s->cur().pair_slots, s->cur().pair_slots, cnt + 1, sizeof(PairOut) / 4, n, 2, s->cur().d_pout + first, 1, &d_o2))) return (h2g_status)rc;
	HIPCHK(hipMemcpyAsync(boffs1, d_o1, (n + 1) * 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(boffs2, d_o2, (n + 1) * 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(res, s->cur().d_pout + first, n * sizeof(PairOut), hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	for(size_t i = 0; i < n; i++) if(res[i].pad) { res[i].overflow &= ~4u; res[i].pad = 0; }      // (every record is returned; the block offset is the device's business)
	if(boffs1[n] > cap1 || boffs2[n] > cap2) return H2G_ERR_ARG;              // (boffs[n] = the bytes needed)
	if((rc = tmp_buf(s, 1, boffs1[n] + 8, &d_b1)) || (rc = tmp_buf(s, 3, boffs2[n] + 8, &d_b2))) return (h2g_status)rc;
	const unsigned g = (unsigned)((n + 255) / 256);
	if(boffs1[n]) hipLaunchKernelGGL(k_compact_gather, dim3(g), dim3(256), 0, s->st, s->cur().d_paln[0] + first * s->cur().pair_slots, s->cur().pair_slots, cnt, (uint32_t)(sizeof(PairOut) / 4),
	                                 (const unsigned long long*)d_o1, n, (uint8_t*)d_b1, s->cur().d_pout + first, (const h2g_alnres*)s->paln_ovf, 0,
	                                 xat, xat ? (const uint32_t*)s->xlp : (const uint32_t*)nullptr);
	if(boffs2[n]) hipLaunchKernelGGL(k_compact_gather, dim3(g), dim3(256), 0, s->st, s->cur().d_paln[1] + first * s->cur().pair_slots, s->cur().pair_slots, cnt + 1, (uint32_t)(sizeof(PairOut) / 4),
	                                 (const unsigned long long*)d_o2, n, (uint8_t*)d_b2, s->cur().d_pout + first, (const h2g_alnres*)s->paln_ovf, 1);
	HIPCHK(hipGetLastError());
	if(boffs1[n]) HIPCHK(hipMemcpyAsync(rec1, d_b1, boffs1[n], hipMemcpyDeviceToHost, s->st));
	if(boffs2[n]) HIPCHK(hipMemcpyAsync(rec2, d_b2, boffs2[n], hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	// the records stay where they are: h2g_sam_text_paired reads them while nothing else has taken the slots (tmp_gen)
	s->cfetch.valid = true; s->cfetch.paired = true; s->cfetch.gen = s->tmp_gen; s->cfetch.batch = s->cur_batch; s->cfetch.first = first; s->cfetch.n = n;
	s->cfetch.d_rec[0] = (const uint8_t*)d_b1; s->cfetch.d_rec[1] = (const uint8_t*)d_b2; s->cfetch.bytes[0] = boffs1[n]; s->cfetch.bytes[1] = boffs2[n];
	s->cfetch.d_boffs[0] = (const uint64_t*)d_o1; s->cfetch.d_boffs[1] = (const uint64_t*)d_o2;
	return H2G_OK;
}

extern "C" h2g_status h2g_align_fetch_compact(h2g_stream* s, h2g_read_result* res, uint8_t* rec, size_t cap, uint64_t* boffs, size_t first, size_t n) {
	if(s) HIPCHK(sync_mach(s));
	if(!s || !res || !rec || !boffs || first + n > s->cur().n_reads || !s->cur().d_rout) return H2G_ERR_ARG;
	if(n == 0) { boffs[0] = 0; return H2G_OK; }
	HIPCHK(hipSetDevice(s->ix->device));
	static_assert(offsetof(ReadOut, nselect) == 4, "ReadOut layout");
	const uint32_t* cnt = reinterpret_cast<const uint32_t*>(s->cur().d_rout + first) + 1;
	void *d_o = nullptr, *d_b = nullptr;
	int rc;
	if((rc = compact_offsets(s, s->cur().d_aln + first * s->cur().aln_slots, s->cur().aln_slots, cnt, sizeof(ReadOut) / 4, n, 0, nullptr, 0, &d_o))) return (h2g_status)rc;
	HIPCHK(hipMemcpyAsync(boffs, d_o, (n + 1) * 8, hipMemcpyDeviceToHost, s->st));
	const h2g_status hr = h2g_align_fetch(s, res, nullptr, first, n);           // (the headers; syncs the stream)
	if(hr != H2G_OK) return hr;
	if(boffs[n] > cap) return H2G_ERR_ARG;
	if((rc = tmp_buf(s, 1, boffs[n] + 8, &d_b))) return (h2g_status)rc;
	s->cfetch.valid = true; s->cfetch.paired = false; s->cfetch.gen = s->tmp_gen; s->cfetch.batch = s->cur_batch; s->cfetch.first = first; s->cfetch.n = n;
	s->cfetch.d_rec[0] = (const uint8_t*)d_b; s->cfetch.d_rec[1] = nullptr; s->cfetch.bytes[0] = boffs[n]; s->cfetch.bytes[1] = 0;
	s->cfetch.d_boffs[0] = (const uint64_t*)d_o; s->cfetch.d_boffs[1] = nullptr;
	if(boffs[n] == 0) return H2G_OK;
	hipLaunchKernelGGL(k_compact_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, s->cur().d_aln + first * s->cur().aln_slots, s->cur().aln_slots, cnt, (uint32_t)(sizeof(ReadOut) / 4),
	                   (const unsigned long long*)d_o, n, (uint8_t*)d_b, (const PairOut*)nullptr, (const h2g_alnres*)nullptr, 0);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(rec, d_b, boffs[n], hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ SAM text from a line plan (include/h2g.h)
// One descriptor per line (made on the host: h2g_sam_plan_*_compact) -> its bytes, by the emitter of h2g_sam_line.h.  k_sam_line_sizes runs it over a sink that counts,
// one lane per line, after checking what the descriptor names in its record (the host has checked everything else: plan_check); the offsets are the scan of the sizes;
// k_sam_line_write runs it over a sink that stores.  Same statements, so the two passes agree on every length.
#define H2G_SAM_LANES 16u          // lanes per line in the write kernel: four lines per wave
#define H2G_SAM_STAGE 256u         // staging bytes per line (LDS): the head and the tail of a line pass through it
struct SamWaveSync {
	// the lanes of a group are lanes of one wave: its LDS accesses are issued in program order, so only the compiler has to be told
	__host__ __device__ static __forceinline__ void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
	}
};
__global__ __launch_bounds__(256) void k_sam_line_sizes(const h2g_line::Ctx c, const h2g_sam_line* lines, size_t n, unsigned long long* sizes, unsigned int* bad) {
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i > n) return;
	if(i == n) { sizes[n] = 0; return; }
	if(!h2g_line::line_records_ok(c, lines[i])) { atomicOr(bad, 1u); sizes[i] = 0; return; }
	h2g_line::CountSink k;
	h2g_line::emit_line(c, lines[i], k);
	sizes[i] = k.n;
}
__global__ __launch_bounds__(256) void k_sam_line_write(const h2g_line::Ctx c, const h2g_sam_line* lines, size_t n, const unsigned long long* offs, char* out) {
	__shared__ char stage[256 / H2G_SAM_LANES][H2G_SAM_STAGE];
	const uint32_t g = threadIdx.x / H2G_SAM_LANES, lane = threadIdx.x % H2G_SAM_LANES;
	const size_t i = blockIdx.x * (size_t)(256 / H2G_SAM_LANES) + g;
	if(i >= n) return;
	h2g_line::GroupSink<H2G_SAM_LANES, H2G_SAM_STAGE, SamWaveSync> k(out + offs[i], stage[g], lane);
	h2g_line::emit_line(c, lines[i], k);
}

// What every text call starts with: the stream must still hold the compact fetch of the right kind; the handle's tables are uploaded when they changed.  Launches nothing.
static h2g_status sam_text_begin(h2g_stream* s, const h2g_sam* S, bool paired) {
	const h2g_stream::CompactFetch& cf = s->cfetch;
	if(!cf.valid || cf.gen != s->tmp_gen || cf.batch != s->cur_batch || cf.paired != paired) {
		snprintf(g_err, sizeof g_err, "h2g_sam_text_%s: the stream's buffers do not hold a compact %s fetch of the selected batch any more (fetch again, then call this before anything else)", paired ? "paired" : "unpaired", paired ? "paired" : "unpaired");
		return H2G_ERR_ARG;
	}
	const BatchCtx& B = s->cur();
	if(!B.has_names || (paired && !B.has_mates) || cf.first + cf.n > B.n_reads) { snprintf(g_err, sizeof g_err, "h2g_sam_text: the selected batch has no names / mates"); return H2G_ERR_ARG; }
	HIPCHK(hipSetDevice(s->ix->device));
	for(int k = 0; k < 4; k++) if(!s->ev_sam[k]) HIPCHK(s->ev_sam[k].create());
	{	// the handle's tables: uploaded once, again when the handle's options changed
		uint64_t uid, gen;
		h2g_line::sam_tables_key(S, &uid, &gen);
		if(uid != s->samtab_uid || gen != s->samtab_gen || !s->d_sam[4]) {
			h2g_line::Tables t;
			h2g_line::sam_tables(S, t);
			const size_t nr = t.refname_offs.size() - 1, ob = (nr + 1) * 4;
			HIPCHK(s->d_sam[4].reserve(ob + t.refnames.size() + t.rg.size() + 64));
			HIPCHK(hipStreamSynchronize(s->st));                      // (a text kernel still reading the former tables)
			HIPCHK(hipMemcpy(s->d_sam[4], t.refname_offs.data(), ob, hipMemcpyHostToDevice));
			if(!t.refnames.empty()) HIPCHK(hipMemcpy((char*)s->d_sam[4].get() + ob, t.refnames.data(), t.refnames.size(), hipMemcpyHostToDevice));
			if(!t.rg.empty()) HIPCHK(hipMemcpy((char*)s->d_sam[4].get() + ob + t.refnames.size(), t.rg.data(), t.rg.size(), hipMemcpyHostToDevice));
			s->samtab_uid = uid; s->samtab_gen = gen; s->samtab_nrefs = (uint32_t)nr; s->samtab_names = (uint32_t)t.refnames.size(); s->samtab_rg = (uint32_t)t.rg.size();
			s->samtab_nalts = t.nalts; s->samtab_strand = t.rna_strandness;
		}
	}
	return H2G_OK;
}
// the line offsets (+ scan tile sums + the check's flag) of n_lines lines: d_sam[2]
static int sam_text_sizes_buf(h2g_stream* s, size_t n_lines, unsigned long long** v, unsigned long long** ts, unsigned int** d_bad) {
	const size_t n1 = n_lines + 1, ntiles = (n1 + H2G_SCAN_TILE - 1) / H2G_SCAN_TILE;
	HIPCHK(s->d_sam[2].reserve((n1 + ntiles + 2) * 8));
	*v = (unsigned long long*)s->d_sam[2].get(); *ts = *v + n1; *d_bad = (unsigned int*)(*ts + ntiles + 1);
	return H2G_OK;
}
// What every text call ends with: the descriptors lie in d_sam[0] and the pool in d_sam[1] -> sizes, scan, the capacity check, write, copy-back.  flag_is_set: the
// check's flag was cleared (and maybe raised) by the caller's own kernels
static h2g_status sam_text_tail(h2g_stream* s, bool paired, size_t n_lines, size_t n_aux, char* out, size_t cap, size_t* used, uint64_t* line_offs, uint64_t uploaded, bool flag_is_set) {
	const h2g_stream::CompactFetch& cf = s->cfetch;
	const BatchCtx& B = s->cur();
	const size_t n1 = n_lines + 1, ntiles = (n1 + H2G_SCAN_TILE - 1) / H2G_SCAN_TILE;
	int rc;
	unsigned long long *v, *ts; unsigned int* d_bad;
	if((rc = sam_text_sizes_buf(s, n_lines, &v, &ts, &d_bad))) return (h2g_status)rc;
	if(!flag_is_set) HIPCHK(hipMemsetAsync(d_bad, 0, 8, s->st));
	h2g_line::Ctx c;
	c.names[0] = B.d_names; c.noffs[0] = B.d_name_offs; c.codes[0] = B.d_codes; c.offs[0] = B.d_offs; c.quals[0] = B.has_quals ? B.d_quals : nullptr;
	c.names[1] = paired ? B.d_names2 : nullptr; c.noffs[1] = paired ? B.d_name_offs2 : nullptr; c.codes[1] = paired ? B.d_codes2 : nullptr; c.offs[1] = paired ? B.d_offs2 : nullptr;
	c.quals[1] = paired && B.has_quals2 ? B.d_quals2 : nullptr;
	c.rec[0] = cf.d_rec[0]; c.rec[1] = cf.d_rec[1]; c.nrec[0] = cf.bytes[0]; c.nrec[1] = cf.bytes[1];
	c.aux = (const char*)s->d_sam[1].get(); c.n_aux = n_aux;
	c.refname_offs = (const uint32_t*)s->d_sam[4].get(); c.refnames = (const char*)s->d_sam[4].get() + ((size_t)s->samtab_nrefs + 1) * 4; c.nrefs = s->samtab_nrefs;
	c.rg = c.refnames + s->samtab_names; c.rg_len = s->samtab_rg; c.rna_strandness = s->samtab_strand; c.nalts = s->samtab_nalts;
	c.first = (uint32_t)cf.first; c.paired = paired ? 1u : 0u; c.long_edits = nullptr;
	const h2g_sam_line* d_lines = (const h2g_sam_line*)s->d_sam[0].get();
	HIPCHK(hipEventRecord(s->ev_sam[0], s->st));
	hipLaunchKernelGGL(k_sam_line_sizes, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s->st, c, d_lines, n_lines, v, d_bad);
	hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles), dim3(256), 0, s->st, v, n1, ts);
	hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, s->st, ts, ntiles);
	hipLaunchKernelGGL(k_scan_add, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s->st, v, n1, (const unsigned long long*)ts);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->ev_sam[1], s->st));
	unsigned long long total = 0; unsigned int bad = 0;
	HIPCHK(hipMemcpyAsync(&total, v + n_lines, 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	if(bad) { snprintf(g_err, sizeof g_err, "h2g_sam_text: a line names a record that does not end inside its mate's bytes, keeps its edits outside itself, or lies on a reference the index does not have"); return H2G_ERR_ARG; }
	*used = (size_t)total;
	if(total > cap || !out) return total == 0 ? H2G_OK : H2G_ERR_ARG;     // (nothing is written: the write kernel is not launched)
	HIPCHK(s->d_sam[3].reserve((size_t)total + 64));
	HIPCHK(hipEventRecord(s->ev_sam[2], s->st));
	hipLaunchKernelGGL(k_sam_line_write, dim3((unsigned)((n_lines + 256 / H2G_SAM_LANES - 1) / (256 / H2G_SAM_LANES))), dim3(256), 0, s->st, c, d_lines, n_lines, (const unsigned long long*)v, (char*)s->d_sam[3].get());
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->ev_sam[3], s->st));
	HIPCHK(hipMemcpyAsync(out, s->d_sam[3], (size_t)total, hipMemcpyDeviceToHost, s->st));
	if(line_offs) HIPCHK(hipMemcpyAsync(line_offs, v, n1 * 8, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	float a = 0, b = 0;
	if(hipEventElapsedTime(&a, s->ev_sam[0], s->ev_sam[1]) != hipSuccess) a = 0;
	if(hipEventElapsedTime(&b, s->ev_sam[2], s->ev_sam[3]) != hipSuccess) b = 0;
	(void)hipGetLastError();
	s->sam_stats.bytes_uploaded = uploaded; s->sam_stats.bytes_written = total; s->sam_stats.kernel_ms = a + b; s->sam_stats.write_kernel_ms = b;
	return H2G_OK;
}
static h2g_status sam_text(h2g_stream* s, const h2g_sam* S, bool paired, const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux, char* out, size_t cap, size_t* used, uint64_t* line_offs) {
	if(!s || !S || !used || (n_lines && !lines) || (n_aux && !aux)) return H2G_ERR_ARG;
	*used = 0;
	h2g_status hr = sam_text_begin(s, S, paired);
	if(hr != H2G_OK) return hr;
	if(n_lines == 0) { if(line_offs) line_offs[0] = 0; return H2G_OK; }
	const h2g_stream::CompactFetch& cf = s->cfetch;
	if(const char* why = h2g_line::plan_check(lines, n_lines, cf.n, paired, cf.bytes[0], cf.bytes[1], n_aux, s->samtab_nrefs)) { snprintf(g_err, sizeof g_err, "h2g_sam_text: %s", why); return H2G_ERR_ARG; }
	HIPCHK(s->d_sam[0].reserve(n_lines * sizeof(h2g_sam_line) + 64));
	HIPCHK(s->d_sam[1].reserve(n_aux + 64));
	HIPCHK(hipMemcpyAsync(s->d_sam[0], lines, n_lines * sizeof(h2g_sam_line), hipMemcpyHostToDevice, s->st));
	if(n_aux) HIPCHK(hipMemcpyAsync(s->d_sam[1], aux, n_aux, hipMemcpyHostToDevice, s->st));
	return sam_text_tail(s, paired, n_lines, n_aux, out, cap, used, line_offs, n_lines * sizeof(h2g_sam_line) + n_aux, false);
}
extern "C" h2g_status h2g_sam_text_unpaired(h2g_stream* s, const h2g_sam* S, const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux, char* out, size_t cap, size_t* used, uint64_t* line_offs) {
	return sam_text(s, S, false, lines, n_lines, aux, n_aux, out, cap, used, line_offs);
}
extern "C" h2g_status h2g_sam_text_paired(h2g_stream* s, const h2g_sam* S, const h2g_sam_line* lines, size_t n_lines, const char* aux, size_t n_aux, char* out, size_t cap, size_t* used, uint64_t* line_offs) {
	return sam_text(s, S, true, lines, n_lines, aux, n_aux, out, cap, used, line_offs);
}
extern "C" h2g_status h2g_get_sam_text_stats(h2g_stream* s, h2g_sam_text_stats* out) {
	if(!s || !out) return H2G_ERR_ARG;
	*out = s->sam_stats;
	return H2G_OK;
}

// ------------------------------------------------------------------------------------------ plain SAM lines planned on the device (include/h2g.h, csrc/h2g_sam_plan.h)
// k_sam_plan_*: one lane per read / pair of the compact fetch.  It reads its result header, walks its records inside [boffs[i], boffs[i + 1]) and leaves a class byte (0 =
// handed on to the host planner), its line count and, for a plain read, its descriptors in two fixed slots.  What does not parse inside its bytes is handed on, never followed.
struct SamPlanArgs { h2g_plan::Opts O; h2g_plan::In in; size_t n; uint8_t* cls; unsigned long long* v; h2g_sam_line* slots; };
__device__ __forceinline__ void sam_plan_done(const SamPlanArgs& a, size_t i, uint32_t c, uint32_t made) {
	const uint32_t want = h2g_plan::lines_of_class(c, a.O.no_unal != 0);      // (what the host derives from the class byte: the two never differ)
	if(made != want) c = h2g_plan::CLS_HOST;
	a.cls[i] = (uint8_t)c;
	a.v[i] = c ? want : 0u;
}
__global__ __launch_bounds__(256) void k_sam_plan_unpaired(const SamPlanArgs a, const ReadOut* res) {
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i > a.n) return;
	if(i == a.n) { a.v[a.n] = 0; return; }
	const h2g_plan::UnpHead h = {res[i].nselect, res[i].best, res[i].secbest, res[i].best_h2, res[i].secbest_h2};
	h2g_plan::Pick pk;
	const uint32_t c = h2g_plan::classify_unpaired(a.O, a.in, h, (uint32_t)i, &pk);
	sam_plan_done(a, i, c, c ? h2g_plan::plan_plain_unpaired(a.O, a.in, c, pk, (uint32_t)i, a.slots + 2 * i) : 0u);
}
__global__ __launch_bounds__(256) void k_sam_plan_paired(const SamPlanArgs a, const h2g_pair_result* res) {
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i > a.n) return;
	if(i == a.n) { a.v[a.n] = 0; return; }
	h2g_plan::Pick pk;
	const uint32_t c = h2g_plan::classify_pair(a.O, a.in, res[i], (uint32_t)i, &pk);
	sam_plan_done(a, i, c, c ? h2g_plan::plan_plain_pair(a.O, a.in, c, pk, (uint32_t)i, a.slots + 2 * i) : 0u);
}
// The merge.  A handed-on read's entry: its index, its lines, its pool bytes, where its descriptors start in the upload.  The count array carries lines in its low and pool
// bytes in its high 32 bits, so one exclusive scan yields every read's first line and the running pool offset its plain lines carry in aux_off.
struct SamHardEntry { uint32_t idx, cnt, aux, start; };
__global__ __launch_bounds__(256) void k_sam_plan_scatter(const SamHardEntry* e, size_t nh, size_t n, const uint8_t* cls, unsigned long long* v, uint32_t* hsrc) {
	const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(j >= nh) return;
	const uint32_t i = e[j].idx;
	if(i >= n || cls[i]) return;
	v[i] = (unsigned long long)e[j].cnt | ((unsigned long long)e[j].aux << 32);
	hsrc[i] = e[j].start;
}
__global__ __launch_bounds__(256) void k_sam_plan_place(const uint8_t* cls, const unsigned long long* v, const uint32_t* hsrc, const h2g_sam_line* slots, const h2g_sam_line* hard, size_t n_hard,
                                                        size_t n, size_t n_lines, h2g_sam_line* lines, unsigned long long* ends, unsigned int* bad)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	if(i >= n) return;
	if(i == 0 && (uint32_t)v[n] != n_lines) atomicOr(bad, 1u);
	const uint32_t b = (uint32_t)v[i], e = (uint32_t)v[i + 1], auxat = (uint32_t)(v[i] >> 32);
	const bool plain = cls[i] != 0;
	const h2g_sam_line* src = plain ? slots + 2 * i : hard + hsrc[i];
	for(uint32_t k = 0; b + k < e; k++) {
		if(b + k >= n_lines || (plain ? k >= 2 : (size_t)hsrc[i] + k >= n_hard)) { atomicOr(bad, 1u); break; }
		const uint4* sw = reinterpret_cast<const uint4*>(src + k);
		uint4 w0 = sw[0], w1 = sw[1], w2 = sw[2], w3 = sw[3];
		if(plain) w2.w = auxat;                                             // aux_off (byte 44): the pool bytes of every read before this one
		uint4* dw = reinterpret_cast<uint4*>(lines + b + k);
		dw[0] = w0; dw[1] = w1; dw[2] = w2; dw[3] = w3;
	}
	ends[i] = e;
}
static_assert(offsetof(h2g_sam_line, aux_off) == 44, "k_sam_plan_place sets aux_off in the third 16-byte word");

static h2g_status sam_text_planned(h2g_stream* s, const h2g_sam* S, bool paired, const h2g_plan::HostSets& rd, size_t n, const void* res, const uint8_t* rec1, const uint64_t* boffs1,
                                   const uint8_t* rec2, const uint64_t* boffs2, uint32_t khits, char* out, size_t cap, size_t* used, uint64_t* line_offs, size_t line_cap, size_t* n_lines_out, uint64_t* line_ends)
{
	if(!s || !S || !used || !res || !rec1 || !boffs1 || (paired && (!rec2 || !boffs2)) || (line_offs && !n_lines_out)) return H2G_ERR_ARG;
	*used = 0;
	if(n_lines_out) *n_lines_out = 0;
	h2g_status hr = sam_text_begin(s, S, paired);
	if(hr != H2G_OK) return hr;
	const h2g_stream::CompactFetch& cf = s->cfetch;
	if(n != cf.n || boffs1[n] != cf.bytes[0] || (paired && boffs2[n] != cf.bytes[1])) { snprintf(g_err, sizeof g_err, "h2g_sam_text_planned: the host arrays are not those of the stream's last compact fetch"); return H2G_ERR_ARG; }
	s->plan_stats = h2g_sam_plan_stats(); s->plan_classes.clear();
	if(n == 0) { if(line_offs) line_offs[0] = 0; return H2G_OK; }
	for(int k = 0; k < 4; k++) if(!s->ev_plan[k]) HIPCHK(s->ev_plan[k].create());
	const BatchCtx& B = s->cur();
	SamPlanArgs a;
	const uint8_t* qc[2] = {nullptr, nullptr};
	h2g_plan::sam_plan_opts(S, a.O, &qc[0], &qc[1]);
	a.O.nrefs = s->samtab_nrefs;
	const size_t ntiles_r = (n + 1 + H2G_SCAN_TILE - 1) / H2G_SCAN_TILE;
	int rc;
	// d_plan[2]: counts [n + 1], tile sums [ntiles + 1], line ends [n], sources [n]
	HIPCHK(s->d_plan[0].reserve(2 * n * sizeof(h2g_sam_line)));
	HIPCHK(s->d_plan[1].reserve(3 * n + 64));
	HIPCHK(s->d_plan[2].reserve((n + 1 + ntiles_r + 1 + n) * 8 + n * 4 + 64));
	uint8_t* d_cls = s->d_plan[1];
	unsigned long long* v = (unsigned long long*)s->d_plan[2].get();
	unsigned long long* ts = v + n + 1;
	unsigned long long* d_ends = ts + ntiles_r + 1;
	uint32_t* d_hsrc = (uint32_t*)(d_ends + n);
	uint64_t uploaded = 0;
	for(int m = 0; m < (paired ? 2 : 1); m++) if(qc[m]) { HIPCHK(hipMemcpyAsync(d_cls + (size_t)(m + 1) * n, qc[m], n, hipMemcpyHostToDevice, s->st)); uploaded += n; }
	a.in.codes[0] = B.d_codes; a.in.offs[0] = B.d_offs; a.in.codes[1] = paired ? B.d_codes2 : nullptr; a.in.offs[1] = paired ? B.d_offs2 : nullptr;
	a.in.qc[0] = qc[0] ? d_cls + n : nullptr; a.in.qc[1] = paired && qc[1] ? d_cls + 2 * n : nullptr;
	a.in.rec[0] = cf.d_rec[0]; a.in.rec[1] = cf.d_rec[1]; a.in.boffs[0] = cf.d_boffs[0]; a.in.boffs[1] = cf.d_boffs[1]; a.in.nrec[0] = cf.bytes[0]; a.in.nrec[1] = cf.bytes[1];
	a.in.first = (uint32_t)cf.first;
	a.n = n; a.cls = d_cls; a.v = v; a.slots = (h2g_sam_line*)s->d_plan[0].get();
	const unsigned g1 = (unsigned)((n + 1 + 255) / 256);
	HIPCHK(hipEventRecord(s->ev_plan[0], s->st));
	if(paired) hipLaunchKernelGGL(k_sam_plan_paired, dim3(g1), dim3(256), 0, s->st, a, reinterpret_cast<const h2g_pair_result*>(B.d_pout + cf.first));
	else hipLaunchKernelGGL(k_sam_plan_unpaired, dim3(g1), dim3(256), 0, s->st, a, (const ReadOut*)(B.d_rout + cf.first));
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s->ev_plan[1], s->st));
	std::vector<uint8_t> cls(n);
	HIPCHK(hipMemcpyAsync(cls.data(), d_cls, n, hipMemcpyDeviceToHost, s->st));
	HIPCHK(hipStreamSynchronize(s->st));
	// the host step: the handed-on reads through the host planner, the plain ones counted by class
	std::vector<uint32_t> hard;
	size_t n_plain_lines = 0;
	for(size_t i = 0; i < n; i++) { if(cls[i]) n_plain_lines += h2g_plan::lines_of_class(cls[i], a.O.no_unal != 0); else hard.push_back((uint32_t)i); }
	std::vector<h2g_sam_line> hl; std::string ha; std::vector<uint64_t> hends;
	h2g_plan::HostPart* part = nullptr;
	const auto t0 = std::chrono::steady_clock::now();
	hr = h2g_plan::plan_subset(S, paired, rd, n, res, rec1, boffs1, rec2, boffs2, khits, hard.data(), hard.size(), hl, ha, hends, &part);
	const float host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if(hr != H2G_OK) { snprintf(g_err, sizeof g_err, "h2g_sam_text_planned: the host planner refused the handed-on reads (malformed records, or a long record without its area)"); return hr; }
	struct Discard { h2g_plan::HostPart* p; ~Discard() { h2g_plan::plan_discard(p); } } guard{part};      // (until the text is delivered)
	const size_t n_lines = n_plain_lines + hl.size(), n_aux = ha.size();
	if(n_lines_out) *n_lines_out = n_lines;
	if(const char* why = h2g_line::plan_check(hl.data(), hl.size(), cf.n, paired, cf.bytes[0], cf.bytes[1], n_aux, s->samtab_nrefs)) { snprintf(g_err, sizeof g_err, "h2g_sam_text_planned: %s", why); return H2G_ERR_ARG; }
	if(n_lines >= 0xffffffffull) return H2G_ERR_ARG;
	const bool short_lines = line_offs && n_lines > line_cap;      // (the bytes needed are still worked out: *used)
	if(n_lines == 0) { if(line_offs) line_offs[0] = 0; }
	else {
		std::vector<SamHardEntry> he(hard.size());
		for(size_t j = 0, b = 0; j < hard.size(); j++) {
			uint64_t ab = 0;
			for(size_t k = b; k < hends[j]; k++) ab += hl[k].aux_len;
			he[j] = {hard[j], (uint32_t)(hends[j] - b), (uint32_t)ab, (uint32_t)b};
			b = hends[j];
		}
		unsigned long long *lv, *lts; unsigned int* d_bad;
		HIPCHK(s->d_sam[0].reserve(n_lines * sizeof(h2g_sam_line) + 64));
		HIPCHK(s->d_sam[1].reserve(n_aux + 64));
		HIPCHK(s->d_plan[3].reserve(he.size() * sizeof(SamHardEntry) + 64));
		HIPCHK(s->d_plan[4].reserve(hl.size() * sizeof(h2g_sam_line) + 64));
		if((rc = sam_text_sizes_buf(s, n_lines, &lv, &lts, &d_bad))) return (h2g_status)rc;
		if(!he.empty()) HIPCHK(hipMemcpyAsync(s->d_plan[3], he.data(), he.size() * sizeof(SamHardEntry), hipMemcpyHostToDevice, s->st));
		if(!hl.empty()) HIPCHK(hipMemcpyAsync(s->d_plan[4], hl.data(), hl.size() * sizeof(h2g_sam_line), hipMemcpyHostToDevice, s->st));
		if(n_aux) HIPCHK(hipMemcpyAsync(s->d_sam[1], ha.data(), n_aux, hipMemcpyHostToDevice, s->st));
		uploaded += he.size() * sizeof(SamHardEntry) + hl.size() * sizeof(h2g_sam_line) + n_aux;
		HIPCHK(hipMemsetAsync(d_bad, 0, 8, s->st));
		HIPCHK(hipMemsetAsync(s->d_sam[0], 0, n_lines * sizeof(h2g_sam_line), s->st));
		HIPCHK(hipEventRecord(s->ev_plan[2], s->st));
		if(!he.empty()) hipLaunchKernelGGL(k_sam_plan_scatter, dim3((unsigned)((he.size() + 255) / 256)), dim3(256), 0, s->st, (const SamHardEntry*)s->d_plan[3].get(), he.size(), n, (const uint8_t*)d_cls, v, d_hsrc);
		hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)ntiles_r), dim3(256), 0, s->st, v, n + 1, ts);
		hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, s->st, ts, ntiles_r);
		hipLaunchKernelGGL(k_scan_add, dim3(g1), dim3(256), 0, s->st, v, n + 1, (const unsigned long long*)ts);
		hipLaunchKernelGGL(k_sam_plan_place, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->st, (const uint8_t*)d_cls, (const unsigned long long*)v, (const uint32_t*)d_hsrc,
		                   (const h2g_sam_line*)s->d_plan[0].get(), (const h2g_sam_line*)s->d_plan[4].get(), hl.size(), n, n_lines, (h2g_sam_line*)s->d_sam[0].get(), d_ends, d_bad);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(s->ev_plan[3], s->st));
		// the shared tail; a line array that is too short: the sizes only (a capacity of 0 writes nothing)
		hr = sam_text_tail(s, paired, n_lines, n_aux, short_lines ? nullptr : out, short_lines ? 0 : cap, used, short_lines ? nullptr : line_offs, uploaded, true);
		if(hr != H2G_OK) return hr;
		if(short_lines) return H2G_ERR_ARG;
		if(*used && (!out || *used > cap)) return H2G_ERR_ARG;
	}
	if(line_ends) {
		if(n_lines) { HIPCHK(hipMemcpyAsync(line_ends, d_ends, n * 8, hipMemcpyDeviceToHost, s->st)); HIPCHK(hipStreamSynchronize(s->st)); }
		else memset(line_ends, 0, n * 8);
	}
	// delivered: now it counts
	guard.p = nullptr;
	h2g_plan::plan_commit(S, part, cls.data(), n);
	float ka = 0, kb = 0;
	if(hipEventElapsedTime(&ka, s->ev_plan[0], s->ev_plan[1]) != hipSuccess) ka = 0;
	if(n_lines == 0 || hipEventElapsedTime(&kb, s->ev_plan[2], s->ev_plan[3]) != hipSuccess) kb = 0;
	(void)hipGetLastError();
	s->plan_stats.device_planned = n - hard.size(); s->plan_stats.host_planned = hard.size(); s->plan_stats.n_lines = n_lines; s->plan_stats.bytes_uploaded = uploaded;
	for(const h2g_sam_line& d : hl) s->plan_stats.whole_lines += (d.bits & H2G_SAM_LINE_WHOLE_LINE) != 0;
	s->plan_stats.plan_kernel_ms = ka + kb; s->plan_stats.host_plan_ms = host_ms;
	s->plan_classes.swap(cls);
	return H2G_OK;
}
extern "C" h2g_status h2g_sam_text_unpaired_planned(h2g_stream* s, const h2g_sam* S, const uint8_t* codes, const uint32_t* offs, const char* quals, const char* nb, const uint32_t* noffs, size_t n,
                                                    const h2g_read_result* res, const uint8_t* rec, const uint64_t* boffs, char* out, size_t cap, size_t* used, uint64_t* line_offs, size_t line_cap,
                                                    size_t* n_lines, uint64_t* line_ends)
{
	const h2g_plan::HostSets rd = {{codes, nullptr}, {offs, nullptr}, {quals, nullptr}, {nb, nullptr}, {noffs, nullptr}};
	return sam_text_planned(s, S, false, rd, n, res, rec, boffs, nullptr, nullptr, 0, out, cap, used, line_offs, line_cap, n_lines, line_ends);
}
extern "C" h2g_status h2g_sam_text_paired_planned(h2g_stream* s, const h2g_sam* S, const uint8_t* codes1, const uint32_t* offs1, const char* quals1, const char* nb1, const uint32_t* noffs1,
                                                  const uint8_t* codes2, const uint32_t* offs2, const char* quals2, const char* nb2, const uint32_t* noffs2, size_t n, const h2g_pair_result* res,
                                                  const uint8_t* rec1, const uint64_t* boffs1, const uint8_t* rec2, const uint64_t* boffs2, uint32_t khits,
                                                  char* out, size_t cap, size_t* used, uint64_t* line_offs, size_t line_cap, size_t* n_lines, uint64_t* line_ends)
{
	const h2g_plan::HostSets rd = {{codes1, codes2}, {offs1, offs2}, {quals1, quals2}, {nb1, nb2}, {noffs1, noffs2}};
	return sam_text_planned(s, S, true, rd, n, res, rec1, boffs1, rec2, boffs2, khits, out, cap, used, line_offs, line_cap, n_lines, line_ends);
}
extern "C" h2g_status h2g_get_sam_plan_stats(h2g_stream* s, h2g_sam_plan_stats* out, uint8_t* classes, size_t cap) {
	if(!s || !out) return H2G_ERR_ARG;
	*out = s->plan_stats;
	if(classes) {
		if(cap < s->plan_classes.size()) return H2G_ERR_ARG;
		if(!s->plan_classes.empty()) memcpy(classes, s->plan_classes.data(), s->plan_classes.size());
	}
	return H2G_OK;
}

// page-locked host memory for the buffers a caller hands to the set_* / fetch_* entry points: copies from / to it run at the link's rate and asynchronously
extern "C" void* h2g_host_alloc(size_t bytes) { void* p = nullptr; if(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
extern "C" void h2g_host_free(void* p) { if(p) (void)hipHostFree(p); }

// The edit lists of the records with more than H2G_MAX_EDITS edits of the resident batch (include/h2g.h): the used prefix of the stream's long-edit
// area, offsets as the records carry them in edits[0].pos.  *n = edits the prefix spans (0: no such record); H2G_ERR_ARG when cap is smaller.
extern "C" h2g_status h2g_align_fetch_long_edits(h2g_stream* s, h2g_edit* out, size_t cap, size_t* n) {
	if(!s || !n) return H2G_ERR_ARG;
	*n = 0;
	if(!s->ran_align || !s->ledits || !s->d_ledits_cur) return H2G_OK;
	HIPCHK(hipSetDevice(s->ix->device));
	HIPCHK(sync_mach(s));
	HIPCHK(hipStreamSynchronize(s->st));
	uint32_t cur[H2G_MSTREAMS_MAX];
	HIPCHK(hipMemcpy(cur, s->d_ledits_cur, sizeof cur, hipMemcpyDeviceToHost));
	// (only the parts the runs since the last upload wrote to: a part left over from an earlier batch keeps its cursor until its lane is used again — ADVICE r5;
	// a full part's cursor is clamped: the reads that found no room are flagged)
	PartSpan span[H2G_MSTREAMS_MAX];
	const size_t hi = part_spans(cur, s->ledits_touched, s->ledits.parts, s->ledits.cap, span);
	*n = hi;
	if(hi == 0) return H2G_OK;
	if(!out || cap < hi) return H2G_ERR_ARG;
	for(unsigned m = 0; m < s->ledits.parts; m++)
		if(span[m].end > span[m].lo) HIPCHK(hipMemcpy(out + span[m].lo, s->ledits + span[m].lo, (span[m].end - span[m].lo) * sizeof(h2g_edit), hipMemcpyDeviceToHost));
	return H2G_OK;
}

// development hook: measurement / debugging knobs of go_run by name (g_knobs, and "mstreams" / "mstreams_light").  Everything in flight is waited for first, so a
// change never meets a queued run.
extern "C" __attribute__((visibility("default"))) int h2g_stream_tune(h2g_stream* s, const char* key, long v) {
	if(!s || !key) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	for(unsigned k_ = 0; k_ < s->n_mst; k_++) HIPCHK(hipStreamSynchronize(s->mst[k_]));   // (whatever st2_busy says: a change never meets a queued run)
	const std::string k(key);
	if(k == "mstreams") { s->mstreams = clamp_mstreams(v); s->gen = 0; return H2G_OK; }   // pins lanes = machine streams (nothing is in flight: every buffer set is free)
	if(k == "mstreams_light") { s->mstreams_light = clamp_mstreams(v); return H2G_OK; }   // S of the light regime (mstreams_policy)
	if(k == "mach_total" && v <= 0) { s->tune.mach_total_auto = 1; s->tune.mach_total = H2G_MACH_TOTAL; return H2G_OK; }      // (0 = the default policy)
	if(k == "drain_grid") v = v < 1 ? 1 : v > 128 ? 128 : v;
	for(const Knob& kn : g_knobs) if(k == kn.key) {
		kn.set(s->tune, v);
		if(kn.is_auto) s->tune.*kn.is_auto = 0;
		return H2G_OK;
	}
	return H2G_ERR_ARG;
}

// development hook (tests): what a stream holds for the machine's passes, by name — "mstreams_rotation" (machine streams in rotation for the last run behind a
// fast pass), "mstreams_used" (machine streams that ever entered the rotation), "mstreams_created" (HIP streams that exist), "pools" (workspace pools allocated), "lanes".  Read-only: nothing is waited for.  -1: no such name
extern "C" __attribute__((visibility("default"))) long h2g_stream_probe(const h2g_stream* s, const char* key) {
	if(!s || !key) return -1;
	const std::string k(key);
	if(k == "mstreams_rotation") return (long)s->rot;
	if(k == "mstreams_used") return (long)s->n_mst;
	if(k == "mstreams_created") { long n = 0; for(hipStream_t m : s->mst) n += m != nullptr; return n; }
	if(k == "lanes") return (long)(s->mstreams ? s->mstreams : H2G_MSTREAMS_MAX);
	if(k == "pools") { long n = 0; for(const h2g_stream::MachStream& m : s->mach) n += bool(m.main.ws) + bool(m.second.ws); return n; }
	return -1;
}

// development hook (h2g_stream_tune "dbg_read" / env H2G_GO_DBG_READ=<read id>): the primitive requests of that read in the last go() launch, 8 words each
extern "C" __attribute__((visibility("default"))) int h2g_go_debug_trace(h2g_stream* s, uint32_t* out, uint32_t cap_words) {
	if(s) HIPCHK(sync_mach(s));   // (results of the machine pass on the second stream)
	if(!s || !out || !s->dbg_buf) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	HIPCHK(hipMemcpy(out, s->dbg_buf, (size_t)cap_words * 4, hipMemcpyDeviceToHost));
	return H2G_OK;
}

// development hook (builds with -DH2G_GO_PROF): the wave-level time split of the last go() launch, 48 slots (h2g_go_kernels.h)
extern "C" __attribute__((visibility("default"))) int h2g_go_prof(h2g_stream* s, unsigned long long* out48) {
	if(!s || !out48) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	HIPCHK(hipMemcpy(out48, s->cnt_cur + H2G_CNT_PROF_GO, 80 * sizeof(unsigned long long), hipMemcpyDeviceToHost));   // [0..47] split, [64..79] control by source ring (H2G_CNT_PROF_GO_CTL)
	return H2G_OK;
}

// development hook (builds with -DH2G_GO_PROF): the wave-level time split of the last fast pass, 48 slots + 24 bail reasons (h2g_k_go_fast.hip)
extern "C" __attribute__((visibility("default"))) int h2g_go_fast_prof(h2g_stream* s, unsigned long long* out72 /* [136] */) {
	if(!s || !out72) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	HIPCHK(hipMemcpy(out72, s->cnt_cur + H2G_CNT_PROF_FAST, 48 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out72 + 48, s->cnt_cur + H2G_CNT_FAST_BAIL_WHY, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(out72 + 72, s->cnt_cur + H2G_CNT_PROF_FAST_SITE, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));   // control time / trips by site
	return H2G_OK;
}
#ifdef H2G_GO_PROF
extern "C" __attribute__((visibility("default"))) int h2g_go_fast_prof_bins(h2g_stream* s, unsigned long long* out256) {
	if(!s || !out256) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	HIPCHK(hipMemcpy(out256, s->cnt_cur + H2G_CNT_PROF_FAST_BINS, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	return H2G_OK;
}
#endif

extern "C" h2g_status h2g_get_counters(h2g_stream* s, h2g_counters* c) {
	if(!s || !c) return H2G_ERR_ARG;
	HIPCHK(sync_all(s));
	unsigned long long v[16];
	unsigned long long* const cb = s->ran_align ? s->cnt_cur : s->d_counters;
	HIPCHK(hipMemcpy(v, cb, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(v + 8, cb + (s->ran_align ? H2G_CNT_SECOND : H2G_CNT_NO_SECOND), 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	// [0..7] the main pass, [8..15] <- H2G_CNT_SECOND: the second pass over its overflowed reads (go_run)
	s->last.n_rank = v[0] + v[8]; s->last.n_side = v[1] + v[9]; s->last.n_sa_steps = v[2] + v[10]; s->last.n_ext = v[3];
	s->last.n_aligned = v[4] + v[12];
	uint32_t nsecond = 0;
	if(s->ovf_cur->ovf_list && s->ran_align) HIPCHK(hipMemcpy(&nsecond, s->ovf_cur->ovf_list + s->max_reads, 4, hipMemcpyDeviceToHost));
	s->last.n_second_pass = nsecond;
	s->last.n_overflow = nsecond ? v[13] : v[5];   // reads still flagged after the last pass that saw them
	s->last.n_queries = s->cur().n_reads * 2;
	float t = 0;
	if(s->ran_seed) {
		if(hipEventElapsedTime(&t, s->tm[TM_SEED0], s->tm[TM_SEED_MID]) == hipSuccess) s->last.ms_search = t;
		if(hipEventElapsedTime(&t, s->tm[TM_SEED_MID], s->tm[TM_SEED1]) == hipSuccess) s->last.ms_resolve_extend = t;
	}
	if(s->ran_align && hipEventElapsedTime(&t, s->tm[TM_MAIN0], s->tm[TM_MAIN1]) == hipSuccess) s->last.ms_align_kernel = t;
	if(s->ran_align && hipEventElapsedTime(&t, s->tm[TM_RUN0], s->tm[TM_RUN1]) == hipSuccess) s->last.ms_align = t;   // every pass
	s->last.n_fast = 0; s->last.n_fast_bail = 0; s->last.ms_fast_kernel = 0; s->last.pad_ = 0; s->last.n_fast_side = 0; s->last.n_fast_sa_steps = 0;
	s->last.ms_drain_kernel = 0; s->last.pad2_ = 0; s->last.n_drain_side = 0; s->last.n_drain_sa_steps = 0; s->last.n_adopted = 0;
	if(s->ran_align && s->ran_fast) {
		unsigned long long f[2], fc[4];
		HIPCHK(hipMemcpy(f, s->cnt_cur + H2G_CNT_FAST_DONE, sizeof f, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(fc, s->cnt_cur + H2G_CNT_FAST_RANK, sizeof fc, hipMemcpyDeviceToHost));
		s->last_bails = (uint32_t)f[1];
		s->last.n_fast = f[0]; s->last.n_fast_bail = f[1];
		s->last.n_fast_side = fc[1]; s->last.n_fast_sa_steps = fc[2];
		s->last.n_rank += fc[0]; s->last.n_side += fc[1]; s->last.n_sa_steps += fc[2]; s->last.n_aligned += fc[3];
		if(hipEventElapsedTime(&t, s->tm[TM_RUN0], s->tm[TM_FAST1]) == hipSuccess) s->last.ms_fast_kernel = t;
		if(s->ran_drain) {
			unsigned long long dc[4]; uint32_t nad = 0;
			HIPCHK(hipMemcpy(dc, s->cnt_cur + H2G_CNT_FAST_RANK + H2G_CNT_DRAIN_OFF, sizeof dc, hipMemcpyDeviceToHost));
			HIPCHK(hipMemcpy(&nad, s->orph_cur, 4, hipMemcpyDeviceToHost));
			s->last.n_drain_side = dc[1]; s->last.n_drain_sa_steps = dc[2]; s->last.n_adopted = nad;
			s->last.n_rank += dc[0]; s->last.n_side += dc[1]; s->last.n_sa_steps += dc[2]; s->last.n_aligned += dc[3];
			if(hipEventElapsedTime(&t, s->ev_dr[0], s->ev_dr[1]) == hipSuccess) s->last.ms_drain_kernel = t;
		}
	}
	(void)hipGetLastError();
	*c = s->last;
	return H2G_OK;
}
