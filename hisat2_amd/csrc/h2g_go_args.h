// h2g_go_args.h — the one kernel-argument block of every go() kernel build, and the extern "C" face of the translation
// units that instantiate them.  Nothing in here depends on a unit's AL_MAX_* capacities: the per-lane workspaces are passed
// as byte pools with strides, the results as fixed-layout records.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include "h2g_align.h"
#include "h2g_graph.h"
#include "h2g_fast.h"

// The counter block of one go_run generation (h2g_stream::d_counters holds H2G_NBUF of them), in 64-bit words.  Block 0 also serves the seed pipeline
// (h2g_seed_extend_run: RANK .. EXT, read by h2g_get_counters before any go() run) and the rank benches' scratch words (BENCH_SUM, BENCH_CHECKSUM).
enum : unsigned {
	H2G_CNT_RANK = 0, H2G_CNT_SIDE = 1, H2G_CNT_STEPS = 2, H2G_CNT_EXT = 3,   // a machine pass (and the seed pipeline): rank calls, sides, SA steps, extensions
	H2G_CNT_ALIGNED = 4, H2G_CNT_OVERFLOW = 5,                                 // ... reads aligned, reads still flagged
	H2G_CNT_FAST_DONE = 6, H2G_CNT_FAST_BAILED = 7,                            // the fast pass: reads it completed, reads it handed on
	H2G_CNT_BENCH_SUM = 6, H2G_CNT_BENCH_CHECKSUM = 7,                         // (the rank benches, block 0: never next to a go() run's)
	H2G_CNT_WORK_FAST = 12, H2G_CNT_WORK_DRAIN = 13, H2G_CNT_WORK_MAIN = 14, H2G_CNT_WORK_SECOND = 15,   // work cursors (a uint32_t in the low half of the word)
	H2G_CNT_PROF_GO = 16, H2G_CNT_PROF_GO_CTL = 80,                            // H2G_GO_PROF: a machine pass's time split (48 words), control by source ring (16)
	H2G_CNT_NO_SECOND = 64,                                                    // [64, 72): written by nobody — the second pass h2g_get_counters reads before any go() run
	H2G_CNT_FAST_BAIL_WHY = 96,                                                // the fast pass's hand-ons by reason (24 words)
	H2G_CNT_FAST_RANK = 120, H2G_CNT_FAST_SIDE = 121, H2G_CNT_FAST_STEPS = 122, H2G_CNT_FAST_ALIGNED = 123,   // the fast launch's rank / side / step / aligned counters ...
	H2G_CNT_DRAIN_OFF = 120,                                                   // ... and the drain launch's, at FastArgs::cnt_off = this behind them: [240, 244)
	H2G_CNT_OVF_CURSOR = 124, H2G_CNT_LEDITS_CURSOR = 126,                     // cursors of the pair-overflow / long-edit areas (uint32_t)
	H2G_CNT_PROF_FAST = 128, H2G_CNT_PROF_FAST_SITE = 176, H2G_CNT_PROF_FAST_TRIPS = 208,   // H2G_GO_PROF: the fast pass's time split (48), ticks (32) and trips (32) by site
	H2G_CNT_SECOND = 256,                                                      // the second pass's own RANK .. OVERFLOW (+ its H2G_GO_PROF words): [256, 512)
	H2G_CNT_PROF_FAST_BINS = 512,                                              // H2G_GO_PROF: the fast pass's time-resolved bins (h2g_fast_prof.h), [512, 768)
#ifdef H2G_GO_PROF
	H2G_CNT_BLOCK = 1024
#else
	H2G_CNT_BLOCK = 512
#endif
};

__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned long long v) {
	for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	if((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// The scheduler's state of one workgroup, in LDS: NQ rings of 16-bit slot ids over SLOTS slots, ring 0 the free slots.  A slot id is in one ring or in one lane.
// Waves reserve positions with one aggregated add on `tail`, take them with a CAS on `head`, and wait on the sentinel for a reserved position to be written.
// Nothing crosses the workgroup: relaxed LDS atomics here, the workgroup-scope fences around the slots' data are the callers'.
template <int NQ, int SLOTS>
struct SlotRings {
	static_assert(NQ <= 64, "the census is one lane per ring");
	static_assert(SLOTS > 0 && (SLOTS & (SLOTS - 1)) == 0, "positions wrap with a mask");
	static_assert(SLOTS <= 0xffff, "a slot id is 16 bits, 0xffff the sentinel");
	static constexpr uint16_t EMPTY = 0xffffu;   // a position that holds no slot id (yet)
	uint32_t head[NQ], tail[NQ];
	uint16_t ring[NQ][SLOTS];

	// every thread of the workgroup: all rings empty, every slot free; ends behind a barrier
	__device__ __forceinline__ void init() {
		for(uint32_t k = threadIdx.x; k < (uint32_t)NQ * SLOTS; k += blockDim.x) (&ring[0][0])[k] = EMPTY;
		if(threadIdx.x < (uint32_t)NQ) { head[threadIdx.x] = 0; tail[threadIdx.x] = 0; }
		__syncthreads();
		for(uint32_t k = threadIdx.x; k < (uint32_t)SLOTS; k += blockDim.x) ring[0][k] = (uint16_t)k;
		if(threadIdx.x == 0) tail[0] = SLOTS;
		__syncthreads();
	}
	// the census: slots in ring `lane` (0 for the lanes behind the last ring)
	__device__ __forceinline__ uint32_t count(int lane) const {
		return lane < NQ ? __atomic_load_n(&tail[lane], __ATOMIC_RELAXED) - __atomic_load_n(&head[lane], __ATOMIC_RELAXED) : 0u;
	}
	// pushes this lane's slot (if `valid`) into ring q; lanes of the wave may push to different rings
	__device__ __forceinline__ void push(bool valid, uint32_t q, uint32_t slot, int lane) {
		unsigned long long todo = __ballot(valid);
		while(todo) {                                                  // one aggregated reservation per ring present in the wave
			const int first = __ffsll((long long)todo) - 1;
			const uint32_t k = (uint32_t)__shfl((int)q, first);
			const unsigned long long m = __ballot(valid && q == k);
			uint32_t base = 0;
			if(lane == first) base = atomicAdd(&tail[k], (uint32_t)__popcll(m));
			base = (uint32_t)__shfl((int)base, first);
			if(valid && q == k) {
				const uint32_t pos = (base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) & (SLOTS - 1);
				__atomic_store_n(&ring[k][pos], (uint16_t)slot, __ATOMIC_RELAXED);
			}
			todo &= ~m;
		}
	}
	// pops one slot of ring q for each lane with `want` set, in lane order, as far as the ring holds any: `got` says whether THIS lane has one (then in `slot`).
	// Returns the count popped (wave-uniform).
	__device__ __forceinline__ uint32_t pop(uint32_t q, int lane, bool want, uint32_t* slot, bool* got) {
		const unsigned long long wm = __ballot(want);
		*got = false;
		if(wm == 0) return 0;
		return take(q, lane, want, (uint32_t)__popcll(wm), (uint32_t)__popcll(wm & ((1ull << lane) - 1ull)), slot, got);
	}
	// the same for the lanes [from, 64) of a full wave (`from` wave-uniform): what a ballot would count is known from the lane index
	__device__ __forceinline__ uint32_t pop_from(uint32_t q, int lane, uint32_t from, uint32_t* slot, bool* got) {
		return take(q, lane, (uint32_t)lane >= from, 64u - from, (uint32_t)lane - from, slot, got);
	}
	// the protocol behind both: lane 0 reserves up to `nwant` positions, the wanting lane of rank r < that count takes position r
	__device__ __forceinline__ uint32_t take(uint32_t q, int lane, bool want, uint32_t nwant, uint32_t r, uint32_t* slot, bool* got) {
		uint32_t n = 0, h = 0;
		if(lane == 0) {
			for(;;) {
				h = __atomic_load_n(&head[q], __ATOMIC_RELAXED);
				const uint32_t t = __atomic_load_n(&tail[q], __ATOMIC_RELAXED);
				n = t - h;
				if(n == 0) break;
				if(n > nwant) n = nwant;
				if(atomicCAS(&head[q], h, h + n) == h) break;
			}
		}
		n = (uint32_t)__shfl((int)n, 0); h = (uint32_t)__shfl((int)h, 0);
		*got = want && r < n;
		if(*got) {
			const uint32_t pos = (h + r) & (SLOTS - 1);
			uint16_t v;
			while((v = __atomic_load_n(&ring[q][pos], __ATOMIC_RELAXED)) == EMPTY) __builtin_amdgcn_s_sleep(1);   // reserved, being written
			__atomic_store_n(&ring[q][pos], EMPTY, __ATOMIC_RELAXED);
			*slot = v;
		}
		return n;
	}
};

// Launches kernel K with `lds` bytes of dynamic LDS.  More than 64 KB of it is an opt-in per kernel and per DEVICE (a process may drive several:
// hisat2-align-amd --gpus N), made once: the flag is a mask over device ids, one per kernel.
template <auto K, class... Args>
static int launch_large_lds(unsigned grid, unsigned threads, unsigned lds, hipStream_t st, const Args&... args) {
	static std::atomic<unsigned long long> lds_ok{0};
	int dev = 0; (void)hipGetDevice(&dev);
	const unsigned long long bit = 1ull << (dev & 63);
	if(!(lds_ok.load(std::memory_order_relaxed) & bit)) { if(hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) (void)hipGetLastError(); lds_ok.fetch_or(bit, std::memory_order_relaxed); }
	hipLaunchKernelGGL(K, dim3(grid), dim3(threads), lds, st, args...);
	return (int)hipGetLastError();
}

struct GoArgs {
	h2g::DGfm g; h2g::DRef ref; h2g::DLocalSet ls; h2g::DAlts alts; h2g::DSpliceDB ssdb;
	h2g::DReads rd1, rd2;                 // rd2 only when paired
	h2g::AlnParams P;
	const char* names1; const uint32_t* noffs1;
	const char* names2; const uint32_t* noffs2;
	uint8_t* pool; size_t ws_stride;      // per read in flight (slot): AlignWS, then GoSlot at slot_off, then GraphSlot at gsl_off
	size_t slot_off, gsl_off;
	uint8_t* gws_base; size_t gws_stride; // GraphWS per lane (graph indexes): scratch of one primitive
	uint8_t* sw_base; size_t sw_stride;   // Smith-Waterman scratch per lane (bowtie2_dp != 0)
	uint8_t* sc_base;                     // combineWith temp_scores per lane: 2 x H2G_COMBINE_MAXLEN int64
	h2g::MachOut O;
	unsigned long long* counters;
	uint32_t* work;                       // next unclaimed position of the read list (device counter, zeroed before the launch)
	const uint32_t* list;                 // nullptr = every read of the batch; else the read ids to process ...
	const uint32_t* nlist;                // ... and how many (device memory: the second pass is launched without a host sync)
	uint32_t paired;
	uint32_t dbg_read; uint32_t* dbg_buf; // development hook: trace of one read id (H2G_GO_DBG_READ): [0] = words used, then 8 words per primitive request
	uint32_t rdid_base;                   // Read::rdid of read 0 of the batch (splice-site visibility window)
	uint32_t defer_overflow;              // 1: a second pass follows; overflowed reads are not counted as aligned here
};
#define H2G_PK_LANE_WORDS_HOST (H2G_PK_WORDS + H2G_PK_WORDS / 2)

// What h2g_kernels.hip knows of one machine unit (a translation unit of h2g_go_kernels.h with its own AL_MAX_* capacities): the layout of a slot,
// the launch geometry, the capacities, and the two things that are code
struct GoUnitDesc {
	size_t ws_bytes, slot_off, gsl_off;   // per read in flight (slot): AlignWS, then GoSlot at slot_off, then GraphSlot at gsl_off (graph units)
	size_t gws_bytes;                     // GraphWS per lane; 0 in the linear units
	int waves;                            // waves per SIMD the kernel is bounded to
	uint32_t threads, slots;              // threads per workgroup, reads in flight per workgroup
	uint32_t lds_ring_bytes, lds_pack_bytes;   // LDS per workgroup: the rings + one packed-read region per mate
	uint32_t caps[5];                     // AL_MAX_GHITS, _RESULTS, _SEARCHED, _DEPTH, _PARTIAL
	size_t (*sw_bytes)(uint32_t maxlen, int wide);   // Smith-Waterman scratch per lane (SwLaneState holds H2G_GHIT_EDITS of THIS unit)
	int (*launch)(const GoArgs*, const h2g::DExonTbl*, const h2g::XlPairs*, unsigned grid, hipStream_t);
};
#define H2G_GO_DECLARE(NAME) extern "C" const GoUnitDesc* h2g_go_unit_##NAME();
H2G_GO_DECLARE(linear) H2G_GO_DECLARE(graph) H2G_GO_DECLARE(linear_big) H2G_GO_DECLARE(graph_big)
H2G_GO_DECLARE(linear_spl) H2G_GO_DECLARE(linear_spl_big) H2G_GO_DECLARE(graph_spl) H2G_GO_DECLARE(graph_spl_big)   // spliced alignment (linear indexes): with the splice-site database joins
H2G_GO_DECLARE(linear_xl) H2G_GO_DECLARE(graph_xl) H2G_GO_DECLARE(linear_spl_xl) H2G_GO_DECLARE(graph_spl_xl)       // -k / --max-seeds beyond the large workspace (h2g_go_xl.h)

// ---- the fast pass (h2g_fast.h / h2g_k_go_fast.hip): one read / pair per lane, state on chip; what it cannot hold goes to `bail_list`
struct FastArgs {
	h2g::DGfm g; h2g::DRef ref; h2g::DLocalSet ls;
	h2g::DReads rd1, rd2;
	h2g::AlnParams P;
	const char* names1; const uint32_t* noffs1;
	const char* names2; const uint32_t* noffs2;
	uint32_t* slots;                      // FG_SLOT_WORDS words per read in flight: packed state, hot words, packed reads, cold words
	h2g::FastOut O;
	unsigned long long* counters;         // a counter block: H2G_CNT_FAST_* (+ cnt_off), completed, bailed, bails by reason
	uint32_t* work;                       // next unclaimed read (zeroed before the launch)
	uint32_t* bail_list; uint32_t* bail_count;
	uint32_t total, paired;
	// graph indexes only (h2g_k_go_fast_graph.hip): the ALT database and the per-LANE scratch of one primitive
	h2g::DAlts alts;
	uint8_t* gws_base; size_t gws_stride;     // GraphWS per lane (group walk, ALT-aware extension)
	uint8_t* sc_base;                         // combineWith temp_scores per lane: 2 x H2G_COMBINE_MAXLEN int64, lane-interleaved per wave
	uint32_t tail;                            // > 0: a workgroup hands its last `tail` reads in flight on to the general machine once the batch is exhausted
	uint32_t dbg_read; uint32_t* dbg_buf;     // development hook (-DFG_DBG_TRACE builds, h2g_stream_tune "dbg_read"): the trips of one read id, 10 words each behind a word count
	// the end of a batch (h2g_k_go_fast.hip, fk_loop): a launch with orphan_T > 0 lists the slots (workgroup x slots per workgroup + slot) of the reads its workgroups still held
	// when they could fetch no more and had thinned out to orphan_T reads; the drain launch (..._launch_drain) resumes the reads of `adopt_list` out of `adopt_slots`
	uint32_t orphan_T; uint32_t* orphan_list; uint32_t* orphan_count;
	const uint32_t* adopt_list; const uint32_t* adopt_count; const uint32_t* adopt_slots;
	uint32_t cnt_off;                         // this launch's rank / side / step / aligned counters are counters[H2G_CNT_FAST_RANK + cnt_off ..]
	uint32_t adopt_slot_words;                // words per slot of `adopt_slots` (the launch that left them may be another build of the pass: same layout, a shorter cold tail)
	uint32_t mate_handover;                   // 1 (with orphan_T > 0, a build without alignMate): pairs that need alignMate are parked in their slots and listed for the drain launch — the alignMate build's
	// spliced runs only (h2g_k_go_fast_spl.hip; at the end: the other builds' fields keep their offsets): the splice-site database and Read::rdid of read 0 of the batch (rd1.ids: per-read ids)
	h2g::DSpliceDB ssdb;
	uint32_t rdid_base;
	// the linear non-spliced builds only: the first partial searches of the batch (h2g_k_ps0.hip writes them in front of the fast launch; FCtx::ps0), FG_PS0_WORDS words per
	// (read, mate, strand); nullptr: no pre-pass ran
	uint32_t* ps0;
};
// the pre-pass: `a` is the fast launch's argument block in device memory, `units` its reads / pairs
extern "C" int h2g_ps0_launch(const FastArgs* a, uint32_t units, bool paired, hipStream_t st);
// What h2g_kernels.hip knows of one build of the pass (h2g_k_go_fast.hip and the units that compile it again); `a` of both launchers is the argument block in DEVICE memory
struct FastUnitDesc {
	int (*launch)(const FastArgs* a, unsigned grid, hipStream_t);
	int (*launch_drain)(const FastArgs* a, unsigned grid, hipStream_t);
	uint32_t threads, lds_bytes;          // per workgroup
	uint32_t slots, slot_bytes;           // reads in flight per workgroup, bytes of one
	uint32_t gws_bytes;                   // GraphWS per lane in global memory; 0 where the build keeps it private (and in the linear builds)
};
extern "C" const FastUnitDesc* h2g_go_fast_unit();
extern "C" const FastUnitDesc* h2g_go_fast_am_unit();      // h2g_k_go_fast_am.hip: alignMate in the pass (FG_ALIGN_MATE = 1)
extern "C" const FastUnitDesc* h2g_go_fast_graph_unit();
extern "C" const FastUnitDesc* h2g_go_fast_spl_unit();     // h2g_k_go_fast_spl.hip: the pass under the spliced rules (FG_SPLICED = 1)
