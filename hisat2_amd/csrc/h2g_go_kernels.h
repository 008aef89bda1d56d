// h2g_go_kernels.h — the go() kernel (HI_Aligner::go per read / per pair) around the micro-op machine of h2g_machine.h.
//
// Reads in flight are SLOTS, not lanes.  A workgroup (H2G_GO_THREADS threads) owns H2G_GO_SLOTS slots of per-read state in HBM
// (AlignWS + the machine's registers + the packed read) and keeps, in LDS, one ring of slot ids per primitive of the machine
// plus a ring of free slots.  Each wavefront loops: pick the primitive with the longest ring, pop up to 64 slots that all
// wait for THAT primitive, run it for all of them at one code site (64 of 64 lanes busy on the same latency-bound loop),
// let each lane run its read's control flow up to the next primitive request (mach_step), and push the slots into the
// rings of what they asked for.  Free slots are refilled from the batch through one global counter.  No lane ever waits
// for an unrelated lane's primitive; nothing crosses a workgroup, so LDS atomics and workgroup-scope fences are all the
// synchronisation there is.
//
// Compiled once per translation unit with that unit's capacities (-DAL_MAX_*): h2g_k_go_linear.hip, h2g_k_go_graph.hip and
// their *_big.hip siblings (large workspaces: the second pass over reads whose lists overflowed, and option sets beyond the
// default capacities) and *_xl.hip siblings (h2g_go_xl.h: -k / --max-seeds beyond the large workspace).  h2g_kernels.hip sees only GoArgs and the GoUnitDesc of H2G_GO_UNIT.
#pragma once
#include <hip/hip_runtime.h>
#include "h2g_core.h"
#include "h2g_align.h"
#include "h2g_go_args.h"

using namespace h2g;

#ifndef H2G_GO_THREADS
#define H2G_GO_THREADS 512
#endif
#ifndef H2G_GO_SLOTS
#define H2G_GO_SLOTS 1024        // reads in flight per workgroup (power of two)
#endif
#define H2G_GO_NQ ((int)SITE_COUNT)   // one ring per request site of the machine (h2g_machine.h H2G_MACH_SITES); ring 0 holds the free slots
#define H2G_PK_LANE_WORDS (H2G_PK_WORDS + H2G_PK_WORDS / 2)

// per-read state of a slot beside its AlignWS: the machine registers between two primitives, and the packed read(s)
struct GoSlot {
	Lane     L;
	uint32_t read;
	uint32_t ro[2], rl[2];           // offset / length of the read in each read set
	uint32_t pk_ok[2];
	uint32_t pk[2][H2G_PK_LANE_WORDS];
};

// packs read i of `rd`: H2G_PK_WORDS 2-bit words then H2G_PK_WORDS/2 N-mask words; false = longer than the packed form holds.
// The codes are fetched four at a time (one unaligned dword per four bases; the buffer is padded past its last read).
__device__ __forceinline__ bool pack_read(const DReads& rd, uint32_t i, uint32_t* pk) {
	const uint32_t ro = rd.offs[i], rl = rd.offs[i + 1] - ro;
	for(uint32_t w = 0; w < H2G_PK_LANE_WORDS; w++) pk[w] = 0;
	if(rl > H2G_PK_MAXLEN) return false;
	const uint8_t* src = rd.codes + ro;
	for(uint32_t w = 0; w < (rl + 15) / 16; w++) {
		uint32_t bits = 0, mask = 0;
#pragma unroll
		for(uint32_t q = 0; q < 4; q++) {
			const uint32_t at = w * 16 + q * 4;
			if(at >= rl) break;
			uint32_t four;
			__builtin_memcpy(&four, src + at, 4);
			const uint32_t left = rl - at;
			if(left < 4) four &= (1u << (8 * left)) - 1u;             // bases of the next read: not ours
			// each byte is a code 0..4: two low bits to the 2-bit word, bit 2 (N) to the mask
			const uint32_t lo = four & 0x03030303u, n = (four >> 2) & 0x01010101u;
			const uint32_t b = (lo | (lo >> 6) | (lo >> 12) | (lo >> 18)) & 0xffu;
			const uint32_t m = (n | (n >> 7) | (n >> 14) | (n >> 21)) & 0xfu;
			bits |= b << (8 * q); mask |= m << (4 * q);
		}
		pk[w] = bits;
		pk[H2G_PK_WORDS + (w >> 1)] |= (w & 1) ? (mask << 16) : mask;
	}
	return true;
}

typedef SlotRings<H2G_GO_NQ, H2G_GO_SLOTS> GoLds;

// the rings (request sites) that wait for primitive `op`, as a bit set over ring ids
__device__ __forceinline__ unsigned long long mach_rings_of_op(uint32_t op) {
	unsigned long long m = 0;
#define X(OPC, PC) if(op == OPC) m |= 1ull << SITE_##PC;
	H2G_MACH_SITES(X)
#undef X
	return m;
}
#ifndef H2G_GO_TOPUP
#define H2G_GO_TOPUP 40      // a trip that popped fewer slots than this from the longest ring is topped up from the other rings of the same primitive
#endif

// The index's exons (--avoid-pseudogene) are a kernel argument of their own behind GoArgs, in the units that read them (H2G_EXT_OPTS): the
// other units keep their argument block, and with it their code
#if H2G_EXT_OPTS
#define H2G_GO_EXONS_PARAM , DExonTbl X
#define H2G_GO_EXONS_ARG(x_) , *(x_)
#else
#define H2G_GO_EXONS_PARAM
#define H2G_GO_EXONS_ARG(x_)
#endif
// ... and so is the side area of the XL units' concordant lists (H2G_XL)
#if H2G_XL
#define H2G_GO_XL_PARAM , XlPairs XP
#define H2G_GO_XL_ARG(p_) , *(p_)
#else
#define H2G_GO_XL_PARAM
#define H2G_GO_XL_ARG(p_)
#endif
// UNIT tells the builds of different translation units (capacities) apart: same template arguments would be ONE symbol
template <bool GRAPH, int WAVES_PER_SIMD, int UNIT>
__global__ __launch_bounds__(H2G_GO_THREADS, WAVES_PER_SIMD) void k_go(GoArgs A H2G_GO_EXONS_PARAM H2G_GO_XL_PARAM)
{
	extern __shared__ uint32_t s_mem[];
	GoLds* Q = reinterpret_cast<GoLds*>(s_mem);
	uint32_t* s_pk = s_mem + (sizeof(GoLds) + 3) / 4;      // [mates][H2G_PK_LANE_WORDS][H2G_GO_THREADS], lane-interleaved
	const int lane = (int)(threadIdx.x & 63);
	const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	const bool paired = A.paired != 0;
	Q->init();                                                // every slot starts free
	AlnCtx C; C.g = &A.g; C.ref = &A.ref; C.ls = &A.ls; C.P = &A.P;
	C.sw = A.sw_base ? A.sw_base + tid * A.sw_stride : nullptr;
	// combineWith temp_scores: one block per wave, lane-interleaved
	C.sc = (int64_t*)(A.sc_base + (tid >> 6) * (size_t)(64 * 2 * H2G_COMBINE_MAXLEN * sizeof(int64_t))) + lane; C.sc_stride = 64;
	C.ssdb = &A.ssdb; C.rdid_base = A.rdid_base;
#if H2G_EXT_OPTS
	ctx_ext_opts(C, A.P);
	C.exons = &X;
#endif
#if H2G_XL
	C.xlp = &XP;
#endif
	C.alts = &A.alts; C.gws = A.gws_base ? (GraphWS*)(A.gws_base + tid * A.gws_stride) : nullptr; C.graph = GRAPH;
	const size_t slot0 = (size_t)blockIdx.x * H2G_GO_SLOTS;
	Mach M;
	M.rd[0] = A.rd1; M.rd[1] = paired ? A.rd2 : A.rd1;
	uint32_t* const my_pk0 = s_pk + threadIdx.x;
	uint32_t* const my_pk1 = s_pk + H2G_PK_LANE_WORDS * H2G_GO_THREADS + threadIdx.x;
	M.rd[0].pk = my_pk0; M.rd[0].pk_stride = H2G_GO_THREADS;
	M.rd[1].pk = my_pk1; M.rd[1].pk_stride = H2G_GO_THREADS;
	M.name[0] = M.name[1] = nullptr; M.namelen[0] = M.namelen[1] = 0; M.read = 0;
	M.ws = nullptr;
	M.out = &A.O; M.paired_input = paired;
	const uint32_t total = A.list ? *A.nlist : A.rd1.n;
	unsigned long long nrank = 0, nsteps = 0, naln = 0, novf = 0, nside = 0;
	bool more = true;                                         // reads left in the batch (wave-local view)
#ifdef H2G_GO_PROF
	// wave-level time split (shader clock ticks): [0] choose + pop + load [1] control + push [2] (unused) [3+op] each primitive;
	// [20+op] slots executed; [32+op] executions; [47] trips
	unsigned long long prof[48], prof_ctl[16];
	uint32_t trip_op = 0;
	for(int k = 0; k < 48; k++) prof[k] = 0;
	for(int k = 0; k < 16; k++) prof_ctl[k] = 0;
	unsigned long long tp0 = __builtin_readcyclecounter(), tp1;
#define PROF(SLOT) do { tp1 = __builtin_readcyclecounter(); prof[SLOT] += tp1 - tp0; tp0 = tp1; } while(0)
#else
#define PROF(SLOT) do {} while(0)
#endif
	for(;;) {
		// ---- choose: the primitive with the longest ring; free slots are refilled when reads remain and nothing is long
		const uint32_t cnt = Q->count(lane);
		const uint32_t nfree = (uint32_t)__shfl((int)cnt, 0);
		uint32_t bestc = (lane >= 1 && lane < H2G_GO_NQ) ? cnt : 0, bestq = (uint32_t)lane;
		for(int o = 32; o > 0; o >>= 1) {
			const uint32_t oc = (uint32_t)__shfl_xor((int)bestc, o), oq = (uint32_t)__shfl_xor((int)bestq, o);
			if(oc > bestc || (oc == bestc && oq < bestq)) { bestc = oc; bestq = oq; }
		}
		bestc = (uint32_t)__shfl((int)bestc, 0); bestq = (uint32_t)__shfl((int)bestq, 0);
		const bool fetch = more && nfree > 0 && (bestc < 64 || nfree >= H2G_GO_SLOTS / 4);
		bool have = false;          // this lane carries a slot in this trip
		bool popped;                // ... out of the latest pop.  Every pop below fills the wave from lane 0 upwards: after n slots the trip's lanes are [0, n)
		uint32_t slot = 0;
		GoSlot* gs = nullptr;
		if(fetch) {
			// ---- new reads into free slots
			const uint32_t n = Q->pop_from(0, lane, 0, &slot, &popped);
			if(n == 0) continue;
#ifdef H2G_GO_PROF
			trip_op = 0;
#endif
			uint32_t base = 0;
			if(lane == 0) base = atomicAdd(A.work, n);
			base = (uint32_t)__shfl((int)base, 0);
			if(base + n >= total) more = false;
			const bool got = popped && base + (uint32_t)lane < total;
			Q->push(popped && !got, 0, slot, lane);    // slots without a read go back
			if(got) {
				have = true;
				const uint32_t i = A.list ? A.list[base + (uint32_t)lane] : base + (uint32_t)lane;
				M.ws = (AlignWS*)(A.pool + (slot0 + slot) * A.ws_stride);
				gs = (GoSlot*)((uint8_t*)M.ws + A.slot_off);
				C.gsl = GRAPH ? (GraphSlot*)((uint8_t*)M.ws + A.gsl_off) : nullptr;
				gs->read = i;
				gs->pk_ok[0] = pack_read(A.rd1, i, gs->pk[0]) ? 1u : 0u;
				for(uint32_t w = 0; w < H2G_PK_LANE_WORDS; w++) my_pk0[w * H2G_GO_THREADS] = gs->pk[0][w];
				M.rd[0].pk_read = gs->pk_ok[0] ? i : 0xffffffffu;
				M.name[0] = A.names1 + A.noffs1[i]; M.namelen[0] = A.noffs1[i + 1] - A.noffs1[i];
				if(paired) {
					gs->pk_ok[1] = pack_read(A.rd2, i, gs->pk[1]) ? 1u : 0u;
					for(uint32_t w = 0; w < H2G_PK_LANE_WORDS; w++) my_pk1[w * H2G_GO_THREADS] = gs->pk[1][w];
					M.rd[1].pk_read = gs->pk_ok[1] ? i : 0xffffffffu;
					M.name[1] = A.names2 + A.noffs2[i]; M.namelen[1] = A.noffs2[i + 1] - A.noffs2[i];
				}
				mach_begin(*C.P, M, i, paired);
				gs->ro[0] = M.ro[0]; gs->ro[1] = M.ro[1]; gs->rl[0] = M.rl[0]; gs->rl[1] = M.rl[1];
			}
			PROF(0);
		} else {
			if(bestc == 0) {
				// nothing queued in this workgroup: done when the batch is exhausted and every slot is free again
				if(!more && nfree == H2G_GO_SLOTS) break;
				__builtin_amdgcn_s_sleep(8);
				if(more) { uint32_t w = 0; if(lane == 0) w = __atomic_load_n(A.work, __ATOMIC_RELAXED); if((uint32_t)__shfl((int)w, 0) >= total) more = false; }
				continue;
			}
			const uint32_t op = mach_site_op(bestq);      // the ring is a request site: one primitive, one resume pc
			uint32_t n = Q->pop_from(bestq, lane, 0, &slot, &popped);
			if(n == 0) continue;
			// A thin trip (the machine behind a fast pass works on the hard reads only: a few hundred slots over ~34 rings) is topped up from the
			// other request sites of the SAME primitive: the primitive still runs at one code site for every lane, the control flow behind it
			// resumes at a few pcs instead of one.  Measured on the repeat-structured leg: profiles/r05_NOTES.md.
			if(n < H2G_GO_TOPUP) {
				unsigned long long cand = __ballot(cnt > 0 && lane >= 1 && lane < H2G_GO_NQ) & mach_rings_of_op(op) & ~(1ull << bestq);
				while(cand && n < 64) {
					const uint32_t q2 = (uint32_t)__ffsll((long long)cand) - 1u;
					cand &= cand - 1ull;
					n += Q->pop_from(q2, lane, n, &slot, &popped);      // the lanes [n, 64) take what ring q2 holds
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
			have = (uint32_t)lane < n;
			if(have) {
				M.ws = (AlignWS*)(A.pool + (slot0 + slot) * A.ws_stride);
				gs = (GoSlot*)((uint8_t*)M.ws + A.slot_off);
				C.gsl = GRAPH ? (GraphSlot*)((uint8_t*)M.ws + A.gsl_off) : nullptr;
				M.L = gs->L;
				M.read = gs->read;
				M.ro[0] = gs->ro[0]; M.ro[1] = gs->ro[1]; M.rl[0] = gs->rl[0]; M.rl[1] = gs->rl[1];
				for(uint32_t w = 0; w < H2G_PK_LANE_WORDS; w++) my_pk0[w * H2G_GO_THREADS] = gs->pk[0][w];
				M.rd[0].pk_read = gs->pk_ok[0] ? M.read : 0xffffffffu;
				if(paired) {
					for(uint32_t w = 0; w < H2G_PK_LANE_WORDS; w++) my_pk1[w * H2G_GO_THREADS] = gs->pk[1][w];
					M.rd[1].pk_read = gs->pk_ok[1] ? M.read : 0xffffffffu;
				}
			}
#ifdef H2G_GO_PROF
			prof[20 + op] += n; prof[32 + op]++; prof[47]++; trip_op = op;
#endif
			PROF(0);
			if(have) mach_exec(C, M, op);          // ONE primitive, one code site, every lane that carries a slot
			PROF(3 + op);
		}
		// ---- control flow of each read up to its next primitive request; then hand the slots on
		uint32_t nextq = 0;
		if(have) {
			if(M.L.pc != PC_FINISHED) mach_step(C, M);
			if(M.L.pc == PC_FINISHED && M.L.op == OP_NONE) {       // OP_FINISH ran: account, the slot is free
				nrank += M.ws->nrank; nsteps += M.ws->nsteps; nside += M.ws->nside;
				naln += (M.L.a0 != 0) && !(A.defer_overflow && M.L.a1 != 0); novf += M.L.a1 != 0;
				nextq = 0;
			} else {
				nextq = mach_site_of(M.L.pc);
				gs->L = M.L;
				if(A.dbg_buf && M.read == A.dbg_read) {
					const uint32_t at = atomicAdd(A.dbg_buf, 8u);
					if(at + 9 < (1u << 20)) { uint32_t* d = A.dbg_buf + 1 + at; d[0] = M.L.pc; d[1] = M.L.op; d[2] = M.L.a0; d[3] = M.L.a1; d[4] = M.L.a2; d[5] = M.L.a3; d[6] = M.L.a4; d[7] = M.L.a5; }
				}
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		Q->push(have, nextq, slot, lane);
#ifdef H2G_GO_PROF
		tp1 = __builtin_readcyclecounter(); prof[1] += tp1 - tp0; prof_ctl[trip_op] += tp1 - tp0; tp0 = tp1;
#endif
	}
#ifdef H2G_GO_PROF
	if(lane == 0) for(int k = 0; k < 48; k++) if(prof[k]) atomicAdd(A.counters + H2G_CNT_PROF_GO + k, prof[k]);
	if(lane == 0) for(int k = 0; k < 16; k++) if(prof_ctl[k]) atomicAdd(A.counters + H2G_CNT_PROF_GO_CTL + k, prof_ctl[k]);
#endif
	wave_add(A.counters + H2G_CNT_RANK, nrank);
	wave_add(A.counters + H2G_CNT_SIDE, nside);
	wave_add(A.counters + H2G_CNT_STEPS, nsteps);
	wave_add(A.counters + H2G_CNT_ALIGNED, naln);
	wave_add(A.counters + H2G_CNT_OVERFLOW, novf);
}

// what h2g_kernels.hip sees of one translation unit: its GoUnitDesc (h2g_go_args.h)
#define H2G_GO_ALIGN256(X) (((X) + 255) & ~(size_t)255)
#define H2G_GO_LDS_RINGS ((uint32_t)((sizeof(GoLds) + 3) / 4 * 4))
#define H2G_GO_LDS_PACK  (H2G_PK_LANE_WORDS * H2G_GO_THREADS * 4u)
template <bool GRAPH, int WAVES, int UNIT>
static int go_launch(const GoArgs* a, const DExonTbl* x, const XlPairs* xp, unsigned grid, hipStream_t st) {
	(void)x; (void)xp;
	return launch_large_lds<k_go<GRAPH, WAVES, UNIT>>(grid, H2G_GO_THREADS, H2G_GO_LDS_RINGS + (a->paired ? 2u : 1u) * H2G_GO_LDS_PACK, st, *a H2G_GO_EXONS_ARG(x) H2G_GO_XL_ARG(xp));
}
static size_t go_sw_bytes(uint32_t maxlen, int wide) { return sw_scratch_bytes(maxlen, wide != 0); }
template <bool GRAPH, int WAVES, int UNIT>
static const GoUnitDesc* go_unit_desc() {
	constexpr size_t ws = H2G_GO_ALIGN256(sizeof(AlignWS)), gs = H2G_GO_ALIGN256(sizeof(GoSlot));
	static const GoUnitDesc d = {ws + gs + (GRAPH ? H2G_GO_ALIGN256(sizeof(GraphSlot)) : 0), ws, ws + gs, GRAPH ? H2G_GO_ALIGN256(sizeof(GraphWS)) : 0,
		WAVES, H2G_GO_THREADS, H2G_GO_SLOTS, H2G_GO_LDS_RINGS, H2G_GO_LDS_PACK,
		{AL_MAX_GHITS, AL_MAX_RESULTS, AL_MAX_SEARCHED, AL_MAX_DEPTH, AL_MAX_PARTIAL}, go_sw_bytes, go_launch<GRAPH, WAVES, UNIT>};
	return &d;
}
#define H2G_GO_UNIT(NAME, GRAPH, WAVES, UNIT) extern "C" const GoUnitDesc* h2g_go_unit_##NAME() { return go_unit_desc<GRAPH, WAVES, UNIT>(); }
