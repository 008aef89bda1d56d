// The fast pass's first partial searches, in front of its loop.
//
// nextBWT picks a strand that has not been searched yet before any other (FPC_NB_PICK, h2g_fast.h), so every read the pass takes runs partial_search_item at offset 0 for
// each of its (mate, strand) combinations — and the result depends on the read, the index and pseudogeneStop / anchorStop / khits only.  In the loop such a search is a trip
// of a wave at 256 registers per lane, two waves per SIMD; here it is one lane of a slim kernel: the packed read in a few LDS words, the 64 B side in registers, nothing else
// alive, so that many more latency chains are in flight per CU.  One lane per (unit, mate, strand), the lanes of a unit adjacent; each writes one 16-byte record (fg_ps0_pack)
// that FPC_NB_PICK takes up instead of asking for the search.
#include "h2g_go_args.h"

using namespace h2g;

#define PS0_THREADS 256

// (bounded to 6 blocks per CU: 70 registers, 7 waves per SIMD, no scratch; unbounded it takes 85 and 5 waves, bounded to 8 it spills 20)
__global__ __launch_bounds__(PS0_THREADS, 6) void k_ps0(const FastArgs* __restrict__ A, uint32_t units)
{
	__shared__ uint32_t s_pk[H2G_PK_WORDS * PS0_THREADS];      // word w of the read of lanes 2k, 2k + 1 (its two strands) at s_pk[w * PS0_THREADS + 2k]
	const bool paired = A->paired != 0;
	const uint32_t sh = paired ? 2u : 1u;                      // lanes per unit: 4 (a pair) or 2 (a single read)
	const uint32_t t = blockIdx.x * PS0_THREADS + threadIdx.x;
	const uint32_t unit = t >> sh, x = t & ((1u << sh) - 1u), mate = x >> 1;
	const uint32_t lane = threadIdx.x & 63u;
	const bool live = unit < units;
	const DReads& rd = mate ? A->rd2 : A->rd1;
	uint32_t* const pk = s_pk + (threadIdx.x & ~1u);
	bool ok = true;
	uint32_t rl = 0;
	if(live) {
		rl = rd.offs[unit + 1] - rd.offs[unit];
		if((x & 1u) == 0) {                                    // the forward lane packs the read for both
			ok = fg_pack_read(rd, unit, pk, PS0_THREADS);
			if(rd.qc && !rd.qc[unit]) ok = false;
		}
	}
	__syncthreads();
	// what fast_begin refuses — a mate too long for the packed form, with an N, or filtered — it refuses for the whole unit
	const unsigned long long bad = __ballot(!ok);
	const bool absent = ((bad >> (lane & ~((1u << sh) - 1u))) & ((1ull << (1u << sh)) - 1ull)) != 0;
	if(!live) return;
	uint32_t rec[FG_PS0_WORDS] = {FG_PS0_ABSENT, FG_PS0_ABSENT, FG_PS0_ABSENT, FG_PS0_ABSENT};
	if(!absent) {
		SeqView sv;
		sv.fwc = nullptr; sv.q = nullptr; sv.len = rl; sv.fw = (x & 1u) == 0;
		sv.pk = pk; sv.pk_stride = PS0_THREADS; sv.pk_nomask = true;
		h2g_fm_hit fh;
		partial_search_item(A->g, sv, 0, A->P.pseudogeneStop != 0, A->P.anchorStop != 0, A->P.khits, &fh);
		fg_ps0_pack(fh, rec);
	}
	*reinterpret_cast<uint4*>(A->ps0 + ((size_t)unit * 4 + x) * FG_PS0_WORDS) = make_uint4(rec[0], rec[1], rec[2], rec[3]);
}

extern "C" int h2g_ps0_launch(const FastArgs* a, uint32_t units, bool paired, hipStream_t st) {
	if(units == 0) return 0;
	const unsigned long long lanes = (unsigned long long)units * (paired ? 4u : 2u);
	hipLaunchKernelGGL(k_ps0, dim3((unsigned)((lanes + PS0_THREADS - 1) / PS0_THREADS)), dim3(PS0_THREADS), 0, st, a, units);
	return (int)hipGetLastError();
}
