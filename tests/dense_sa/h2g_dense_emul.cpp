// h2g_dense_emul.cpp — TEST-ONLY: the host instantiation of tests/emul with the dense SA table (h2g_core.h sa_dense_build_rows / sa_resolve_row).
// Compiled by tests/test_dense_sa_cpu.py, once as it is and once with -DH2G_SA_DIST_SAT=8 (most rows then miss the table and take the fallback).
#include "../emul/h2g_emul.cpp"
#include <map>

struct DenseTab { std::vector<uint32_t> v; std::vector<uint8_t> d; };
static std::map<Emu*, DenseTab> g_tabs;

extern "C" {

uint32_t h2gemu_dense_sat() { return H2G_SA_DIST_SAT; }

// builds the table of e's global index the way a wave of the device build does (64 interleaved row sets per chunk of 4096 rows) and keeps it, detached
void h2gemu_dense_build(Emu* e) {
	DenseTab& t = g_tabs[e];
	const uint64_t n = e->dg.gbwtLen;
	t.v.assign(n, 0xdeadbeefu); t.d.assign(n, 0xee);
	for(uint64_t base = 0; base < n; base += 4096) {
		const uint64_t lim = base + 4096 < n ? base + 4096 : n;
		for(uint32_t lane = 0; lane < 64; lane++) sa_dense_build_rows(e->dg, base + lane, 64, lim, t.v.data(), t.d.data());
	}
}
void h2gemu_dense_attach(Emu* e, uint32_t on) {
	DenseTab& t = g_tabs[e];
	e->dg.sa_dense = on ? t.v.data() : nullptr; e->dg.sa_dist = on ? t.d.data() : nullptr;
}
// every row: the table against sa_walk, and sa_resolve_row (table attached) against sa_walk.  out[0] rows whose entry is wrong, [1] rows sa_resolve_row
// resolves differently (offset or steps), [2] rows not in the table (saturated), [3] the longest walk
void h2gemu_dense_check(Emu* e, uint64_t* out) {
	DenseTab& t = g_tabs[e];
	DGfm plain = e->dg, dense = e->dg;
	plain.sa_dense = nullptr; plain.sa_dist = nullptr;
	dense.sa_dense = t.v.data(); dense.sa_dist = t.d.data();
	out[0] = out[1] = out[2] = out[3] = 0;
	for(uint64_t row = 0; row < plain.gbwtLen; row++) {
		uint32_t steps = 0, s2 = 7;
		const uint32_t off = sa_walk(plain, (uint32_t)row, &steps);
		const uint32_t d = steps < H2G_SA_DIST_SAT ? steps : H2G_SA_DIST_SAT;
		if(t.d[row] != d || (d != H2G_SA_DIST_SAT && t.v[row] != off)) out[0]++;
		if(d == H2G_SA_DIST_SAT) out[2]++;
		if(steps > out[3]) out[3] = steps;
		const uint32_t o2 = sa_resolve_row(dense, (uint32_t)row, &s2);
		if(o2 != off || s2 != steps + 7) out[1]++;
	}
}


static uint64_t fnv(uint64_t h, const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for(size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } return h; }
// Every read / pair of the batch through the general machine and through the fast path (as h2gemu_fast_check runs them), each into zeroed rows:
// out[0] = hash of the machine's PairOut / ReadOut and record rows, [1] = the same of what the fast path completed, [2] = reads it completed,
// [3] = the machine's nsteps summed.  codes2 == nullptr: unpaired.
void h2gemu_dense_digest(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                         const uint32_t* noffs2, uint64_t* out) {
	AlnParams P; AlnCtx C;
	emu_ctx(e, 1, &P, &C);
	const bool paired = codes2 != nullptr;
	AlignWS* ws = new AlignWS();
	Mach M;
	M.ws = ws; M.rd[0] = e->reads(); M.rd[1] = M.rd[0];
	if(paired) { M.rd[1].codes = codes2; M.rd[1].offs = offs2; M.rd[1].quals = nullptr; }
	const uint32_t n = M.rd[0].n, slots = 16;
	std::vector<h2g_alnres> r1(slots), r2(slots);
	FCtx F;
	F.g = &e->dg; F.ref = &e->dr; F.ls = &e->dls; F.P = &P;
	F.rd[0] = M.rd[0]; F.rd[1] = M.rd[1];
	uint32_t pk[2][H2G_PK_WORDS];
	F.pk[0] = pk[0]; F.pk[1] = pk[1]; F.pk_stride = 1;
	static int64_t sc_[2 * H2G_COMBINE_MAXLEN];
	F.sc = sc_; F.sc_stride = 1;
	uint32_t words[FW_TOTAL];
	FWords W; W.hot = words; W.hot_stride = 1; W.cold = words + FW_HOT;
	uint64_t hm = 1469598103934665603ull, hf = hm;
	out[2] = out[3] = 0;
	for(uint32_t i = 0; i < n; i++) {
		M.name[0] = F.name[0] = names1 + noffs1[i]; M.namelen[0] = F.namelen[0] = noffs1[i + 1] - noffs1[i];
		M.name[1] = F.name[1] = paired ? names2 + noffs2[i] : nullptr; M.namelen[1] = F.namelen[1] = paired ? noffs2[i + 1] - noffs2[i] : 0;
		PairOut po; ReadOut ro;
		for(int pass = 0; pass < 2; pass++) {
			memset((void*)&po, 0, sizeof po); memset((void*)&ro, 0, sizeof ro);
			memset((void*)r1.data(), 0, slots * sizeof(h2g_alnres)); memset((void*)r2.data(), 0, slots * sizeof(h2g_alnres));
			MachOut O; O.rout = nullptr; O.aln = nullptr; O.aln_slots = 0; O.pout = nullptr; O.paln[0] = O.paln[1] = nullptr; O.pair_slots = 0;
			if(paired) { O.pout = &po - i; O.paln[0] = r1.data() - (size_t)i * slots; O.paln[1] = r2.data() - (size_t)i * slots; O.pair_slots = slots; }
			else { O.rout = &ro - i; O.aln = r1.data() - (size_t)i * slots; O.aln_slots = slots; }
			uint64_t* h = pass ? &hf : &hm;
			if(pass == 0) {
				mach_run_single(C, M, i, paired, O);
				out[3] += paired ? po.nsteps : ro.nsteps;
			} else {
				F.O.rout = O.rout; F.O.aln = O.aln; F.O.aln_slots = O.aln_slots; F.O.pout = O.pout; F.O.paln[0] = O.paln[0]; F.O.paln[1] = O.paln[1]; F.O.pair_slots = O.pair_slots;
				memset(words, 0xa5, sizeof words);
				bool ok = fg_pack_read(F.rd[0], i, pk[0], 1);
				if(paired) ok = fg_pack_read(F.rd[1], i, pk[1], 1) && ok;
				FState S;
				memset((void*)&S, 0xa5, sizeof S);
				if(!fast_run_single(F, S, W, i, paired, ok)) { const uint32_t why = S.bail; *h = fnv(*h, &why, sizeof why); continue; }
				out[2]++;
			}
			if(paired) *h = fnv(*h, &po, sizeof po); else *h = fnv(*h, &ro, sizeof ro);
			*h = fnv(*h, r1.data(), slots * sizeof(h2g_alnres));
			*h = fnv(*h, r2.data(), slots * sizeof(h2g_alnres));
		}
	}
	out[0] = hm; out[1] = hf;
	delete ws;
}

}
