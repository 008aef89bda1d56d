// h2g_lsa_emul.cpp — TEST-ONLY: the host instantiation of tests/emul with the dense table of local rows (h2g_align.h lsa_build_rows / lsa_resolve_row,
// h2g_fast.h fast_op_lcoords_walk).  Compiled by tests/test_dense_lsa_cpu.py, once as it is and once with -DH2G_LSA_DIST_SAT=4 (one local row in eight is
// sampled, so most rows then miss the table and take the fallback).
#include "../emul/h2g_emul.cpp"
#include <map>

struct LsaTab { std::vector<uint32_t> v; std::vector<uint64_t> base; };
static std::map<Emu*, LsaTab> g_ltabs;

extern "C" {

uint32_t h2gemu_lsa_sat() { return H2G_LSA_DIST_SAT; }

// builds the table of e's local indexes the way a workgroup of the device build does (a quarter of an index's rows per wave, 64 interleaved row sets per
// quarter) and keeps it, detached
void h2gemu_lsa_build(Emu* e) {
	LsaTab& t = g_ltabs[e];
	const DLocalSet& ls = e->dls;
	t.base.assign(ls.n + 1, 0);
	for(uint32_t i = 0; i < ls.n; i++) t.base[i + 1] = t.base[i] + (uint64_t)ls.desc[i].len + 1;
	t.v.assign(t.base[ls.n], 0xdeadbeefu);
	for(uint32_t i = 0; i < ls.n; i++) {
		const DLocalDesc* d = &ls.desc[i];
		uint32_t* tab = t.v.data() + t.base[i];
		if(d->len == 0) { tab[0] = H2G_LSA_MISS; continue; }
		const uint32_t rows = d->len + 1, per = (rows + 3) / 4;
		LIdxR lx; lx.init(&ls, d);
		for(uint32_t w = 0; w < 4; w++) {
			const uint32_t lo = w * per, hi = lo + per < rows ? lo + per : rows;
			for(uint32_t lane = 0; lane < 64; lane++) lsa_build_rows(lx, (0xffffu << ls.offRate) & 0xffffu, ls.offRate, ls.words + d->offs_off, lo + lane, 64u, hi, tab);
		}
	}
}
void h2gemu_lsa_attach(Emu* e, uint32_t on) {
	LsaTab& t = g_ltabs[e];
	e->dls.lsa = on ? t.v.data() : nullptr; e->dls.lsa_base = on ? t.base.data() : nullptr;
}
// every row of every local index, the '$' row included: the entry against sa_walk_idx over the machine's own view of the index (LIdx), and lsa_resolve_row
// (table attached) against that walk.  out[0] entries that are wrong, [1] rows lsa_resolve_row resolves differently (offset or steps), [2] rows not in the
// table (saturated), [3] the longest walk, [4] rows, [5] '$' rows checked, [6] local indexes with more than one fragment, [7] non-empty local indexes
// shorter than the interval, [8] empty local indexes, [9] local indexes
void h2gemu_lsa_check(Emu* e, uint64_t* out) {
	LsaTab& t = g_ltabs[e];
	DLocalSet plain = e->dls, dense = e->dls;
	plain.lsa = nullptr; plain.lsa_base = nullptr;
	dense.lsa = t.v.data(); dense.lsa_base = t.base.data();
	for(int k = 0; k < 10; k++) out[k] = 0;
	out[9] = plain.n;
	const uint32_t offMask = (0xffffu << plain.offRate) & 0xffffu;
	for(uint32_t i = 0; i < plain.n; i++) {
		const DLocalDesc* d = &plain.desc[i];
		if(d->len == 0) { out[8]++; if(t.v[t.base[i]] != H2G_LSA_MISS) out[0]++; continue; }
		if(d->nFrag > 1) out[6]++;
		if(d->len < H2G_LOCAL_INTERVAL) out[7]++;
		LIdx lp; lp.ls = &plain; lp.d = d;
		LIdx ld; ld.ls = &dense; ld.d = &dense.desc[i];
		for(uint32_t row = 0; row <= d->len; row++) {
			uint32_t steps = 0, s2 = 7;
			const uint32_t off = sa_walk_idx(lp, row, offMask, plain.offRate, plain.words + d->offs_off, true, &steps);
			const bool sat = steps >= H2G_LSA_DIST_SAT || off > 0xffffu;
			const uint32_t want = sat ? H2G_LSA_MISS : off | (steps << 16);
			if(t.v[t.base[i] + row] != want) out[0]++;
			if(sat) out[2]++;
			if(steps > out[3]) out[3] = steps;
			out[4]++;
			if(lp.is_zoff(row)) out[5]++;
			const uint32_t o2 = lsa_resolve_row(ld, dense, i, row, &s2);
			if(o2 != off || s2 != steps + 7) out[1]++;
		}
	}
}

static uint64_t fnv(uint64_t h, const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for(size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } return h; }
// Every read / pair of the batch through the general machine and through the fast path, one lane at a time, each into zeroed rows:
// out[0] = hash of the machine's PairOut / ReadOut and record rows, [1] = the same of what the fast path completed (and the bail code of what it did not),
// [2] = reads it completed, [3] = the machine's nsteps summed, [4] = reads whose table was switched on in the middle of a walk.  codes2 == nullptr: unpaired.
// midwalk != 0: every read starts its fast path WITHOUT the table; the first time fast_op_lcoords stores a walk under way ("again") the table is attached and
// the read goes on with it — the slot a drain launch adopts from a fast launch queued before the build's end.  The machine's pass then runs without the table.
void h2gemu_lsa_digest(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                       const uint32_t* noffs2, uint32_t midwalk, uint64_t* out) {
	AlnParams P; AlnCtx C;
	emu_ctx(e, 1, &P, &C);
	const bool paired = codes2 != nullptr;
	const bool was_on = e->dls.lsa != nullptr;
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
	out[2] = out[3] = out[4] = 0;
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
			if(midwalk) h2gemu_lsa_attach(e, 0);
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
				// fast_run_single (h2g_fast.h), with the switch
				bool switched = false;
				fast_begin(F, S, i, paired, ok);
				while(S.pc != FPC_DONE && S.pc != FPC_BAIL) {
					if(S.op == FOP_NONE) fast_step(F, S, W);
					if(S.op != FOP_NONE) {
						uint32_t pw[FS_WORDS];
						const uint32_t op = S.op;
						if(fg_site_of(S.pc) == 0 || fg_site_op(fg_site_of(S.pc)) != op) { S.pc = FPC_BAIL; S.bail = FB_OTHER; break; }
						fs_pack(S, [&](uint32_t k, uint32_t v) { pw[k] = v; });
						memset((void*)&S, 0x5a, sizeof S);
						fs_unpack(S, [&](uint32_t k) { return pw[k]; });
						fast_exec(F, S, W, op);
						if(midwalk && !switched && op == FOP_LCOORDS && S.op == FOP_LCOORDS) { h2gemu_lsa_attach(e, 1); switched = true; out[4]++; }
					}
				}
				if(S.pc != FPC_DONE) { const uint32_t why = S.bail; *h = fnv(*h, &why, sizeof why); continue; }
				out[2]++;
			}
			if(paired) *h = fnv(*h, &po, sizeof po); else *h = fnv(*h, &ro, sizeof ro);
			*h = fnv(*h, r1.data(), slots * sizeof(h2g_alnres));
			*h = fnv(*h, r2.data(), slots * sizeof(h2g_alnres));
		}
	}
	if(midwalk) h2gemu_lsa_attach(e, was_on ? 1 : 0);
	out[0] = hm; out[1] = hf;
	delete ws;
}

}
