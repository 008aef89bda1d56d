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

// lanes_digest (tests/emul): out[0] machine hash, [1] fast hash, [2] reads completed, [3] the machine's nsteps; and [4] = reads whose table was switched on in
// the middle of a walk.
// midwalk != 0: every read starts its fast path WITHOUT the table; the first time fast_op_lcoords stores a walk under way ("again") the table is attached and
// the read goes on with it — the slot a drain launch adopts from a fast launch queued before the build's end.  The machine's pass then runs without the table.
void h2gemu_lsa_digest(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                       const uint32_t* noffs2, uint32_t midwalk, uint64_t* out) {
	const bool was_on = e->dls.lsa != nullptr;
	out[4] = 0;
	if(midwalk) h2gemu_lsa_attach(e, 0);
	lanes_digest(e, codes2, offs2, names1, noffs1, names2, noffs2, out, [&](FastLane& FL, uint32_t i, bool paired) {
		// fast_run_single (h2g_fast.h), with the switch
		const FCtx& F = FL.F; FState& S = FL.S; const FWords& W = FL.W;
		bool switched = false;
		fast_begin(F, S, i, paired, FL.begin(i, paired));
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
		if(midwalk) h2gemu_lsa_attach(e, 0);                 // (the next read's machine pass and its first trips run without the table)
		return S.pc == FPC_DONE;
	});
	if(midwalk) h2gemu_lsa_attach(e, was_on ? 1 : 0);
}

}
