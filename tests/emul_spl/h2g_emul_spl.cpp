// h2g_emul_spl.cpp — TEST-ONLY host instantiation of the fast pass under the SPLICED rules (h2g_fast.h with FG_SPLICED = 1: the configuration of
// hisat2_amd/csrc/h2g_k_go_fast_spl.hip) next to the spliced general machine: the emulator as it is, plus the loop of h2gemu_fast_check with spliced
// alignment on and the emulator's splice-site database handed to the pass.  Compiled by tests/test_spl_fast_cpu.py with -DFG_SPLICED=1 -DFG_ALIGN_MATE=0
// and the EDITS32 defines of tests/emul/Makefile.
#if !defined(FG_SPLICED) || !FG_SPLICED
#error "compile with -DFG_SPLICED=1"
#endif
#include "../emul/h2g_emul.cpp"

// Every read / pair of the batch through the fast pass (spliced rules) and — the ones it completes — through the spliced machine: PairOut / ReadOut
// and every record must be equal.  stats[0] completed, [1] mismatching, [2 + why] bails by reason; done_flags[i] = 1: completed.
// spl_flags[i] (may be null) = 1: the MACHINE's result of read / pair i holds a record with a splice edit — computed for EVERY read, completed or not.
extern "C" void h2gemu_fast_check_spl(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                                      const uint32_t* noffs2, uint64_t* stats, uint32_t* bad_ids, uint32_t cap, uint8_t* done_flags, uint8_t* spl_flags) {
	AlnParams P; AlnCtx C;
	emu_ctx(e, 0, &P, &C);
	const bool paired = codes2 != nullptr;
	AlignWS* ws = new AlignWS();
	Mach M;
	M.ws = ws; M.rd[0] = e->reads(); M.rd[1] = M.rd[0];
	if(paired) { M.rd[1].codes = codes2; M.rd[1].offs = offs2; M.rd[1].quals = e->quals2.empty() ? nullptr : e->quals2.data(); }
	const uint32_t n = M.rd[0].n, slots = 16;
	std::vector<PairOut> fp(n);
	std::vector<ReadOut> fr(n);
	std::vector<h2g_alnres> f1((size_t)n * slots), f2((size_t)n * slots), m1(slots), m2(slots);
	FCtx F;
	F.g = &e->dg; F.ref = &e->dr; F.ls = &e->dls; F.P = &P;
	F.rd[0] = M.rd[0]; F.rd[1] = M.rd[1];
	F.ssdb = &e->dssdb; F.rdid_base = e->rdid_base;
	uint32_t pk[2][H2G_PK_WORDS];
	F.pk[0] = pk[0]; F.pk[1] = pk[1]; F.pk_stride = 1;
	static int64_t sc_[2 * H2G_COMBINE_MAXLEN];
	F.sc = sc_; F.sc_stride = 1;
	for(int k = 0; k < 2 + (int)FB_COUNT; k++) stats[k] = 0;
	if(!e->dg.linear) { stats[1] = ~0ull; delete ws; return; }      // the spliced build of the pass is for linear indexes
	F.O.rout = fr.data(); F.O.aln = f1.data(); F.O.aln_slots = slots; F.O.pout = fp.data(); F.O.paln[0] = f1.data(); F.O.paln[1] = f2.data(); F.O.pair_slots = slots;
	uint32_t words[FW_TOTAL];
	FWords W; W.hot = words; W.hot_stride = 1; W.cold = words + FW_HOT;
	uint32_t nbad = 0;
	auto has_splice = [](const AlnRec& r) { for(uint32_t k = 0; k < r.nedits && k < H2G_GHIT_EDITS; k++) if(r.edits[k].type == H2G_EDIT_SPL) return true; return false; };
	for(uint32_t i = 0; i < n; i++) {
		F.name[0] = names1 + noffs1[i]; F.namelen[0] = noffs1[i + 1] - noffs1[i];
		F.name[1] = paired ? names2 + noffs2[i] : nullptr; F.namelen[1] = paired ? noffs2[i + 1] - noffs2[i] : 0;
		memset(words, 0xa5, sizeof words);
		bool ok = fg_pack_read(F.rd[0], i, pk[0], 1);
		if(paired) ok = fg_pack_read(F.rd[1], i, pk[1], 1) && ok;
		FState S;
		memset(&S, 0xa5, sizeof S);
		const bool done = fast_run_single(F, S, W, i, paired, ok);
		if(done_flags) done_flags[i] = done ? 1 : 0;
		if(!done) stats[2 + (S.bail < FB_COUNT ? S.bail : FB_OTHER)]++; else stats[0]++;
		// the spliced machine on the same read
		M.name[0] = F.name[0]; M.namelen[0] = F.namelen[0]; M.name[1] = F.name[1]; M.namelen[1] = F.namelen[1];
		MachOut O; O.rout = nullptr; O.aln = nullptr; O.aln_slots = 0; O.pout = nullptr; O.paln[0] = O.paln[1] = nullptr; O.pair_slots = 0;
		bool same = true, spl = false;
		if(paired) {
			PairOut one; O.pout = &one - i; O.paln[0] = m1.data() - (size_t)i * slots; O.paln[1] = m2.data() - (size_t)i * slots; O.pair_slots = slots;   // (the machine writes pout[i])
			mach_run_single(C, M, i, true, O);
			for(int m = 0; m < 2; m++) for(uint32_t k = 0; k < ws->m[m].nres; k++) spl = spl || has_splice(ws->m[m].res[k]);
			if(done) {
				const PairOut& f = fp[i];
				same = one.nres[0] == f.nres[0] && one.nres[1] == f.nres[1] && one.npairs == f.npairs && one.overflow == f.overflow && one.nrank == f.nrank &&
				       one.nsteps == f.nsteps && one.depth == f.depth && one.nside == f.nside && one.rnd_state == f.rnd_state &&
				       memcmp(one.pair_i, f.pair_i, sizeof one.pair_i) == 0 && memcmp(one.pair_j, f.pair_j, sizeof one.pair_j) == 0;
				for(uint32_t k = 0; same && k < f.nres[0]; k++) same = rec_equal(f1[(size_t)i * slots + k], ws->m[0].res[k]);
				for(uint32_t k = 0; same && k < f.nres[1]; k++) same = rec_equal(f2[(size_t)i * slots + k], ws->m[1].res[k]);
			}
		} else {
			ReadOut one; O.rout = &one - i; O.aln = m1.data() - (size_t)i * slots; O.aln_slots = slots;
			mach_run_single(C, M, i, false, O);
			for(uint32_t k = 0; k < ws->m[0].nres; k++) spl = spl || has_splice(ws->m[0].res[k]);
			if(done) {
				const ReadOut& f = fr[i];
				same = one.nres == f.nres && one.nselect == f.nselect && one.overflow == f.overflow && one.nrank == f.nrank && one.nsteps == f.nsteps &&
				       one.depth == f.depth && one.nside == f.nside && one.best == f.best && one.secbest == f.secbest && one.best_h2 == f.best_h2 &&
				       one.secbest_h2 == f.secbest_h2;
				for(uint32_t k = 0; same && k < f.nselect; k++) same = one.select[k] == f.select[k];
				for(uint32_t k = 0; same && k < f.nselect; k++) {
					const h2g_alnres &a = f1[(size_t)i * slots + k], &b = m1[k];
					same = a.fw == b.fw && a.tidx == b.tidx && a.toff == b.toff && a.len == b.len && a.trim5 == b.trim5 && a.trim3 == b.trim3 && a.nedits == b.nedits &&
					       a.splicescore == b.splicescore && a.score == b.score && memcmp(a.edits, b.edits, a.nedits * sizeof(h2g_edit)) == 0;
				}
			}
		}
		if(spl_flags) spl_flags[i] = spl ? 1 : 0;
		if(done && !same) { stats[1]++; if(nbad < cap) bad_ids[nbad++] = i; }
	}
	delete ws;
}
