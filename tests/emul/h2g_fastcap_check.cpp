// h2g_fastcap_check — TEST-ONLY stand-alone program (its own main; nothing is loaded into an interpreter): every read / pair of a text file through the general
// machine and through the fast pass (h2g_fast.h) on one host lane each, in the SHIPPED configuration of the pass (tests/emul/Makefile: h2g_fastcap_check over a
// linear index, h2g_fastcap_check_g with FG_GRAPH=1), and a read-out of how far the read filled the pass's compact state.  The pass is driven by a loop of this
// program's own over fast_begin / fast_step / fast_exec, with the round trip through the packed state that fast_run_single makes between two trips; after every
// step and every primitive the counters of the state are sampled.  tests/test_fast_caps_cpu.py reads the output; the `sanitize` target builds the same program
// with -fsanitize=address,undefined.
//
//   h2g_fastcap_check caps
//   h2g_fastcap_check run <index> <reads> [<mates2>] [params=<file>]
// A read file is one line of A/C/G/T/N per read; params=<file>: the raw bytes of an h2g_align_params block.  One line per read / pair:
//   done bail equal nghits nco nres0 nres1 nsearched0 nsearched1 npairs nframes nlocal pool np0 np1 np2 np3 edits
// done: the pass completed it; bail: the FB_* reason (0 when done); equal: what it completed is the machine's result (1 for a read it did not complete);
// the rest: the largest value seen of FState::nghits, gh_nco / f_ncoords, nres0/1, nsearched0/1, npairs, nframes_max, f_nlocal, the pool entries in use
// (hot entries taken + popcount of pool_x), rb_np of each (mate, strand), and the most edits of any hit in the result, searched and genome-hit lists.
#include "h2g_emul.cpp"
#include <stdio.h>
#include <string>

struct ReadSet { std::vector<uint8_t> codes; std::vector<uint32_t> offs; std::string names; std::vector<uint32_t> noffs; };
static void load_reads(const char* fn, ReadSet& R) {
	FILE* f = fopen(fn, "r");
	if(!f) { fprintf(stderr, "cannot open %s\n", fn); exit(2); }
	std::vector<char> line(1 << 16);
	R.offs.push_back(0); R.noffs.push_back(0);
	while(fgets(line.data(), (int)line.size(), f)) {
		for(const char* p = line.data(); *p && *p != '\n'; p++) R.codes.push_back(*p == 'A' ? 0 : *p == 'C' ? 1 : *p == 'G' ? 2 : *p == 'T' ? 3 : 4);
		R.offs.push_back((uint32_t)R.codes.size());
		R.names += std::to_string(R.offs.size() - 2);
		R.noffs.push_back((uint32_t)R.names.size());
	}
	fclose(f);
	R.codes.resize(R.codes.size() + 8, 0);                   // (word-wise readers may touch a few bytes past the last read)
}

struct Marks {
	uint32_t nghits, nco, nres[2], nsearched[2], npairs, nframes, nlocal, pool, np[4], edits;
	void up(uint32_t& m, uint32_t v) { if(v > m) m = v; }
	// the state between two trips (the word store's pool and lists are the read's own from FPC_GO_INIT on: `started`)
	void sample(const FState& S, const FWords& W, bool started) {
		up(nghits, S.nghits); up(nco, S.gh_nco); up(nco, S.f_ncoords);
		up(nres[0], S.nres0); up(nres[1], S.nres1); up(nsearched[0], S.nsearched0); up(nsearched[1], S.nsearched1);
		up(npairs, S.npairs); up(nframes, S.nframes_max); up(nlocal, S.f_nlocal);
		for(uint32_t x = 0; x < 4; x++) up(np[x], fs_b4(S.rb_np, x));
		if(!started) return;
		uint32_t inuse = (uint32_t)__builtin_popcount(S.pool_x);
		for(uint32_t k = 0; k < FG_NLONG; k++) inuse += W.ld(FW_LONG + FG_LW * k + 2) != 0;
		up(pool, inuse);
		auto ned = [&](uint32_t hb) { return (W.ld(hb + 5) >> 1) & 7u; };
		for(uint32_t m = 0; m < S.nm; m++) {
			for(uint32_t k = 0; k < fs_nres(S, m) && k < FG_NRES; k++) up(edits, ned(fg_res_hit(m, k)));
			for(uint32_t i = 0; i < fs_nsearched(S, m) && i < FG_NSRCH; i++) up(edits, ned(FW_SRCH + m * FG_NSRCH * (1 + FG_HW) + i * (1 + FG_HW) + 1));
		}
		for(uint32_t k = 0; k < S.nghits && k < FG_NGH; k++) up(edits, ned(fg_gbase(k)));
	}
};

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if(cmd == "caps") {
		printf("FG_FE %d FG_NCO %d FG_NGH %d FG_NRES %d FG_NSRCH %d FG_NPAIR %d FG_NFRAME %d FG_NLOCAL %d FG_NLONG %d FG_NLONGC %d FG_GRAPH %d FG_ALIGN_MATE %d FS_WORDS %d FW_HOT %d FW_TOTAL %d H2G_GHIT_EDITS %d\n",
		       FG_FE, FG_NCO, FG_NGH, FG_NRES, FG_NSRCH, FG_NPAIR, FG_NFRAME, FG_NLOCAL, FG_NLONG, FG_NLONGC, FG_GRAPH, FG_ALIGN_MATE, FS_WORDS, (int)FW_HOT, (int)FW_TOTAL, H2G_GHIT_EDITS);
		return 0;
	}
	if(cmd != "run" || argc < 4) { fprintf(stderr, "usage: h2g_fastcap_check caps | run <index> <reads> [<mates2>] [params=<file>]\n"); return 2; }
	Emu* e = nullptr;
	if(h2gemu_load(argv[2], &e) != 0) { fprintf(stderr, "cannot load %s\n", argv[2]); return 2; }
	const std::unique_ptr<Emu> owner(e);                     // (freed on every way out: the sanitized build reports leaks)
	if((e->dg.linear != 0) == (FG_GRAPH != 0)) { fprintf(stderr, "%s is not the kind of index this program's pass is built for\n", argv[2]); return 2; }
	if(strncmp(argv[argc - 1], "params=", 7) == 0) {
		h2g_align_params hp;
		FILE* f = fopen(argv[argc - 1] + 7, "rb");
		if(!f || fread(&hp, sizeof hp, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[argc - 1] + 7); return 2; }
		fclose(f);
		h2gemu_set_params(e, &hp);
		argc--;
	}
	ReadSet R, R2;
	load_reads(argv[3], R);
	h2gemu_set_reads(e, R.codes.data(), R.offs.data(), nullptr, R.offs.size() - 1);
	const bool paired = argc > 4;
	if(paired) { load_reads(argv[4], R2); if(R2.offs.size() != R.offs.size()) { fprintf(stderr, "the mate files differ in length\n"); return 2; } }
	MachLane ML(e, 1, paired ? R2.codes.data() : nullptr, paired ? R2.offs.data() : nullptr, nullptr);
	FastLane FL(e, ML);
	const uint32_t n = ML.n(), slots = 16;
	std::vector<h2g_alnres> f1(slots), f2(slots), m1(slots), m2(slots);
	const AlignWS& ws = *ML.ws;
	for(uint32_t i = 0; i < n; i++) {
		ML.name(i, R.names.data(), R.noffs.data(), paired ? R2.names.data() : nullptr, paired ? R2.noffs.data() : nullptr);
		PairOut fp, mp; ReadOut fr, mr;
		memset((void*)&fp, 0, sizeof fp); memset((void*)&fr, 0, sizeof fr);
		memset((void*)f1.data(), 0, slots * sizeof(h2g_alnres)); memset((void*)f2.data(), 0, slots * sizeof(h2g_alnres));
		FL.out(MachLane::single(i, slots, paired, fp, fr, f1.data(), f2.data()));
		const bool packed_ok = FL.begin(i, paired);
		FState& S = FL.S;
		Marks M;
		memset(&M, 0, sizeof M);
		fast_begin(FL.F, S, i, paired, packed_ok);
		bool started = false;
		while(S.pc != FPC_DONE && S.pc != FPC_BAIL) {
			if(S.op == FOP_NONE) {
				fast_step(FL.F, S, FL.W);
				started = started || !(S.pc == FPC_BAIL && S.bail == FB_INPUT);
				M.sample(S, FL.W, started);
			}
			if(S.op != FOP_NONE) {
				// what the queued kernel does between two trips: the state through its packed form (and the site table must know the resume pc)
				uint32_t pw[FS_WORDS];
				const uint32_t op = S.op;
				if(fg_site_of(S.pc) == 0 || fg_site_op(fg_site_of(S.pc)) != op) { S.pc = FPC_BAIL; S.bail = FB_OTHER; break; }
				fs_pack(S, [&](uint32_t k, uint32_t v) { pw[k] = v; });
				memset((void*)&S, 0x5a, sizeof S);
				fs_unpack(S, [&](uint32_t k) { return pw[k]; });
				fast_exec(FL.F, S, FL.W, S.op);
				M.sample(S, FL.W, started);
			}
		}
		const bool done = S.pc == FPC_DONE;
		const uint32_t bail = done ? 0u : (uint32_t)S.bail;
		bool same = true;
		if(done) {
			ML.run(i, paired, MachLane::single(i, slots, paired, mp, mr, m1.data(), m2.data()));
			same = paired ? pairout_equal(mp, fp) && rows_equal(f1.data(), ws.m[0].res, fp.nres[0]) && rows_equal(f2.data(), ws.m[1].res, fp.nres[1])
			              : readout_equal(mr, fr) && abi_rows_equal(f1.data(), m1.data(), fr.nselect);
			for(int m = 0; m < (paired ? 2 : 1); m++) {
				const uint32_t nr = paired ? fp.nres[m] : fr.nselect;
				for(uint32_t k = 0; k < nr && k < slots; k++) M.up(M.edits, (m ? f2 : f1)[k].nedits);
			}
		}
		printf("%d %u %d %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", (int)done, bail, (int)same, M.nghits, M.nco, M.nres[0], M.nres[1], M.nsearched[0], M.nsearched[1],
		       M.npairs, M.nframes, M.nlocal, M.pool, M.np[0], M.np[1], M.np[2], M.np[3], M.edits);
	}
	return 0;
}
