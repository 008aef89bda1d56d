// ps0_check.cpp — TEST-ONLY stand-alone program: the fast pass's first partial searches taken from a table (h2g_fast.h fg_ps0_*, FPC_NB_PICK; the
// device fills the table in hisat2_amd/csrc/h2g_k_ps0.hip) against the searches run as requests, on the host lanes of tests/emul.
// Built with -fsanitize=address,undefined and run by tests/test_ps0_cpu.py:  ps0_check index_base reads.bin
// reads.bin: u32 n, u32 offs[n + 1], u8 codes[offs[n]] (the golden reads).  Exit status 0 = every check passed.
//  (a) every golden read and every edge read, both strands: fg_ps0_pack(partial_search_item at offset 0) -> fg_ps0_load gives the a0 - a5 FPC_NB_AFTER_PS
//      consumes — compared with the search's fields and, for a read the pass takes, with what fast_op_psearch leaves;
//  (b) fast_run_single with a host-built table and with a null pointer: FState, word store, outputs and counters byte-identical, singles and pairs.
#include "../emul/h2g_emul.cpp"
#include <stdio.h>
#include <string>

typedef std::vector<uint8_t> Rd;

static int g_fail = 0;
#define CHECK(COND, ...) do { if(!(COND)) { if(g_fail < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } g_fail++; } } while(0)

static void flatten(const std::vector<Rd>& v, std::vector<uint8_t>& codes, std::vector<uint32_t>& offs) {
	codes.clear(); offs.assign(1, 0);
	for(const Rd& r : v) { codes.insert(codes.end(), r.begin(), r.end()); offs.push_back((uint32_t)codes.size()); }
	codes.resize(codes.size() + 8, 0);                      // (fg_pack_read reads whole words)
}

// the table k_ps0 writes: what fast_begin refuses for one mate is absent for the whole unit
static void build_table(const DGfm& g, const AlnParams& P, const DReads& rd1, const DReads& rd2, bool paired, uint32_t n, std::vector<uint32_t>& tbl) {
	tbl.assign((size_t)n * 4 * FG_PS0_WORDS, FG_PS0_ABSENT);
	for(uint32_t u = 0; u < n; u++) {
		uint32_t pk[2][H2G_PK_WORDS];
		bool ok = fg_pack_read(rd1, u, pk[0], 1) && !(rd1.qc && !rd1.qc[u]);
		if(paired) ok = (fg_pack_read(rd2, u, pk[1], 1) && !(rd2.qc && !rd2.qc[u])) && ok;
		if(!ok) continue;
		for(uint32_t x = 0; x < (paired ? 4u : 2u); x++) {
			const DReads& rd = x >> 1 ? rd2 : rd1;
			SeqView sv;
			sv.fwc = nullptr; sv.q = nullptr; sv.len = rd.offs[u + 1] - rd.offs[u]; sv.fw = (x & 1u) == 0;
			sv.pk = pk[x >> 1]; sv.pk_stride = 1; sv.pk_nomask = true;
			h2g_fm_hit fh;
			partial_search_item(g, sv, 0, P.pseudogeneStop != 0, P.anchorStop != 0, P.khits, &fh);
			fg_ps0_pack(fh, &tbl[((size_t)u * 4 + x) * FG_PS0_WORDS]);
		}
	}
}

struct Counts { uint64_t completed = 0, searches = 0, nrank = 0, nside = 0, units = 0, mismatch = 0; };

// fast_run_single's loop without the packed-state round trip, counting the partial-search requests
static uint64_t count_searches(FastLane& FL, uint32_t i, bool paired) {
	uint64_t n = 0;
	fast_begin(FL.F, FL.S, i, paired, FL.begin(i, paired));
	while(FL.S.pc != FPC_DONE && FL.S.pc != FPC_BAIL) {
		if(FL.S.op == FOP_NONE) fast_step(FL.F, FL.S, FL.W);
		if(FL.S.op != FOP_NONE) { n += FL.S.op == FOP_PSEARCH; fast_exec(FL.F, FL.S, FL.W, FL.S.op); }
	}
	return n;
}

// (b) over one batch: reads1 alone (reads2 == nullptr) or as pairs
static void check_lanes(Emu* e, const std::vector<Rd>& reads1, const std::vector<Rd>* reads2, const char* what) {
	std::vector<uint8_t> c1, c2; std::vector<uint32_t> o1, o2;
	flatten(reads1, c1, o1);
	const bool paired = reads2 != nullptr;
	if(paired) flatten(*reads2, c2, o2);
	const uint32_t n = (uint32_t)reads1.size(), slots = 16;
	h2gemu_set_reads(e, c1.data(), o1.data(), nullptr, n);
	MachLane ML(e, 1, paired ? c2.data() : nullptr, paired ? o2.data() : nullptr, nullptr);
	FastLane FL(e, ML);
	std::vector<uint32_t> tbl;
	build_table(e->dg, ML.P, FL.F.rd[0], FL.F.rd[1], paired, n, tbl);
	std::string names; std::vector<uint32_t> noffs(1, 0);
	for(uint32_t i = 0; i < n; i++) { names += std::to_string(i); noffs.push_back((uint32_t)names.size()); }
	std::vector<h2g_alnres> r1(slots), r2(slots), k1(slots), k2(slots);
	Counts with, without;
	for(uint32_t i = 0; i < n; i++) {
		ML.name(i, names.data(), noffs.data(), paired ? names.data() : nullptr, noffs.data());
		PairOut po, kpo; ReadOut ro, kro;
		FState kS; std::vector<uint32_t> kwords(FW_TOTAL);
		bool kdone = false;
		for(int pass = 0; pass < 2; pass++) {                 // 0: every search a request; 1: the first ones from the table
			memset((void*)&po, 0, sizeof po); memset((void*)&ro, 0, sizeof ro);
			memset((void*)r1.data(), 0, slots * sizeof(h2g_alnres)); memset((void*)r2.data(), 0, slots * sizeof(h2g_alnres));
			FL.out(MachLane::single(i, slots, paired, po, ro, r1.data(), r2.data()));
			FL.F.ps0 = pass ? tbl.data() : nullptr;
			const bool done = FL.run(i, paired);
			for(uint32_t k = ro.nselect; k < H2G_SELECT_CAP; k++) ro.select[k] = 0;      // (never set: tests/emul row_digest)
			Counts& c = pass ? with : without;
			c.units++; c.completed += done;
			if(done) { c.nrank += paired ? po.nrank : ro.nrank; c.nside += paired ? po.nside : ro.nside; }
			if(pass == 0) {
				kS = FL.S; memcpy(kwords.data(), FL.words, sizeof FL.words); kpo = po; kro = ro; k1 = r1; k2 = r2; kdone = done;
			} else {
				const bool same = done == kdone && memcmp(&kS, &FL.S, sizeof kS) == 0 && memcmp(kwords.data(), FL.words, sizeof FL.words) == 0 &&
					memcmp(&kpo, &po, sizeof po) == 0 && memcmp(&kro, &ro, sizeof ro) == 0 &&
					memcmp(k1.data(), r1.data(), slots * sizeof(h2g_alnres)) == 0 && memcmp(k2.data(), r2.data(), slots * sizeof(h2g_alnres)) == 0;
				CHECK(same, "%s unit %u: table and request paths differ (done %d/%d pc %u/%u bail %u/%u nrank %u/%u nside %u/%u)", what, i, (int)kdone, (int)done,
				      (unsigned)kS.pc, (unsigned)FL.S.pc, (unsigned)kS.bail, (unsigned)FL.S.bail, (unsigned)kS.nrank, (unsigned)FL.S.nrank, (unsigned)kS.nside, (unsigned)FL.S.nside);
				if(!same) with.mismatch++;
			}
			FL.F.ps0 = pass ? tbl.data() : nullptr;
			c.searches += count_searches(FL, i, paired);
		}
	}
	FL.F.ps0 = nullptr;
	printf("%s: %llu units, completed %llu / %llu, partial-search requests %llu -> %llu, nrank %llu / %llu, nside %llu / %llu\n", what, (unsigned long long)with.units,
	       (unsigned long long)without.completed, (unsigned long long)with.completed, (unsigned long long)without.searches, (unsigned long long)with.searches,
	       (unsigned long long)without.nrank, (unsigned long long)with.nrank, (unsigned long long)without.nside, (unsigned long long)with.nside);
	CHECK(with.completed == without.completed && with.nrank == without.nrank && with.nside == without.nside, "%s: totals differ", what);
	if(without.completed > 0) CHECK(with.searches < without.searches, "%s: the table took no search out of the loop", what);
}

// (a) for one read
static void check_record(Emu* e, const AlnParams& P, const Rd& r, FastLane& FL) {
	std::vector<uint8_t> codes(r); codes.resize(codes.size() + 8, 0);
	const uint32_t offs[2] = {0, (uint32_t)r.size()};
	DReads rd; rd.codes = codes.data(); rd.offs = offs; rd.quals = nullptr; rd.n = 1;
	uint32_t pk[H2G_PK_WORDS];
	const bool eligible = fg_pack_read(rd, 0, pk, 1);
	for(int fwi = 0; fwi < 2; fwi++) {
		SeqView sv = seq_view(rd, 0, fwi == 0);
		h2g_fm_hit fh;
		partial_search_item(e->dg, sv, 0, P.pseudogeneStop != 0, P.anchorStop != 0, P.khits, &fh);
		uint32_t tbl[4 * FG_PS0_WORDS];
		for(uint32_t k = 0; k < 4 * FG_PS0_WORDS; k++) tbl[k] = 0xdeadbeefu;
		fg_ps0_pack(fh, tbl + (size_t)fwi * FG_PS0_WORDS);
		FState S; memset((void*)&S, 0xa5, sizeof S);
		const bool have = fg_ps0_load(tbl, 0, (uint32_t)fwi, S);
		CHECK(have, "len %zu strand %d: a packed record reads as absent", r.size(), fwi);
		// the fields FPC_NB_AFTER_PS takes out of a0 - a5
		CHECK(S.a0 == fh.top && S.a1 == fh.bot, "len %zu strand %d: top/bot %u %u != %u %u", r.size(), fwi, S.a0, S.a1, fh.top, fh.bot);
		CHECK((S.a2 & 0xffu) == fh.len && ((S.a2 >> 8) & 0xffu) == fh.hit_type && ((S.a2 >> 16) & 1u) == (fh.done ? 1u : 0u) && ((S.a2 >> 17) & 1u) == (fh.anchorStop ? 1u : 0u) &&
		      (S.a2 >> 18) == fh.numUniqueSearch, "len %zu strand %d: a2 %08x (len %u type %u done %u anchor %u nus %u)", r.size(), fwi, S.a2, fh.len, fh.hit_type, fh.done, fh.anchorStop, fh.numUniqueSearch);
		CHECK(S.a3 == fh.cur && (S.a4 & 0xffffu) == fh.nrank && (S.a4 >> 16) == fh.nside && S.a5 == 0, "len %zu strand %d: cur %u/%u nrank %u/%u nside %u/%u bwoff %u", r.size(), fwi,
		      S.a3, fh.cur, S.a4 & 0xffffu, fh.nrank, S.a4 >> 16, fh.nside, S.a5);
		if(!eligible) continue;
		// ... and all six words against the request's own code site, over the packed read as the pass sees it
		FState T; memset((void*)&T, 0, sizeof T);
		T.paired = 0; T.sv_rdi = 0; T.sv_fw = fwi == 0; T.ro0 = 0; T.rl0 = (uint32_t)r.size(); T.a0 = 0;
		const DReads keep = FL.F.rd[0];
		FL.F.rd[0] = rd; memcpy(FL.pk[0], pk, sizeof pk);
		fast_op_psearch(FL.F, T);
		FL.F.rd[0] = keep;
		CHECK(T.a0 == S.a0 && T.a1 == S.a1 && T.a2 == S.a2 && T.a3 == S.a3 && T.a4 == S.a4 && T.a5 == S.a5, "len %zu strand %d: record %u %u %08x %u %08x %u != request %u %u %08x %u %08x %u",
		      r.size(), fwi, S.a0, S.a1, S.a2, S.a3, S.a4, S.a5, T.a0, T.a1, T.a2, T.a3, T.a4, T.a5);
	}
}

int main(int argc, char** argv) {
	if(argc < 3) { fprintf(stderr, "usage: ps0_check index_base reads.bin\n"); return 2; }
	Emu* e = nullptr;
	if(h2gemu_load(argv[1], &e) != 0 || !e->dg.linear) { fprintf(stderr, "cannot load a linear index from %s\n", argv[1]); return 2; }
	std::vector<Rd> golden;
	{
		FILE* f = fopen(argv[2], "rb");
		uint32_t n = 0;
		if(!f || fread(&n, 4, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
		std::vector<uint32_t> offs(n + 1);
		if(fread(offs.data(), 4, n + 1, f) != n + 1) return 2;
		std::vector<uint8_t> codes(offs[n]);
		if(fread(codes.data(), 1, codes.size(), f) != codes.size()) return 2;
		fclose(f);
		for(uint32_t i = 0; i < n; i++) golden.emplace_back(codes.begin() + offs[i], codes.begin() + offs[i + 1]);
	}
	if(golden.size() < 8) { fprintf(stderr, "too few reads\n"); return 2; }
	// the edge reads: prefixes of golden reads 0 + 1 joined, and golden reads with one N
	const uint32_t ft = e->dg.ftabChars;
	std::vector<Rd> edge;
	{
		Rd two(golden[0]); two.insert(two.end(), golden[1].begin(), golden[1].end());
		while(two.size() < H2G_PK_MAXLEN + 1) two.insert(two.end(), golden[2].begin(), golden[2].end());
		const uint32_t lens[] = {0, 1, ft, ft + 1, ft + 2, 30, 101, H2G_PK_MAXLEN, H2G_PK_MAXLEN + 1};
		for(uint32_t L : lens) {
			edge.emplace_back(two.begin(), two.begin() + L);
			if(L >= 30 && L <= golden[3].size()) edge.emplace_back(golden[3].end() - L, golden[3].end());   // ... and a suffix, which aligns as well
		}
		const size_t L = golden[4].size();
		const size_t at[] = {3, L - 4, ft / 2, L - 1 - ft / 2, L / 2, ft + 5, L - ft - 6};      // inside the first ftabChars bases of either strand's search, and beyond them
		for(size_t p : at) { Rd r(golden[4]); if(p < L) r[p] = 4; edge.push_back(r); }
	}
	{
		std::vector<uint8_t> c; std::vector<uint32_t> o;
		flatten(golden, c, o);
		h2gemu_set_reads(e, c.data(), o.data(), nullptr, golden.size());
	}
	{
		MachLane ML2(e, 1);
		FastLane FL(e, ML2);
		for(const Rd& r : golden) check_record(e, ML2.P, r, FL);
		for(const Rd& r : edge) check_record(e, ML2.P, r, FL);
		printf("records: %zu golden + %zu edge reads, both strands\n", golden.size(), edge.size());
	}
	// (b) the golden reads alone and as pairs (read i with the reverse complement of read i + 1, and with itself reversed: a concordant pair of one fragment)
	std::vector<Rd> mates, self;
	for(size_t i = 0; i < golden.size(); i++) {
		const Rd& s = golden[(i + 1) % golden.size()];
		Rd m(s.rbegin(), s.rend()); for(uint8_t& c : m) c = c < 4 ? 3 - c : 4;
		mates.push_back(m);
		Rd t(golden[i].rbegin(), golden[i].rend()); for(uint8_t& c : t) c = c < 4 ? 3 - c : 4;
		self.push_back(t);
	}
	check_lanes(e, golden, nullptr, "golden reads");
	check_lanes(e, golden, &mates, "golden pairs");
	check_lanes(e, golden, &self, "golden self pairs");
	check_lanes(e, edge, nullptr, "edge reads");
	std::vector<Rd> edge2(edge.begin() + 1, edge.end()); edge2.push_back(edge[0]);      // unequal mates, an empty mate on either side, an N in one mate
	check_lanes(e, edge, &edge2, "edge pairs");
	delete e;
	if(g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
	printf("ps0_check ok\n");
	return 0;
}
