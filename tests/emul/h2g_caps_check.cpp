// h2g_caps_check — TEST-ONLY stand-alone program (its own main; nothing is loaded into an interpreter): the host instantiation of the graph primitives, the general
// machine and the fast lane at ONE of the shipped capacity sets, chosen on the compile line exactly as for h2g_emul.cpp (-DH2GEMU_CAPS=0 the *_big units',
// 1 the default units', 2 the graph fast pass's own header), driven over text vectors and printing text, so that what it reads and writes does not depend on
// the capacities (the ctypes mirrors of tests/ do: they have the default layouts).  Built plain by tests/emul/Makefile and with -fsanitize=address,undefined by
// its `sanitize` target; tests/test_graph_caps_cpu.py compares its output with the reference's vectors.
//
//   h2g_caps_check caps
//   h2g_caps_check coords  <index> <vectors>            line: top bot node_top node_bot hitlen nie {node extra}*
//   h2g_caps_check psearch <index> <reads> <vectors>    line: read fw
//   h2g_caps_check extend  <index> <reads> <vectors>    line: read fw rdoff len tidx toff joinedOff mm
//   h2g_caps_check adjust  <index> <reads> <vectors>    line: read fw rdoff len tidx toff joinedOff
//   h2g_caps_check machine <index> <reads> [<mates2>] [params=<file>]   one line per read / pair: a digest of the machine's result
//   h2g_caps_check fast    <index> <reads> [<mates2>] [params=<file>]   one line per read / pair: completed, bail reason, digest of the lane's result
// A read file is one line of A/C/G/T/N per read.
#include "h2g_emul.cpp"
#include <stdio.h>
#include <string>

static std::vector<std::vector<uint32_t>> load_vectors(const char* fn) {
	std::vector<std::vector<uint32_t>> out;
	FILE* f = fopen(fn, "r");
	if(!f) { fprintf(stderr, "cannot open %s\n", fn); exit(2); }
	std::vector<char> line(1 << 16);
	while(fgets(line.data(), (int)line.size(), f)) {
		std::vector<uint32_t> v;
		char* p = line.data();
		while(true) {
			char* q = nullptr;
			const unsigned long long x = strtoull(p, &q, 10);
			if(q == p) break;
			v.push_back((uint32_t)x);
			p = q;
		}
		out.push_back(v);
	}
	fclose(f);
	return out;
}

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

static void print_edits(const h2g_edit* e, uint32_t n) {
	for(uint32_t k = 0; k < n; k++) printf(" %u:%c>%c:%d:%lld", e[k].pos, (char)e[k].chr, (char)e[k].qchr, (int)e[k].type, e[k].snp == H2G_MAX ? -1LL : (long long)e[k].snp);
}

// What fast_check_lanes (h2g_emul.cpp) compares between the pass and the machine, as one number per read, so that two PROGRAMS can be compared: the ReadOut /
// PairOut fields of readout_equal / pairout_equal and, of every selected / reported record, the fields and edits of rec_equal.
template <class R> static uint64_t rec_digest(uint64_t h, const R& a) {
	const uint32_t f[8] = {a.fw, a.tidx, a.toff, a.len, a.trim5, a.trim3, a.nedits, a.splicescore};
	h = fnv(h, f, sizeof f);
	const int64_t sc = a.score;
	h = fnv(h, &sc, sizeof sc);
	for(uint32_t k = 0; k < a.nedits && k < H2G_MAX_EDITS; k++) {
		const uint32_t e[6] = {a.edits[k].pos, a.edits[k].chr, a.edits[k].qchr, a.edits[k].type, a.edits[k].pad, a.edits[k].snp};
		h = fnv(h, e, sizeof e);
	}
	return h;
}
static uint64_t readout_digest(uint64_t h, const ReadOut& a, const h2g_alnres* rows) {
	const int64_t f[11] = {a.nres, a.nselect, a.overflow, a.nrank, a.nsteps, a.depth, a.nside, a.best, a.secbest, a.best_h2, a.secbest_h2};
	h = fnv(h, f, sizeof f);
	for(uint32_t k = 0; k < a.nselect; k++) { const uint32_t s = a.select[k]; h = fnv(h, &s, sizeof s); h = rec_digest(h, rows[k]); }
	return h;
}
static uint64_t pairout_digest(uint64_t h, const PairOut& a) {
	const uint32_t f[9] = {a.nres[0], a.nres[1], a.npairs, a.overflow, a.nrank, a.nsteps, a.depth, a.nside, a.rnd_state};
	h = fnv(h, f, sizeof f);
	h = fnv(h, a.pair_i, sizeof a.pair_i);
	return fnv(h, a.pair_j, sizeof a.pair_j);
}

int main(int argc, char** argv) {
	const std::string cmd = argc > 1 ? argv[1] : "";
	if(cmd == "caps") {
		printf("H2G_IEDGE_CAP %d H2G_GW_MAXELT %d H2G_GW_MAXST %d H2G_GW_MAXROWS %d H2G_GHIT_EDITS %d H2G_NEW_EDITS %d H2G_AWA_CAND %d H2G_AWA_DEPTH %d FG_GRAPH %d FB_GWALK %d\n",
		       H2G_IEDGE_CAP, H2G_GW_MAXELT, H2G_GW_MAXST, H2G_GW_MAXROWS, H2G_GHIT_EDITS, H2G_NEW_EDITS, H2G_AWA_CAND, H2G_AWA_DEPTH, FG_GRAPH, (int)FB_GWALK);
		return 0;
	}
	if(argc < 4) { fprintf(stderr, "usage: h2g_caps_check <caps|coords|psearch|extend|adjust|machine|fast> <index> ...\n"); return 2; }
	Emu* e = nullptr;
	if(h2gemu_load(argv[2], &e) != 0) { fprintf(stderr, "cannot load %s\n", argv[2]); return 2; }
	const std::unique_ptr<Emu> owner(e);                     // (freed on every way out: the sanitized build reports leaks)
	if(e->dg.linear) { fprintf(stderr, "%s is not a graph index\n", argv[2]); return 2; }
	if(cmd == "coords") {
		const auto V = load_vectors(argv[3]);
		std::unique_ptr<GwCtx> x(new GwCtx());
		std::vector<h2g_coord> co(H2G_GW_MAXELT);
		for(const auto& v : V) {
			IEdges ie;
			ie.n = v[5];                                       // the true count; the list stores what it can hold (include/h2g.h)
			for(uint32_t k = 0; k < ie.n && k < H2G_IEDGE_CAP; k++) { ie.e[k][0] = v[6 + 2 * k]; ie.e[k][1] = v[7 + 2 * k]; }
			h2g_sa_result res;
			genome_coords_graph_item(e->dg, x.get(), v[0], v[1], v[2], v[3], &ie, v[1] - v[0], v[4], false, co.data(), (uint32_t)co.size(), &res);
			printf("%u %u %u %u", res.ok, res.ncoords, res.straddled, res.nsteps);
			for(uint32_t k = 0; k < res.ncoords; k++) printf(" %u:%u:%u", co[k].tidx, co[k].toff, co[k].joinedOff);
			putchar('\n');
		}
		return 0;
	}
	ReadSet R, R2;
	load_reads(argv[3], R);
	h2gemu_set_reads(e, R.codes.data(), R.offs.data(), nullptr, R.offs.size() - 1);
	const DReads rd = e->reads();
	if(cmd == "psearch" || cmd == "extend" || cmd == "adjust") {
		if(argc < 5) return 2;
		const auto V = load_vectors(argv[4]);
		std::unique_ptr<AwaWS> W(new AwaWS());
		DScoring sc;
		for(const auto& v : V) {
			const SeqView sv = seq_view(rd, v[0], v[1] != 0);
			if(cmd == "psearch") {
				h2g_fm_hit o;
				IEdges ie;
				partial_search_graph_item(e->dg, sv, 0, false, true, 10, 20, &o, &ie);
				printf("%u %u %u %u %u %u %u %u %u %u %u %u %u | %u", o.top, o.bot, o.node_top, o.node_bot, o.bwoff, o.len, o.hit_type, o.cur, o.done, o.numPartialSearch,
				       o.numUniqueSearch, o.pseudogeneStop, o.anchorStop, ie.n);
				for(uint32_t k = 0; k < ie.n && k < H2G_IEDGE_CAP; k++) printf(" %u:%u", ie.e[k][0], ie.e[k][1]);
				putchar('\n');
			} else if(cmd == "extend") {
				h2g_ghit h;
				memset(&h, 0, sizeof h);
				h.read = v[0]; h.fw = v[1]; h.rdoff = v[2]; h.len = v[3]; h.tidx = v[4]; h.toff = v[5]; h.joinedOff = v[6];
				uint32_t le = 0, re = 0;
				const bool ext = extend_item_alts(e->dr, e->dalts, sc, sv, &h, v[7], H2G_MAX, H2G_MAX, &le, &re, W.get());
				printf("%u %d %u %u %u %u %u %u %lld %u", h.overflow, (int)ext, h.rdoff, h.len, h.toff, h.joinedOff, le, re, (long long)h.score, h.nedits);
				if(!h.overflow) print_edits(h.edits, h.nedits);
				putchar('\n');
			} else {
				const uint32_t cap = 8;
				std::vector<h2g_ghit> hits(cap);
				uint32_t nh = 0, ovf = 0;
				adjust_with_alt(e->dg, e->dr, e->dalts, sv, v[2], v[3], v[4], v[5], v[6], hits.data(), &nh, cap, W.get(), &ovf);
				printf("%u %u", ovf, nh);
				for(uint32_t k = 0; k < nh && !ovf; k++) {
					printf(" | %u %u %u %u %u", hits[k].rdoff, hits[k].len, hits[k].toff, hits[k].joinedOff, hits[k].nedits);
					print_edits(hits[k].edits, hits[k].nedits);
				}
				putchar('\n');
			}
		}
		return 0;
	}
	if(cmd == "machine" || cmd == "fast") {
		// a trailing "params=<file>": the raw bytes of an h2g_align_params block (the options of the run; api.AlignParams writes them)
		if(strncmp(argv[argc - 1], "params=", 7) == 0) {
			h2g_align_params hp;
			FILE* f = fopen(argv[argc - 1] + 7, "rb");
			if(!f || fread(&hp, sizeof hp, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[argc - 1] + 7); return 2; }
			fclose(f);
			h2gemu_set_params(e, &hp);
			argc--;
		}
		const bool paired = argc > 4;
		if(paired) { load_reads(argv[4], R2); if(R2.offs.size() != R.offs.size()) return 2; }
		MachLane ML(e, 1, paired ? R2.codes.data() : nullptr, paired ? R2.offs.data() : nullptr, nullptr);
		FastLane FL(e, ML);
		const uint32_t n = ML.n(), slots = 16;
		std::vector<h2g_alnres> r1(slots), r2(slots);
		for(uint32_t i = 0; i < n; i++) {
			ML.name(i, R.names.data(), R.noffs.data(), paired ? R2.names.data() : nullptr, paired ? R2.noffs.data() : nullptr);
			PairOut po; ReadOut ro;
			const MachOut O = MachLane::single(i, slots, paired, po, ro, r1.data(), r2.data());
			memset((void*)&po, 0, sizeof po); memset((void*)&ro, 0, sizeof ro);
			memset((void*)r1.data(), 0, slots * sizeof(h2g_alnres)); memset((void*)r2.data(), 0, slots * sizeof(h2g_alnres));
			uint64_t h = 1469598103934665603ull;
			if(cmd == "machine") {
				ML.run(i, paired, O);
				if(paired) { h = pairout_digest(h, po); for(int m = 0; m < 2; m++) for(uint32_t k = 0; k < po.nres[m] && k < slots; k++) h = rec_digest(h, ML.ws->m[m].res[k]); }
				else h = readout_digest(h, ro, r1.data());
				printf("%016llx %u\n", (unsigned long long)h, paired ? po.overflow : ro.overflow);
			} else {
				FL.out(O);
				const bool done = FL.run(i, paired);
				if(done && paired) { h = pairout_digest(h, po); for(int m = 0; m < 2; m++) for(uint32_t k = 0; k < po.nres[m] && k < slots; k++) h = rec_digest(h, (m ? r2 : r1)[k]); }
				else if(done) h = readout_digest(h, ro, r1.data());
				printf("%d %u %016llx\n", (int)done, done ? 0u : (uint32_t)FL.S.bail, done ? (unsigned long long)h : 0ull);
			}
		}
		return 0;
	}
	fprintf(stderr, "unknown command %s\n", cmd.c_str());
	return 2;
}
