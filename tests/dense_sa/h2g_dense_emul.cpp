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

// lanes_digest (tests/emul) with the pass run as h2gemu_fast_check runs it: out[0] machine hash, [1] fast hash, [2] reads completed, [3] the machine's nsteps
void h2gemu_dense_digest(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                         const uint32_t* noffs2, uint64_t* out) {
	lanes_digest(e, codes2, offs2, names1, noffs1, names2, noffs2, out, [](FastLane& FL, uint32_t i, bool paired) { return FL.run(i, paired); });
}

}
