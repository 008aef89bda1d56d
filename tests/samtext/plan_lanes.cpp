// plan_lanes.cpp — stand-alone host check of the plain SAM planner (hisat2_amd/csrc/h2g_sam_plan.h): it drives classify_* / plan_plain_* read by read, as a kernel lane
// does, over heap copies of exactly the read's own bytes (records of mate 1, records of mate 2, bases), so that a walk that leaves its read's bytes is an address error.
// The inputs include damaged bytes: an nedits that runs past the read's end, a truncated last record, a trailer whose count lies beyond its bytes, pairings that name
// records a mate does not have.  Those must come out handed on (class 0) or dropped as the host planner drops them.  Plain reads are checked against what the case's
// author expects of the descriptors.  Built with -fsanitize=address,undefined by tests/test_sam_plan_split_cpu.py; it has no device code and never runs on a GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../hisat2_amd/csrc/h2g_sam_plan.h"

using namespace h2g_plan;

static int failures = 0, cases = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; if(failures < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while(0)

typedef std::vector<uint8_t> Bytes;
struct E { uint32_t pos; uint8_t type; uint32_t snp; };

static void put32(Bytes& b, uint32_t v) { for(int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }
static Bytes rec(uint32_t fw, uint32_t tidx, uint32_t toff, uint32_t len, int64_t score, const std::vector<E>& ed, uint32_t trim5 = 0, uint32_t trim3 = 0, int64_t nedits = -1) {
	Bytes b;
	put32(b, fw); put32(b, tidx); put32(b, toff); put32(b, len); put32(b, trim5); put32(b, trim3); put32(b, nedits < 0 ? (uint32_t)ed.size() : (uint32_t)nedits); put32(b, 0);
	put32(b, (uint32_t)(uint64_t)score); put32(b, (uint32_t)((uint64_t)score >> 32));
	for(const E& e : ed) { put32(b, e.pos); b.push_back('A'); b.push_back('C'); b.push_back(e.type); b.push_back(e.type == 5 ? 0xA0 : 0); put32(b, e.snp); }
	if(b.size() % 8) put32(b, 0);
	return b;
}
static Bytes trailer(uint32_t count, uint32_t held) {      // `count` pairs claimed, `held` present
	Bytes b(40, 0);
	b[4] = (uint8_t)count; b[5] = (uint8_t)(count >> 8); b[6] = (uint8_t)(count >> 16); b[7] = (uint8_t)(count >> 24);
	const uint32_t tag = H2G_PAIR_TRAILER_TAG;
	memcpy(&b[24], &tag, 4);
	for(uint32_t k = 0; k < held; k++) put32(b, 0);
	if(b.size() % 8) put32(b, 0);
	return b;
}
static Bytes cat(const std::vector<Bytes>& v) { Bytes o; for(const Bytes& x : v) o.insert(o.end(), x.begin(), x.end()); return o; }
static Bytes cut(Bytes b, size_t drop) { b.resize(b.size() - drop); return b; }

// exactly sized heap copies: one allocation per array, nothing behind it
struct Heap {
	std::vector<void*> all;
	template <class T> T* copy(const T* p, size_t n) { T* q = (T*)malloc(n * sizeof(T)); if(n) memcpy(q, p, n * sizeof(T)); all.push_back(q); return q; }
	~Heap() { for(void* p : all) free(p); }
};

static const Opts OPT = {0.0, (double)0.15f, 2, /* nalts */ 4, /* nrefs */ 3, 0, 1, 1, 0};

struct PairCase { Bytes r1, r2; std::vector<std::pair<int, int> > pairs; uint32_t npairs_claimed; uint32_t len1, len2; int want; Opts o; const char* what; };

static void run_pair(const PairCase& c) {
	cases++;
	Heap H;
	h2g_pair_result pr;
	memset(&pr, 0, sizeof pr);
	pr.npairs = c.npairs_claimed;
	for(size_t k = 0; k < c.pairs.size() && k < H2G_PAIR_CAP; k++) { pr.pair_i[k] = (uint8_t)c.pairs[k].first; pr.pair_j[k] = (uint8_t)c.pairs[k].second; }
	const h2g_pair_result* res = H.copy(&pr, 1);
	const uint64_t bo1[2] = {0, c.r1.size()}, bo2[2] = {0, c.r2.size()};
	const uint32_t o1[2] = {0, c.len1}, o2[2] = {0, c.len2};
	Bytes codes1(c.len1, 1), codes2(c.len2, 2);
	In in;
	in.codes[0] = H.copy(codes1.data(), codes1.size()); in.codes[1] = H.copy(codes2.data(), codes2.size());
	in.offs[0] = H.copy(o1, 2); in.offs[1] = H.copy(o2, 2);
	in.qc[0] = in.qc[1] = nullptr;
	in.rec[0] = H.copy(c.r1.data(), c.r1.size()); in.rec[1] = H.copy(c.r2.data(), c.r2.size());
	in.boffs[0] = H.copy(bo1, 2); in.boffs[1] = H.copy(bo2, 2);
	in.nrec[0] = c.r1.size(); in.nrec[1] = c.r2.size();
	in.first = 0;
	Pick pk;
	const uint32_t cls = classify_pair(c.o, in, res[0], 0, &pk);
	CHECK((int)cls == c.want, "%s: class %u, expected %d", c.what, cls, c.want);
	if(!cls) return;
	h2g_sam_line* out = (h2g_sam_line*)malloc(2 * sizeof(h2g_sam_line));
	H.all.push_back(out);
	memset(out, 0xEE, 2 * sizeof(h2g_sam_line));
	const uint32_t nl = plan_plain_pair(c.o, in, cls, pk, 0, out);
	CHECK(nl == lines_of_class(cls, c.o.no_unal != 0), "%s: %u lines", c.what, nl);
	for(uint32_t k = 0; k < nl; k++) {
		const h2g_sam_line& d = out[k];
		const bool aligned = d.rec_off != ~0ull;
		CHECK(d.read == 0 && d.aux_len == 0 && d.cigar_len == 0 && d.mdz_len == 0 && d.mate <= 1 && (d.flag & 1), "%s: line %u", c.what, k);
		CHECK(d.mapq == (aligned ? 60 : 0) && d.nh == (aligned ? 1u : 0u) && ((d.flag & 4) != 0) == !aligned, "%s: line %u mapq / nh / flag", c.what, k);
		CHECK(!aligned || (d.rec_off % 8 == 0 && d.rec_off + 40 <= in.nrec[d.mate]), "%s: line %u rec_off", c.what, k);
		CHECK(d.yt == (cls == CLS_P_CONC ? 1 : cls == CLS_P_DISC ? 2 : 3), "%s: line %u yt", c.what, k);
		CHECK(((d.flag & 2) != 0) == (cls == CLS_P_CONC) && ((d.flag & 0x40) != 0) == (d.mate == 0) && ((d.flag & 0x80) != 0) == (d.mate == 1), "%s: line %u flag %u", c.what, k, d.flag);
		CHECK(((d.bits & H2G_SAM_LINE_STAR_SEQ) != 0) == ((d.mate ? c.len2 : c.len1) == 0), "%s: line %u star", c.what, k);
	}
	if(cls == CLS_P_CONC && nl == 2) CHECK(out[0].tlen == -out[1].tlen && out[0].tlen != 0 && (out[0].bits & H2G_SAM_LINE_HAS_TLEN), "%s: tlen %lld / %lld", c.what, (long long)out[0].tlen, (long long)out[1].tlen);
}

static void run_unpaired(const Bytes& r, UnpHead h, uint32_t len, int want, const char* what) {
	cases++;
	Heap H;
	const uint64_t bo[2] = {0, r.size()};
	const uint32_t o[2] = {0, len};
	Bytes codes(len, 4);
	In in;
	memset(&in, 0, sizeof in);
	in.codes[0] = H.copy(codes.data(), codes.size()); in.offs[0] = H.copy(o, 2);
	in.rec[0] = H.copy(r.data(), r.size()); in.boffs[0] = H.copy(bo, 2); in.nrec[0] = r.size();
	Pick pk;
	const uint32_t cls = classify_unpaired(OPT, in, h, 0, &pk);
	CHECK((int)cls == want, "%s: class %u, expected %d", what, cls, want);
	if(!cls) return;
	h2g_sam_line* out = (h2g_sam_line*)malloc(sizeof(h2g_sam_line));
	H.all.push_back(out);
	const uint32_t nl = plan_plain_unpaired(OPT, in, cls, pk, 0, out);
	CHECK(nl == 1 && out[0].mate == 0 && out[0].yt == 0 && !(out[0].flag & 1), "%s: line", what);
	CHECK(out[0].yf == (len < 2 ? 1 : 2), "%s: yf %u (every base is an N)", what, out[0].yf);
}

int main() {
	const std::vector<E> none, mm = {{3, 3, ~0u}, {17, 3, ~0u}}, gap = {{3, 1, ~0u}}, spl = {{9, 5, 0}}, alt = {{9, 3, 2}};
	const Bytes A = rec(1, 0, 1000, 50, -6, mm), B = rec(0, 0, 1200, 50, 0, none), A2 = rec(1, 1, 70000, 50, -12, none);
	Opts nomix = OPT; nomix.report_mixed = 0;
	Opts nodisc = OPT; nodisc.report_discordant = 0;
	Opts nounal = OPT; nounal.no_unal = 1;
	Opts db = OPT; db.db_tlen = 1;
	const std::vector<PairCase> P = {
		{A, B, {{0, 0}}, 1, 50, 50, CLS_P_CONC, OPT, "concordant"},
		{cat({A2, A}), B, {{1, 0}}, 1, 50, 50, CLS_P_CONC, OPT, "concordant, second record"},
		{A, rec(0, 0, 1148, 50, 0, none), {{0, 0}}, 1, 50, 50, CLS_P_CONC, db, "up_right + 99 == dn_left, database: not consulted"},
		{A, rec(0, 0, 1149, 50, 0, none), {{0, 0}}, 1, 50, 50, CLS_P_CONC, db, "up_right + 100 == dn_left, database: not consulted"},
		{A, rec(0, 0, 1150, 50, 0, none), {{0, 0}}, 1, 50, 50, CLS_HOST, db, "up_right + 100 < dn_left, database"},
		{A, rec(0, 0, 1900, 50, 0, none), {{0, 0}}, 1, 50, 50, CLS_HOST, db, "far mates, database"},
		{A, B, {{0, 0}, {0, 0}}, 2, 50, 50, CLS_HOST, OPT, "two pairings"},
		{A, B, {{4, 0}}, 1, 50, 50, CLS_P_DISC, OPT, "pair_i beyond n1: dropped, then discordant"},
		{A, B, {{0, 9}, {0, 0}}, 2, 50, 50, CLS_P_CONC, OPT, "pair_j beyond n2: dropped, one left"},
		{A, B, {{0, 0}}, 77, 50, 50, CLS_HOST, OPT, "npairs beyond the list's capacity: the list is read to its capacity, never beyond"},
		{A, B, {}, 0, 50, 50, CLS_P_DISC, OPT, "discordant"},
		{A, B, {}, 0, 50, 50, CLS_P_BOTH, nodisc, "both as unpaired mates"},
		{A, Bytes(), {}, 0, 50, 0, CLS_P_MATE1, OPT, "mate 1 alone, mate 2 empty"},
		{A, Bytes(), {}, 0, 50, 50, CLS_P_MATE1, nounal, "mate 1 alone, --no-unal"},
		{Bytes(), B, {}, 0, 50, 50, CLS_P_MATE2, OPT, "mate 2 alone"},
		{Bytes(), Bytes(), {}, 0, 1, 0, CLS_P_NONE, OPT, "neither"},
		{Bytes(), Bytes(), {}, 0, 50, 50, CLS_P_NONE, nounal, "neither, --no-unal"},
		{cat({A, A2}), B, {}, 0, 50, 50, CLS_HOST, OPT, "two unpaired records"},
		{cat({A, A2}), B, {}, 0, 50, 50, CLS_P_NONE, nomix, "two unpaired records, --no-mixed"},
		{rec(1, 0, 1000, 50, -6, gap), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "gap"},
		{A, rec(0, 0, 1200, 50, 0, spl), {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "splice"},
		{rec(1, 0, 1000, 50, -6, alt), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "ALT edit"},
		{rec(1, 7, 1000, 50, -6, none), B, {}, 0, 50, 50, CLS_HOST, OPT, "a reference the index does not have"},
		{rec(1, 0, 1000, 50, -6, none, 0, 0, 40), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "long record"},
		// damaged bytes
		{rec(1, 0, 1000, 50, -6, none, 0, 0, 20), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "nedits runs past the read's end"},
		{rec(1, 0, 1000, 50, -6, none, 0, 0, 0x7fffffff), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "a huge nedits (a long record's marker that is not there)"},
		{cat({A, cut(A2, 8)}), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "truncated last record (prefix cut)"},
		{cat({B, cut(A, 16)}), B, {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "truncated last record (edits cut)"},
		{cut(A, 40), B, {}, 0, 50, 50, CLS_HOST, OPT, "less than a prefix"},
		{cat({A, trailer(1, 1)}), B, {}, 0, 50, 50, CLS_HOST, OPT, "a trailer"},
		{cat({A, trailer(1000, 1)}), B, {}, 0, 50, 50, CLS_HOST, OPT, "a trailer with a count beyond its bytes"},
		{trailer(0x7fffffff, 0), B, {}, 0, 50, 50, CLS_HOST, OPT, "a trailer alone, huge count"},
		{A, cat({B, trailer(1, 1)}), {{0, 0}}, 1, 50, 50, CLS_HOST, OPT, "a trailer behind mate 2"},
	};
	for(int rep = 0; rep < 8; rep++) for(const PairCase& c : P) run_pair(c);
	const int32_t NO = INT32_MIN;
	run_unpaired(Bytes(), {0, NO, NO, 0, 0}, 50, CLS_U_UNAL, "unaligned");
	run_unpaired(Bytes(), {0, NO, NO, 0, 0}, 0, CLS_U_UNAL, "unaligned, empty read");
	run_unpaired(A, {1, -6, NO, 0xffff, 0}, 50, CLS_U_UNIQ, "unique");
	run_unpaired(A, {1, -6, -9, 0xffff, 0xffff}, 50, CLS_U_UNIQ, "unique, worse second best");
	run_unpaired(A, {1, -6, -6, 0xffff, 0xffff}, 50, CLS_HOST, "tied");
	run_unpaired(cat({A, A2}), {2, -6, -12, 0xffff, 0xffff}, 50, CLS_HOST, "two selected");
	run_unpaired(rec(1, 0, 5, 50, -6, gap), {1, -6, NO, 0xffff, 0}, 50, CLS_HOST, "gap");
	run_unpaired(Bytes(), {1, -6, NO, 0xffff, 0}, 50, CLS_HOST, "nselect without a record");
	run_unpaired(cut(A, 8), {1, -6, NO, 0xffff, 0}, 50, CLS_HOST, "record cut short");
	run_unpaired(rec(1, 0, 5, 50, -6, none, 0, 0, 31), {1, -6, NO, 0xffff, 0}, 50, CLS_HOST, "nedits past the end");
	run_unpaired(trailer(3, 0), {1, -6, NO, 0xffff, 0}, 50, CLS_HOST, "a trailer where a record should be");
	printf("%d cases, %d failures\n", cases, failures);
	return failures ? 1 : 0;
}
