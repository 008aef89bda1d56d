// line_check.cpp — stand-alone host check of the SAM line emitter (hisat2_amd/csrc/h2g_sam_line.h): for every case it builds the arrays a line reads, exactly sized on
// the heap, and asserts that the counting sink's byte count, the single writer's text, what the host's string sink appends and the text the lane-group sink leaves —
// driven lane by lane, sixteen lanes a line as the write kernel runs it, each lane with a staging buffer of its own, into a buffer of exactly the counted size — all
// equal a naive string build.  A record beyond H2G_MAX_EDITS keeps its edits in a long-edit area, as the host's format calls meet it.
// Built with -fsanitize=address,undefined by tests/test_sam_plan_cpu.py; it has no device code and never runs on a GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../hisat2_amd/csrc/h2g_sam_line.h"

using namespace h2g_line;

static int failures = 0, cases = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; if(failures < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while(0)

struct NoSync { static void sync() {} };
enum { NL = 16, STAGE = 256 };

struct Ed { uint32_t pos; char chr; uint8_t type; uint32_t snp; uint8_t pad; };
struct Case {
	std::string name = "read";
	uint32_t rdlen = 30; int code_mode = 0;            // 0: 0..3, 1: some 4, 2: some above 4
	bool quals = true;
	bool aligned = true, fw = true, opp = false, opp_other_ref = false;
	uint32_t tidx = 0, toff = 99, trim5 = 0, trim3 = 0; int64_t score = -6;
	std::vector<Ed> edits;
	uint32_t otoff = 500; int64_t oscore = -3;
	int32_t oref_tidx = -1; uint32_t oref_toff = 0;
	int64_t tlen = 0; int32_t zs = 0; uint32_t nh = 1; uint16_t flag = 0; uint8_t mapq = 60, mate = 0, yt = 0, yf = 0; uint16_t bits = 0;
	std::string cigar, mdz, zsz, whole;                // aux lines
	std::string rg; int strandness = 0; uint32_t nalts = 0;
};

static const std::vector<std::string> REFS = {"chr1", "2", "a_longer_reference_name.with.dots"};

static std::string num(int64_t v) { return std::to_string((long long)v); }

static std::string naive(const Case& c, const std::vector<uint8_t>& codes, const std::string& q) {
	if(c.bits & H2G_SAM_LINE_WHOLE_LINE) return c.whole;
	std::string o, nm = c.name;
	if((c.bits & H2G_SAM_LINE_STRIP_MATE_SUFFIX) && nm.size() >= 2 && nm[nm.size() - 2] == '/' && strchr("123", nm.back())) nm.resize(nm.size() - 2);
	if(nm.size() > 255) nm.resize(255);
	const size_t sp = nm.find_first_of(" \t\n\v\f\r");
	if(sp != std::string::npos) nm.resize(sp);
	o = nm + "\t" + num(c.flag) + "\t";
	const bool al = c.aligned, pp = (c.flag & 1) != 0, auxcm = (c.bits & H2G_SAM_LINE_AUX_CIGAR_MDZ) != 0;
	const uint32_t otidx = c.opp_other_ref ? (c.tidx + 1) % (uint32_t)REFS.size() : c.tidx;
	o += (al ? REFS[c.tidx] : c.oref_tidx != -1 ? REFS[c.oref_tidx] : std::string("*")) + "\t";
	o += (al ? num((int64_t)c.toff + 1) : c.oref_tidx != -1 ? num((int64_t)c.oref_toff + 1) : std::string("0")) + "\t";
	o += (al ? num(c.mapq) : std::string("0")) + "\t";
	if(al && auxcm) o += c.cigar;
	else if(al) o += (c.trim5 ? num(c.trim5) + "S" : "") + num(c.rdlen - c.trim5 - c.trim3) + "M" + (c.trim3 ? num(c.trim3) + "S" : "");
	else o += "*";
	o += "\t";
	if(al && pp) o += c.opp && otidx != c.tidx ? REFS[otidx] : "="; else o += c.oref_tidx != -1 ? "=" : "*";
	o += "\t";
	if(al && pp) o += num((int64_t)(c.opp ? c.otoff : c.toff) + 1); else o += c.oref_tidx != -1 ? num((int64_t)c.oref_toff + 1) : "0";
	o += "\t" + ((c.bits & H2G_SAM_LINE_HAS_TLEN) ? num(c.tlen) : std::string("0")) + "\t";
	const bool fw = !al || c.fw;
	if((c.bits & H2G_SAM_LINE_STAR_SEQ) || c.rdlen == 0) o += "*\t*\t";
	else {
		std::string s, qq;
		for(uint32_t i = 0; i < c.rdlen; i++) {
			const uint8_t x = codes[fw ? i : c.rdlen - 1 - i];
			s.push_back(x > 3 ? 'N' : fw ? "ACGT"[x] : "TGCA"[x]);
			qq.push_back(c.quals ? q[fw ? i : c.rdlen - 1 - i] : 'I');
		}
		o += s + "\t" + qq + "\t";
	}
	const char* YT[4] = {"UU", "CP", "DP", "UP"};
	const char* YF[4] = {"", "\tYF:Z:LN", "\tYF:Z:NS", "\tYF:Z:QC"};
	const std::string ytyf = std::string("YT:Z:") + YT[c.yt] + YF[c.yf] + (c.rg.empty() ? "" : "\t" + c.rg);
	if(!al) return o + ytyf + "\n";
	o += "AS:i:" + num(c.score);
	if(c.bits & H2G_SAM_LINE_HAS_ZS) o += "\tZS:i:" + num(c.zs);
	o += "\tXN:i:0";
	uint32_t mm = 0, go = 0, gx = 0, nm_ = 0;
	for(size_t j = 0; j < c.edits.size(); j++) {
		const Ed& e = c.edits[j];
		if(e.type == 5 || e.snp < c.nalts) continue;
		nm_++;
		if(e.type == 3) mm++;
		else { gx++; const bool cont = j > 0 && c.edits[j - 1].type == e.type && c.edits[j - 1].snp >= c.nalts && (e.type == 1 ? c.edits[j - 1].pos == e.pos : c.edits[j - 1].pos + 1 == e.pos); if(!cont) go++; }
	}
	o += "\tXM:i:" + num(mm) + "\tXO:i:" + num(go) + "\tXG:i:" + num(gx) + "\tNM:i:" + num(nm_) + "\tMD:Z:";
	if(auxcm) o += c.mdz;
	else {
		const uint32_t lt = c.rdlen - c.trim5 - c.trim3;
		std::vector<std::pair<uint32_t, char>> v;
		for(const Ed& e : c.edits) v.push_back({c.fw ? e.pos : lt - 1 - e.pos, e.chr});
		if(!c.fw) std::vector<std::pair<uint32_t, char>>(v.rbegin(), v.rend()).swap(v);
		uint32_t at = 0;
		for(auto& pe : v) { o += num(pe.first - at); o.push_back(pe.second); at = pe.first + 1; }
		o += num(lt - at);
	}
	if((c.bits & H2G_SAM_LINE_HAS_YS) && c.opp) o += "\tYS:i:" + num(c.oscore);
	o += "\t" + ytyf;
	if(c.strandness) {
		const bool m1 = (c.bits & H2G_SAM_LINE_SENSE_MATE1) != 0;
		// sam.h:940-966: F / FR: mate 1 on the forward strand is '+'; R / RF: '-'; mate 2 is the other way round under FR / RF and always '+' under F / R
		bool minus;
		if(m1) minus = c.fw ? (c.strandness == 2 || c.strandness == 4) : (c.strandness == 1 || c.strandness == 3);
		else minus = c.fw ? c.strandness == 3 : c.strandness == 4;
		o += std::string("\tXS:A:") + (minus ? "-" : "+");
	} else {
		uint32_t sense = 1;
		for(const Ed& e : c.edits) {
			if(e.type != 5) continue;
			const uint32_t d = (e.pad >> 4) & 7;
			if(sense == 1) sense = d;
			else if(d != 1 && ((sense == 2 || sense == 4) != (d == 2 || d == 4))) { sense = 1; break; }
		}
		if(sense != 1) o += std::string("\tXS:A:") + ((sense == 2 || sense == 4) ? "+" : "-");
	}
	o += "\tNH:i:" + num(c.nh);
	if(!c.zsz.empty()) o += "\tZs:Z:" + c.zsz;
	return o + "\n";
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 20); }

static void run_case(const char* what, const Case& c) {
	cases++;
	// the line is read 1 of 3 (or mate 2's read 1), so offsets are not zero; every array is exactly as long as what the line may read
	const uint32_t m = c.mate;
	std::vector<uint8_t> codes1(7 + c.rdlen + 3);
	std::vector<uint32_t> offs = {0, 7, 7 + c.rdlen, 10 + c.rdlen};
	for(uint8_t& x : codes1) x = (uint8_t)(rnd() & 3);
	std::vector<uint8_t> rd(c.rdlen);
	for(uint32_t i = 0; i < c.rdlen; i++) {
		uint8_t x = (uint8_t)(rnd() & 3);
		if(c.code_mode == 1 && (i % 5) == 0) x = 4;
		if(c.code_mode == 2 && (i % 3) == 0) x = (uint8_t)(5 + rnd() % 250);
		rd[i] = codes1[7 + i] = x;
	}
	std::string q(c.rdlen, '!'), quals(10 + c.rdlen, '#');
	for(uint32_t i = 0; i < c.rdlen; i++) quals[7 + i] = q[i] = (char)(33 + rnd() % 41);
	std::string names = "before" + c.name + "after";
	std::vector<uint32_t> noffs = {0, 6, 6 + (uint32_t)c.name.size(), 11 + (uint32_t)c.name.size()};
	// records: the line's, then (other mate's bytes) the opposite one; each ends where its edits end
	// (a record beyond H2G_MAX_EDITS holds one entry, the offset of its edits in the long-edit area; the area starts with entries of other records)
	const bool is_long = c.edits.size() > H2G_MAX_EDITS;
	std::vector<h2g_edit> area(is_long ? 3 + c.edits.size() : 0);
	auto record = [&area](uint32_t fw, uint32_t tidx, uint32_t toff, uint32_t len, uint32_t t5, uint32_t t3, int64_t score, const std::vector<Ed>& ed) {
		const bool lng = ed.size() > H2G_MAX_EDITS;
		std::vector<uint64_t> b((40 + 12 * (lng ? 1 : ed.size()) + 7) / 8);
		h2g_alnres* r = reinterpret_cast<h2g_alnres*>(b.data());
		r->fw = fw; r->tidx = tidx; r->toff = toff; r->len = len; r->trim5 = t5; r->trim3 = t3; r->nedits = (uint32_t)ed.size(); r->splicescore = 0; r->score = score;
		h2g_edit* e = reinterpret_cast<h2g_edit*>(reinterpret_cast<uint8_t*>(b.data()) + 40);
		if(lng) { e[0].pos = 3; e[0].snp = 0x4c4f4e47u; e = area.data() + 3; }
		for(size_t j = 0; j < ed.size(); j++) { e[j].pos = ed[j].pos; e[j].chr = (uint8_t)ed[j].chr; e[j].qchr = 'A'; e[j].type = ed[j].type; e[j].pad = ed[j].pad; e[j].snp = ed[j].snp; }
		return b;
	};
	std::vector<uint64_t> pad8(2, 0);
	std::vector<uint64_t> rec = pad8, orec = pad8;
	h2g_sam_line L;
	memset(&L, 0, sizeof L);
	L.rec_off = L.orec_off = ~0ull;
	const uint32_t otidx = c.opp_other_ref ? (c.tidx + 1) % (uint32_t)REFS.size() : c.tidx;
	if(c.aligned && !(c.bits & H2G_SAM_LINE_WHOLE_LINE)) { const auto b = record(c.fw ? 1u : 0u, c.tidx, c.toff, c.rdlen, c.trim5, c.trim3, c.score, c.edits); L.rec_off = rec.size() * 8; rec.insert(rec.end(), b.begin(), b.end()); }
	if(c.opp && !(c.bits & H2G_SAM_LINE_WHOLE_LINE)) { const auto b = record(1, otidx, c.otoff, 10, 0, 0, c.oscore, {}); L.orec_off = orec.size() * 8; orec.insert(orec.end(), b.begin(), b.end()); }
	std::string aux = "xy";
	L.aux_off = (uint32_t)aux.size();
	if(c.bits & H2G_SAM_LINE_WHOLE_LINE) aux += c.whole;
	else { if(c.bits & H2G_SAM_LINE_AUX_CIGAR_MDZ) { aux += c.cigar + c.mdz; L.cigar_len = (uint16_t)c.cigar.size(); L.mdz_len = (uint16_t)c.mdz.size(); } aux += c.zsz; }
	L.aux_len = (uint32_t)aux.size() - L.aux_off;
	L.read = 1; L.nh = c.nh; L.tlen = c.tlen; L.zs = c.zs; L.oref_tidx = c.oref_tidx; L.oref_toff = c.oref_toff; L.flag = c.flag; L.mapq = c.mapq; L.mate = c.mate; L.yt = c.yt; L.yf = c.yf; L.bits = c.bits;
	std::string refnames; std::vector<uint32_t> roffs(1, 0);
	for(const std::string& r : REFS) { refnames += r; roffs.push_back((uint32_t)refnames.size()); }
	// exact heap copies (std::string keeps a terminator and may keep slack: a read one past the end would go unseen)
	auto exact = [](const void* p, size_t n) { std::vector<char>* v = new std::vector<char>((const char*)p, (const char*)p + n); return v; };
	std::vector<char>* x_names = exact(names.data(), names.size()); std::vector<char>* x_quals = exact(quals.data(), quals.size()); std::vector<char>* x_aux = exact(aux.data(), aux.size());
	std::vector<char>* x_ref = exact(refnames.data(), refnames.size()); std::vector<char>* x_rg = exact(c.rg.data(), c.rg.size());
	Ctx x;
	memset(&x, 0, sizeof x);
	x.names[m] = x_names->data(); x.noffs[m] = noffs.data(); x.codes[m] = codes1.data(); x.offs[m] = offs.data(); x.quals[m] = c.quals ? x_quals->data() : nullptr;
	x.rec[m] = reinterpret_cast<const uint8_t*>(rec.data()); x.nrec[m] = rec.size() * 8; x.rec[m ^ 1] = reinterpret_cast<const uint8_t*>(orec.data()); x.nrec[m ^ 1] = orec.size() * 8;
	x.aux = x_aux->data(); x.n_aux = aux.size(); x.refnames = x_ref->data(); x.refname_offs = roffs.data(); x.nrefs = (uint32_t)REFS.size();
	x.rg = x_rg->data(); x.rg_len = (uint32_t)c.rg.size(); x.rna_strandness = c.strandness; x.nalts = c.nalts; x.first = 0; x.paired = 1;
	x.long_edits = is_long ? area.data() : nullptr;
	CHECK(line_records_ok(x, L) == !is_long, "%s: the case's own records are refused, or a record the kernels cannot read is let through", what);
	const std::string want = naive(c, rd, q);
	CountSink cs;
	emit_line(x, L, cs);
	CHECK(cs.n == want.size(), "%s: counted %llu bytes, the line has %zu", what, (unsigned long long)cs.n, want.size());
	if(cs.n == want.size()) {
		std::vector<char>* out = new std::vector<char>(want.size(), (char)0x7f);
		PtrSink ps = {out->data()};
		emit_line(x, L, ps);
		CHECK(ps.p == out->data() + want.size() && std::string(out->data(), out->size()) == want, "%s: the single writer wrote\n  %s  for\n  %s", what, std::string(out->data(), out->size()).c_str(), want.c_str());
		std::string text = "the line before\n";
		append_line(x, L, text);
		CHECK(text == "the line before\n" + want, "%s: the string sink appended\n  %s  for\n  %s", what, text.c_str(), want.c_str());
		std::vector<char>* gout = new std::vector<char>(want.size(), (char)0x7f);
		for(uint32_t lane = 0; lane < NL; lane++) {
			std::vector<char>* stage = new std::vector<char>(STAGE, (char)0x7e);
			GroupSink<NL, STAGE, NoSync> gs(gout->data(), stage->data(), lane);
			emit_line(x, L, gs);
			CHECK(gs.at == want.size() && gs.fill == 0, "%s: lane %u ends at %llu of %zu", what, lane, (unsigned long long)gs.at, want.size());
			delete stage;
		}
		CHECK(std::string(gout->data(), gout->size()) == want, "%s: the lane group wrote\n  %s  for\n  %s", what, std::string(gout->data(), gout->size()).c_str(), want.c_str());
		delete out; delete gout;
	}
	delete x_names; delete x_quals; delete x_aux; delete x_ref; delete x_rg;
}

static std::vector<Ed> mismatches(uint32_t n, uint32_t lt, bool ends) {
	std::vector<Ed> v;
	for(uint32_t k = 0; k < n; k++) {
		uint32_t pos = n == 1 ? (ends ? 0 : lt / 2) : (uint32_t)((uint64_t)k * (lt - 1) / (n - 1));      // 32 of them: position 0 and the last included
		if(n == 1 && ends && k == 0 && (rnd() & 1)) pos = lt - 1;
		v.push_back({pos, "ACGT"[rnd() & 3], 3, 0xffffffffu, 0});
	}
	return v;
}

int main() {
	char what[256];
	// names: lengths, blanks, endings (with and without the pair's suffix rule)
	for(size_t len : {0, 1, 254, 255, 256, 300}) for(int strip = 0; strip < 2; strip++) {
		Case c; c.name = std::string(len, 'n'); c.bits = strip ? H2G_SAM_LINE_STRIP_MATE_SUFFIX : 0; c.flag = strip ? 0x41 : 0;
		snprintf(what, sizeof what, "name of %zu bytes, strip %d", len, strip); run_case(what, c);
	}
	for(size_t at : {0, 254, 255}) { Case c; c.name = std::string(300, 'b'); c.name[at] = at == 254 ? '\t' : ' '; snprintf(what, sizeof what, "blank at %zu", at); run_case(what, c); }
	for(const char* end : {"/1", "/2", "/3", "/4", "/", "1"}) for(int strip = 0; strip < 2; strip++) for(size_t body : {0, 5, 254, 255}) {
		Case c; c.name = std::string(body, 'e') + end; c.bits = strip ? H2G_SAM_LINE_STRIP_MATE_SUFFIX : 0; c.flag = strip ? 0x81 : 0;
		snprintf(what, sizeof what, "name ending %s after %zu bytes, strip %d", end, body, strip); run_case(what, c);
	}
	// read lengths x strands x code kinds x qualities, aligned (where there is room) and unaligned
	for(uint32_t len : {0u, 1u, 15u, 16u, 17u, 63u, 64u, 65u, 255u, 256u, 257u, 1024u}) for(int fw = 0; fw < 2; fw++) for(int cm = 0; cm < 3; cm++) for(int ql = 0; ql < 2; ql++) for(int al = 0; al < 2; al++) {
		Case c; c.rdlen = len; c.fw = fw; c.code_mode = cm; c.quals = ql; c.aligned = al && len >= 1; c.flag = (uint16_t)(c.aligned ? (fw ? 0 : 16) : 4);
		if(c.aligned && len >= 2) c.edits = mismatches(1, len, true);
		snprintf(what, sizeof what, "read of %u bases, fw %d, codes %d, quals %d, aligned %d", len, fw, cm, ql, (int)c.aligned); run_case(what, c);
	}
	// trims at both ends, mismatch counts, strands
	for(uint32_t t5 : {0u, 1u, 12u}) for(uint32_t t3 : {0u, 2u, 30u}) for(uint32_t ne : {0u, 1u, 32u}) for(int fw = 0; fw < 2; fw++) for(int ends = 0; ends < 2; ends++) {
		Case c; c.rdlen = 101; c.trim5 = t5; c.trim3 = t3; c.fw = fw; c.flag = fw ? 0 : 16; c.edits = mismatches(ne, 101 - t5 - t3, ends);
		snprintf(what, sizeof what, "trims %u / %u, %u mismatches, fw %d, ends %d", t5, t3, ne, fw, ends); run_case(what, c);
	}
	// a record beyond H2G_MAX_EDITS: its mismatches are read from the long-edit area
	for(uint32_t ne : {33u, 40u, 97u}) for(int fw = 0; fw < 2; fw++) {
		Case c; c.rdlen = 101; c.trim5 = 1; c.trim3 = 2; c.fw = fw; c.flag = fw ? 0 : 16; c.nalts = 2; c.edits = mismatches(ne, 98, true);
		c.edits[5].snp = 1;
		snprintf(what, sizeof what, "%u mismatches in the long-edit area, fw %d", ne, fw); run_case(what, c);
	}
	// POS, TLEN, NH, MAPQ, ZS, the opposite record
	for(uint32_t toff : {0u, 0xffffffffu}) for(int64_t tlen : {(int64_t)0, (int64_t)1 << 62, -((int64_t)1 << 62), (int64_t)-1}) for(uint32_t nh : {0u, 9u, 10u, 128u}) for(int opp = 0; opp < 3; opp++) {
		Case c; c.toff = toff; c.otoff = toff ? 0 : 0xffffffffu; c.tlen = tlen; c.nh = nh; c.opp = opp > 0; c.opp_other_ref = opp == 2; c.tidx = 2;
		c.flag = 0x63; c.bits = H2G_SAM_LINE_HAS_TLEN | H2G_SAM_LINE_HAS_YS | H2G_SAM_LINE_HAS_ZS | H2G_SAM_LINE_STRIP_MATE_SUFFIX | H2G_SAM_LINE_SENSE_MATE1; c.zs = nh ? -(int32_t)nh : INT32_MIN; c.mapq = (uint8_t)(nh * 2 - nh / 128);
		c.score = toff ? INT32_MIN : 0; c.oscore = -77; c.mate = opp == 1;
		snprintf(what, sizeof what, "toff %u, tlen %lld, nh %u, opp %d", toff, (long long)tlen, nh, opp); run_case(what, c);
	}
	// every yt x yf, RG present and absent, each strandness code, either mate sense, either strand; aligned and unaligned (placed at its partner, or nowhere)
	for(int yt = 0; yt < 4; yt++) for(int yf = 0; yf < 4; yf++) for(int rg = 0; rg < 2; rg++) for(int st = 0; st < 5; st++) for(int m1 = 0; m1 < 2; m1++) for(int fw = 0; fw < 2; fw++) for(int al = 0; al < 3; al++) {
		Case c; c.yt = (uint8_t)yt; c.yf = (uint8_t)yf; c.rg = rg ? "RG:Z:group one" : ""; c.strandness = st; c.fw = fw; c.aligned = al == 0; c.bits = m1 ? H2G_SAM_LINE_SENSE_MATE1 : 0;
		if(al == 2) { c.oref_tidx = 1; c.oref_toff = 0xffffffffu; }
		c.flag = (uint16_t)(al ? 0x45 : 0x41);
		snprintf(what, sizeof what, "yt %d yf %d rg %d strandness %d mate1 %d fw %d al %d", yt, yf, rg, st, m1, fw, al); run_case(what, c);
	}
	// --omit-sec-seq
	{ Case c; c.bits = H2G_SAM_LINE_STAR_SEQ; c.flag = 256; run_case("secondary without SEQ", c); }
	// lines from the pool: CIGAR + MD:Z of gapped / spliced alignments (short and longer than the staging buffer), Zs:Z on simple and pool lines, ALT edits that do not count, XS:A from splices
	for(int k = 0; k < 4; k++) for(int zs = 0; zs < 2; zs++) for(int fw = 0; fw < 2; fw++) {
		Case c; c.rdlen = 120; c.fw = fw; c.flag = fw ? 0 : 16; c.bits = H2G_SAM_LINE_AUX_CIGAR_MDZ; c.nalts = 5;
		c.cigar = k == 3 ? std::string() : "40M2I78M"; c.mdz = "10A29^CC78";
		c.edits = {{10, 'A', 3, 0xffffffffu, 0}, {40, '-', 2, 0xffffffffu, 0}, {41, '-', 2, 0xffffffffu, 0}, {60, 'C', 1, 0xffffffffu, 0}, {60, 'C', 1, 0xffffffffu, 0}, {70, 'T', 3, 2, 0}, {80, 'G', 1, 4, 0}};
		if(k == 1) { c.edits.push_back({90, (char)200, 5, 0x3f000000u, (uint8_t)(2 << 4)}); c.edits.push_back({100, 20, 5, 0x3f000000u, (uint8_t)(4 << 4)}); }
		if(k == 2) { c.edits.push_back({90, 100, 5, 0x3f000000u, (uint8_t)(3 << 4)}); c.edits.push_back({100, 20, 5, 0x3f000000u, (uint8_t)(2 << 4)}); }
		if(k == 3) { for(int r = 0; r < 60; r++) { c.cigar += "1M1D"; c.mdz += "1^A"; } c.cigar += "60M"; c.mdz += "60"; }
		if(zs) c.zsz = "70|S|rs12,9|D|rs9";
		snprintf(what, sizeof what, "pool line kind %d, Zs %d, fw %d", k, zs, fw); run_case(what, c);
	}
	{ Case c; c.nalts = 3; c.edits = {{4, 'A', 3, 1, 0}, {9, 'C', 3, 0xffffffffu, 0}}; c.zsz = "4|S|rs1"; run_case("simple line with Zs:Z", c); }
	// WHOLE_LINE: the pool's bytes and nothing else
	for(size_t len : {1, 16, 17, 700}) { Case c; c.bits = H2G_SAM_LINE_WHOLE_LINE; c.whole = std::string(len - 1, 'w') + "\n"; snprintf(what, sizeof what, "whole line of %zu bytes", len); run_case(what, c); }
	printf("%d cases, %d failures\n", cases, failures);
	return failures ? 1 : 0;
}
