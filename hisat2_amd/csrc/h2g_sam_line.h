// h2g_sam_line.h — one SAM line from its descriptor (include/h2g.h h2g_sam_line), the reads and the records: the byte-producing half of append_mate (h2g_sam.cpp),
// and the only place that states the bytes of a line.  The host's format calls (every record layout), its plan-to-text call and the kernels all write through
// emit_line.  It is templated on a sink, so the pass that sizes a line (CountSink), the host's writer (StrSink) and the kernels' lane-group writer (GroupSink) run
// the same statements and cannot disagree on a length.
// Nothing here decides anything: FLAG, MAPQ, TLEN, ZS:i, YT / YF, NH and the CIGAR / MD:Z of gapped lines come with the descriptor (append_mate; make_line of
// h2g_sam_plan.h for the plain lines planned on the device).
#ifndef H2G_SAM_LINE_H_
#define H2G_SAM_LINE_H_
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>
#include "../../include/h2g.h"
#ifndef H2G_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define H2G_HD __host__ __device__ __forceinline__
#else
#define H2G_HD inline
#endif
#endif

namespace h2g_line {

// what a line reads besides its descriptor; every pointer is a host pointer for the host's sinks and a device pointer in the kernels
struct Ctx {
	const char* names[2]; const uint32_t* noffs[2];        // read names of mate 1 / mate 2 (unpaired runs: [0] only)
	const uint8_t* codes[2]; const uint32_t* offs[2];      // codes 0..4 (above: N), one byte per base
	const char* quals[2];                                  // phred+33, or nullptr: 'I'
	const uint8_t* rec[2]; uint64_t nrec[2];               // what a line's rec_off / orec_off count from, per mate, and the bytes there: the compact records of the fetch
	                                                       // (h2g_align_*_fetch_compact); in the host's format calls the records of any layout (nrec is not read there)
	const char* aux; uint64_t n_aux;
	const char* refnames; const uint32_t* refname_offs; uint32_t nrefs;   // cut at the first blank, after the chrname mode
	const char* rg; uint32_t rg_len;                       // "RG:Z:<id>" or empty
	int32_t rna_strandness; uint32_t nalts;
	uint32_t first;                                        // lines[].read counts from here
	uint32_t paired;
	const h2g_edit* long_edits;                            // host only: the batch's long-edit area (h2g_sam_set_long_edits), or nullptr.  The kernels do not read it
};

H2G_HD bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace of the C locale
H2G_HD uint32_t ndigits(uint64_t u) { uint32_t n = 1; while(u >= 10) { u /= 10; n++; } return n; }

// counts bytes; touches no output
struct CountSink {
	uint64_t n = 0;
	H2G_HD void ch(char) { n++; }
	H2G_HD void lit(const char*, uint32_t len) { n += len; }
	H2G_HD void num(int64_t v) { const uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v; n += ndigits(u) + (v < 0); }
	H2G_HD void bytes(const char*, uint64_t len) { n += len; }
	H2G_HD void seq(const uint8_t*, uint32_t len, bool) { n += len; }
	H2G_HD void qual(const char*, uint32_t len, bool) { n += len; }
	H2G_HD void finish() {}
};

// one writer into memory that has room (the pieces of the host's StrSink below; tests/samtext/line_check.cpp)
struct PtrSink {
	char* p;
	H2G_HD void ch(char c) { *p++ = c; }
	H2G_HD void lit(const char* s, uint32_t len) { for(uint32_t i = 0; i < len; i++) p[i] = s[i]; p += len; }
	H2G_HD void num(int64_t v) {
		uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
		if(v < 0) *p++ = '-';
		const uint32_t nd = ndigits(u);
		for(uint32_t k = nd; k-- > 0;) { p[k] = (char)('0' + u % 10); u /= 10; }
		p += nd;
	}
	H2G_HD void bytes(const char* s, uint64_t len) { for(uint64_t i = 0; i < len; i++) p[i] = s[i]; p += len; }
	H2G_HD void seq(const uint8_t* c, uint32_t len, bool fw) {
		for(uint32_t i = 0; i < len; i++) { const uint8_t x = c[fw ? i : len - 1 - i]; p[i] = "ACGTN"[fw ? (x > 4 ? 4 : x) : (x > 3 ? 4 : 3 - x)]; }
		p += len;
	}
	H2G_HD void qual(const char* q, uint32_t len, bool fw) { for(uint32_t i = 0; i < len; i++) p[i] = q ? q[fw ? i : len - 1 - i] : 'I'; p += len; }
	H2G_HD void finish() {}
};

// A group of NL lanes writes one line.  Every lane of the group runs the emitter with the same arguments, so the control flow is uniform within the group.  Small
// pieces (numbers, tags, single characters: the head and the tail of a line) are collected in a staging buffer of STAGE bytes that the group shares (LDS in the
// kernel); every lane writes the same bytes to the same places there.  A bulk piece (name, reference name, CIGAR / MD:Z / Zs:Z from the pool, SEQ, QUAL) first
// flushes the staging buffer, then is produced straight from its source.  Either way byte k of a piece is stored by lane k mod NL: consecutive lanes store to
// consecutive addresses.  Stores are single bytes: a line starts wherever the one before it ended, so no wider store is aligned for more than one line in NL.
// Between filling and flushing the buffer, sync() orders the group's accesses (a wave-level fence in the kernel; nothing where one lane runs at a time with a
// buffer of its own, as the host's checker drives it: tests/samtext/line_check.cpp).
template <uint32_t NL, uint32_t STAGE, class Sync>
struct GroupSink {
	char* out; uint64_t at; char* stage; uint32_t fill; uint32_t lane;
	H2G_HD GroupSink(char* o, char* st, uint32_t ln) : out(o), at(0), stage(st), fill(0), lane(ln) {}
	H2G_HD void flush() {
		if(!fill) return;
		Sync::sync();
		for(uint32_t i = lane; i < fill; i += NL) out[at + i] = stage[i];
		Sync::sync();
		at += fill; fill = 0;
	}
	H2G_HD void room(uint32_t n) { if(fill + n > STAGE) flush(); }
	H2G_HD void ch(char c) { room(1); stage[fill++] = c; }
	H2G_HD void lit(const char* s, uint32_t len) { room(len); for(uint32_t i = 0; i < len; i++) stage[fill + i] = s[i]; fill += len; }
	H2G_HD void num(int64_t v) {
		room(21);
		uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
		if(v < 0) stage[fill++] = '-';
		const uint32_t nd = ndigits(u);
		for(uint32_t k = nd; k-- > 0;) { stage[fill + k] = (char)('0' + u % 10); u /= 10; }
		fill += nd;
	}
	H2G_HD void bytes(const char* s, uint64_t len) {
		if(len <= 8 && len <= STAGE) { room((uint32_t)len); for(uint32_t i = 0; i < (uint32_t)len; i++) stage[fill + i] = s[i]; fill += (uint32_t)len; return; }
		flush();
		for(uint64_t i = lane; i < len; i += NL) out[at + i] = s[i];
		at += len;
	}
	H2G_HD void seq(const uint8_t* c, uint32_t len, bool fw) {
		flush();
		for(uint32_t i = lane; i < len; i += NL) { const uint8_t x = c[fw ? i : len - 1 - i]; out[at + i] = "ACGTN"[fw ? (x > 4 ? 4 : x) : (x > 3 ? 4 : 3 - x)]; }
		at += len;
	}
	H2G_HD void qual(const char* q, uint32_t len, bool fw) {
		flush();
		for(uint32_t i = lane; i < len; i += NL) out[at + i] = q ? q[fw ? i : len - 1 - i] : 'I';
		at += len;
	}
	H2G_HD void finish() { flush(); }
};

enum { EDIT_READ_GAP = 1, EDIT_REF_GAP = 2, EDIT_MM = 3, EDIT_SPL = 5 };
#define H2G_LINE_LIT(k, s) (k).lit(s, (uint32_t)(sizeof(s) - 1))

// The edits of a record.  One with more than H2G_MAX_EDITS keeps them in the long-edit area, edits[0].pos their offset there: the host's format calls reach them (they
// have checked the area's extent), the kernels never meet such a record (record_ok refuses it; the host sends its line whole).
H2G_HD const h2g_edit* edits_of(const Ctx& c, const h2g_alnres* rs) {
#if !defined(__HIP_DEVICE_COMPILE__)
	if(rs->nedits > H2G_MAX_EDITS) return c.long_edits + rs->edits[0].pos;
#endif
	return rs->edits;
}

template <class Sink>
H2G_HD void put_ref_name(Sink& k, const Ctx& c, uint32_t tidx) { k.bytes(c.refnames + c.refname_offs[tidx], c.refname_offs[tidx + 1] - c.refname_offs[tidx]); }

template <class Sink>
H2G_HD void put_yt_yf_rg(Sink& k, const Ctx& c, const h2g_sam_line& L) {
	if(L.yt == 1) H2G_LINE_LIT(k, "YT:Z:CP"); else if(L.yt == 2) H2G_LINE_LIT(k, "YT:Z:DP"); else if(L.yt == 3) H2G_LINE_LIT(k, "YT:Z:UP"); else H2G_LINE_LIT(k, "YT:Z:UU");
	if(L.yf == 1) H2G_LINE_LIT(k, "\tYF:Z:LN"); else if(L.yf == 2) H2G_LINE_LIT(k, "\tYF:Z:NS"); else if(L.yf == 3) H2G_LINE_LIT(k, "\tYF:Z:QC");
	if(c.rg_len) { k.ch('\t'); k.bytes(c.rg, c.rg_len); }
}

// The line of descriptor L.  The caller has checked what h2g_sam_plan_check / the sizes kernel check: every offset below lies inside its array.
template <class Sink>
H2G_HD void emit_line(const Ctx& c, const h2g_sam_line& L, Sink& k) {
	if(L.bits & H2G_SAM_LINE_WHOLE_LINE) { k.bytes(c.aux + L.aux_off, L.aux_len); k.finish(); return; }
	const uint32_t m = L.mate, i = c.first + L.read;
	const h2g_alnres* rs = L.rec_off == ~0ull ? nullptr : reinterpret_cast<const h2g_alnres*>(c.rec[m] + L.rec_off);
	const h2g_alnres* rso = L.orec_off == ~0ull ? nullptr : reinterpret_cast<const h2g_alnres*>(c.rec[m ^ 1u] + L.orec_off);
	const uint32_t rdlen = c.offs[m][i + 1] - c.offs[m][i];
	const bool fw = !rs || (rs->fw & H2G_FW_STRAND) != 0;
	{	// QNAME: SamConfig::printReadName, at most 255 bytes and up to the first blank
		const char* nm = c.names[m] + c.noffs[m][i];
		uint32_t n = c.noffs[m][i + 1] - c.noffs[m][i];
		if((L.bits & H2G_SAM_LINE_STRIP_MATE_SUFFIX) && n >= 2 && nm[n - 2] == '/' && (nm[n - 1] == '1' || nm[n - 1] == '2' || nm[n - 1] == '3')) n -= 2;
		if(n > 255) n = 255;
		uint32_t e = 0;
		while(e < n && !is_space(nm[e])) e++;
		k.bytes(nm, e);
	}
	k.ch('\t'); k.num(L.flag); k.ch('\t');
	if(rs) put_ref_name(k, c, rs->tidx); else if(L.oref_tidx != -1) put_ref_name(k, c, (uint32_t)L.oref_tidx); else k.ch('*');
	k.ch('\t');
	if(rs) k.num((int64_t)rs->toff + 1); else if(L.oref_tidx != -1) k.num((int64_t)L.oref_toff + 1); else k.ch('0');
	k.ch('\t');
	if(rs) k.num(L.mapq); else k.ch('0');
	k.ch('\t');
	const bool auxcm = (L.bits & H2G_SAM_LINE_AUX_CIGAR_MDZ) != 0;
	if(rs && auxcm) k.bytes(c.aux + L.aux_off, L.cigar_len);
	else if(rs) {
		if(rs->trim5 > 0) { k.num(rs->trim5); k.ch('S'); }
		k.num((int64_t)(uint32_t)(rdlen - rs->trim5 - rs->trim3)); k.ch('M');
		if(rs->trim3 > 0) { k.num(rs->trim3); k.ch('S'); }
	} else k.ch('*');
	k.ch('\t');
	const bool part_of_pair = (L.flag & 1) != 0;
	if(rs && part_of_pair) { if(rso && rs->tidx != rso->tidx) put_ref_name(k, c, rso->tidx); else k.ch('='); }
	else if(L.oref_tidx != -1) k.ch('=');
	else k.ch('*');
	k.ch('\t');
	if(rs && part_of_pair) k.num((int64_t)(rso ? rso->toff : rs->toff) + 1);
	else if(L.oref_tidx != -1) k.num((int64_t)L.oref_toff + 1);
	else k.ch('0');
	k.ch('\t');
	if(L.bits & H2G_SAM_LINE_HAS_TLEN) k.num(L.tlen); else k.ch('0');
	k.ch('\t');
	if((L.bits & H2G_SAM_LINE_STAR_SEQ) || rdlen == 0) H2G_LINE_LIT(k, "*\t*\t");
	else {
		k.seq(c.codes[m] + c.offs[m][i], rdlen, fw); k.ch('\t');
		k.qual(c.quals[m] ? c.quals[m] + c.offs[m][i] : nullptr, rdlen, fw); k.ch('\t');
	}
	if(!rs) { put_yt_yf_rg(k, c, L); k.ch('\n'); k.finish(); return; }
	H2G_LINE_LIT(k, "AS:i:"); k.num(rs->score);
	if(L.bits & H2G_SAM_LINE_HAS_ZS) { H2G_LINE_LIT(k, "\tZS:i:"); k.num(L.zs); }
	H2G_LINE_LIT(k, "\tXN:i:0");
	const uint32_t ne = rs->nedits;
	const h2g_edit* e = edits_of(c, rs);
	uint32_t num_mm = 0, num_go = 0, num_gx = 0, NM = 0;
	for(uint32_t j = 0; j < ne; j++) {
		if(e[j].type == EDIT_SPL) continue;
		if(e[j].snp >= c.nalts) NM++;
		if(e[j].type == EDIT_MM) { if(e[j].snp >= c.nalts) num_mm++; }
		else if(e[j].type == EDIT_READ_GAP) {
			if(e[j].snp >= c.nalts) { num_go++; num_gx++; }
			while(j + 1 < ne && e[j + 1].pos == e[j].pos && e[j + 1].type == EDIT_READ_GAP) { j++; if(e[j].snp >= c.nalts) { num_gx++; NM++; } }
		} else if(e[j].type == EDIT_REF_GAP) {
			if(e[j].snp >= c.nalts) { num_go++; num_gx++; }
			while(j + 1 < ne && e[j + 1].pos == e[j].pos + 1 && e[j + 1].type == EDIT_REF_GAP) { j++; if(e[j].snp >= c.nalts) { num_gx++; NM++; } }
		}
	}
	H2G_LINE_LIT(k, "\tXM:i:"); k.num(num_mm);
	H2G_LINE_LIT(k, "\tXO:i:"); k.num(num_go);
	H2G_LINE_LIT(k, "\tXG:i:"); k.num(num_gx);
	H2G_LINE_LIT(k, "\tNM:i:"); k.num(NM);
	H2G_LINE_LIT(k, "\tMD:Z:");
	if(auxcm) k.bytes(c.aux + L.aux_off + L.cigar_len, L.mdz_len);
	else {	// every edit a mismatch: a run length (0 between two mismatches and at either end), then the reference base
		const uint32_t lt = rdlen - rs->trim5 - rs->trim3;
		uint32_t at = 0;
		for(uint32_t j = 0; j < ne; j++) {
			const h2g_edit& x = e[fw ? j : ne - 1 - j];
			const uint32_t pos = fw ? x.pos : lt - 1 - x.pos;
			if(pos > at) k.num((int64_t)(pos - at)); else k.ch('0');
			k.ch((char)x.chr);
			at = pos + 1;
		}
		if(lt > at) k.num((int64_t)(lt - at)); else k.ch('0');
	}
	if((L.bits & H2G_SAM_LINE_HAS_YS) && rso) { H2G_LINE_LIT(k, "\tYS:i:"); k.num(rso->score); }
	k.ch('\t');
	put_yt_yf_rg(k, c, L);
	if(c.rna_strandness != 0) {
		char strand = '+';
		const int s = c.rna_strandness;
		if(L.bits & H2G_SAM_LINE_SENSE_MATE1) { if(fw) { if(s == 2 || s == 4) strand = '-'; } else if(s == 1 || s == 3) strand = '-'; }
		else { if(fw) { if(s == 3) strand = '-'; } else if(s == 4) strand = '-'; }
		H2G_LINE_LIT(k, "\tXS:A:"); k.ch(strand);
	} else {
		uint32_t sense = 1;
		for(uint32_t j = 0; j < ne; j++) {
			if(e[j].type != EDIT_SPL) continue;
			const uint32_t d = ((uint32_t)e[j].pad >> 4) & 7u;
			if(sense == 1) sense = d;
			else if(d != 1) {
				if((sense == 2 || sense == 4) && d != 2 && d != 4) { sense = 1; break; }
				if((sense == 3 || sense == 5) && d != 3 && d != 5) { sense = 1; break; }
			}
		}
		if(sense != 1) { H2G_LINE_LIT(k, "\tXS:A:"); k.ch((sense == 2 || sense == 4) ? '+' : '-'); }
	}
	H2G_LINE_LIT(k, "\tNH:i:"); k.num((int64_t)L.nh);
	const uint32_t zl = L.aux_len - (auxcm ? (uint32_t)L.cigar_len + L.mdz_len : 0u);
	if(zl) { H2G_LINE_LIT(k, "\tZs:Z:"); k.bytes(c.aux + L.aux_off + (auxcm ? (uint32_t)L.cigar_len + L.mdz_len : 0u), zl); }
	k.ch('\n');
	k.finish();
}

// What a descriptor names in its records, checked where the records are (the host's text call; the sizes kernel on the device): the record and its inline edits end
// inside the mate's bytes, and every reference index is one.  The caller has checked rec_off + 40 <= nrec (h2g_sam_plan_check).
H2G_HD bool record_ok(const Ctx& c, uint32_t m, uint64_t off, bool whole_line) {
	if(off == ~0ull) return true;
	const h2g_alnres* r = reinterpret_cast<const h2g_alnres*>(c.rec[m] + off);
	if(whole_line) return true;                        // (the line is in the pool: the record is not read)
	if(r->nedits > H2G_MAX_EDITS) return false;        // such a record's edits are not inline: only a WHOLE_LINE may name it
	if(off + 40u + 12ull * r->nedits > c.nrec[m]) return false;
	return r->tidx < c.nrefs;
}
H2G_HD bool line_records_ok(const Ctx& c, const h2g_sam_line& L) {
	const bool whole = (L.bits & H2G_SAM_LINE_WHOLE_LINE) != 0;
	return record_ok(c, L.mate, L.rec_off, whole) && record_ok(c, L.mate ^ 1u, L.orec_off, whole);
}

// ---- host side of the text calls (h2g_sam.cpp) ---------------------------------------------------------------------------------
// The host's writer, for the format calls and for h2g_sam_text_from_plan_host: the line goes to the end of a string, in one pass (no sizing pass: the string grows).
// SEQ and QUAL pass through a buffer on the stack, PtrSink's loops filling it, so that the string's new bytes are written once.
struct StrSink {
	std::string& o;
	void ch(char c) { o.push_back(c); }
	void lit(const char* s, uint32_t len) { o.append(s, len); }
	void num(int64_t v) {      // backwards from the end of a buffer: no digit count first
		char b[24];
		int k = 24;
		uint64_t u = v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v;
		do { b[--k] = (char)('0' + u % 10); u /= 10; } while(u);
		if(v < 0) b[--k] = '-';
		o.append(b + k, (size_t)(24 - k));
	}
	void bytes(const char* s, uint64_t len) { o.append(s, (size_t)len); }
	void seq(const uint8_t* c, uint32_t len, bool fw) {
		char b[256];
		for(uint32_t at = 0; at < len; at += 256) { const uint32_t m = len - at < 256 ? len - at : 256; PtrSink k = {b}; k.seq(c + (fw ? at : len - at - m), m, fw); o.append(b, m); }
	}
	void qual(const char* q, uint32_t len, bool fw) {
		if(q && fw) { o.append(q, len); return; }
		if(!q) { o.append(len, 'I'); return; }
		char b[256];
		for(uint32_t at = 0; at < len; at += 256) { const uint32_t m = len - at < 256 ? len - at : 256; PtrSink k = {b}; k.qual(q + (len - at - m), m, false); o.append(b, m); }
	}
	void finish() {}
};
inline void append_line(const Ctx& c, const h2g_sam_line& L, std::string& o) { StrSink k = {o}; emit_line(c, L, k); }
// the per-handle tables a text call needs: rebuilt when uid / gen differ from what the caller holds
struct Tables { uint64_t uid = 0, gen = 0; std::string refnames; std::vector<uint32_t> refname_offs; std::string rg; int32_t rna_strandness = 0; uint32_t nalts = 0; };
void sam_tables_key(const struct ::h2g_sam* S, uint64_t* uid, uint64_t* gen);
void sam_tables(const struct ::h2g_sam* S, Tables& t);
// everything about lines[0 .. n_lines) that needs no record: read < n, mate against the run kind, offsets 8-aligned with a record prefix inside the mate's bytes, pool ranges,
// oref_tidx.  nullptr = fine, else what is wrong (a static text)
const char* plan_check(const h2g_sam_line* lines, size_t n_lines, size_t n_reads, bool paired, uint64_t nrec1, uint64_t nrec2, size_t n_aux, uint32_t nrefs);

}  // namespace h2g_line
#endif
