// h2g_sam_plan.h — the deciding half of append_mate (h2g_sam.cpp) for PLAIN reads and pairs, as code that the host and the kernels share: it makes the h2g_sam_line
// descriptors (include/h2g.h) that h2g_sam_plan_*_compact makes, field for field, for the reads whose lines are closed-form functions of their result header and their
// one or two records.  Every other read is HANDED ON to the host planner, which stays in one copy (selection with draws, the MAPQ ladder, left-alignment, Zs:Z, the
// splice-site database in TLEN, add_splice_sites).  The leaves both planners need (hisat2_score / score_of, sam_flag, the ends of a fragment, the read filters) live here
// and h2g_sam.cpp calls them.  Neither planner writes text: a descriptor becomes bytes in the emitter of h2g_sam_line.h alone, in the kernels or, for the host's format
// calls, right where append_mate has filled it.
//
// The predicate "plain" (stated here once; tests/sam_split_util.py restates it independently):
//   A record PARSES when its 40-byte prefix and its inline edits lie inside its read's bytes [boffs[i], boffs[i + 1]) and it is no pair trailer.  A read's bytes parse when
//   they are whole records back to back up to their end.  Bytes that do not parse are handed on, never followed.
//   A record is DEVICE-PLANNABLE when nedits <= H2G_MAX_EDITS, every inline edit is EDIT_MM with snp >= nalts (no gap, no splice, no ALT edit: no pool bytes, no Zs:Z,
//   nothing for add_splice_sites), and tidx is a reference of the index.
//   Unpaired read i is plain when nselect <= 1, its record (if any) is device-plannable, and it is not the case that secbest is valid and equals best in score and h2
//   (the MAPQ ladder's case; anything else is MAPQ 60).
//   Pair i: walk both mates' bytes as compact_walk does -> n1, n2.  A pair trailer (H2G_PAIR_TRAILER_TAG) makes the pair not plain.  The pairings are filtered by
//   pair_i < n1 && pair_j < n2 -> np.  The pair is plain when every record it prints or reads is device-plannable and it is one of
//     (a) unique concordant: np == 1; with a non-empty splice-site database and template-length adjustment on, the mates must not satisfy up_right + 100 < dn_left (the
//         one case in which fragment_length consults the database); ZS:i per mate comes from every record of the mate, which are only scored: none may have
//         nedits > H2G_MAX_EDITS;
//     (b) discordant: np == 0, report_discordant, n1 == 1 && n2 == 1;
//     (c) neither: np == 0 otherwise, and with u_m = report_mixed ? n_m : 0, u1 <= 1 && u2 <= 1 (both unaligned / one mate aligned / both aligned as unpaired mates).
//   With one key select_by_score draws nothing: rnd_state is never read for a plain pair.
//   Two deliberate tightenings beyond that statement, both on the safe side (more is handed on, never less): a record whose tidx is not a reference of the index is not
//   plannable — an unaligned mate's line names its partner's reference, which nothing downstream checks on the device —, and a trailer tag among MATE 2's records hands
//   the pair on as well, although the host's walk merely stops there (no fetch writes one; such bytes are damaged).
//   Everything else is handed on: np >= 2, more than one unpaired record per mate, gapped / spliced / ALT / long records, tied best scores, the database TLEN case, trailers.
#ifndef H2G_SAM_PLAN_H_
#define H2G_SAM_PLAN_H_
#include "h2g_core.h"
#include "h2g_sam_line.h"

namespace h2g_plan {

enum { PAIR_CONCORD_M1 = 1, PAIR_CONCORD_M2, PAIR_DISCORD_M1, PAIR_DISCORD_M2, PAIR_UNP_M1, PAIR_UNP_M2, PAIR_UNPAIRED };   // aligner_result.h:404-412

struct Score {        // AlnScore (aligner_result.h:44-330): score, then hisat2_score (fewer trimmed bases wins)
	bool valid = false;
	int64_t score = 0, h2 = 0;
	H2G_HD bool gt(const Score& o) const { if(!o.valid) return valid; if(!valid) return false; return score > o.score || (score == o.score && h2 > o.h2); }
	H2G_HD bool eq(const Score& o) const { return valid && o.valid && score == o.score && h2 == o.h2; }
};
// AlnScore::calculate_hisat2_score aligner_result.h:322-350: score, repeat (never), transcript (1 = spliced: near splice sites,
// reportHit hi_aligner.h:6100-6143), splice score (mean intron length of the short-anchored splices / 100), trimmed bases
H2G_HD int64_t hisat2_score(int64_t sc, uint32_t trim, int transcript = 0, uint32_t splicescore = 0) {
	if(sc > INT32_MAX) sc = INT32_MAX; else if(sc < INT32_MIN) sc = INT32_MIN;
	const int64_t t = trim > 0xFFFF ? 0 : 0xFFFF - (int64_t)trim;
	int64_t spl = (int64_t)splicescore / 100;
	spl = spl > 255 ? 0 : 255 - spl;
	return (int64_t)(((uint64_t)sc << 32) | ((uint64_t)transcript << 24) | ((uint64_t)spl << 16) | (uint64_t)t);
}
// `ed`: the record's nedits edits (inline, or from the long-edit area on the host)
H2G_HD Score score_of(const h2g_alnres& r, const h2g_edit* ed) {
	Score s; s.valid = true; s.score = r.score;
	int transcript = 0;                  // 2: every splice is a database site, 1: spliced (GenomeHit::spliced hi_aligner.h:1086)
	if(r.fw & H2G_FW_TCLASS) transcript = (int)((r.fw >> H2G_FW_TCLASS_SHIFT) & 3u);   // the class reportHit gave it (--avoid-pseudogene / --tmo)
	else {
		bool all_known = true;
		for(uint32_t i = 0; i < r.nedits; i++) if(ed[i].type == h2g_line::EDIT_SPL) { transcript = 1; all_known = all_known && (ed[i].pad >> 7) != 0; }
		if(transcript && all_known) transcript = 2;
	}
	s.h2 = hisat2_score(r.score, r.trim5 + r.trim3, transcript, r.splicescore);
	return s;
}
H2G_HD Score add(const Score& a, const Score& b) { Score s; s.valid = a.valid; s.score = a.score + b.score; s.h2 = a.h2 + b.h2; return s; }
// the rs1u_ / rs2u_ loop of AlnSetSumm::init, one record at a time
H2G_HD void summ_step(Score& best, Score& secbest, const Score& sc) {
	const bool g1 = sc.gt(best), g2 = !g1 && sc.gt(secbest);      // (field by field: a lane keeps both in registers)
	const Score ob = best;
	secbest.valid = g1 ? ob.valid : g2 ? sc.valid : secbest.valid; secbest.score = g1 ? ob.score : g2 ? sc.score : secbest.score; secbest.h2 = g1 ? ob.h2 : g2 ? sc.h2 : secbest.h2;
	best.valid = g1 ? sc.valid : ob.valid; best.score = g1 ? sc.score : ob.score; best.h2 = g1 ? sc.h2 : ob.h2;
}

struct Flags {        // AlnFlags (aligner_result.h:414-640); the filters are "passed" bits
	int  pairing = PAIR_UNPAIRED;
	bool primary = true, oppAligned = false, oppFw = true, nfilt = true, lenfilt = true, qcfilt = true;
	H2G_HD bool partOfPair() const { return pairing < PAIR_UNPAIRED; }
	H2G_HD bool concordant() const { return pairing == PAIR_CONCORD_M1 || pairing == PAIR_CONCORD_M2; }
	H2G_HD bool discordant() const { return pairing == PAIR_DISCORD_M1 || pairing == PAIR_DISCORD_M2; }
	H2G_HD bool unpairedMate() const { return pairing == PAIR_UNP_M1 || pairing == PAIR_UNP_M2; }
	H2G_HD bool readMate1() const { return pairing == PAIR_CONCORD_M1 || pairing == PAIR_DISCORD_M1 || pairing == PAIR_UNP_M1; }
};
// FLAG of a line (aln_sink.h:3060-3100)
H2G_HD int sam_flag(const Flags& fl, const h2g_alnres* rs, const h2g_alnres* rso) {
	int f = 0;
	if(fl.partOfPair()) {
		f |= 1;
		if(fl.concordant()) f |= 2;
		if(!fl.oppAligned) f |= 8;
		f |= fl.readMate1() ? 0x40 : 0x80;
		if(fl.oppAligned && rso != nullptr && !(rso->fw & H2G_FW_STRAND)) f |= 0x20;
	}
	if(!fl.primary) f |= 0x100;
	if(rs && !(rs->fw & H2G_FW_STRAND)) f |= 0x10;
	if(!rs) f |= 4;
	return f;
}

// AlnRes::setFragmentLength aligner_result.h:1631-1697 up to where the splice-site database comes in; trims extend both ends (getExtendedCoords :1156).  rfextent_ does not
// count introns (calcRefExtent :1880) while refcoord_right() does (:1256), so each alignment has two (start, end) pairs — (st, en) anchored at its left end, (st2, en2) at
// its right end — and the upstream mate enters with the right-anchored pair: introns inside the mates do not count towards TLEN.
struct FragEnds { int64_t up, dn, up_right, dn_left; bool imUpstream; };
H2G_HD void frag_coords(const h2g_alnres& r, const h2g_edit* ed, int64_t& st, int64_t& en, int64_t& st2, int64_t& en2) {
	int64_t ext = r.len, spl = 0;
	for(uint32_t i = 0; i < r.nedits; i++) {
		if(ed[i].type == h2g_line::EDIT_REF_GAP) ext--; else if(ed[i].type == h2g_line::EDIT_READ_GAP) ext++;
		else if(ed[i].type == h2g_line::EDIT_SPL) spl += (int64_t)((uint32_t)ed[i].chr | ((uint32_t)ed[i].qchr << 8) | (((uint32_t)ed[i].pad & 15u) << 16));
	}
	st = (int64_t)r.toff - r.trim5; en = (int64_t)r.toff + ext - 1 + r.trim3;
	st2 = st + spl; en2 = en + spl;
}
H2G_HD FragEnds fragment_ends(const h2g_alnres& me, const h2g_edit* edme, const h2g_alnres& o, const h2g_edit* edo, bool meMate1) {
	int64_t st, en, st2, en2, ost, oen, ost2, oen2;
	frag_coords(me, edme, st, en, st2, en2);
	frag_coords(o, edo, ost, oen, ost2, oen2);
	const bool mfw = (me.fw & H2G_FW_STRAND) != 0, ofw = (o.fw & H2G_FW_STRAND) != 0;
	FragEnds f;
	if(st < ost) f.imUpstream = true;
	else if(st == ost) {
		if(mfw && ofw && meMate1) f.imUpstream = true;
		else if(mfw && !ofw) f.imUpstream = true;
		else f.imUpstream = false;
	} else f.imUpstream = false;
	const bool u = f.imUpstream;
	f.up = u ? (st2 < ost ? st2 : ost) : (st < ost2 ? st : ost2);
	f.dn = u ? (en2 > oen ? en2 : oen) : (en > oen2 ? en : oen2);
	f.up_right = u ? (en2 < oen ? en2 : oen) : (en < oen2 ? en : oen2);
	f.dn_left = u ? (st2 > ost ? st2 : ost) : (st > ost2 ? st : ost2);
	return f;
}
// TLEN from the ends and the longest database intron between the mates (0 without a database)
H2G_HD int64_t fragment_length_of(const FragEnds& f, int64_t intron_len) { const int64_t fl = 1 + f.dn - f.up - intron_len; return f.imUpstream ? fl : -fl; }

// Scoring::nFilter / length filter as the worker applies them (hisat2.cpp:3404-3440): which YF:Z flag an unaligned read gets
H2G_HD void read_filters(uint32_t ncType, double ncConst, double ncCoeff, const uint8_t* codes, uint32_t len, bool* lenfilt, bool* nfilt) {
	*lenfilt = len >= 2;                     // rdlens <= multiseedMms(0) || < 2  => filtered
	uint32_t ns = 0;
	for(uint32_t i = 0; i < len; i++) ns += codes[i] > 3;
	*nfilt = h2g::nceil_pass(ncType, ncConst, ncCoeff, len, ns);   // the device's filter (h2g_core.h)
}

// ---- the plain planner ------------------------------------------------------------------------------------------------------------------------
// the handle's small state
struct Opts { double ncConst, ncCoeff; uint32_t ncType, nalts, nrefs; uint8_t no_unal, report_discordant, report_mixed, db_tlen /* a database exists and TLEN adjustment is on */; };
// What a planner reads: host pointers on the host, device pointers in the kernels.  Reads and qualities count from `first` (the resident batch); res, boffs and qc count
// from the call's read 0.  boffs are byte offsets into rec (n + 1 entries per mate); qc: the handle's filter bytes for the range, or nullptr
struct In {
	const uint8_t* codes[2]; const uint32_t* offs[2];
	const uint8_t* qc[2];
	const uint8_t* rec[2]; const uint64_t* boffs[2]; uint64_t nrec[2];
	uint32_t first;
};
// the result header of an unpaired read, whichever struct carries it (h2g_read_result on the host, the kernels' row on the device)
struct UnpHead { uint32_t nselect; int32_t best, secbest; uint32_t best_h2, secbest_h2; };

// class codes: 0 = handed on
enum { CLS_HOST = 0, CLS_U_UNAL = 1, CLS_U_UNIQ = 2, CLS_P_CONC = 3, CLS_P_DISC = 4, CLS_P_NONE = 5, CLS_P_MATE1 = 6, CLS_P_MATE2 = 7, CLS_P_BOTH = 8 };
// lines a plain read of class c prints
H2G_HD uint32_t lines_of_class(uint32_t c, bool no_unal) {
	switch(c) {
		case CLS_U_UNAL: return no_unal ? 0u : 1u;
		case CLS_U_UNIQ: return 1u;
		case CLS_P_CONC: case CLS_P_DISC: case CLS_P_BOTH: return 2u;
		case CLS_P_NONE: return no_unal ? 0u : 2u;
		case CLS_P_MATE1: case CLS_P_MATE2: return no_unal ? 1u : 2u;
		default: return 0u;
	}
}

H2G_HD bool plannable(const h2g_alnres& r, const Opts& O) {
	if(r.nedits > H2G_MAX_EDITS || r.tidx >= O.nrefs) return false;
	for(uint32_t k = 0; k < r.nedits; k++) if(r.edits[k].type != h2g_line::EDIT_MM || r.edits[k].snp < O.nalts) return false;
	return true;
}
// the bytes [b, e) of one read, clipped to the mate's bytes
H2G_HD bool read_bytes(const In& in, uint32_t m, uint32_t i, uint64_t& b, uint64_t& e) {
	b = in.boffs[m][i]; e = in.boffs[m][i + 1];
	return b <= e && e <= in.nrec[m] && (b & 7u) == 0;
}
// one walk over a mate's bytes: the count, whether they parse, the summary over every record, and where record `track` starts
struct Walk { uint32_t n; bool ok, trailer, scorable; Score best, secbest; uint64_t off_t; };
H2G_HD Walk walk_mate(const uint8_t* rec, uint64_t b, uint64_t e, uint32_t track) {
	Walk w; w.n = 0; w.ok = true; w.trailer = false; w.scorable = true; w.off_t = ~0ull;
	uint64_t p = b;
	while(p + 40 <= e) {
		const h2g_alnres* r = reinterpret_cast<const h2g_alnres*>(rec + p);
		if(r->nedits == H2G_PAIR_TRAILER_TAG) { w.trailer = true; break; }
		const uint64_t bytes = H2G_COMPACT_BYTES(r->nedits);
		if(p + bytes > e) { w.ok = false; break; }
		if(r->nedits > H2G_MAX_EDITS) w.scorable = false;
		else summ_step(w.best, w.secbest, score_of(*r, r->edits));
		if(w.n == track) w.off_t = p;
		w.n++; p += bytes;
	}
	if(!w.trailer && p != e) w.ok = false;
	return w;
}
// where record idx of bytes that parse starts (the rare pairing that is not the first listed)
H2G_HD uint64_t find_record(const uint8_t* rec, uint64_t b, uint64_t e, uint32_t idx) {
	uint64_t p = b;
	for(uint32_t k = 0; p + 40 <= e; k++) {
		const h2g_alnres* r = reinterpret_cast<const h2g_alnres*>(rec + p);
		if(r->nedits == H2G_PAIR_TRAILER_TAG) break;
		if(k == idx) return p;
		p += H2G_COMPACT_BYTES(r->nedits);
	}
	return ~0ull;
}

// what classification found and planning needs: where the record each mate prints starts (~0: none), and each mate's second-best score (ZS:i).  Scalars only: a
// lane keeps no array
struct Pick { uint64_t off0, off1; Score sec0, sec1; };
H2G_HD const h2g_alnres* rec_ptr(const uint8_t* rec, uint64_t off) { return off == ~0ull ? nullptr : reinterpret_cast<const h2g_alnres*>(rec + off); }
H2G_HD uint64_t record_of(const uint8_t* rec, uint64_t b, uint64_t e, const Walk& w, uint32_t track, uint32_t idx) { return idx == track ? w.off_t : find_record(rec, b, e, idx); }
H2G_HD bool plannable_at(const uint8_t* rec, uint64_t off, const Opts& O) { return off != ~0ull && plannable(*reinterpret_cast<const h2g_alnres*>(rec + off), O); }

H2G_HD uint32_t classify_unpaired(const Opts& O, const In& in, const UnpHead& h, uint32_t i, Pick* pk) {
	pk->off0 = pk->off1 = ~0ull; pk->sec0 = pk->sec1 = Score();
	if(h.nselect > 1) return CLS_HOST;
	if(h.secbest != INT32_MIN && h.best != INT32_MIN && h.best == h.secbest && h.best_h2 == h.secbest_h2) return CLS_HOST;
	if(h.secbest != INT32_MIN) { pk->sec0.valid = true; pk->sec0.score = h.secbest; }
	if(h.nselect == 0) return CLS_U_UNAL;
	uint64_t b, e;
	if(!read_bytes(in, 0, i, b, e) || b + 40 > e) return CLS_HOST;
	const h2g_alnres* r = reinterpret_cast<const h2g_alnres*>(in.rec[0] + b);
	if(r->nedits == H2G_PAIR_TRAILER_TAG || r->nedits > H2G_MAX_EDITS || b + H2G_COMPACT_BYTES(r->nedits) > e || !plannable(*r, O)) return CLS_HOST;
	pk->off0 = b;
	return CLS_U_UNIQ;
}

H2G_HD uint32_t classify_pair(const Opts& O, const In& in, const h2g_pair_result& pr, uint32_t i, Pick* pk) {
	pk->off0 = pk->off1 = ~0ull; pk->sec0 = pk->sec1 = Score();
	uint64_t b0, e0, b1, e1;
	if(!read_bytes(in, 0, i, b0, e0) || !read_bytes(in, 1, i, b1, e1)) return CLS_HOST;
	const uint32_t lim = pr.npairs < H2G_PAIR_CAP ? pr.npairs : H2G_PAIR_CAP;
	const uint32_t t0 = lim ? pr.pair_i[0] : 0u, t1 = lim ? pr.pair_j[0] : 0u;
	const Walk w0 = walk_mate(in.rec[0], b0, e0, t0), w1 = walk_mate(in.rec[1], b1, e1, t1);
	if(!w0.ok || !w1.ok || w0.trailer || w1.trailer) return CLS_HOST;
	uint32_t np = 0, pa = 0, pb = 0;
	for(uint32_t k = 0; k < lim; k++) if(pr.pair_i[k] < w0.n && pr.pair_j[k] < w1.n) { if(np == 0) { pa = pr.pair_i[k]; pb = pr.pair_j[k]; } np++; }
	if(np >= 2) return CLS_HOST;
	if(np == 1) {
		if(!w0.scorable || !w1.scorable) return CLS_HOST;
		const uint64_t oa = record_of(in.rec[0], b0, e0, w0, t0, pa), ob = record_of(in.rec[1], b1, e1, w1, t1, pb);
		if(!plannable_at(in.rec[0], oa, O) || !plannable_at(in.rec[1], ob, O)) return CLS_HOST;
		if(O.db_tlen) {   // both records hold mismatches only: their ends are toff - trim5 and toff + len - 1 + trim3 (frag_coords without gaps or introns), whichever mate is upstream
			const h2g_alnres* ra = rec_ptr(in.rec[0], oa);
			const h2g_alnres* rb = rec_ptr(in.rec[1], ob);
			const int64_t sa = (int64_t)ra->toff - ra->trim5, ea = (int64_t)ra->toff + ra->len - 1 + ra->trim3;
			const int64_t sb = (int64_t)rb->toff - rb->trim5, eb = (int64_t)rb->toff + rb->len - 1 + rb->trim3;
			const int64_t up_right = ea < eb ? ea : eb, dn_left = sa > sb ? sa : sb;
			if(up_right + 100 < dn_left) return CLS_HOST;
		}
		pk->off0 = oa; pk->off1 = ob; pk->sec0 = w0.secbest; pk->sec1 = w1.secbest;
		return CLS_P_CONC;
	}
	if(O.report_discordant && w0.n == 1 && w1.n == 1) {
		const uint64_t oa = record_of(in.rec[0], b0, e0, w0, t0, 0), ob = record_of(in.rec[1], b1, e1, w1, t1, 0);
		if(!plannable_at(in.rec[0], oa, O) || !plannable_at(in.rec[1], ob, O)) return CLS_HOST;
		pk->off0 = oa; pk->off1 = ob;
		return CLS_P_DISC;
	}
	const uint32_t u0 = O.report_mixed ? w0.n : 0u, u1 = O.report_mixed ? w1.n : 0u;
	if(u0 > 1 || u1 > 1) return CLS_HOST;
	if(u0) { pk->off0 = record_of(in.rec[0], b0, e0, w0, t0, 0); if(!plannable_at(in.rec[0], pk->off0, O)) return CLS_HOST; }
	if(u1) { pk->off1 = record_of(in.rec[1], b1, e1, w1, t1, 0); if(!plannable_at(in.rec[1], pk->off1, O)) return CLS_HOST; }
	return u0 && u1 ? CLS_P_BOTH : u0 ? CLS_P_MATE1 : u1 ? CLS_P_MATE2 : CLS_P_NONE;
}

// One descriptor, as append_mate fills it for a record without pool bytes (or for no record).  aux_off is left 0: the merge sets it.
struct LineIn {
	uint32_t read, rdlen, nh;
	const h2g_alnres* rs; const h2g_alnres* rso; uint64_t rec_off, orec_off;
	Flags fl; bool summ_paired; Score sco;
	int64_t orefid, orefoff;
};
// a whole descriptor to its slot: four 16-byte stores per lane in the kernels
H2G_HD void put_line(h2g_sam_line* dst, const h2g_sam_line& d) {
#if defined(__HIP_DEVICE_COMPILE__)
	static_assert(sizeof(h2g_sam_line) == 64, "four 16-byte words");
	uint4* t = reinterpret_cast<uint4*>(dst);          // (the layout: include/h2g.h; h2g_sam.cpp asserts the offsets)
	t[0] = make_uint4(d.read, d.nh, (uint32_t)d.rec_off, (uint32_t)(d.rec_off >> 32));
	t[1] = make_uint4((uint32_t)d.orec_off, (uint32_t)(d.orec_off >> 32), (uint32_t)(uint64_t)d.tlen, (uint32_t)((uint64_t)d.tlen >> 32));
	t[2] = make_uint4((uint32_t)d.zs, (uint32_t)d.oref_tidx, d.oref_toff, d.aux_off);
	t[3] = make_uint4(d.aux_len, (uint32_t)d.flag | ((uint32_t)d.cigar_len << 16), (uint32_t)d.mdz_len | ((uint32_t)d.mapq << 16) | ((uint32_t)d.mate << 24),
	                  (uint32_t)d.yt | ((uint32_t)d.yf << 8) | ((uint32_t)d.bits << 16));
#else
	*dst = d;
#endif
}
H2G_HD void make_line(const LineIn& x, h2g_sam_line* out) {
	h2g_sam_line d = h2g_sam_line();
	const Flags& fl = x.fl;
	const h2g_alnres* rs = x.rs; const h2g_alnres* rso = x.rso;
	const bool mate1 = fl.pairing == PAIR_UNPAIRED || fl.readMate1();
	const bool has_tlen = rs && rso && x.summ_paired && (rs->tidx == rso->tidx || fl.concordant());
	const bool star_seq = x.rdlen == 0;                                  // (every plain line is primary: --omit-sec-seq never applies)
	d.read = x.read; d.nh = x.nh;
	d.rec_off = rs ? x.rec_off : ~0ull; d.orec_off = rso ? x.orec_off : ~0ull;
	d.tlen = has_tlen ? fragment_length_of(fragment_ends(*rs, rs->edits, *rso, rso->edits, fl.readMate1()), 0) : 0;
	d.zs = rs && x.sco.valid ? (int32_t)x.sco.score : 0;
	d.oref_tidx = (int32_t)x.orefid; d.oref_toff = x.orefid != -1 ? (uint32_t)x.orefoff : 0;
	d.flag = (uint16_t)sam_flag(fl, rs, rso); d.mapq = rs ? 60 : 0; d.mate = mate1 ? 0 : 1;
	d.yt = (uint8_t)(fl.concordant() ? 1 : fl.discordant() ? 2 : fl.unpairedMate() ? 3 : 0);
	d.yf = (uint8_t)(!fl.lenfilt ? 1 : !fl.nfilt ? 2 : !fl.qcfilt ? 3 : 0);
	d.bits = (uint16_t)((rs && x.sco.valid ? H2G_SAM_LINE_HAS_ZS : 0) | (rs && x.summ_paired && rso ? H2G_SAM_LINE_HAS_YS : 0) | (has_tlen ? H2G_SAM_LINE_HAS_TLEN : 0) |
	                    (star_seq ? H2G_SAM_LINE_STAR_SEQ : 0) | (fl.partOfPair() ? H2G_SAM_LINE_STRIP_MATE_SUFFIX : 0) | (mate1 ? H2G_SAM_LINE_SENSE_MATE1 : 0));
	put_line(out, d);
}
H2G_HD uint32_t read_len(const In& in, uint32_t m, uint32_t i) { return in.offs[m][in.first + i + 1] - in.offs[m][in.first + i]; }
H2G_HD void mate_filters(const Opts& O, const In& in, uint32_t m, uint32_t i, Flags& fl) {
	read_filters(O.ncType, O.ncConst, O.ncCoeff, in.codes[m] + in.offs[m][in.first + i], read_len(in, m, i), &fl.lenfilt, &fl.nfilt);
	fl.qcfilt = !in.qc[m] || in.qc[m][i] != 0;
}

// the lines of a plain unpaired read of class c -> out[0 .. return)
H2G_HD uint32_t plan_plain_unpaired(const Opts& O, const In& in, uint32_t c, const Pick& pk, uint32_t i, h2g_sam_line* out) {
	if(c == CLS_U_UNAL && O.no_unal) return 0;
	LineIn x;
	x.read = i; x.rdlen = read_len(in, 0, i); x.nh = c == CLS_U_UNIQ ? 1u : 0u;
	x.rs = c == CLS_U_UNIQ ? rec_ptr(in.rec[0], pk.off0) : nullptr; x.rso = nullptr; x.rec_off = pk.off0; x.orec_off = ~0ull;
	x.fl = Flags(); mate_filters(O, in, 0, i, x.fl);
	x.summ_paired = false; x.sco = pk.sec0; x.orefid = -1; x.orefoff = -1;
	make_line(x, out);
	return 1;
}
// one mate's line of a plain pair (0 lines: an unaligned mate under --no-unal).  oref: the aligned mate an unaligned line is placed at
H2G_HD uint32_t pair_mate_line(const Opts& O, uint32_t i, uint32_t rdlen, const h2g_alnres* rs, const h2g_alnres* rso, uint64_t off, uint64_t ooff, const Flags& fl, bool summ_paired,
                               const Score& sco, const h2g_alnres* oref, h2g_sam_line* out) {
	if(!rs && O.no_unal) return 0;
	LineIn x;
	x.read = i; x.rdlen = rdlen; x.nh = rs ? 1u : 0u; x.rs = rs; x.rso = rso; x.rec_off = off; x.orec_off = ooff; x.fl = fl; x.summ_paired = summ_paired; x.sco = sco;
	x.orefid = oref ? (int64_t)oref->tidx : -1; x.orefoff = oref ? (int64_t)oref->toff : -1;
	make_line(x, out);
	return 1;
}
// the lines of a plain pair of class c -> out[0 .. return)
H2G_HD uint32_t plan_plain_pair(const Opts& O, const In& in, uint32_t c, const Pick& pk, uint32_t i, h2g_sam_line* out) {
	const h2g_alnres* r0 = rec_ptr(in.rec[0], pk.off0);
	const h2g_alnres* r1 = rec_ptr(in.rec[1], pk.off1);
	const uint32_t len0 = read_len(in, 0, i), len1 = read_len(in, 1, i);
	Flags f0, f1;
	mate_filters(O, in, 0, i, f0); mate_filters(O, in, 1, i, f1);
	if(c == CLS_P_CONC || c == CLS_P_DISC || c == CLS_P_BOTH) {
		f0.pairing = c == CLS_P_CONC ? PAIR_CONCORD_M1 : c == CLS_P_DISC ? PAIR_DISCORD_M1 : PAIR_UNP_M1;
		f1.pairing = c == CLS_P_CONC ? PAIR_CONCORD_M2 : c == CLS_P_DISC ? PAIR_DISCORD_M2 : PAIR_UNP_M2;
		f0.oppAligned = f1.oppAligned = true;
		const bool sp = c != CLS_P_BOTH;                                   // (mates aligned as unpaired mates: the summary is not a pair's)
		pair_mate_line(O, i, len0, r0, r1, pk.off0, pk.off1, f0, sp, c == CLS_P_CONC ? pk.sec0 : Score(), nullptr, out);
		pair_mate_line(O, i, len1, r1, r0, pk.off1, pk.off0, f1, sp, c == CLS_P_CONC ? pk.sec1 : Score(), nullptr, out + 1);
		return 2;
	}
	f0.pairing = PAIR_UNP_M1; f1.pairing = PAIR_UNP_M2;
	f0.oppAligned = r1 != nullptr; f1.oppAligned = r0 != nullptr;
	// the aligned mate's line first, then the other mate's unaligned line placed at it (g_.reportUnaligned); neither aligned: mate 1, mate 2
	uint32_t n;
	if(c == CLS_P_MATE2) {
		n = pair_mate_line(O, i, len1, r1, nullptr, pk.off1, ~0ull, f1, false, Score(), nullptr, out);
		n += pair_mate_line(O, i, len0, nullptr, nullptr, ~0ull, ~0ull, f0, false, Score(), r1, out + n);
	} else {
		n = pair_mate_line(O, i, len0, r0, nullptr, pk.off0, ~0ull, f0, false, Score(), nullptr, out);
		n += pair_mate_line(O, i, len1, nullptr, nullptr, ~0ull, ~0ull, f1, false, Score(), r0, out + n);
	}
	return n;
}

}  // namespace h2g_plan

// ---- host side (h2g_sam.cpp), called by the text calls of h2g_kernels.hip -----------------------------------------------------------------------
namespace h2g_plan {
struct HostSets { const uint8_t* codes[2]; const uint32_t* offs[2]; const char* quals[2]; const char* names[2]; const uint32_t* noffs[2]; };
struct HostPart;                                       // what the host planner counted for its subset, held back until the text is delivered
// the handle's small state and its filter bytes (nullptr = none)
void sam_plan_opts(const struct ::h2g_sam* S, Opts& o, const uint8_t** qc1, const uint8_t** qc2);
// the host planner over reads idx[0 .. nidx) (ascending) of a compact fetch: their descriptors (read = the read's own index, pool offsets into `aux`), the pool in read order
// and lines emitted up to and including each.  Nothing is counted into the handle: *part holds it.  res: h2g_pair_result[n] (paired) or h2g_read_result[n].
h2g_status plan_subset(const struct ::h2g_sam* S, bool paired, const HostSets& rd, size_t n, const void* res, const uint8_t* rec1, const uint64_t* boffs1, const uint8_t* rec2,
                       const uint64_t* boffs2, uint32_t khits, const uint32_t* idx, size_t nidx, std::vector<h2g_sam_line>& lines, std::string& aux, std::vector<uint64_t>& ends, HostPart** part);
// the text was delivered: count the subset and the plain reads of classes[0 .. n) into the handle (part may be nullptr: nothing was handed on); frees part
void plan_commit(const struct ::h2g_sam* S, HostPart* part, const uint8_t* classes, size_t n);
void plan_discard(HostPart* part);
}  // namespace h2g_plan
#endif
