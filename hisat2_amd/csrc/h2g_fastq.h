// h2g_fastq.h — the record arithmetic of FASTQ parsing on the device (include/h2g.h, h2g_set_reads_fastq): which newlines a 16-byte chunk of the text holds, what a
// DEVICE-PARSABLE ("plain") record is and what it yields in closed form, and which text byte an output byte is a copy of.  The same functions run in the kernels
// (h2g_kernels.hip) and, lane by lane, in the stand-alone checker tests/fastq/fq_check.cpp, which compares them with the command line's host parser
// (Reader::parse_record, h2g_cli_reads.h; reference pat.cpp:725-1010) and is built with the host sanitizers.  Nothing here touches memory it is not handed.
//
// A record is four lines, cut at every fourth '\n'.  It is plain when
//   line 0 starts with '@' and its name (the rest, less one trailing '\r') is not empty (the host names such a record by its running number);
//   line 1, less one trailing '\r', holds only '.' and letters: every one is a base, so the read's untrimmed length Lraw is the line's length (the host skips every
//           other character; such a record is handed on);
//   line 2 starts with '+';
//   line 3's quality characters — up to the first '\r' or the line's end — hold no blank, and their count nq satisfies Lraw <= nq <= Lraw + 1;
//   under phred64 every quality character that is kept (those of the trimmed read) is in [64, 128).
// Every record the host would end the run on is not plain, so the host's messages stay the host's.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#ifndef H2G_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define H2G_HD __host__ __device__ __forceinline__
#else
#define H2G_HD inline
#endif
#endif

namespace h2g_fq {

struct Opts { uint32_t trim5, trim3, phred64; };

// ---- newlines of a 16-byte chunk: the four words of one dwordx4 load, of which the first m bytes belong to the text
// 0x80 in every byte of w that is '\n' (exact: no carry crosses a byte)
H2G_HD uint32_t nl_bits(uint32_t w) {
	const uint32_t x = w ^ 0x0a0a0a0au;
	return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
}
// one bit per byte of the chunk (bit k = byte k is '\n'), bytes at and past m masked off
H2G_HD uint32_t nl_mask16(const uint32_t w[4], uint32_t m) {
	uint32_t mask = 0;
	for(uint32_t j = 0; j < 4; j++) {
		const uint32_t b = nl_bits(w[j]);
		mask |= (((b >> 7) & 1u) | ((b >> 14) & 2u) | ((b >> 21) & 4u) | ((b >> 28) & 8u)) << (4 * j);
	}
	return m >= 16 ? mask : mask & ((1u << m) - 1u);
}
H2G_HD uint32_t popc16(uint32_t m) { uint32_t c = 0; for(; m; m &= m - 1) c++; return c; }

// ---- how many records a text holds.  n_nl: its newlines.  Whole records are n_nl / 4.  When the text ends the input (final), whatever follows them — n_nl is no
// multiple of 4, or the last byte is no '\n' — is one more record: a fourth line without '\n' (complete), or fewer than four lines (never plain: the host decides
// what it is).
H2G_HD uint64_t whole_records(uint64_t n_nl) { return n_nl / 4; }

// The line ends of record r: e[k] = index of the '\n' that ends line k, n_text where the text ends first.  nlpos[j] = index of newline j, for j < n_nl_known.
struct Lines { uint32_t s, e[4]; bool four; };
H2G_HD Lines record_lines(const uint32_t* nlpos, uint64_t n_nl_known, uint32_t n_text, uint64_t r) {
	Lines l;
	l.s = r == 0 ? 0u : nlpos[4 * r - 1] + 1u;
	l.four = true;
	for(uint32_t k = 0; k < 4; k++) {
		const uint64_t j = 4 * r + k;
		if(j < n_nl_known) l.e[k] = nlpos[j];
		else { l.e[k] = n_text; if(k < 3) l.four = false; }      // (a fourth line may end with the text; an earlier one may not)
	}
	return l;
}

H2G_HD bool is_fq_base(unsigned char c) { const unsigned char d = (unsigned char)(c | 0x20); return c == '.' || (d >= 'a' && d <= 'z'); }
// base_code of h2g_cli_reads.h over the FASTQ table: '.' and n / N are N = 4, c g t 1 2 3, every other letter A = 0
H2G_HD uint8_t fq_code(unsigned char c) {
	switch(c | 0x20) { case 'c': return 1; case 'g': return 2; case 't': return 3; case 'n': case '.': return 4; }      // ('.' | 0x20 == '.')
	return 0;
}
H2G_HD char fq_qual(unsigned char c, uint32_t phred64) { return (char)(phred64 ? c - 31 : c); }

// ---- four characters at a time.  The text starts at an address that is a multiple of 4 and is readable up to the next multiple of 4 past its end (the library's
// buffer and the checker's are); the aligned word `wi` holds bytes 4 wi .. 4 wi + 3, byte k in bits 8 k.
// 0x80 in every byte of x that is 0 (exact: no carry crosses a byte)
H2G_HD uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
// word wi of the text with the bytes outside [b, e) replaced by those of `fill`
H2G_HD uint32_t word_of(const char* t, uint32_t wi, uint32_t b, uint32_t e, uint32_t fill) {
	uint32_t w;
	memcpy(&w, __builtin_assume_aligned(t + 4 * (size_t)wi, 4), 4);
	const uint32_t lo = 4 * wi;
	uint32_t keep = 0xffffffffu;
	if(b > lo) keep &= 0xffffffffu << (8 * (b - lo));
	if(e < lo + 4) keep &= 0xffffffffu >> (8 * (lo + 4 - e));
	return (w & keep) | (fill & ~keep);
}
// every byte of w is '.' or a letter (is_fq_base)
H2G_HD bool all_fq_bases(uint32_t w) {
	const uint32_t x = (w | 0x20202020u) & 0x7f7f7f7fu;
	const uint32_t letter = (x + 0x1f1f1f1fu) & ~(x + 0x05050505u) & ~w & 0x80808080u;      // 'a' <= x < '{', and the byte itself below 128
	return (letter | zero_bytes(w ^ 0x2e2e2e2eu)) == 0x80808080u;
}

// What a record yields: the trimmed length, the name's length, where name, bases and qualities start in the text.
struct Rec { uint32_t L, name_len, name_src, seq_src, qual_src, plain; };
H2G_HD Rec eval_record(const char* t, const Lines& l, const Opts& o) {
	Rec r = {0, 0, 0, 0, 0, 0};
	if(!l.four) return r;
	if(l.s >= l.e[0] || t[l.s] != '@') return r;
	uint32_t ne = l.e[0];
	if(ne > l.s + 1 && t[ne - 1] == '\r') ne--;
	r.name_src = l.s + 1;
	r.name_len = ne - r.name_src;
	if(r.name_len == 0) return r;
	const uint32_t sb = l.e[0] + 1;
	uint32_t se = l.e[1];
	if(se > sb && t[se - 1] == '\r') se--;
	for(uint32_t wi = sb >> 2; 4 * wi < se; wi++) if(!all_fq_bases(word_of(t, wi, sb, se, 0x41414141u))) return r;
	const uint32_t Lraw = se - sb;
	if(l.e[1] + 1 >= l.e[2] || t[l.e[1] + 1] != '+') return r;
	const uint32_t qb = l.e[2] + 1;
	uint32_t qe = l.e[3];
	for(uint32_t wi = qb >> 2; 4 * wi < l.e[3]; wi++) {
		const uint32_t w = word_of(t, wi, qb, l.e[3], 0x49494949u);
		const uint32_t cr = zero_bytes(w ^ 0x0d0d0d0du);
		uint32_t sp = zero_bytes(w ^ 0x20202020u);
		if(cr) { const uint32_t k = (uint32_t)__builtin_ctz(cr) >> 3; qe = 4 * wi + k; sp &= (1u << (8 * k)) - 1u; }      // (blanks behind the '\r' are not the record's)
		if(sp) return r;
		if(cr) break;
	}
	const uint32_t nq = qe - qb;
	if(nq < Lraw || nq > Lraw + 1) return r;
	const uint32_t t5 = o.trim5 < Lraw ? o.trim5 : Lraw;
	const uint32_t t3 = o.trim3 < Lraw - t5 ? o.trim3 : Lraw - t5;
	r.L = Lraw - t5 - t3;
	r.seq_src = sb + t5;
	r.qual_src = qb + t5;
	if(o.phred64) for(uint32_t wi = r.qual_src >> 2; 4 * wi < r.qual_src + r.L; wi++)
		if((word_of(t, wi, r.qual_src, r.qual_src + r.L, 0x40404040u) & 0xc0c0c0c0u) != 0x40404040u) { r.L = 0; return r; }      // every kept byte in [64, 128)
	r.plain = 1;
	return r;
}

// ---- output bytes.  offs[0 .. n] are the scanned lengths (offs[n] = the total); src[r] = where record r's bytes start in the text.
// Walks consecutive output bytes: seek() places the cursor on byte b < offs[n] (one binary search), next() yields the text index of the byte under it and moves on,
// crossing records (and skipping empty ones) without another search.
struct Cursor {
	const unsigned long long* offs; const uint32_t* src; uint32_t n;
	uint32_t r, k, len;
	H2G_HD void seek(const unsigned long long* offs_, const uint32_t* src_, uint32_t n_, uint64_t b) {
		offs = offs_; src = src_; n = n_;
		uint32_t lo = 0, hi = n;           // invariant: offs[lo] <= b < offs[hi]
		while(hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if(offs[mid] <= b) lo = mid; else hi = mid; }
		r = lo; k = (uint32_t)(b - offs[lo]); len = (uint32_t)(offs[lo + 1] - offs[lo]);
	}
	H2G_HD uint32_t rec() const { return r; }
	H2G_HD uint32_t next() {
		const uint32_t at = src[r] + k;
		if(++k < len) return at;
		k = 0;
		do { r++; len = r < n ? (uint32_t)(offs[r + 1] - offs[r]) : 1u; } while(len == 0);      // (past the last record the cursor is never read again)
		return at;
	}
};

}  // namespace h2g_fq
