// h2g_cli.cpp — `hisat2-align-amd`: the reference's `hisat2-align-s -x <index> -U/-1/-2 … -S out.sam` command line for the
// part of HISAT2 that is built here (--no-spliced-alignment; linear or SNP-graph index; unpaired or paired reads).
// Host code only: batched read ingestion (FASTA / FASTQ, the parse rules of pat.cpp:725-1010; tabbed and QSEQ files, pat.cpp:1159-1503 and
// read_qseq.cpp) behind one record stream (`Source`: a record is an unpaired read or a pair; -1/-2 with -U, tabbed files that mix both), the C ABI of
// include/h2g.h for HI_Aligner::go on the GPU, include/h2g_sam.h for the sink + SAM text (N1).  There is no CPU aligner in
// here: without a GPU h2g_index_load fails and so does this program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <math.h>
#include <string>
#include <map>
#include <array>
#include <vector>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <chrono>
#include <algorithm>
#include <time.h>
#include <fcntl.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <zlib.h>
#include "../../include/h2g.h"
#include "../../include/h2g_sam.h"
#include "h2g_align.h"      // h2g::Rng (--non-deterministic)

namespace {

struct Batch {
	std::vector<uint8_t>  codes;
	std::vector<uint32_t> offs, noffs;
	std::string           quals, names;
	bool                  have_quals = false;
	std::vector<uint8_t>  filt;                  // QSEQ sources only, one per read: 0 = the record's filter field is '0' (--qc-filter), 1 = it passes
	std::string           orig;                  // --un / --al ...: the records' text as it stood in the input, record i = [ooffs[i], ooffs[i + 1]); kept only when asked for
	std::vector<uint64_t> ooffs;
	size_t n() const { return offs.empty() ? 0 : offs.size() - 1; }
	void clear() { codes.clear(); offs.assign(1, 0); noffs.assign(1, 0); quals.clear(); names.clear(); filt.clear(); orig.clear(); ooffs.assign(1, 0); }
	// appends the reads of `pb` (parsed with the same options)
	void append(const Batch& pb) {
		const uint32_t cb = (uint32_t)codes.size(), nb = (uint32_t)names.size();
		const uint64_t ob = orig.size();
		codes.insert(codes.end(), pb.codes.begin(), pb.codes.end());
		names += pb.names;
		quals += pb.quals;
		filt.insert(filt.end(), pb.filt.begin(), pb.filt.end());
		for(size_t k = 1; k < pb.offs.size(); k++) { offs.push_back(cb + pb.offs[k]); noffs.push_back(nb + pb.noffs[k]); }
		if(pb.ooffs.size() > 1) { orig += pb.orig; for(size_t k = 1; k < pb.ooffs.size(); k++) ooffs.push_back(ob + pb.ooffs[k]); }
	}
	// appends read i of `s`
	void take(const Batch& s, size_t i) {
		codes.insert(codes.end(), s.codes.begin() + s.offs[i], s.codes.begin() + s.offs[i + 1]);
		offs.push_back((uint32_t)codes.size());
		names.append(s.names, s.noffs[i], s.noffs[i + 1] - s.noffs[i]);
		noffs.push_back((uint32_t)names.size());
		if(s.have_quals) quals.append(s.quals, s.offs[i], s.offs[i + 1] - s.offs[i]);
		if(!s.filt.empty()) filt.push_back(s.filt[i]);
		if(s.ooffs.size() > 1) { orig.append(s.orig, s.ooffs[i], s.ooffs[i + 1] - s.ooffs[i]); ooffs.push_back(orig.size()); }
	}
};
enum ReadFormat { FMT_FASTA, FMT_FASTQ, FMT_TAB5, FMT_TAB6, FMT_QSEQ };
// how a quality string is encoded (qual.h charToPhred33 / intToPhred33): Phred+33, Phred+64, Solexa+64; `ints`: whitespace-separated numbers
struct QualCoding { bool phred64 = false, solexa = false, ints = false; };
// Solexa to Phred: Q = 10 log10(10^(sol / 10) + 1), rounded; below -10 it is 0
struct SolexaTable { uint8_t q[266]; SolexaTable() { for(int s = -10; s < 256; s++) q[s + 10] = (uint8_t)(10.0 * log10(pow(10.0, s / 10.0) + 1.0) + 0.5); } };
inline int solexa_to_phred(int sol) { static const SolexaTable t; return sol < -10 ? 0 : t.q[(sol > 255 ? 255 : sol) + 10]; }
inline char qual_char_to_phred33(char c, const QualCoding& qc) {
	if(qc.solexa) return (char)(solexa_to_phred((int)c - 64) + 33);
	if(qc.phred64) {
		if(c < 64) { fprintf(stderr, "Saw ASCII character %d but expected 64-based Phred qual.\nTry not specifying --solexa1.3-quals/--phred64-quals.\n", (int)c); exit(1); }
		return (char)(c - 31);
	}
	return c;
}
inline char qual_int_to_phred33(int q, const QualCoding& qc) {
	const int p = (qc.solexa ? solexa_to_phred(q) : (q <= 93 ? q : 93)) + 33;
	if(p < 33) { fprintf(stderr, "Saw negative Phred quality %d.\n", p - 33); exit(1); }
	return (char)p;
}
[[noreturn]] inline void too_few_qualities(const char* nm, size_t nlen) { fprintf(stderr, "Error: Read %.*s has more read characters than quality values.\n", (int)nlen, nm); exit(1); }
[[noreturn]] inline void too_many_qualities(const char* nm, size_t nlen) { fprintf(stderr, "Error: Read %.*s has more quality values than read characters.\n", (int)nlen, nm); exit(1); }
[[noreturn]] inline void wrong_quality_format(const char* nm, size_t nlen) {
	fprintf(stderr, "Error: Encountered one or more spaces while parsing the quality string for read %.*s.  If this is a FASTQ file with integer (non-ASCII-encoded) qualities, "
	                "try re-running with the --integer-quals option.\n", (int)nlen, nm);
	exit(1);
}

// asc2dnacat > 0 (alphabet.cpp:36-58): DNA letters, IUPAC codes, N and '-' are read characters; asc2dna (alphabet.cpp:298)
inline bool is_read_char(int c) {
	switch(c | 0x20) { case 'a': case 'b': case 'c': case 'd': case 'g': case 'h': case 'k': case 'm': case 'n': case 'r': case 's': case 't':
	                   case 'v': case 'w': case 'x': case 'y': return true; }
	return c == '-';
}
inline uint8_t base_code(int c) { switch(c | 0x20) { case 'c': return 1; case 'g': return 2; case 't': return 3; case 'n': return 4; } return 0; }
// the per-character tests as tables (0xff = not a base of the record): FASTA keeps is_read_char() characters, FASTQ and QSEQ keep '.' (as N) and every isalpha() character,
// the tabbed formats every isalpha() character
struct BaseTables {
	uint8_t fa[256], fq[256], tab[256];
	BaseTables() {
		for(int c = 0; c < 256; c++) {
			fa[c] = is_read_char(c) ? base_code(c) : 0xff;
			const int d = c == '.' ? 'N' : c;
			fq[c] = isalpha(d) ? base_code(d) : 0xff;
			tab[c] = isalpha(c) ? base_code(c) : 0xff;
		}
	}
};
inline const BaseTables& base_tables() { static const BaseTables t; return t; }
// appends the bases of [q, e) to `codes` through table `tb`: written unconditionally, kept when they are bases (no branch per character, no push_back)
inline void append_bases(std::vector<uint8_t>& codes, const char* q, const char* e, const uint8_t* tb) {
	const size_t at = codes.size();
	codes.resize(at + (size_t)(e - q));
	uint8_t* o = codes.data() + at;
	for(; q < e; q++) { const uint8_t v = tb[(unsigned char)*q]; *o = v; o += v != 0xff; }
	codes.resize((size_t)(o - codes.data()));
}

// Sequential stream of reads over a list of files of one format, parsed in parallel: a file is mapped, the record starts are found by all
// threads (FASTA: lines beginning with '>'; FASTQ: every fourth line; tabbed and QSEQ: every line that is not blank), and each fill() hands
// contiguous record ranges to the threads and concatenates their output in file order.  FASTA / FASTQ: pat.cpp FastaPatternSource /
// FastqPatternSource; --tab5 / --tab6: TabbedPatternSource (pat.cpp:1159-1503), where a line is an unpaired read (name seq qual) or a pair
// (name seq1 qual1 seq2 qual2, or with a second name before seq2), decided line by line; --qseq: QseqPatternSource (read_qseq.cpp).
class Reader {
public:
	Reader(const std::vector<std::string>& files, ReadFormat fmt, int threads, uint32_t trim5 = 0, uint32_t trim3 = 0)
		: files_(files), fmt_(fmt), fasta_(fmt == FMT_FASTA), T_(threads < 1 ? 1 : threads), trim5_(trim5), trim3_(trim3) {}
	~Reader() { unmap(); }
	// up to `max` records into `b`.  Tabbed formats: `mate` takes the second mates (an empty read for a record that is an unpaired read, so that
	// the two batches stay index-aligned) and `kinds` one byte per record, 1 = pair.
	size_t fill(Batch& b, size_t max, Batch* mate = nullptr, std::vector<uint8_t>* kinds = nullptr) {
		size_t got = 0;
		const bool tabbed = fmt_ == FMT_TAB5 || fmt_ == FMT_TAB6;
		if(!fasta_) b.have_quals = true;
		if(mate) mate->have_quals = true;
		while(got < max) {
			if(cur_ >= nrec()) { if(!next_file()) break; continue; }
			const size_t take = std::min(max - got, nrec() - cur_);
			const size_t T = std::min<size_t>((size_t)T_, take / 4096 + 1);
			std::vector<Batch> part(T), part2(tabbed ? T : 0);
			std::vector<std::vector<uint8_t> > pk(tabbed ? T : 0);
			auto work = [&](size_t t) {
				Batch& pb = part[t];
				pb.clear();
				if(tabbed) part2[t].clear();
				const size_t rb = cur_ + take * t / T, re = cur_ + take * (t + 1) / T;
				for(size_t r = rb; r < re; r++) {
					if(tabbed) parse_tabbed(r, pb, part2[t], pk[t]);
					else if(fmt_ == FMT_QSEQ) parse_qseq(r, pb);
					else parse_record(r, pb);
					if(keep_orig_) { pb.orig.append(p_ + starts_[r], starts_[r + 1] - starts_[r]); pb.ooffs.push_back(pb.orig.size()); }
				}
			};
			std::vector<std::thread> th;
			for(size_t t = 1; t < T; t++) th.emplace_back(work, t);
			work(0);
			for(auto& x : th) x.join();
			for(size_t t = 0; t < T; t++) {
				b.append(part[t]);
				if(tabbed && mate) mate->append(part2[t]);
				if(tabbed && kinds) kinds->insert(kinds->end(), pk[t].begin(), pk[t].end());
			}
			cur_ += take; got += take; count_ += take;
		}
		return got;
	}
private:
	size_t nrec() const { return starts_.empty() ? 0 : starts_.size() - 1; }
	void unmap() { if(p_ && !inflated_.empty()) { inflated_.clear(); inflated_.shrink_to_fit(); } else if(p_) munmap((void*)p_, n_); p_ = nullptr; n_ = 0; starts_.clear(); cur_ = 0; }
	bool next_file() {
		unmap();
		if(fi_ >= files_.size()) return false;
		const std::string& fn = files_[fi_++];
		if(fn.size() > 3 && fn.compare(fn.size() - 3, 3, ".gz") == 0) {     // gzipped input (the reference reads it through zlib too)
			gzFile g = gzopen(fn.c_str(), "rb");
			if(!g) { fprintf(stderr, "Error: could not open %s\n", fn.c_str()); exit(1); }
			gzbuffer(g, 1 << 20);
			inflated_.clear();
			std::vector<char> chunk(8 << 20);
			int got;
			while((got = gzread(g, chunk.data(), (unsigned)chunk.size())) > 0) inflated_.insert(inflated_.end(), chunk.begin(), chunk.begin() + got);
			gzclose(g);
			if(inflated_.empty()) return true;
			p_ = inflated_.data(); n_ = inflated_.size();
		} else {
			const int fd = open(fn.c_str(), O_RDONLY);
			if(fd < 0) { fprintf(stderr, "Error: could not open %s\n", fn.c_str()); exit(1); }
			struct stat sb;
			fstat(fd, &sb);
			n_ = (size_t)sb.st_size;
			if(n_ == 0) { close(fd); return true; }
			p_ = (const char*)mmap(nullptr, n_, PROT_READ, MAP_PRIVATE, fd, 0);
			close(fd);
			if(p_ == MAP_FAILED) { fprintf(stderr, "Error: could not map %s\n", fn.c_str()); exit(1); }
		}
		const size_t T = std::min<size_t>((size_t)T_, n_ / (1 << 20) + 1);
		std::vector<std::vector<size_t> > loc(T);
		std::vector<size_t> nl(T + 1, 0);
		std::vector<std::thread> th;
		if(fasta_) {
			auto scan = [&](size_t t) {
				const size_t b = n_ * t / T, e = n_ * (t + 1) / T;
				for(size_t i = b; i < e; i++) if(p_[i] == '>' && (i == 0 || p_[i - 1] == '\n')) loc[t].push_back(i);
			};
			for(size_t t = 1; t < T; t++) th.emplace_back(scan, t);
			scan(0);
			for(auto& x : th) x.join();
			if(p_[0] != '>' && p_[0] != '#' && p_[0] != ';' && p_[0] != '\n' && p_[0] != '\r') { fprintf(stderr, "Error: reads file does not look like a FASTA file\n"); exit(1); }
		} else if(fmt_ != FMT_FASTQ) {
			// one record per line; blank lines are skipped (TabbedPatternSource::readPair, QseqPatternSource::read)
			auto scan = [&](size_t t) {
				const size_t b = n_ * t / T, e = n_ * (t + 1) / T;
				for(size_t i = b; i < e; i++) if(p_[i] != '\n' && p_[i] != '\r' && (i == 0 || p_[i - 1] == '\n')) loc[t].push_back(i);
			};
			for(size_t t = 1; t < T; t++) th.emplace_back(scan, t);
			scan(0);
			for(auto& x : th) x.join();
		} else {
			auto cnt = [&](size_t t) { const size_t b = n_ * t / T, e = n_ * (t + 1) / T; size_t c = 0; for(size_t i = b; i < e; i++) c += p_[i] == '\n'; nl[t + 1] = c; };
			for(size_t t = 1; t < T; t++) th.emplace_back(cnt, t);
			cnt(0);
			for(auto& x : th) x.join();
			th.clear();
			for(size_t t = 0; t < T; t++) nl[t + 1] += nl[t];
			auto scan = [&](size_t t) {
				const size_t b = n_ * t / T, e = n_ * (t + 1) / T;
				size_t line = nl[t];                       // index of the line that starts after the next newline is line+1
				if(b == 0 && (line & 3) == 0) loc[t].push_back(0);
				for(size_t i = b; i < e; i++) if(p_[i] == '\n') { line++; if((line & 3) == 0 && i + 1 < n_) loc[t].push_back(i + 1); }
			};
			for(size_t t = 1; t < T; t++) th.emplace_back(scan, t);
			scan(0);
			for(auto& x : th) x.join();
			if(p_[0] != '@') { fprintf(stderr, "Error: reads file does not look like a FASTQ file\n"); exit(1); }
		}
		for(auto& v : loc) starts_.insert(starts_.end(), v.begin(), v.end());
		if(fmt_ == FMT_FASTQ) while(!starts_.empty() && (starts_.back() >= n_ || p_[starts_.back()] != '@')) starts_.pop_back();   // trailing blank lines
		starts_.push_back(n_);
		return true;
	}
	// -5 / -3 (gTrim5 / gTrim3, pat.cpp:820-832, 930-1010): bases dropped from the 5' / 3' end of the read that starts at codes[c0]; returns the 5' count
	size_t trim(Batch& b, size_t c0) const {
		size_t L = b.codes.size() - c0;
		const size_t t5 = std::min<size_t>(trim5_, L);
		if(t5) { b.codes.erase(b.codes.begin() + c0, b.codes.begin() + c0 + t5); L -= t5; }
		const size_t t3 = std::min<size_t>(trim3_, L);
		if(t3) b.codes.resize(b.codes.size() - t3);
		return t5;
	}
	// --int-quals: the numbers of [ql, qe) as Phred+33 characters (tokenizeQualLine + intToPhred33)
	void int_quals(const char* ql, const char* qe, std::string& out) const {
		out.clear();
		for(const char* q = ql; q < qe;) {
			while(q < qe && (*q == ' ' || *q == '\t' || *q == '\r')) q++;
			if(q >= qe) break;
			const char* t0 = q;
			while(q < qe && *q != ' ' && *q != '\t' && *q != '\r') q++;
			out.push_back(qual_int_to_phred33(atoi(std::string(t0, q).c_str()), qc_));
		}
	}
	void parse_record(size_t r, Batch& b) const {
		const char* q = p_ + starts_[r];
		const char* end = p_ + starts_[r + 1];
		q++;                                                         // '>' or '@'
		const char* nm = q;
		while(q < end && *q != '\n') q++;
		size_t nlen = (size_t)(q - nm);
		if(nlen && nm[nlen - 1] == '\r') nlen--;
		if(nlen == 0) b.names += std::to_string(count_ + (r - cur_)); else b.names.append(nm, nlen);
		b.noffs.push_back((uint32_t)b.names.size());
		if(q < end) q++;
		const size_t c0 = b.codes.size();
		if(fasta_) {
			append_bases(b.codes, q, end, base_tables().fa);
			trim(b, c0);
			b.offs.push_back((uint32_t)b.codes.size());
			return;
		}
		// FastqPatternSource::read (pat.cpp:932-945): '.' is N, every isalpha() character is a base through asc2dna
		// (alphabet.cpp:298: A C G T N, every other letter reads as A); anything else is skipped
		if(*(nm - 1) != '@') { fprintf(stderr, "Error: reads file does not look like a FASTQ file (record %llu does not start with '@'; wrapped records are not supported)\n", (unsigned long long)(count_ + (r - cur_))); exit(1); }
		{ const char* le = (const char*)memchr(q, '\n', (size_t)(end - q)); if(!le) le = end; append_bases(b.codes, q, le, base_tables().fq); q = le; }
		if(q + 1 < end && q[1] != '+') { fprintf(stderr, "Error: FASTQ record %.*s: the line after the sequence does not start with '+' (sequences wrapped over several lines are not supported)\n", (int)nlen, nm); exit(1); }
		const size_t Lraw = b.codes.size() - c0;
		const size_t t5 = trim(b, c0);
		b.offs.push_back((uint32_t)b.codes.size());
		const size_t L = b.codes.size() - c0;
		if(q < end) q++;
		while(q < end && *q != '\n') q++;                            // '+' line
		if(q < end) q++;
		const char* ql = q;
		if(qc_.ints) {                                               // pat.cpp:1000-1021
			while(q < end && *q != '\n') q++;
			static thread_local std::string conv;
			int_quals(ql, q, conv);
			if(conv.size() < Lraw) too_few_qualities(nm, nlen);
			if(conv.size() > Lraw + 1) too_many_qualities(nm, nlen);
			b.quals.append(conv, t5, L);
			return;
		}
		while(q < end && *q != '\n' && *q != '\r') q++;
		if(memchr(ql, ' ', (size_t)(q - ql))) wrong_quality_format(nm, nlen);      // pat.cpp:1044-1045, :1074-1078
		if((size_t)(q - ql) < Lraw) too_few_qualities(nm, nlen);
		if((size_t)(q - ql) > Lraw + 1) too_many_qualities(nm, nlen);
		b.quals.append(ql + t5, L);
		if(qc_.phred64 || qc_.solexa) for(size_t k = b.quals.size() - L; k < b.quals.size(); k++) b.quals[k] = qual_char_to_phred33(b.quals[k], qc_);   // charToPhred33 qual.h:106-147
	}
	// one name / sequence / quality triple of a tabbed or QSEQ line (TabbedPatternSource::parseSeq / parseQuals, the same in read_qseq.cpp).
	// [sq, se) and [ql, qe) are the two fields; `strict` (tabbed): the untrimmed count of qualities must reach the read's, QSEQ asks only for those it keeps
	void seq_and_quals(Batch& b, const char* sq, const char* se, const char* ql, const char* qe, const uint8_t* table, const char* nm, size_t nlen, bool strict) const {
		const size_t c0 = b.codes.size();
		append_bases(b.codes, sq, se, table);
		const size_t Lraw = b.codes.size() - c0;
		trim(b, c0);
		b.offs.push_back((uint32_t)b.codes.size());
		const size_t L = b.codes.size() - c0;
		static thread_local std::string conv;
		if(qc_.ints) {
			int_quals(ql, qe, conv);
			if(conv.size() < Lraw) too_few_qualities(nm, nlen);
			b.quals.append(conv, std::min<size_t>(trim5_, Lraw), L);
			return;
		}
		// the reference reads at most L + <-5> quality characters and stops at the first white space; the 5' trim is counted in full even when the read is shorter
		const size_t want = L + trim5_;
		size_t nq = 0;
		const char* q = ql;
		for(; q < qe && nq < want; q++) {
			if(*q == ' ') wrong_quality_format(nm, nlen);
			if(isspace((unsigned char)*q)) break;
			nq++;
		}
		if(strict ? nq < want : (nq > trim5_ ? nq - trim5_ : 0) < L) too_few_qualities(nm, nlen);
		const size_t at = b.quals.size();
		if(L) b.quals.append(ql + trim5_, L);
		if(qc_.phred64 || qc_.solexa) for(size_t k = at; k < b.quals.size(); k++) b.quals[k] = qual_char_to_phred33(b.quals[k], qc_);
	}
	void put_name(Batch& b, const char* nm, size_t nlen, size_t r) const {
		if(nlen == 0) b.names += std::to_string(count_ + (r - cur_)); else b.names.append(nm, nlen);
		b.noffs.push_back((uint32_t)b.names.size());
	}
	// the tab-separated fields of the line that starts record r (without its line end)
	size_t split_line(size_t r, const char** f, size_t cap) const {
		const char* q = p_ + starts_[r];
		const char* end = (const char*)memchr(q, '\n', starts_[r + 1] - starts_[r]);
		if(!end) end = p_ + starts_[r + 1];
		if(end > q && end[-1] == '\r') end--;
		size_t nf = 0;
		f[nf++] = q;
		for(; q < end && nf < cap; q++) if(*q == '\t') f[nf++] = q + 1;
		f[nf] = end + 1;                                             // (field k is [f[k], f[k + 1] - 1))
		return nf;
	}
	void parse_tabbed(size_t r, Batch& a, Batch& m, std::vector<uint8_t>& kinds) const {
		const char* f[8];
		const size_t nf = split_line(r, f, 7);
		auto len = [&](size_t k) { return (size_t)(f[k + 1] - 1 - f[k]); };
		const bool six = fmt_ == FMT_TAB6;
		if(nf != 3 && nf != (six ? 6u : 5u)) {
			fprintf(stderr, "Error: record %llu of the tabbed read file has %zu fields; expected 3 (unpaired read) or %d (pair)\n", (unsigned long long)(count_ + (r - cur_)), nf, six ? 6 : 5);
			exit(1);
		}
		const uint8_t* tb = base_tables().tab;
		put_name(a, f[0], len(0), r);
		const char* nm = a.names.data() + a.noffs[a.noffs.size() - 2];
		const size_t nlen = a.noffs.back() - a.noffs[a.noffs.size() - 2];
		seq_and_quals(a, f[1], f[2] - 1, f[2], f[3] - 1, tb, nm, nlen, true);
		if(nf == 3) {                                                // an unpaired read: the mate batch gets an empty read under an empty name
			m.offs.push_back((uint32_t)m.codes.size()); m.noffs.push_back((uint32_t)m.names.size());
			kinds.push_back(0);
			return;
		}
		// a tab5 pair has one name for both mates (the seed of each mate's PRNG is drawn from it as parsed: "/1" and "/2" are appended later, pat.cpp:187-193)
		const size_t s2 = six ? 4 : 3;
		if(six) put_name(m, f[3], len(3), r); else put_name(m, nm, nlen, r);
		const char* nm2 = m.names.data() + m.noffs[m.noffs.size() - 2];
		seq_and_quals(m, f[s2], f[s2 + 1] - 1, f[s2 + 1], f[s2 + 2] - 1, tb, nm2, m.noffs.back() - m.noffs[m.noffs.size() - 2], true);
		kinds.push_back(1);
	}
	void parse_qseq(size_t r, Batch& b) const {
		const char* f[13];
		const size_t nf = split_line(r, f, 12);
		auto len = [&](size_t k) { return (size_t)(f[k + 1] - 1 - f[k]); };
		if(nf < 11) { fprintf(stderr, "Error: record %llu of the QSEQ file has %zu fields; expected 11\n", (unsigned long long)(count_ + (r - cur_)), nf); exit(1); }
		// machine_run_lane_tile_x_y_index/mate
		if(len(0) == 0) fprintf(stderr, "Warning: read had an empty name field\n");
		for(size_t k = 0; k < 8; k++) { b.names.append(f[k], len(k)); if(k < 7) b.names.push_back(k == 6 ? '/' : '_'); }
		b.noffs.push_back((uint32_t)b.names.size());
		const char* nm = b.names.data() + b.noffs[b.noffs.size() - 2];
		const size_t nlen = b.noffs.back() - b.noffs[b.noffs.size() - 2];
		if(len(8) == 0) {
			fprintf(stderr, "Warning: skipping empty QSEQ read with name '%.*s'\n", (int)nlen, nm);
			b.offs.push_back((uint32_t)b.codes.size());
		} else seq_and_quals(b, f[8], f[9] - 1, f[9], f[10] - 1, base_tables().fq, nm, nlen, false);
		b.filt.push_back(len(10) == 0 || f[10][0] != '0' ? 1 : 0);
	}
public:
	QualCoding qc_;
	bool keep_orig_ = false;        // --un / --al ...: the batches carry the records' original text
private:
	std::vector<std::string> files_;
	ReadFormat fmt_;
	bool fasta_;
	int T_;
	uint32_t trim5_ = 0, trim3_ = 0;
	size_t fi_ = 0;
	const char* p_ = nullptr;
	size_t n_ = 0, cur_ = 0;
	std::vector<size_t> starts_;
	std::vector<char> inflated_;
	uint64_t count_ = 0;
};

// A window of the record stream: up to a batch of consecutive records.  A record is one unpaired read or one pair.  `a` holds the unpaired reads and the
// first mates, `b` the second mates; in a window of a tabbed file the two stay index-aligned (an unpaired read has an empty read in `b`) and `kinds` says
// which records are pairs.
struct Win {
	Batch a, b;
	std::vector<uint8_t> kinds;       // filled only when the window mixes pairs and unpaired reads (1 = pair)
	bool paired = false;              // (when it does not mix) every record is a pair
	size_t n = 0, npairs = 0;
	uint64_t first_id = 0;            // Read::rdid of its first record
	uint64_t skipped = 0;             // -s: records skipped just before it
};
// The record stream in front of the batches, in the order the reference hands records to its workers: the -1/-2 pairs and then the -U reads, with read ids that
// restart at the -U reads (PairedDualPatternSource pat.cpp:215-306), or the lines of the --tab5 / --tab6 files, each an unpaired read or a pair
// (PairedSoloPatternSource pat.cpp:158-208; -1/-2/-U are ignored then, pat.cpp:438-452).  -s and -u count records of a segment: a worker takes a record when
// skip <= rdid < upto + skip and ends at the first record past that (hisat2.cpp:3319, :3634).
class Source {
public:
	Source(const std::vector<std::string>& m1, const std::vector<std::string>& m2, const std::vector<std::string>& u, const std::vector<std::string>& tab,
	       ReadFormat fmt, int threads, uint32_t trim5, uint32_t trim3, const QualCoding& qc, bool keep_orig, uint64_t skip, uint64_t upto) : skip_(skip), upto_(upto) {
		auto mk = [&](const std::vector<std::string>& files) { Reader* r = new Reader(files, fmt, threads, trim5, trim3); r->qc_ = qc; r->keep_orig_ = keep_orig; return r; };
		if(!tab.empty()) segs_.push_back(Seg{mk(tab), nullptr, true});
		else {
			if(!m1.empty() && !m2.empty()) segs_.push_back(Seg{mk(m1), mk(m2), false});
			if(!u.empty()) segs_.push_back(Seg{mk(u), nullptr, false});
		}
	}
	~Source() { for(Seg& s : segs_) { delete s.a; delete s.b; } }
	Source(const Source&) = delete;
	bool short_mates() const { return short_mates_; }         // the -2 files ran out before the -1 files
	bool next(Win& w, size_t max) {
		w.a.clear(); w.b.clear(); w.kinds.clear(); w.n = w.npairs = 0; w.skipped = 0; w.paired = false;
		while(si_ < segs_.size()) {
			Seg& s = segs_[si_];
			Batch ja, jb;
			std::vector<uint8_t> jk;
			if(!s.started) {                                      // -s: the skipped records are parsed (their ids count) but not aligned
				s.started = true; s.budget = upto_;
				for(uint64_t left = skip_; left > 0;) {
					ja.clear(); jb.clear(); jk.clear();
					const size_t g = fill(s, ja, jb, jk, (size_t)std::min<uint64_t>(left, 1u << 20));
					if(!g) break;
					left -= g; s.id += g; w.skipped += g;
				}
			}
			if(s.budget == 0) {                                   // -u reached: with records left here the run ends, else the next segment starts
				ja.clear(); jb.clear();
				if(fill(s, ja, jb, jk, 1)) { si_ = segs_.size(); return false; }
				si_++;
				continue;
			}
			const size_t g = fill(s, w.a, w.b, w.kinds, (size_t)std::min<uint64_t>(max, s.budget));
			if(!g || short_mates_) { si_++; if(short_mates_) return false; continue; }
			w.first_id = s.id; s.id += g; s.budget -= g; w.n = g;
			if(s.tabbed) {
				for(uint8_t k : w.kinds) w.npairs += k;
				w.paired = w.npairs == g;
				if(w.npairs == 0 || w.npairs == g) w.kinds.clear();
			} else { w.paired = s.b != nullptr; w.npairs = w.paired ? g : 0; }
			return true;
		}
		return false;
	}
private:
	struct Seg { Reader* a; Reader* b; bool tabbed; uint64_t id = 0, budget = 0; bool started = false; };
	size_t fill(Seg& s, Batch& a, Batch& b, std::vector<uint8_t>& kinds, size_t w) {
		if(s.tabbed) return s.a->fill(a, w, &b, &kinds);
		if(!s.b) return s.a->fill(a, w);
		// the two mate files are parsed side by side (each fill is threaded in itself; one after the other they were a second per 10 M pairs, and the main thread waited for them)
		size_t nb = 0;
		std::thread tb([&]() { nb = s.b->fill(b, w); });
		const size_t n = s.a->fill(a, w);
		tb.join();
		if(nb < n) short_mates_ = true;                           // (-2 ran out before -1: the reference's error; a longer -2 is not looked at)
		return n;
	}
	std::vector<Seg> segs_;
	size_t si_ = 0;
	uint64_t skip_, upto_;
	bool short_mates_ = false;
};

// --un / --al / --un-conc / --al-conc / --al-conc-disc (and -gz): the reference's wrapper script sorts every read's original record by the flags of its
// non-secondary SAM line(s); here the command line's formatter stage does, from the lines it has just formatted.
struct ReadFile {
	FILE* f = nullptr; gzFile g = nullptr;
	void open(const std::string& fn, bool gz) {
		if(gz) g = gzopen(fn.c_str(), "wb"); else f = fopen(fn.c_str(), "wb");
		if(!g && !f) { fprintf(stderr, "Error: could not open %s for writing\n", fn.c_str()); exit(1); }
	}
	bool bad = false;                 // a write or the close failed
	void put(const char* p, size_t n) { if(!n) return; if(g) { if(gzwrite(g, p, (unsigned)n) != (int)n) bad = true; } else if(f && fwrite(p, 1, n, f) != n) bad = true; }
	void close() { if(g && gzclose(g) != Z_OK) bad = true; if(f && fclose(f) != 0) bad = true; g = nullptr; f = nullptr; }
};
enum { RS_UN, RS_AL, RS_UN_CONC, RS_AL_CONC, RS_AL_CONC_DISC, RS_KINDS };
const char* const rs_names[RS_KINDS] = {"un", "al", "un-conc", "al-conc", "al-conc-disc"};
bool is_directory(const std::string& p) { struct stat sb; return stat(p.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode); }
// the file name(s) of one of these options: an unpaired kind writes to its argument (<dir>/un-seqs, <dir>/al-seqs for a directory); a -conc kind to two files,
// named after the argument's base name: every '%' becomes 1 / 2, else .1 / .2 goes before the last extension, else it is appended (<dir>/un-conc-mate.1 ...)
void read_sink_names(int kind, const std::string& arg, std::string* fn1, std::string* fn2) {
	std::string dir, base;
	if(is_directory(arg) || (!arg.empty() && arg.back() == '/')) { dir = arg; if(dir.back() != '/') dir.push_back('/'); }
	else { const size_t sl = arg.rfind('/'); if(sl == std::string::npos) base = arg; else { dir = arg.substr(0, sl + 1); base = arg.substr(sl + 1); } }
	if(kind == RS_UN || kind == RS_AL) { *fn1 = base.empty() ? dir + rs_names[kind] + "-seqs" : arg; fn2->clear(); return; }
	if(base.empty()) base = std::string(rs_names[kind]) + "-mate";
	std::string b1 = base, b2 = base;
	const size_t dot = base.rfind('.');
	if(base.find('%') != std::string::npos) { for(char& c : b1) if(c == '%') c = '1'; for(char& c : b2) if(c == '%') c = '2'; }
	else if(dot != std::string::npos) { b1.insert(dot, ".1"); b2.insert(dot, ".2"); }
	else { b1 += ".1"; b2 += ".2"; }
	*fn1 = dir + b1; *fn2 = dir + b2;
}
// which read-file option `a` is: 0 none of them, 1 + 2 kind + (1 if -gz), -1 a -bz2 / -lz4 form (refused by name)
int read_sink_option(const std::string& a) {
	for(int k = 0; k < RS_KINDS; k++) {
		const std::string o = std::string("--") + rs_names[k];
		if(a == o) return 1 + 2 * k;
		if(a == o + "-gz") return 2 + 2 * k;
		if(a == o + "-bz2" || a == o + "-lz4") return -1;
	}
	return 0;
}
struct ReadSorter {
	bool on = false;
	ReadFile out[RS_KINDS][2];
	bool have[RS_KINDS] = {false, false, false, false, false};
	void open(int kind, const std::string& arg, bool gz) {
		std::string f1, f2;
		read_sink_names(kind, arg, &f1, &f2);
		out[kind][0].open(f1, gz);
		if(!f2.empty()) out[kind][1].open(f2, gz);
		have[kind] = true; on = true;
	}
	bool close() { bool ok = true; for(auto& k : out) for(ReadFile& f : k) { f.close(); ok = ok && !f.bad; } return ok; }   // false: writing one of the files failed
	// one record: its SAM lines [t, te) and the original text of its read (unpaired) or of its two mates
	void record(const char* t, const char* te, const char* o1, size_t n1, const char* o2, size_t n2) {
		while(t < te) {
			const char* le = (const char*)memchr(t, '\n', (size_t)(te - t));
			if(!le) le = te;
			const char* tab = (const char*)memchr(t, '\t', (size_t)(le - t));
			const unsigned fl = tab ? (unsigned)strtoul(tab + 1, nullptr, 10) : 0x100u;
			t = le + 1;
			if(fl & 0x100u) continue;                                 // one write per read, however many -k lines it has
			const bool m1 = (fl & 0x40u) != 0, m2 = (fl & 0x80u) != 0;
			if(!m1 && !m2) { ReadFile& f = out[(fl & 4u) ? RS_UN : RS_AL][0]; f.put(o1, n1); continue; }
			const int m = m1 ? 0 : 1;
			const char* o = m1 ? o1 : o2;
			const size_t n = m1 ? n1 : n2;
			out[(fl & 2u) ? RS_AL_CONC : RS_UN_CONC][m].put(o, n);
			if(!(fl & 4u) || !(fl & 8u)) out[RS_AL_CONC_DISC][m].put(o, n);
		}
	}
};

std::vector<std::string> split_commas(const char* s) {
	std::vector<std::string> v;
	std::string cur;
	for(; *s; s++) { if(*s == ',') { if(!cur.empty()) v.push_back(cur); cur.clear(); } else cur.push_back(*s); }
	if(!cur.empty()) v.push_back(cur);
	return v;
}
void die(const char* what) { fprintf(stderr, "hisat2-align-amd: %s (%s)\n", what, h2g_last_error()); exit(1); }
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char** argv) {
	std::string base, outfn, stats_fn;
	std::vector<std::string> u, m1, m2, m12;
	ReadFormat tab_fmt = FMT_TAB5;
	bool qseq = false, qc_filter = false, from_front_end = false;
	QualCoding qcoding;
	std::string rs_arg[RS_KINDS];
	bool rs_gz[RS_KINDS] = {false, false, false, false, false};
	bool fasta = false, nohead = false, parse_only = false, no_unal = false;
	std::string known_ss, novel_ss, novel_out;
	bool tlen_adjust = true;
	bool no_sq = false, omit_sec_seq = false;
	std::vector<std::pair<bool, std::string> > rg_args;
	bool new_summary = false;
	std::string summary_file;
	int chrname_mode = 0;
	bool quiet = false, raw_input = false, cmdline_input = false;
	bool report_mixed = true, report_discordant = true;
	int strandness = 0;
	uint64_t skip = 0, upto = ~0ull;
	uint32_t trim5 = 0, trim3 = 0;
	size_t batch = 1u << 20;
	bool saw_batch = false;
	int device = 0, threads = 1, gpus = 1;
	uint32_t ss_window_opt = 0;
	std::string cmdline;
	std::vector<const char*> opts;                        // the alignment options and their arguments, in order: parsed by the library (h2g_align_params_apply_options)
	bool arbitrary_random = false;
	for(int i = 0; i < argc; i++) { if(i) cmdline.push_back(' '); cmdline += argv[i]; }
	for(int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		auto need = [&](const char* o) { if(i + 1 >= argc) { fprintf(stderr, "option %s needs an argument\n", o); exit(1); } return argv[++i]; };
		if(a == "-x") base = need("-x");
		else if(a == "-U") { auto v = split_commas(need("-U")); u.insert(u.end(), v.begin(), v.end()); }
		else if(a == "-1") { auto v = split_commas(need("-1")); m1.insert(m1.end(), v.begin(), v.end()); }
		else if(a == "-2") { auto v = split_commas(need("-2")); m2.insert(m2.end(), v.begin(), v.end()); }
		else if(a == "--tab5" || a == "--12") { auto v = split_commas(need(a.c_str())); m12.insert(m12.end(), v.begin(), v.end()); tab_fmt = FMT_TAB5; }   // hisat2.cpp:1122-1124
		else if(a == "--tab6") { auto v = split_commas(need("--tab6")); m12.insert(m12.end(), v.begin(), v.end()); tab_fmt = FMT_TAB6; }
		else if(a == "--qseq") qseq = true;
		else if(a == "--wrapper") from_front_end = std::string(need("--wrapper")) == "basic-0";   // the front end hisat2-amd announces itself as the reference's script does (hisat2.cpp ARG_WRAPPER)
		else if(a == "--qc-filter") qc_filter = true;                          // reads whose QSEQ filter field is '0' are not aligned (hisat2.cpp:3433-3439)
		else if(a == "--solexa-quals") qcoding.solexa = true;
		else if(a == "--int-quals" || a == "--integer-quals") qcoding.ints = true;
		else if(int rk = read_sink_option(a)) {                                  // --un / --al / --un-conc / --al-conc / --al-conc-disc <path>, each also as -gz
			if(rk < 0) { fprintf(stderr, "hisat2-align-amd: option %s is not built: the -bz2 / -lz4 forms of --un / --al are not (plain and -gz are; see DESIGN.md, scope)\n", a.c_str()); return 1; }
			const int kind = (rk - 1) / 2;
			rs_arg[kind] = need(a.c_str()); rs_gz[kind] = (rk - 1) % 2 != 0;
		}
		else if(a == "-S") outfn = need("-S");
		else if(a == "-r") raw_input = true;                                   // one sequence per line (RawPatternSource pat.h)
		else if(a == "-c") cmdline_input = true;                               // -U / -1 / -2 are comma-separated sequences (VectorPatternSource)
		else if(a == "-f") fasta = true;
		else if(a == "-q") fasta = false;
		else if(a == "-p" || a == "--threads") threads = atoi(need("-p"));        // host threads for parsing and SAM formatting
		else if(a == "--ss-window") ss_window_opt = (uint32_t)strtoul(need("--ss-window"), nullptr, 10);   // reads a temporary splice site stays invisible for: 1000 x <-p> of the reference (hisat2.cpp:3687), decoupled from this program's host threads
		else if(a == "--rna-strandness") {
			const std::string v = need("--rna-strandness");
			strandness = v == "F" ? 1 : v == "R" ? 2 : v == "FR" ? 3 : v == "RF" ? 4 : 0;
			if(!strandness) { fprintf(stderr, "Error: should be one of F, R, FR, or RF \n"); return 1; }
		}
		else if(a == "--known-splicesite-infile") known_ss = need("--known-splicesite-infile");
		else if(a == "--novel-splicesite-infile") novel_ss = need("--novel-splicesite-infile");
		else if(a == "--novel-splicesite-outfile") novel_out = need("--novel-splicesite-outfile");
		else if(a == "--no-templatelen-adjustment") tlen_adjust = false;
		else if(a == "--rg-id") rg_args.push_back({true, need("--rg-id")});    // hisat2.cpp:1389-1407, in command-line order
		else if(a == "--rg") rg_args.push_back({false, need("--rg")});
		else if(a == "--no-sq" || a == "--sam-no-sq" || a == "--sam-nosq" || a == "--sam-noSQ") no_sq = true;
		else if(a == "--omit-sec-seq" || a == "--sam-omit-sec-seq") omit_sec_seq = true;
		else if(a == "--phred64" || a == "--phred64-quals" || a == "--solexa1.3-quals") qcoding.phred64 = true;   // hisat2.cpp ARG_PHRED64
		else if(a == "--phred33" || a == "--phred33-quals") qcoding.phred64 = false;
		else if(a == "--remove-chrname") chrname_mode |= 1;
		else if(a == "--add-chrname") chrname_mode |= 2;
		else if(a == "--new-summary") new_summary = true;
		else if(a == "--summary-file") summary_file = need("--summary-file");
		else if(a == "--no-mixed") report_mixed = false;                       // hisat2.cpp:1162
		else if(a == "--no-discordant") report_discordant = false;             // hisat2.cpp:1161
		else if(a == "--non-deterministic" || a == "--nondeterministic") arbitrary_random = true;   // hisat2.cpp:1207
		else if(a == "--no-hd" || a == "--no-head") nohead = true;
		else if(a == "--batch") { batch = (size_t)atoll(need("--batch")); saw_batch = true; }
		else if(a == "--device") device = atoi(need("--device"));
		else if(a == "--gpus") gpus = atoi(need("--gpus"));                        // batches round-robin over <int> devices, output in read order
		else if(a == "-s" || a == "--skip") skip = (uint64_t)atoll(need("-s"));     // skip the first <int> reads / pairs (hisat2.cpp:3319)
		else if(a == "-u" || a == "--upto" || a == "--qupto") upto = (uint64_t)atoll(need("-u"));
		else if(a == "-5" || a == "--trim5") trim5 = (uint32_t)atoi(need("-5"));
		else if(a == "-3" || a == "--trim3") trim3 = (uint32_t)atoi(need("-3"));
		else if(a == "--no-unal") no_unal = true;
		else if(a == "--quiet") quiet = true;                                      // gQuiet: no alignment summary on stderr (hisat2.cpp:4165)
		else if(a == "--version") { printf("hisat2-align-amd (h2g) — output format of HISAT2 2.2.3\n"); return 0; }
		else if(a == "--reorder" || a == "-t" || a == "--time" || a == "--mm") {}   // output is always in read order; --mm (index mapping) has nothing to act on here
		else if(a == "--h2g-stats") stats_fn = need("--h2g-stats");               // writes {reads, second_pass, overflow} as JSON (tests, bench)
		else if(a == "--parse-only") parse_only = true;                           // test hook: ingest the reads, print counts + checksums
		else if(const int arity = h2g_align_option_arity(argv[i]); arity >= 0) { opts.push_back(argv[i]); if(arity) opts.push_back(need(argv[i])); }   // every option that ends in a field of h2g_align_params
		else { fprintf(stderr, "hisat2-align-amd: option %s is not built (see DESIGN.md, scope)\n", a.c_str()); return 1; }
	}
	if(base.empty() || (m12.empty() && u.empty() && (m1.empty() || m2.empty()))) {
		fprintf(stderr, "usage: hisat2-align-amd -x <ht2-base> {-U <r.fq> | -1 <m1.fq> -2 <m2.fq> | --tab5 <r.tab5> | --tab6 <r.tab6>} [-f|-q|--qseq] --no-spliced-alignment [--bowtie2-dp 0|1|2] [-S out.sam]\n");
		return 1;
	}
	// the alignment options: the library's one parser (h2g_options.cpp), before anything touches a device; -k and the presets follow with the index type
	h2g_align_params P; h2g_align_params_init(&P, nullptr);
	P.no_spliced_alignment = 0;                           // the command line's default is the reference's: spliced alignment
	h2g_align_presets presets;
	{
		char err[512];
		if(h2g_align_params_apply_options(&P, &presets, opts.data(), opts.size(), err, sizeof err) != H2G_OK) { fprintf(stderr, "%s\n", err); return 1; }
	}
	bool sorting = false;
	for(int k = 0; k < RS_KINDS; k++) sorting = sorting || !rs_arg[k].empty();
	if(sorting && !from_front_end) {
		// as in the reference, where these are options of the `hisat2` script and hisat2-align-s refuses them
		for(int k = 0; k < RS_KINDS; k++) if(!rs_arg[k].empty()) {
			fprintf(stderr, "hisat2-align-amd: option --%s%s is not built into hisat2-align-amd itself: it is an option of the front end, hisat2-amd (the same command line)\n", rs_names[k], rs_gz[k] ? "-gz" : "");
			return 1;
		}
	}
	if(sorting && (cmdline_input || raw_input)) { fprintf(stderr, "hisat2-align-amd: --un / --al and their kin are not built for -c / -r input (see DESIGN.md, scope)\n"); return 1; }
	if(!m12.empty()) { cmdline_input = raw_input = false; }      // the tabbed files are the read set (pat.cpp:438-452)
	const ReadFormat fmt = !m12.empty() ? tab_fmt : qseq ? FMT_QSEQ : (fasta || cmdline_input || raw_input) ? FMT_FASTA : FMT_FASTQ;
	const bool have_pairs = m12.empty() && !m1.empty() && !m2.empty(), have_singles = m12.empty() && !u.empty();
	// -c / -r: the reads have no names (the reference numbers them, like FASTA records with an empty name) and no qualities ('I'): they are
	// handed to the FASTA reader as ">\n<sequence>\n" records through a temporary file
	static std::vector<std::string> tmp_inputs;   // (static: the exit handler below outlives main's frame)
	if(cmdline_input || raw_input) {
		auto as_fasta = [&](std::vector<std::string>& list) {
			if(list.empty()) return;
			std::string text;
			for(const std::string& item : list) {
				if(cmdline_input) { text += ">\n"; text += item; text += "\n"; continue; }
				FILE* f = fopen(item.c_str(), "rb");
				if(!f) { fprintf(stderr, "Error: could not open %s\n", item.c_str()); exit(1); }
				std::string line;
				int c;
				auto flush = [&]() { while(!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back(); if(!line.empty()) { text += ">\n"; text += line; text += "\n"; } line.clear(); };
				while((c = fgetc(f)) != EOF) { if(c == '\n') flush(); else line.push_back((char)c); }
				flush();
				fclose(f);
			}
			char path[] = "/tmp/h2g_reads_XXXXXX";
			const int fd = mkstemp(path);
			if(fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) { fprintf(stderr, "Error: cannot write a temporary read file\n"); exit(1); }
			close(fd);
			list.assign(1, path);
			tmp_inputs.push_back(path);
		};
		as_fasta(u); as_fasta(m1); as_fasta(m2);
		fasta = true;
	}
	// the -c / -r temporary read files go away on every way out, exit() included
	atexit([] { for(const std::string& p : tmp_inputs) unlink(p.c_str()); tmp_inputs.clear(); });
	struct TmpGuard { std::vector<std::string>& v; ~TmpGuard() { for(const std::string& p : v) unlink(p.c_str()); v.clear(); } } tmp_guard{tmp_inputs};
	if(parse_only) {
		// records, bases and a checksum over every window of <--batch> records (codes, names, qualities and lengths of the unpaired reads and first mates, then those of the
		// second mates), then the number of pairs and of unpaired reads; one line per --un / --al option with the file name(s) it would write
		Source src(m1, m2, u, m12, fmt, threads, trim5, trim3, qcoding, false, skip, upto);
		Win w;
		uint64_t n = 0, bases = 0, npairs = 0, h = 1469598103934665603ull;
		auto mix = [&](const void* p, size_t len) { const uint8_t* c = (const uint8_t*)p; for(size_t i = 0; i < len; i++) { h ^= c[i]; h *= 1099511628211ull; } };
		while(src.next(w, batch)) {
			n += w.n; npairs += w.npairs;
			for(int m = 0; m < (w.npairs ? 2 : 1); m++) {
				const Batch& b = m ? w.b : w.a;
				bases += b.codes.size();
				mix(b.codes.data(), b.codes.size()); mix(b.names.data(), b.names.size()); mix(b.quals.data(), b.quals.size());
				for(size_t i = 1; i <= w.n; i++) {
					if(m && !w.kinds.empty() && !w.kinds[i - 1]) continue;    // (an unpaired read has no second mate)
					const uint32_t l = b.offs[i] - b.offs[i - 1], nl = b.noffs[i] - b.noffs[i - 1]; mix(&l, 4); mix(&nl, 4);
				}
			}
		}
		if(src.short_mates()) { fprintf(stderr, "Error, fewer reads in file specified with -2 than in file specified with -1\n"); return 1; }
		printf("%llu %llu %016llx %llu %llu\n", (unsigned long long)n, (unsigned long long)bases, (unsigned long long)h, (unsigned long long)npairs, (unsigned long long)(n - npairs));
		for(int k = 0; k < RS_KINDS; k++) if(!rs_arg[k].empty()) {
			std::string f1, f2;
			read_sink_names(k, rs_arg[k], &f1, &f2);
			printf("--%s%s\t%s%s%s\n", rs_names[k], rs_gz[k] ? "-gz" : "", f1.c_str(), f2.empty() ? "" : "\t", f2.c_str());
		}
		return 0;
	}
	// Temporary splice sites (the reference's default): a read sees the junctions of reads at least W = 1000 * p ids before it
	// (hisat2.cpp:3687; -p 1 means W = 0, every read after the other).  The batches are waves of <= W reads run one after the other.
	const bool temp_ss = !P.no_spliced_alignment && !P.no_temp_splicesite;
	uint32_t ss_window = 0, ss_wave = 0;      // the reference's visibility window, and the reads of one wave here (the window, or ONE read when it is 0)
	if(temp_ss) {
		// -p 1 (and no --ss-window): the reference's window is 0 (hisat2.cpp:3687) — a read sees the junctions of EVERY read before it, a strict
		// chain.  It runs as waves of one read: exact, and as slow as a chain is (a device round trip per read); meant for small inputs — the
		// reference's bare default invocation `hisat2 -x idx -U reads` then simply works.  -p >= 2 / --ss-window are the throughput modes.
		ss_window = ss_window_opt ? ss_window_opt : (threads < 2 ? 0u : 1000u * (uint32_t)threads);
		ss_wave = ss_window ? ss_window : 1u;
		// a wave sizes the streams and the result rows (one shard per device): bound it — the reference's own window at its largest useful
		// -p (1000 x 256 threads) is far below this, and an absurd value would only be an allocation failure later
		const uint32_t ss_wave_max = 4u * 1024u * 1024u;
		if(ss_wave > ss_wave_max) {
			fprintf(stderr, "hisat2-align-amd: --ss-window %u (or 1000 x -p) makes waves of more than %u reads; a wave is one resident batch per device "
			                "(streams and result rows are sized by it, --batch does not apply to the temporary-splice-site mode): use --ss-window <= %u, "
			                "or --no-temp-splicesite with --batch\n", ss_wave, ss_wave_max, ss_wave_max);
			return 1;
		}
		batch = ss_wave;   // a wave is exactly one shard per device (want()): a smaller --batch would complete shards (and merge their junctions) in the middle of a wave
	}
	if(temp_ss && have_pairs && have_singles) {
		// the reference's read ids restart at the -U reads: which temporary splice sites its window then shows them is not a function of the input
		fprintf(stderr, "hisat2-align-amd: -1/-2 together with -U is not built for the temporary-splice-site mode (the reference's read ids restart at the -U reads, and "
		                "the sites its window shows them depend on thread timing): give --no-temp-splicesite or --no-spliced-alignment\n");
		return 1;
	}
	const double t0 = now();
	h2g_load_opts lo; h2g_load_opts_init(&lo); lo.device = device; lo.load_local = 1;
	// --gpus N: one index replica and one stream per device; batch k runs on device k mod N while the others are in flight, and
	// the batches are completed (fetched, formatted, written) strictly in order, so the output is the single-GPU output.
	// H2G_GPUS_SHARE_DEVICE=1 (test hook) lets the N streams share the devices that exist.
	if(gpus < 1) gpus = 1;
	int ndev = h2g_device_count();
	if(ndev < 1) die("no GPU");
	if(gpus > ndev && !getenv("H2G_GPUS_SHARE_DEVICE")) { fprintf(stderr, "hisat2-align-amd: --gpus %d but %d device(s) visible\n", gpus, ndev); return 1; }
	// One stream per device.  (H2G_STREAMS_PER_DEVICE=2 puts batch k - 1 on the device while the main thread fetches and formats batch k - 2: measured on 10 M pairs, E. coli-size
	// index — 2.77 s against 2.74 s to /dev/null, and slower to a file: the kernels are 0.16 s of the run, there is nothing to hide; profiles/r05_NOTES.md §12.)
	const int ndevs_asked = gpus;
	{
		const char* e = getenv("H2G_STREAMS_PER_DEVICE");
		const int per = e && !temp_ss ? atoi(e) : 1;
		if(per > 1) gpus *= per;
	}
	// The dense SA table (include/h2g.h, H2G_DENSE_SA) is for a process whose index serves batch after batch: its build is 80 ms of device time at 256 Mbp, about a second
	// at GRCh38 size, for 1.3 ms less device time per million pairs — and this program is bound by its host side (parsing, SAM text), not by the device.  Measured on
	// 1 M pairs it cost 0.05 s of 0.6 s (profiles/r07_dense_sa.md), so the command line leaves it out unless the variable says otherwise.
	setenv("H2G_DENSE_SA", "0", 0);
	std::vector<h2g_index*> ixs((size_t)gpus, nullptr);
	for(int g = 0; g < gpus; g++) {
		const int dev = (device + g % ndevs_asked) % ndev;
		for(int q = 0; q < g; q++) if((device + q % ndevs_asked) % ndev == dev) ixs[g] = ixs[q];      // shared device: share the replica
		if(ixs[g]) continue;
		lo.device = dev;
		if(h2g_index_load(base.c_str(), &lo, &ixs[g]) != H2G_OK) die("cannot load the index onto the GPU");
	}
	h2g_index* ix = ixs[0];
	h2g_sam* sam = nullptr;
	if(h2g_sam_open(base.c_str(), &sam) != H2G_OK) die("cannot read reference names");
	if(chrname_mode == 3) { fprintf(stderr, "Error: --remove-chrname and --add-chrname cannot be used at the same time\n"); return 1; }   // hisat2.cpp:3958
	if(chrname_mode) h2g_sam_set_chrname_mode(sam, chrname_mode);
	{   // -k / --max-seeds and the presets wait for the index type (hisat2.cpp:1882-1909, 3903)
		h2g_index_info info;
		if(h2g_index_get_info(ix, &info) != H2G_OK) die("h2g_index_get_info");
		h2g_align_params_presets(&P, (int)info.linear, &presets);
	}
	if(!P.no_spliced_alignment && P.max_intronlen > 0xfffffu) {
		fprintf(stderr, "hisat2-align-amd: --max-intronlen %u is beyond the 1048575 bases a splice edit holds here\n", P.max_intronlen);
		return 1;
	}
	if(P.min_intronlen > P.max_intronlen) {   // hisat2.cpp:4278
		fprintf(stderr, "--min-intronlen(%u) should not be greater than --max-intronlen(%u)\n", P.min_intronlen, P.max_intronlen);
		return 1;
	}
	if(P.khits < 1 || P.khits > H2G_KHITS_MAX || P.kseeds > H2G_KSEEDS_MAX || P.kseeds < P.khits) {
		fprintf(stderr, "hisat2-align-amd: -k %u / --max-seeds %u is outside the built range (1 <= -k <= %u, -k <= --max-seeds <= %u)\n", P.khits, P.kseeds,
		        (unsigned)H2G_KHITS_MAX, (unsigned)H2G_KSEEDS_MAX);
		return 1;
	}
	// -k above 32 or --max-seeds above 64 runs on the extra-large units, whose result rows grow with -k (2 k + 4 records of 424 bytes per mate and pair):
	// 64 k reads per batch keep them near 14 GB at -k 128 where the default batch would need 220 GB
	// (not in the temporary-splice-site mode: there a batch is one wave)
	if((P.khits > 32 || P.kseeds > 64) && !saw_batch && ss_wave == 0 && batch > (1u << 16)) batch = 1u << 16;
	// splice sites from files (hisat2.cpp:4100-4120): one database for go() on every device and for TLEN
	std::vector<h2g_splice_site> sites;                  // the splice-site database: file sites, then the temporary ones by first appearance
	std::map<std::array<uint32_t, 4>, size_t> site_at;    // (text, left, right, dir) -> position in `sites`
	auto publish_sites = [&]() {
		for(int g = 0; g < gpus; g++) {
			bool first = true;
			for(int q = 0; q < g; q++) if(ixs[(size_t)q] == ixs[(size_t)g]) first = false;
			if(first && h2g_index_set_splice_sites(ixs[(size_t)g], sites.data(), sites.size(), ss_window) != H2G_OK) die("cannot upload the splice sites");
		}
		h2g_sam_set_splice_sites(sam, sites.data(), sites.size(), ss_window);
	};
	if(!P.no_spliced_alignment && (!known_ss.empty() || !novel_ss.empty())) {
		for(int pass = 0; pass < 2; pass++) {
			const std::string& fn = pass == 0 ? known_ss : novel_ss;
			if(fn.empty()) continue;
			const size_t n = h2g_sam_read_splice_site_file(sam, fn.c_str(), pass == 0, nullptr, 0);
			if(n == (size_t)-1) { fprintf(stderr, "Error: Could not open %s\n", fn.c_str()); return 1; }
			const size_t at = sites.size();
			sites.resize(at + n);
			h2g_sam_read_splice_site_file(sam, fn.c_str(), pass == 0, sites.data() + at, n);
		}
		{   // SpliceSiteDB::read keeps the first of equal sites (splice_site.cpp:750)
			std::vector<h2g_splice_site> uniq;
			for(const h2g_splice_site& x : sites) {
				const std::array<uint32_t, 4> key = {x.tidx, x.left, x.right, (uint32_t)x.dir};
				if(site_at.emplace(key, uniq.size()).second) uniq.push_back(x);
			}
			sites.swap(uniq);
		}
		publish_sites();
	} else if(temp_ss) publish_sites();                    // (the window of the wave scheme; the sites arrive wave after wave)
	if(!temp_ss && !P.no_spliced_alignment && !novel_out.empty() && h2g_sam_novel_splice_sites_text(sam, nullptr, 0) > 0) {
		// write (the outfile) + read (a file's or the index's sites) without the temporary-site window: the reference then lets every read see
		// the junctions of whichever reads its threads happened to finish first (window 0, hisat2.cpp:3687, :4092-4093) — not a function of the input
		fprintf(stderr, "hisat2-align-amd: --novel-splicesite-outfile with --no-temp-splicesite and a splice-site database (file or --ss index) "
		        "makes the reference's output depend on thread timing; drop --no-temp-splicesite (output == hisat2 -p <int> --reorder)\n");
		return 1;
	}
	if(temp_ss || (!P.no_spliced_alignment && !novel_out.empty())) h2g_sam_collect_novel_sites(sam, 1);   // SpliceSiteDB's `write` (hisat2.cpp:4092)
	h2g_sam_set_templatelen_adjustment(sam, tlen_adjust);
	h2g_sam_set_report_policy(sam, report_discordant, report_mixed);
	for(const auto& r : rg_args) h2g_sam_add_read_group(sam, r.first ? r.second.c_str() : nullptr, r.first ? nullptr : r.second.c_str());
	h2g_sam_set_header_options(sam, no_sq, omit_sec_seq);
	h2g_sam_set_new_summary(sam, new_summary);
	h2g_sam_set_score_min(sam, P.score_min_type, P.score_min_const, P.score_min_coeff);
	h2g_sam_set_n_ceil(sam, P.n_ceil_type, P.n_ceil_const, P.n_ceil_coeff);
	h2g_sam_set_secondary(sam, (int)P.secondary);
	h2g_sam_set_rna_strandness(sam, strandness);
	FILE* out = outfn.empty() ? stdout : fopen(outfn.c_str(), "wb");
	if(!out) { fprintf(stderr, "cannot open %s\n", outfn.c_str()); return 1; }
	// output text buffer: raw storage, grown without value-initialising hundreds of MB per batch
	struct RawBuf { char* p = nullptr; size_t n = 0; void resize(size_t m) { if(m > n) { free(p); p = (char*)malloc(m); n = m; if(!p) { fprintf(stderr, "out of memory\n"); exit(1); } } } char* data() { return p; } size_t size() const { return n; } ~RawBuf() { free(p); } };
	RawBuf hdr_buf;
	RawBuf& buf = hdr_buf;          // (the header; the batches' text goes through the writer's ring below)
	buf.resize(1 << 20);
	if(!nohead) {
		const size_t need = h2g_sam_header(sam, cmdline.c_str(), nullptr, 0);
		buf.resize(need + 1);
		h2g_sam_header(sam, cmdline.c_str(), buf.data(), buf.size());
		fwrite(buf.data(), 1, need, out);
	}
	const double t1 = now();
	h2g_sam_set_threads(sam, threads);
	// --no-unal with the read files: the reads are sorted by the flags of every line, the unaligned ones included, so the sink prints them and the formatter stage
	// leaves the lines with flag 0x4 out afterwards, as the reference's script does (it takes --no-unal away from its binary)
	const bool drop_unal = sorting && no_unal;
	h2g_sam_set_no_unal(sam, no_unal && !drop_unal ? 1 : 0);
	Source src(m1, m2, u, m12, fmt, threads, trim5, trim3, qcoding, sorting, skip, upto);
	ReadSorter sorter;
	for(int k = 0; k < RS_KINDS; k++) if(!rs_arg[k].empty()) sorter.open(k, rs_arg[k], rs_gz[k]);
	// --non-deterministic: every read / pair takes two draws, mate 1's seed then mate 2's, from one RandomSource seeded with time(0) (hisat2.cpp:3273,
	// :3311-3314; the reference keeps one per worker thread), in read order, before the -s test — skipped reads draw too.  H2G_ARB_SEED=<n> (test hook)
	// replaces time(0).
	h2g::Rng arb;
	arb.init(getenv("H2G_ARB_SEED") ? (uint32_t)strtoul(getenv("H2G_ARB_SEED"), nullptr, 10) : (uint32_t)time(0));
	std::vector<uint32_t> arb1, arb2;
	// (-s / -u: the record stream skips and counts, Source::next; -u counts the reads after the skipped ones, qUpto += skipReads hisat2.cpp:1959-1963)
	// Formatting on a thread of its own (round 6): the main thread fetches batch k + 1's records while batch k's text is written — what the device returns goes to one of two sets of page-locked
	// buffers, the formatter works through them in order.  Not with temporary splice sites / a novel-site file: there a batch's junctions must be in the database before the next wave starts.
	const bool async_fmt = !temp_ss && novel_out.empty() && !(getenv("H2G_CLI_ASYNC_FMT") && atoi(getenv("H2G_CLI_ASYNC_FMT")) == 0);
	const int G = gpus, H = gpus + (async_fmt ? 3 : 2);  // G streams (one per device) in flight, H host batch buffers: batch k + 1 is parsed
	std::vector<Batch> A((size_t)H), B((size_t)H);     // (on a thread of its own) into buffer (k + 1) mod H while batch k is uploaded and up to G earlier ones are on the GPUs / being written
	// What one device run takes: a run of records of one kind.  A window that mixes pairs and unpaired reads (a tabbed file) becomes two items, its pairs (merge 1) and then
	// its unpaired reads (merge 2), whose text is put back into record order (`order`: 1 = pair) before it is written: N records in windows of B make at most
	// 2 ceil(N / B) device runs however the kinds alternate.  With temporary splice sites the read ids must be exact: the two items carry their records' ids (h2g_set_read_ids), both see the wave's one snapshot of the database and their junctions are merged after the second.
	struct Item { size_t n = 0; bool paired = false; uint64_t first_id = 0, skipped = 0; int merge = 0; std::vector<uint8_t> order; std::vector<uint32_t> ids; std::vector<uint64_t> ids64; };   // ids: Read::rdid per read, for the two items of a mixed window
	struct Str { h2g_stream* st = nullptr; size_t reads = 0, bases = 0; long batch = -1; size_t n = 0; uint64_t first_id = 0; bool paired = false; int merge = 0; };
	uint64_t nsubmitted = 0, nruns = 0;
	std::vector<Str> S((size_t)G);
	uint64_t nreads = 0, naligned = 0, novf = 0, nsecond = 0;
	double t_gpu = 0, t_fmt = 0, t_parse = 0, t_up = 0, t_fetch = 0, t_stream = 0;
	// what comes back from the device lands in page-locked memory (h2g_host_alloc): the copies run at the link's rate.  The records travel compact
	// (h2g_align_*_fetch_compact: 40 bytes + 12 per edit held instead of 424 per record) and are formatted in that layout.
	struct Pinned {
		uint8_t* p = nullptr; size_t cap = 0;
		void need(size_t n) { if(n <= cap) return; h2g_host_free(p); cap = n + n / 4 + 4096; p = (uint8_t*)h2g_host_alloc(cap); if(!p) { fprintf(stderr, "hisat2-align-amd: cannot allocate %zu bytes of page-locked memory\n", cap); exit(1); } }
		~Pinned() { h2g_host_free(p); }
	};
	struct PinSet { Pinned res, rec1, rec2, o1, o2; std::vector<h2g_edit> long_edits; size_t nlong = 0; };
	PinSet pins[2];
	std::string ovf_names;
	// Temporary splice sites on G devices: a wave of W reads is cut into G shards that run side by side — a read never sees the junctions of
	// its own wave (readid + W > its id), so the shards need nothing from one another; every shard's junctions join the database (on every
	// device) before the next wave starts (the exchange between two waves is the junction list, tens of bytes per site).
	size_t wave_left = ss_wave;                           // reads the current wave still takes
	// ---- the writer: the text of a batch goes to the output on a thread of its own (6 GB of SAM per 10 M pairs: a third of the run when the main thread wrote it).
	// Three text buffers go round; the batches are written in the order they were formatted (one writer, a FIFO).
	RawBuf wtext[3];
	size_t wused[3] = {0, 0, 0};
	std::mutex wm; std::condition_variable wcv;
	std::deque<int> wqueue, wfree = {0, 1, 2};
	bool wdone = false, werr = false;
	std::thread writer([&]() {
		for(;;) {
			int i;
			{ std::unique_lock<std::mutex> lk(wm); wcv.wait(lk, [&] { return !wqueue.empty() || wdone; }); if(wqueue.empty()) return; i = wqueue.front(); wqueue.pop_front(); }
			if(wused[i] && fwrite(wtext[i].data(), 1, wused[i], out) != wused[i]) werr = true;
			{ std::lock_guard<std::mutex> lk(wm); wfree.push_back(i); }
			wcv.notify_all();
		}
	});
	auto wacquire = [&]() { std::unique_lock<std::mutex> lk(wm); wcv.wait(lk, [&] { return !wfree.empty(); }); const int i = wfree.front(); wfree.pop_front(); return i; };
	auto wsubmit = [&](int i, size_t used_) { { std::lock_guard<std::mutex> lk(wm); wused[i] = used_; wqueue.push_back(i); } wcv.notify_all(); };
	auto wfinish = [&]() { { std::lock_guard<std::mutex> lk(wm); wdone = true; } wcv.notify_all(); writer.join(); };
	// ---- the parser: batch j is read into buffer j mod H as soon as that buffer is free (batch j - H is written), ahead of the main thread
	std::mutex pm; std::condition_variable pcv;
	long parsed = 0, completed_cnt = 0;
	std::vector<Item> meta((size_t)H);
	bool perr = false;
	double t_parse_busy = 0;
	// the formatter's queue: jobs in fetch order; pinned set j is free again once its job has been formatted
	struct FmtJob { long batch; size_t n; uint64_t first_id; int set; bool paired; int merge; };
	// a mixed window: the text and record ends of its two items, until both are formatted
	RawBuf mtext[2];
	size_t mused[2] = {0, 0};
	std::vector<uint64_t> mends[2];
	std::mutex fm; std::condition_variable fcv;
	std::deque<FmtJob> fqueue;
	bool set_busy[2] = {false, false}, fdone = false;
	long nfetched = 0;
	// format + hand to the writer: the item whose records lie in pinned set `job.set`.
	// the SAM text of one item into `buf` (grown as needed); `ends`: where each record's text ends, when asked for
	auto format_item = [&](const FmtJob& job, RawBuf& buf, size_t& used, std::vector<uint64_t>* ends) {
		Batch& a = A[(size_t)(job.batch % H)]; Batch& b = B[(size_t)(job.batch % H)];
		PinSet& ps = pins[job.set];
		const size_t n = job.n;
		const bool paired = job.paired;
		used = 0;
		h2g_sam_set_first_read_id(sam, job.first_id);
		const std::vector<uint64_t>& ids64 = meta[(size_t)(job.batch % H)].ids64;
		h2g_sam_set_read_ids(sam, ids64.empty() ? nullptr : ids64.data());
		h2g_sam_set_long_edits(sam, ps.nlong ? ps.long_edits.data() : nullptr, ps.nlong);
		if(ends) { ends->resize(n); h2g_sam_set_record_ends(sam, ends->data()); }
		const bool qc = qc_filter && !a.filt.empty();
		h2g_sam_set_read_filter(sam, qc ? a.filt.data() : nullptr, qc && paired ? b.filt.data() : nullptr);
		if(paired) {
			h2g_pair_result* pres = (h2g_pair_result*)ps.res.p;
			uint64_t *ao1 = (uint64_t*)ps.o1.p, *ao2 = (uint64_t*)ps.o2.p;
			buf.resize(n * 1400 + 6 * (a.codes.size() + b.codes.size()) + 4096);
			h2g_status rc = h2g_sam_format_paired_compact(sam, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(),
			                                      b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n,
			                                      pres, ps.rec1.p, ao1, ps.rec2.p, ao2, P.khits, buf.data(), buf.size(), &used);
			if(rc != H2G_OK) {
				buf.resize(used + 16);
				rc = h2g_sam_format_paired_compact(sam, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(),
				                           b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n,
				                           pres, ps.rec1.p, ao1, ps.rec2.p, ao2, P.khits, buf.data(), buf.size(), &used);
				if(rc != H2G_OK) die("h2g_sam_format_paired_compact");
			}
			for(size_t i = 0; i < n; i++) { naligned += pres[i].npairs > 0; if(pres[i].overflow) { novf++; if(ovf_names.size() < 4096) { ovf_names.append(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i]); ovf_names += " (bits " + std::to_string(pres[i].overflow) + ")\n"; } } }
		} else {
			h2g_read_result* res = (h2g_read_result*)ps.res.p;
			uint64_t* ao1 = (uint64_t*)ps.o1.p;
			buf.resize(n * 700 + 3 * a.codes.size() + 4096);
			h2g_status rc = h2g_sam_format_unpaired_compact(sam, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(), n,
			                                        res, ps.rec1.p, ao1, buf.data(), buf.size(), &used);
			if(rc != H2G_OK) {
				buf.resize(used + 16);
				rc = h2g_sam_format_unpaired_compact(sam, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(), n,
				                             res, ps.rec1.p, ao1, buf.data(), buf.size(), &used);
				if(rc != H2G_OK) die("h2g_sam_format_unpaired_compact");
			}
			for(size_t i = 0; i < n; i++) { naligned += res[i].nselect > 0; if(res[i].overflow) { novf++; if(ovf_names.size() < 4096) { ovf_names.append(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i]); ovf_names += " (bits " + std::to_string(res[i].overflow) + ")\n"; } } }
		}
		h2g_sam_set_record_ends(sam, nullptr);
		h2g_sam_set_read_ids(sam, nullptr);
		h2g_sam_set_read_filter(sam, nullptr, nullptr);
	};
	// the original text of record i of an item goes to the --un / --al files its lines [t, te) name
	auto sort_record = [&](const Batch& a, const Batch* b, size_t i, const char* t, const char* te) {
		sorter.record(t, te, a.orig.data() + a.ooffs[i], (size_t)(a.ooffs[i + 1] - a.ooffs[i]),
		              b && b->ooffs.size() > i + 1 ? b->orig.data() + b->ooffs[i] : nullptr, b && b->ooffs.size() > i + 1 ? (size_t)(b->ooffs[i + 1] - b->ooffs[i]) : 0);
	};
	auto format_job = [&](const FmtJob& job) {
		Batch& a = A[(size_t)(job.batch % H)]; Batch& b = B[(size_t)(job.batch % H)];
		const size_t n = job.n;
		size_t used = 0;
		const double tf = now();
		if(job.merge == 1) {                          // the pairs of a mixed window wait for its unpaired reads
			format_item(job, mtext[0], mused[0], &mends[0]);
			t_fmt += now() - tf;
			nreads += n;
			return;
		}
		const int wi = wacquire();
		RawBuf& buf = wtext[wi];
		if(job.merge == 2) {
			format_item(job, mtext[1], mused[1], &mends[1]);
			Batch& pa = A[(size_t)((job.batch - 1) % H)]; Batch& pb = B[(size_t)((job.batch - 1) % H)];
			const std::vector<uint8_t>& order = meta[(size_t)(job.batch % H)].order;
			used = mused[0] + mused[1];
			buf.resize(used + 16);
			size_t at = 0, ip = 0, is = 0;
			for(uint8_t k : order) {
				const int m = k ? 0 : 1;
				size_t& i = k ? ip : is;
				const uint64_t t0_ = i ? mends[m][i - 1] : 0, t1_ = mends[m][i];
				memcpy(buf.data() + at, mtext[m].data() + t0_, (size_t)(t1_ - t0_));
				if(sorter.on) sort_record(k ? pa : a, k ? &pb : nullptr, i, buf.data() + at, buf.data() + at + (t1_ - t0_));
				at += (size_t)(t1_ - t0_);
				i++;
			}
		} else {
			std::vector<uint64_t>& ends = mends[0];
			format_item(job, buf, used, sorter.on ? &ends : nullptr);
			if(sorter.on) for(size_t i = 0; i < n; i++) sort_record(a, job.paired ? &b : nullptr, i, buf.data() + (i ? ends[i - 1] : 0), buf.data() + ends[i]);
		}
		if(drop_unal) {                               // --no-unal: the lines with flag 0x4 go, in place
			char* o = buf.data();
			for(const char* t = buf.data(), *te = buf.data() + used; t < te;) {
				const char* le = (const char*)memchr(t, '\n', (size_t)(te - t));
				le = le ? le + 1 : te;
				const char* tab = (const char*)memchr(t, '\t', (size_t)(le - t));
				if(!(tab && (strtoul(tab + 1, nullptr, 10) & 4u))) { memmove(o, t, (size_t)(le - t)); o += le - t; }
				t = le;
			}
			used = (size_t)(o - buf.data());
		}
		t_fmt += now() - tf;
		wsubmit(wi, used);
		if(temp_ss || !novel_out.empty()) {   // the junctions of the lines just written join the database (SpliceSiteDB::addSpliceSite: smallest read id per site)
			static std::vector<h2g_splice_site> novel;
			const size_t k = h2g_sam_take_novel_sites(sam, nullptr, 0);
			novel.resize(k);
			if(k) h2g_sam_take_novel_sites(sam, novel.data(), k);
			// only what is new (or whose smallest read id went down) goes to the devices and the formatter: they merge it into their sorted
			// copies (h2g_index_add_splice_sites) — the cost of a wave is its own junctions, not the database's size
			static std::vector<h2g_splice_site> delta;
			delta.clear();
			if(temp_ss) for(const h2g_splice_site& x : novel) {
				const std::array<uint32_t, 4> key = {x.tidx, x.left, x.right, (uint32_t)x.dir};
				auto it = site_at.find(key);
				if(it == site_at.end()) { site_at.emplace(key, sites.size()); sites.push_back(x); delta.push_back(x); }
				else if(!sites[it->second].fromfile && x.readid < sites[it->second].readid) { sites[it->second].readid = x.readid; delta.push_back(sites[it->second]); }
			}
			if(!delta.empty()) {
				for(int g2 = 0; g2 < gpus; g2++) {
					bool first = true;
					for(int q = 0; q < g2; q++) if(ixs[(size_t)q] == ixs[(size_t)g2]) first = false;
					if(first && h2g_index_add_splice_sites(ixs[(size_t)g2], delta.data(), delta.size()) != H2G_OK) die("cannot upload the splice sites");
				}
				h2g_sam_add_splice_sites(sam, delta.data(), delta.size());
			}
		}
		nreads += n;
		{ std::lock_guard<std::mutex> lk(pm); completed_cnt += job.merge == 2 ? 2 : 1; }      // (its read buffers are free for the parser; a mixed window's pairs were kept for its merge)
		pcv.notify_all();
	};
	std::thread formatter;
	if(async_fmt) formatter = std::thread([&]() {
		for(;;) {
			FmtJob job;
			{ std::unique_lock<std::mutex> lk(fm); fcv.wait(lk, [&] { return !fqueue.empty() || fdone; }); if(fqueue.empty()) return; job = fqueue.front(); fqueue.pop_front(); }
			format_job(job);
			{ std::lock_guard<std::mutex> lk(fm); set_busy[job.set] = false; }
			fcv.notify_all();
		}
	});
	auto ffinish = [&]() { if(formatter.joinable()) { { std::lock_guard<std::mutex> lk(fm); fdone = true; } fcv.notify_all(); formatter.join(); } };
	// fetch (+ format + write, or hand to the formatter) the batch that stream `g` carries
	auto complete = [&](int g) {
		Str& sg = S[(size_t)g];
		if(sg.batch < 0) return;
		h2g_stream* st = sg.st;
		const size_t n = sg.n;
		const bool paired = sg.paired;
		const int set = (int)(nfetched % 2);
		if(async_fmt) { std::unique_lock<std::mutex> lk(fm); fcv.wait(lk, [&] { return !set_busy[set]; }); set_busy[set] = true; }
		PinSet& ps = pins[set];
		const double tq0 = now();
		{	// records with more than H2G_MAX_EDITS edits (long deletions: one edit per base) keep their lists in the stream's long-edit area
			size_t nl = 0;
			h2g_status lrc = h2g_align_fetch_long_edits(st, nullptr, 0, &nl);
			if(nl) { ps.long_edits.resize(nl); lrc = h2g_align_fetch_long_edits(st, ps.long_edits.data(), ps.long_edits.size(), &nl); }
			if(lrc != H2G_OK) die("h2g_align_fetch_long_edits");
			ps.nlong = nl;
		}
		if(paired) {
			ps.res.need(n * sizeof(h2g_pair_result)); ps.o1.need((n + 1) * 8); ps.o2.need((n + 1) * 8);
			ps.rec1.need(n * 64 + 4096); ps.rec2.need(n * 64 + 4096);
			h2g_pair_result* pres = (h2g_pair_result*)ps.res.p;
			uint64_t *ao1 = (uint64_t*)ps.o1.p, *ao2 = (uint64_t*)ps.o2.p;
			ao1[n] = 0; ao2[n] = 0;
			if(const h2g_status frc = h2g_align_pairs_fetch_compact(st, pres, ps.rec1.p, ps.rec1.cap, ao1, ps.rec2.p, ps.rec2.cap, ao2, 0, n); frc != H2G_OK) {
				// one retry, and only for "buffer too small": H2G_ERR_ARG with the bytes needed in boffs[n] (zeroed above: page-locked memory starts uninitialised)
				if(frc != H2G_ERR_ARG || (ao1[n] <= ps.rec1.cap && ao2[n] <= ps.rec2.cap)) die("h2g_align_pairs_fetch_compact");
				ps.rec1.need(ao1[n] + 8); ps.rec2.need(ao2[n] + 8);
				if(h2g_align_pairs_fetch_compact(st, pres, ps.rec1.p, ps.rec1.cap, ao1, ps.rec2.p, ps.rec2.cap, ao2, 0, n) != H2G_OK) die("h2g_align_pairs_fetch_compact");
			}
		} else {
			ps.res.need(n * sizeof(h2g_read_result)); ps.o1.need((n + 1) * 8); ps.rec1.need(n * 64 + 4096);
			h2g_read_result* res = (h2g_read_result*)ps.res.p;
			uint64_t* ao1 = (uint64_t*)ps.o1.p;
			ao1[n] = 0;
			if(const h2g_status frc = h2g_align_fetch_compact(st, res, ps.rec1.p, ps.rec1.cap, ao1, 0, n); frc != H2G_OK) {
				if(frc != H2G_ERR_ARG || ao1[n] <= ps.rec1.cap) die("h2g_align_fetch_compact");
				ps.rec1.need(ao1[n] + 8);
				if(h2g_align_fetch_compact(st, res, ps.rec1.p, ps.rec1.cap, ao1, 0, n) != H2G_OK) die("h2g_align_fetch_compact");
			}
		}
		{ h2g_counters hc; if(h2g_get_counters(st, &hc) == H2G_OK) nsecond += hc.n_second_pass; }
		t_fetch += now() - tq0;
		const FmtJob job{sg.batch, n, sg.first_id, set, paired, sg.merge};
		nfetched++;
		sg.batch = -1;                                  // (the stream's rows are copied: it can take the next batch)
		if(async_fmt) { { std::lock_guard<std::mutex> lk(fm); fqueue.push_back(job); } fcv.notify_all(); }
		else format_job(job);
	};
	std::thread parser([&]() {
		size_t pwave_left = ss_wave;
		long j = 0;
		Win w;
		Batch sa, sb;
		// hands one item to the main thread: into buffer j mod H as soon as that buffer is free
		auto emit = [&](Batch& a, Batch* b, Item&& it, bool bad) {
			{ std::unique_lock<std::mutex> lk(pm); pcv.wait(lk, [&] { return j < completed_cnt + H; }); }
			std::swap(A[(size_t)(j % H)], a);
			if(b) std::swap(B[(size_t)(j % H)], *b);
			{ std::lock_guard<std::mutex> lk(pm); meta[(size_t)(j % H)] = std::move(it); perr = perr || bad; parsed = j + 1; }
			pcv.notify_all();
			j++;
		};
		for(;;) {
			const double tp = now();
			size_t want = batch;
			if(temp_ss) { const size_t shard = (ss_wave + (size_t)gpus - 1) / (size_t)gpus; want = std::min(want, std::min(shard, pwave_left)); }
			const bool more = src.next(w, want);
			const bool bad = src.short_mates();
			if(!more || bad) { t_parse_busy += now() - tp; w.a.clear(); emit(w.a, nullptr, Item(), bad); return; }
			if(temp_ss) { pwave_left -= w.n; if(pwave_left == 0) pwave_left = ss_wave; }
			uint64_t skipped = w.skipped;
			if(w.kinds.empty()) {
				t_parse_busy += now() - tp;
				Item it; it.n = w.n; it.paired = w.paired; it.first_id = w.first_id; it.skipped = skipped;
				emit(w.a, w.paired ? &w.b : nullptr, std::move(it), false);
				continue;
			}
			{                                           // a window of both kinds: its pairs, then its unpaired reads, each read under its record's id
				Batch pa, pb;
				pa.clear(); pb.clear(); sa.clear();
				pa.have_quals = pb.have_quals = sa.have_quals = true;
				Item ip, is;
				for(size_t i = 0; i < w.n; i++) {
					Item& it = w.kinds[i] ? ip : is;
					if(w.kinds[i]) { pa.take(w.a, i); pb.take(w.b, i); } else sa.take(w.a, i);
					it.ids.push_back((uint32_t)(w.first_id + i)); it.ids64.push_back(w.first_id + i);
				}
				t_parse_busy += now() - tp;
				ip.n = w.npairs; ip.paired = true; ip.first_id = w.first_id; ip.skipped = skipped; ip.merge = 1;
				is.n = w.n - w.npairs; is.first_id = w.first_id; is.merge = 2; is.order.swap(w.kinds);
				emit(pa, &pb, std::move(ip), false);
				emit(sa, nullptr, std::move(is), false);
			}
		}
	});
	struct Joiner { std::thread& t; ~Joiner() { if(t.joinable()) t.detach(); } } pjoin{parser}, wjoin{writer}, fjoin{formatter};      // (an early `return` / exit leaves no joinable thread behind)
	for(long k = 0;; k++) {
		Batch& a = A[(size_t)(k % H)]; Batch& b = B[(size_t)(k % H)];
		double tp = now();
		size_t n;
		bool perr_now, paired;
		uint64_t first_id, skipped;
		int merge;
		{
			std::unique_lock<std::mutex> lk(pm);
			pcv.wait(lk, [&] { return parsed > k; });
			const Item& it = meta[(size_t)(k % H)];
			n = it.n; paired = it.paired; first_id = it.first_id; skipped = it.skipped; merge = it.merge; perr_now = perr;
		}
		if(perr_now) {
			// the parser has returned (it stops at the short file); the writer waits on a condition variable that lives in this frame: both threads are
			// joined before the frame goes (a detached waiter would block the variable's destructor for ever)
			fprintf(stderr, "Error, fewer reads in file specified with -2 than in file specified with -1\n");
			parser.join();
			ffinish();
			wfinish();
			return 1;
		}
		t_parse += now() - tp;                         // (what the main thread waited for the parser)
		if(n == 0 && merge == 0) break;
		const int g = (int)(k % G);
		const double tg = now();
		if(temp_ss) {                                  // a wave needs the sites of every earlier one: nothing of them stays in flight when it starts
			if(wave_left == ss_wave) for(long q = k - G; q < k; q++) if(q >= 0) complete((int)(q % G));
			wave_left -= n;
			if(wave_left == 0) wave_left = ss_wave;
		}
		complete(g);                                   // the batch this stream still carries (k - G): the oldest one in flight
		Str& sg = S[(size_t)g];
		size_t bases = a.codes.size();
		if(paired && b.codes.size() > bases) bases = b.codes.size();
		if(!sg.st || n > sg.reads || bases > sg.bases) {
			if(sg.st) h2g_stream_free(sg.st);
			sg.reads = n > batch ? n : batch; sg.bases = bases + bases / 4 + 1024;
			const double ts = now();
			if(h2g_stream_create(ixs[(size_t)g], sg.reads, sg.bases, &sg.st) != H2G_OK) die("cannot create the device stream");
			t_stream += now() - ts;
		}
		const double tq0 = now();
		if(h2g_set_reads(sg.st, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, n) != H2G_OK) die("h2g_set_reads");
		if(h2g_set_read_names(sg.st, a.names.data(), a.noffs.data(), n) != H2G_OK) die("h2g_set_read_names");
		// read ids are 32 bits in the splice-site window test (DSpliceSite::readid): past that the temporary sites' visibility would wrap silently
		const std::vector<uint32_t>& ids = meta[(size_t)(k % H)].ids;      // (the slot is the parser's again only after this item was formatted)
		if(!ids.empty() && h2g_set_read_ids(sg.st, ids.data()) != H2G_OK) die("h2g_set_read_ids");
		if(temp_ss && (ids.empty() ? first_id + n : meta[(size_t)(k % H)].ids64.back() + 1) > 0xffffffffull) die("read ids beyond 2^32 with temporary splice sites (use --no-temp-splicesite or split the input)");
		P.first_read_id = (uint32_t)first_id;
		sg.first_id = first_id;
		nsubmitted += n;
		// the chain mode (window 0: waves of ONE read) is exact and meant for small inputs; an input that turns out not to be small is told so,
		// loudly and once (a small run's stderr stays the reference's summary, byte for byte)
		if(temp_ss && ss_window == 0 && nsubmitted >= 20000 && nsubmitted - n < 20000 && !getenv("H2G_QUIET_CHAIN_WARNING"))
			fprintf(stderr, "Warning: hisat2-align-amd: -p 1 with temporary splice sites is the reference's strict read-after-read chain (window 0, hisat2.cpp:3687): "
			                "it runs as waves of ONE read - a device round trip and a database merge per read; 20000 reads in, this input is not small. "
			                "Use -p >= 2 or --ss-window W (output == hisat2 -p W/1000 --reorder), or --no-temp-splicesite, for throughput.\n");
		if(paired) {
			if(h2g_set_mates(sg.st, b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n) != H2G_OK) die("h2g_set_mates");
		}
		if(arbitrary_random) {                         // this batch's draws, in read order (the batches are submitted in read order whatever the device); the skipped reads draw too
			for(uint64_t r = 0; r < 2 * skipped; r++) arb.nextU32();
			arb1.resize(n); arb2.resize(n);
			for(size_t r = 0; r < n; r++) { arb1[r] = arb.nextU32(); arb2[r] = arb.nextU32(); }
			if(h2g_set_read_seeds(sg.st, arb1.data(), paired ? arb2.data() : nullptr, n) != H2G_OK) die("h2g_set_read_seeds");
		}
		// --qc-filter: a read whose QSEQ filter field is '0' is not aligned (every other format's reads pass)
		if(qc_filter && !a.filt.empty() && h2g_set_read_filter(sg.st, a.filt.data(), paired ? b.filt.data() : nullptr) != H2G_OK) die("h2g_set_read_filter");
		if(paired) {
			if(h2g_align_pairs_run(sg.st, &P) != H2G_OK) die("h2g_align_pairs_run");
		} else if(h2g_align_run(sg.st, &P) != H2G_OK) die("h2g_align_run");
		nruns++;
		t_up += now() - tq0;
		sg.batch = k; sg.n = n; sg.paired = paired; sg.merge = merge;
		t_gpu += now() - tg;
	}
	{   // drain, oldest first
		long oldest = -1;
		for(;;) {
			int gi = -1;
			for(int g = 0; g < G; g++) if(S[(size_t)g].batch >= 0 && (gi < 0 || S[(size_t)g].batch < oldest)) { gi = g; oldest = S[(size_t)g].batch; }
			if(gi < 0) break;
			const double tg = now();
			complete(gi);
			t_gpu += now() - tg;
		}
	}
	if(parser.joinable()) parser.join();
	ffinish();
	wfinish();
	if(werr) { fprintf(stderr, "Error: writing the SAM output failed\n"); return 1; }
	if(out != stdout) fclose(out); else fflush(out);
	if(!sorter.close()) { fprintf(stderr, "Error: writing the --un / --al read files failed\n"); return 1; }
	if(!novel_out.empty()) {                              // hisat2.cpp:4189-4197
		FILE* nf = fopen(novel_out.c_str(), "w");
		if(nf) {
			const size_t need = h2g_sam_novel_splice_sites_text(sam, nullptr, 0);
			std::vector<char> tb(need + 1);
			h2g_sam_novel_splice_sites_text(sam, tb.data(), need);
			fwrite(tb.data(), 1, need, nf);
			fclose(nf);
		}
	}
	const double t2 = now();
	{   // the reference's alignment summary (aln_sink.h:1637), same text
		const size_t need = h2g_sam_summary(sam, nullptr, 0);
		std::vector<char> sb(need + 1);
		h2g_sam_summary(sam, sb.data(), need);
		if(!quiet) fwrite(sb.data(), 1, need, stderr);
		if(!quiet && !summary_file.empty()) { FILE* sf = fopen(summary_file.c_str(), "w"); if(sf) { fwrite(sb.data(), 1, need, sf); fclose(sf); } }   // hisat2.cpp:4175
	}
	(void)naligned; (void)nreads;
	// Reads whose lists overflow the default device workspace are re-run on the device with the large one (h2g_align_run's
	// second pass).  What is still flagged after that is NOT known to equal the reference's output: name it and fail.
	if(novf) fprintf(stderr, "Error: %llu %s exceeded even the large device workspace (h2g overflow bit); their SAM records are not verified "
	                 "against hisat2 -- rerun these with the reference aligner:\n%s", (unsigned long long)novf, "reads / pairs", ovf_names.c_str());
	if(getenv("H2G_CLI_TIMING")) fprintf(stderr, "time: index load %.2f s, align+fetch %.2f s (waited for the parser thread %.2f s; it parsed for %.2f s), SAM formatting %.2f s, total %.2f s [stream create %.2f, upload+launch %.2f, wait+fetch %.2f]\n", t1 - t0, t_gpu,
	        t_parse, t_parse_busy, t_fmt, t2 - t0, t_stream, t_up, t_fetch);
	if(!stats_fn.empty()) {
		FILE* sf = fopen(stats_fn.c_str(), "w");
		if(sf) { fprintf(sf, "{\"reads\": %llu, \"second_pass\": %llu, \"overflow\": %llu, \"runs\": %llu}\n", (unsigned long long)nreads, (unsigned long long)nsecond, (unsigned long long)novf, (unsigned long long)nruns); fclose(sf); }
	}
	// (Measured and not shipped, round 6: ending the process here without the frees below saves this run 0.1 s and costs the NEXT process 1.7 s — the driver reclaims 40 GB of
	// device memory of a process that did not return it while the next one is already allocating: profiles/r06_zc_ab.log.)
	for(auto& sg : S) if(sg.st) h2g_stream_free(sg.st);
	h2g_sam_close(sam);
	for(int g = 0; g < gpus; g++) { bool dup = false; for(int q = 0; q < g; q++) dup |= ixs[(size_t)q] == ixs[(size_t)g]; if(!dup) h2g_index_free(ixs[(size_t)g]); }
	return novf ? 3 : 0;
}
