// h2g_cli_reads.h — read ingestion of the command line (h2g_cli.cpp): batches of reads (`Batch`), the quality codings and base tables, the parallel parser of one
// list of files (`Reader`: FASTA / FASTQ, the parse rules of pat.cpp:725-1010; tabbed and QSEQ files, pat.cpp:1159-1503 and read_qseq.cpp) and the record stream in
// front of the batches (`Source`: a record is an unpaired read or a pair; -1/-2 with -U, tabbed files that mix both).  Header-only, host code.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <math.h>
#include <string>
#include <vector>
#include <thread>
#include <algorithm>
#include <fcntl.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <zlib.h>
#include "../../include/h2g.h"

namespace h2g_cli {

struct Batch {
	std::vector<uint8_t>  codes;
	std::vector<uint32_t> offs, noffs;
	std::string           quals, names;
	bool                  have_quals = false;
	std::vector<uint8_t>  filt;                  // QSEQ sources only, one per read: 0 = the record's filter field is '0' (--qc-filter), 1 = it passes
	std::string           orig;                  // --un / --al ...: the records' text as it stood in the input, record i = [ooffs[i], ooffs[i + 1]); kept only when asked for
	std::vector<uint64_t> ooffs;
	// --h2g-device-parse: the FASTQ text of the batch's raw_n records for h2g_set_reads_fastq, every record exactly four lines: a file's last record is cut behind its fourth
	// line (blank lines behind it are not the record's) and, where the file ends earlier, filled up with '\n' — raw_short then has (record, its bytes in the file), so that the
	// host parser sees it as it stood.  The arrays above are filled from the device afterwards.  raw_first: the running number of its first record (the name of a record without one)
	std::string           raw;
	size_t                raw_n = 0;
	uint64_t              raw_first = 0;
	std::vector<std::pair<size_t, size_t> > raw_short;
	size_t n() const { return offs.empty() ? 0 : offs.size() - 1; }
	void clear() { codes.clear(); offs.assign(1, 0); noffs.assign(1, 0); quals.clear(); names.clear(); filt.clear(); orig.clear(); ooffs.assign(1, 0); raw.clear(); raw_n = 0; raw_first = 0; raw_short.clear(); }
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

// the bytes of a file, inflated when its name ends in .gz (-F plans over whole files); false: it could not be opened
inline bool read_whole_file(const std::string& fn, std::vector<char>& out) {
	out.clear();
	gzFile g = gzopen(fn.c_str(), "rb");      // (zlib hands a file that is not gzipped through as it is)
	if(!g) return false;
	gzbuffer(g, 1 << 20);
	std::vector<char> chunk(8 << 20);
	int got;
	while((got = gzread(g, chunk.data(), (unsigned)chunk.size())) > 0) out.insert(out.end(), chunk.begin(), chunk.begin() + got);
	gzclose(g);
	return got == 0;
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
			if(raw_) {      // the records' bytes travel as they are; records of two files are concatenated
				if(b.raw_n == 0) b.raw_first = count_;
				size_t end = starts_[cur_ + take], lines = 4;
				if(cur_ + take == nrec()) {      // the file's last record ends behind its fourth line, or with the file
					lines = 0;
					for(end = starts_[nrec() - 1]; end < n_ && lines < 4; end++) lines += p_[end] == '\n';
				}
				b.raw.append(p_ + starts_[cur_], end - starts_[cur_]);
				b.raw_n += take;
				if(lines < 4) { b.raw_short.emplace_back(b.raw_n - 1, end - starts_[nrec() - 1]); b.raw.append(4 - lines, '\n'); }
				cur_ += take; got += take; count_ += take;
				continue;
			}
			const size_t T = std::min<size_t>((size_t)T_, take / 4096 + 1);
			std::vector<Batch> part(T), part2(tabbed ? T : 0);
			std::vector<std::vector<uint8_t> > pk(tabbed ? T : 0);
			// (fork-join: `work` captures by reference and runs on helper threads that are joined before this block ends)
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
	// the records of b.raw through parse_record, under this reader's options: what fill() would have made of them (the names of records without one and the
	// messages of malformed ones included).  For the items h2g_set_reads_fastq hands back to the host, and for the records -s skips.  max: the first so many records only
	// (a -2 file may hold more records than its -1 file: nobody looks at them)
	void parse_raw(Batch& b, size_t max = ~(size_t)0) const {
		Reader t(std::vector<std::string>(), fmt_, 1, trim5_, trim3_);
		t.qc_ = qc_;
		std::string text;
		text.swap(b.raw);
		const uint64_t first = b.raw_first;
		std::vector<std::pair<size_t, size_t> > shorter;
		shorter.swap(b.raw_short);
		b.clear();
		b.have_quals = true;
		t.p_ = text.data(); t.n_ = text.size(); t.count_ = first;
		size_t line = 0;
		if(t.n_) t.starts_.push_back(0);
		for(size_t i = 0; i < t.n_; i++) if(t.p_[i] == '\n') { line++; if((line & 3) == 0) t.starts_.push_back(i + 1); }      // (every record of the text is four lines)
		t.ends_.assign(t.starts_.begin() + (t.starts_.empty() ? 0 : 1), t.starts_.end());
		for(const auto& x : shorter) if(x.first < t.ends_.size()) t.ends_[x.first] = t.starts_[x.first] + x.second;
		for(size_t r = 0; r < t.nrec() && r < max; r++) t.parse_record(r, b);
		t.p_ = nullptr; t.starts_.clear();                                                  // (the text is not a mapped file)
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
		std::vector<std::thread> th;   // (fork-join: the scans below capture by reference; every helper thread is joined before its branch ends)
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
		const char* end = p_ + (ends_.empty() ? starts_[r + 1] : ends_[r]);
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
	bool raw_ = false;              // --h2g-device-parse (FASTQ): fill() hands on the records' bytes (Batch::raw) instead of parsing them
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
	std::vector<size_t> ends_;      // parse_raw only: where record r ends when that is not where record r + 1 starts
	std::vector<char> inflated_;
	uint64_t count_ = 0;
};

// A window of the record stream: up to a batch of consecutive records.  A record is one unpaired read or one pair.  `a` holds the unpaired reads and the
// first mates, `b` the second mates; in a window of a tabbed file the two stay index-aligned (an unpaired read has an empty read in `b`) and `kinds` says
// which records are pairs.
struct Win {
	Batch a, b;
	std::vector<h2g_window_seg> wsegs;   // -F: the segments the window's reads are cut from (the device expands them itself), and the reads' ids
	std::vector<uint64_t> ids64;
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
	       ReadFormat fmt, int threads, uint32_t trim5, uint32_t trim3, const QualCoding& qc, bool keep_orig, uint64_t skip, uint64_t upto, bool raw = false) : skip_(skip), upto_(upto) {
		auto mk = [&](const std::vector<std::string>& files) { Reader* r = new Reader(files, fmt, threads, trim5, trim3); r->qc_ = qc; r->keep_orig_ = keep_orig; r->raw_ = raw && fmt == FMT_FASTQ; return r; };
		if(!tab.empty()) segs_.push_back(Seg{mk(tab), nullptr, true});
		else {
			if(!m1.empty() && !m2.empty()) segs_.push_back(Seg{mk(m1), mk(m2), false});
			if(!u.empty()) segs_.push_back(Seg{mk(u), nullptr, false});
		}
	}
	// -F <len>,<step>: the reads are the windows [first, first + n) of a plan (include/h2g.h; the -s / -u selection is the caller's, h2g_window_plan_select)
	Source(const h2g_window_plan* plan, uint64_t first, uint64_t n) : plan_(plan), wcur_(first), wleft_(n), skip_(0), upto_(0) {}
	~Source() { for(Seg& s : segs_) { delete s.a; delete s.b; } }
	Source(const Source&) = delete;
	bool short_mates() const { return short_mates_; }         // the -2 files ran out before the -1 files
	// the reader whose options a batch's raw text is parsed under when the device hands it back (every reader of a source has the same)
	const Reader* any_reader() const { return segs_.empty() ? nullptr : segs_[0].a; }
	bool next(Win& w, size_t max) {
		w.a.clear(); w.b.clear(); w.kinds.clear(); w.n = w.npairs = 0; w.skipped = 0; w.paired = false;
		w.wsegs.clear(); w.ids64.clear();
		if(plan_) return next_windows(w, max);
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
					parse_if_raw(s, ja, jb, g);                     // (no device sees them: a malformed one among them ends the run as it does without --h2g-device-parse)
					left -= g; s.id += g; w.skipped += g;
				}
			}
			if(s.budget == 0) {                                   // -u reached: with records left here the run ends, else the next segment starts
				ja.clear(); jb.clear();
				if(fill(s, ja, jb, jk, 1)) { parse_if_raw(s, ja, jb, 1); si_ = segs_.size(); return false; }
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
	// the next up to `max` windows, expanded on the host for the SAM text: codes, names (the record's prefix and the decimal offset) and ids
	bool next_windows(Win& w, size_t max) {
		if(wleft_ == 0 || max == 0) return false;
		const uint64_t g = std::min<uint64_t>(max, wleft_);
		h2g_window_plan_info pi;
		h2g_window_plan_get_info(plan_, &pi);
		w.wsegs.resize(h2g_window_plan_segments(plan_, wcur_, g, nullptr, 0));
		h2g_window_plan_segments(plan_, wcur_, g, w.wsegs.data(), w.wsegs.size());
		const uint8_t* text = h2g_window_plan_text(plan_);
		const char* pre = h2g_window_plan_prefixes(plan_);
		w.a.codes.reserve((size_t)g * pi.len);
		char num[24];
		for(const h2g_window_seg& s : w.wsegs) for(uint64_t j = 0; j < s.n_windows; j++) {
			const uint8_t* t = text + s.text_start + j * pi.step;
			w.a.codes.insert(w.a.codes.end(), t, t + pi.len);
			w.a.offs.push_back((uint32_t)w.a.codes.size());
			w.a.names.append(pre + s.prefix_start, s.prefix_len);
			w.a.names.append(num, (size_t)snprintf(num, sizeof num, "%llu", (unsigned long long)(s.name_off0 + j * pi.step)));
			w.a.noffs.push_back((uint32_t)w.a.names.size());
			w.ids64.push_back(s.rdid0 + j * pi.step);
		}
		w.n = (size_t)g; w.first_id = w.ids64.front();
		if(!wstarted_) { w.skipped = wcur_; wstarted_ = true; }
		wcur_ += g; wleft_ -= g;
		return true;
	}
	const h2g_window_plan* plan_ = nullptr;
	uint64_t wcur_ = 0, wleft_ = 0;
	bool wstarted_ = false;
	struct Seg { Reader* a; Reader* b; bool tabbed; uint64_t id = 0, budget = 0; bool started = false; };
	size_t fill(Seg& s, Batch& a, Batch& b, std::vector<uint8_t>& kinds, size_t w) {
		if(s.tabbed) return s.a->fill(a, w, &b, &kinds);
		if(!s.b) return s.a->fill(a, w);
		// the two mate files are parsed side by side (each fill is threaded in itself; one after the other they were a second per 10 M pairs, and the main thread waited for them)
		size_t nb = 0;
		std::thread tb([&nb, &s, &b, w]() { nb = s.b->fill(b, w); });
		const size_t n = s.a->fill(a, w);
		tb.join();
		if(nb < n) short_mates_ = true;                           // (-2 ran out before -1: the reference's error; a longer -2 is not looked at)
		return n;
	}
	// --h2g-device-parse: records that are read and dropped (-s, the probe behind -u) go through the host parser, as they do without the flag
	static void parse_if_raw(const Seg& s, Batch& a, Batch& b, size_t n) {
		if(a.raw_n) s.a->parse_raw(a, n);
		if(s.b && b.raw_n) s.b->parse_raw(b, n);
	}
	std::vector<Seg> segs_;
	size_t si_ = 0;
	uint64_t skip_, upto_;
	bool short_mates_ = false;
};

}  // namespace h2g_cli
