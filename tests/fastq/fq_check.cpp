// fq_check.cpp — drives the functions of csrc/h2g_fastq.h lane by lane, as the kernels of h2g_set_reads_fastq do (16-byte chunks, 256-lane workgroups, the scans between
// them), and compares what they write with the command line's host parser (Reader, csrc/h2g_cli_reads.h) byte for byte.  Texts with one record that is not plain must be
// flagged at that record.  With file arguments it also prints, per file, how many of its records are plain ("plain <file> <plain> <records>").
// Stand-alone host program, built by tests/test_fastq_cpu.py with -fsanitize=address,undefined: every buffer has exactly the size the library gives it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../hisat2_amd/csrc/h2g_fastq.h"
#include "../../hisat2_amd/csrc/h2g_cli_reads.h"

using namespace h2g_fq;
static int g_fail = 0, g_checks = 0;
#define CHECK(c, ...) do { g_checks++; if(!(c)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Out {
	uint64_t n = 0, consumed = 0, n_not_plain = 0, first_not_plain = 0;
	uint32_t max_len = 0;
	std::vector<uint8_t> codes; std::vector<char> quals, names;
	std::vector<uint32_t> offs, noffs;
	uint64_t nb = 0, nn = 0;
};

static bool same(const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }
static void excl_scan(std::vector<unsigned long long>& v) { unsigned long long run = 0; for(auto& x : v) { const unsigned long long t = x; x = run; run += t; } }

// what h2g_set_reads_fastq does with one text, lane by lane
static Out device_parse(const std::string& text, const Opts& o, bool final, uint64_t max_records) {
	Out out;
	const uint32_t n_text = (uint32_t)text.size();
	std::vector<uint8_t> t(((size_t)n_text + 15) / 16 * 16 + 16, 0xaa);      // (the library's buffer: the text and what a last dwordx4 load reads past it)
	memcpy(t.data(), text.data(), n_text);
	// 1. newline counts per workgroup of 256 lanes x 16 bytes, their scan, every newline's index
	const size_t nblk = ((size_t)n_text + 4095) / 4096;
	std::vector<unsigned long long> blk(nblk + 1, 0);
	auto lane_mask = [&](uint64_t b0) { uint32_t w[4]; memcpy(w, t.data() + b0, 16); return nl_mask16(w, n_text - b0 < 16 ? (uint32_t)(n_text - b0) : 16u); };
	for(size_t b = 0; b < nblk; b++) for(uint32_t l = 0; l < 256; l++) { const uint64_t b0 = ((uint64_t)b * 256 + l) * 16; if(b0 < n_text) blk[b] += popc16(lane_mask(b0)); }
	excl_scan(blk);
	const uint64_t nl = blk[nblk];
	{ uint64_t naive = 0; for(char c : text) naive += c == '\n'; CHECK(naive == nl, "newline count %llu vs %llu", (unsigned long long)nl, (unsigned long long)naive); }
	const bool rest = nl % 4 != 0 || (n_text && text[n_text - 1] != '\n');
	uint64_t n = whole_records(nl) + (final && rest ? 1 : 0);
	if(max_records && max_records < n) n = max_records;
	out.n = n;
	if(n == 0) return out;
	const uint64_t known = nl < 4 * n ? nl : 4 * n;
	std::vector<uint32_t> nlpos(known);                                      // (exactly the entries the kernel may write)
	for(size_t b = 0; b < nblk; b++) {
		uint64_t idx = blk[b];
		for(uint32_t l = 0; l < 256; l++) {
			const uint64_t b0 = ((uint64_t)b * 256 + l) * 16;
			if(b0 >= n_text) break;
			for(uint32_t m = lane_mask(b0); m; m &= m - 1, idx++) if(idx < known) nlpos[idx] = (uint32_t)b0 + (uint32_t)__builtin_ctz(m);
		}
	}
	// 2. the per-record table
	std::vector<unsigned long long> lsz(n + 1, 0), nsz(n + 1, 0);
	std::vector<uint32_t> src(3 * n);
	out.first_not_plain = n;
	for(uint64_t r = 0; r < n; r++) {
		const Rec x = eval_record((const char*)t.data(), record_lines(nlpos.data(), known, n_text, r), o);
		lsz[r] = x.L; nsz[r] = x.name_len; src[r] = x.name_src; src[n + r] = x.seq_src; src[2 * n + r] = x.qual_src;
		if(!x.plain) { out.n_not_plain++; if(r < out.first_not_plain) out.first_not_plain = r; }
		else if(x.L > out.max_len) out.max_len = x.L;
	}
	out.consumed = known == 4 * n ? (uint64_t)nlpos[4 * n - 1] + 1 : n_text;
	if(out.n_not_plain) return out;
	// 3. the scans; 4. the writes, one lane per 16 output bytes
	excl_scan(lsz); excl_scan(nsz);
	out.nb = lsz[n]; out.nn = nsz[n];
	out.offs.resize(n + 1); out.noffs.resize(n + 1);
	for(uint64_t r = 0; r <= n; r++) { out.offs[r] = (uint32_t)lsz[r]; out.noffs[r] = (uint32_t)nsz[r]; }
	out.codes.assign((out.nb + 15) / 16 * 16, 0xee); out.quals.assign((out.nb + 15) / 16 * 16, (char)0xee); out.names.assign((out.nn + 15) / 16 * 16, (char)0xee);
	for(uint64_t c = 0; c < (out.nb + 15) / 16; c++) {
		const uint64_t b0 = c * 16;
		const uint32_t m = out.nb - b0 < 16 ? (uint32_t)(out.nb - b0) : 16u;
		Cursor cur;
		cur.seek(lsz.data(), src.data() + n, (uint32_t)n, b0);
		uint8_t wa[16] = {0}, wb[16] = {0};
		for(uint32_t k = 0; k < m; k++) {
			const uint32_t delta = src[2 * n + cur.r] - src[n + cur.r];
			const uint32_t at = cur.next();
			CHECK(at < n_text && at + delta < n_text, "source past the text");
			wa[k] = fq_code(t[at]); wb[k] = (uint8_t)fq_qual(t[at + delta], o.phred64);
		}
		memcpy(out.codes.data() + b0, wa, 16); memcpy(out.quals.data() + b0, wb, 16);
	}
	for(uint64_t c = 0; c < (out.nn + 15) / 16; c++) {
		const uint64_t b0 = c * 16;
		const uint32_t m = out.nn - b0 < 16 ? (uint32_t)(out.nn - b0) : 16u;
		Cursor cur;
		cur.seek(nsz.data(), src.data(), (uint32_t)n, b0);
		uint8_t wa[16] = {0};
		for(uint32_t k = 0; k < m; k++) { const uint32_t at = cur.next(); CHECK(at < n_text, "source past the text"); wa[k] = t[at]; }
		memcpy(out.names.data() + b0, wa, 16);
	}
	return out;
}

static std::string tmp_file(const std::string& text) {
	char fn[] = "/tmp/fq_check_XXXXXX";
	const int fd = mkstemp(fn);
	if(fd < 0 || write(fd, text.data(), text.size()) != (ssize_t)text.size()) { perror("fq_check: temporary file"); exit(2); }
	close(fd);
	return fn;
}
static void host_parse(const std::string& text, const Opts& o, size_t max, h2g_cli::Batch& b) {
	const std::string fn = tmp_file(text);
	{
		h2g_cli::Reader rd(std::vector<std::string>{fn}, h2g_cli::FMT_FASTQ, 1, o.trim5, o.trim3);
		rd.qc_.phred64 = o.phred64 != 0;
		b.clear();
		rd.fill(b, max);
	}
	unlink(fn.c_str());
}

struct Gen { bool crlf = false, last_nl = true, phred64 = false; uint32_t fixed_len = 0; };
static const uint32_t RAGGED[] = {0, 1, 15, 16, 17, 63, 64, 65, 100, 128, 129, 250};
static std::string record(uint32_t i, uint32_t len, uint32_t nlen, const Gen& g, bool extra_qual) {
	static const char bases[] = "ACGTACGTACGTACGTNn.acgtRYKMSWBDHVxU";
	std::string nm = "r" + std::to_string(i);
	while(nm.size() < nlen) nm.push_back("_/:abcXYZ 019"[rnd_below(13)]);
	nm.resize(nlen < 1 ? 1 : nlen);
	if(nm[0] == ' ') nm[0] = 'r';
	std::string s, q;
	for(uint32_t k = 0; k < len; k++) { s.push_back(bases[rnd_below(rnd_below(8) ? 16 : (uint32_t)sizeof bases - 1)]); q.push_back((char)((g.phred64 ? 64 : 33) + rnd_below(41))); }
	if(extra_qual) q.push_back((char)((g.phred64 ? 64 : 33) + 5));
	const char* e = g.crlf ? "\r\n" : "\n";
	return "@" + nm + e + s + e + "+" + (rnd_below(4) ? "" : nm) + e + q + e;
}
static std::string make_text(uint32_t nrec, const Gen& g) {
	std::string t;
	for(uint32_t i = 0; i < nrec; i++) {
		const uint32_t len = g.fixed_len ? g.fixed_len : (i == nrec / 2 ? 1000u : RAGGED[rnd_below(12)]);
		t += record(i, len, 1 + rnd_below(i % 50 == 0 ? 200 : 24), g, rnd_below(10) == 0);
	}
	if(!g.last_nl && !t.empty()) t.resize(t.size() - (g.crlf ? 2 : 1));
	return t;
}

static void compare(const char* what, const std::string& text, const Opts& o, uint64_t max_records, uint64_t want_n) {
	const Out d = device_parse(text, o, true, max_records);
	CHECK(d.n == want_n && d.n_not_plain == 0 && d.first_not_plain == d.n, "%s: %llu records (%llu wanted), %llu not plain", what, (unsigned long long)d.n, (unsigned long long)want_n, (unsigned long long)d.n_not_plain);
	if(d.n != want_n || d.n_not_plain) return;
	h2g_cli::Batch b;
	host_parse(text, o, (size_t)want_n, b);
	CHECK(b.n() == d.n, "%s: host parsed %zu records", what, b.n());
	if(b.n() != d.n) return;
	if(d.n == 0) return;
	CHECK(d.offs == b.offs, "%s: offs differ", what);
	CHECK(d.noffs == b.noffs, "%s: name offs differ", what);
	CHECK(d.nb == b.codes.size() && same(d.codes.data(), b.codes.data(), d.nb), "%s: codes differ", what);
	CHECK(d.nb == b.quals.size() && same(d.quals.data(), b.quals.data(), d.nb), "%s: qualities differ", what);
	CHECK(d.nn == b.names.size() && same(d.names.data(), b.names.data(), d.nn), "%s: names differ", what);
	for(uint64_t k = d.nb; k < d.codes.size(); k++) CHECK(d.codes[k] == 0 && d.quals[k] == 0, "%s: the last chunk's tail is not zero", what);
	uint32_t mx = 0;
	for(size_t i = 0; i < b.n(); i++) mx = std::max(mx, b.offs[i + 1] - b.offs[i]);
	CHECK(mx == d.max_len, "%s: longest read %u vs %u", what, d.max_len, mx);
	// the consumed bytes are where record want_n starts
	uint64_t nl = 0, at = text.size();
	for(size_t i = 0; i < text.size(); i++) if(text[i] == '\n' && ++nl == 4 * want_n) { at = i + 1; break; }
	CHECK(d.consumed == at, "%s: consumed %llu vs %llu", what, (unsigned long long)d.consumed, (unsigned long long)at);
}

// one record of `nrec` broken in each way the host ends the run on (or names by number): flagged at that record
static void check_not_plain() {
	static const char* kinds[] = {"empty name", "digit in the sequence", "missing +", "one quality short", "two qualities over", "blank in the qualities", "below 64 under phred64"};
	for(int kind = 0; kind < 7; kind++) for(int crlf = 0; crlf < 2; crlf++) {
		Gen g; g.crlf = crlf != 0; g.phred64 = kind == 6; g.fixed_len = 40;
		const char* e = g.crlf ? "\r\n" : "\n";
		const uint32_t nrec = 300, bad = 217;
		std::string t;
		for(uint32_t i = 0; i < nrec; i++) {
			if(i != bad) { t += record(i, 40, 1 + rnd_below(30), g, false); continue; }
			std::string nm = "bad", s(40, 'A'), plus = "+", q(40, g.phred64 ? 'h' : 'I');
			switch(kind) {
				case 0: nm = ""; break;
				case 1: s[7] = '3'; break;
				case 2: plus = "-"; break;
				case 3: q.resize(39); break;
				case 4: q += "II"; break;
				case 5: q[11] = ' '; break;
				case 6: q[20] = '5'; break;
			}
			t += "@" + nm + e + s + e + plus + e + q + e;
		}
		const Opts o = {0, 0, g.phred64 ? 1u : 0u};
		const Out d = device_parse(t, o, true, 0);
		CHECK(d.n == nrec && d.n_not_plain == 1 && d.first_not_plain == bad, "%s%s: %llu not plain, first %llu", kinds[kind], crlf ? " (CRLF)" : "", (unsigned long long)d.n_not_plain, (unsigned long long)d.first_not_plain);
		const Out d2 = device_parse(t, o, true, bad);                       // the record lies beyond max_records
		CHECK(d2.n == bad && d2.n_not_plain == 0, "%s: not plain beyond max_records", kinds[kind]);
		if(kind == 6) {   // the bad character trimmed away: the host never converts it
			const Opts o2 = {21, 0, 1};
			CHECK(device_parse(t, o2, true, 0).n_not_plain == 0, "a trimmed phred64 character counts");
			compare("phred64 character trimmed", t, o2, 0, nrec);
		}
	}
	// fewer than four lines at the end of the input; a text that does not end its input keeps them
	const std::string whole = "@a\nACGT\n+\nIIII\n", part = "@b\nACGT\n+";
	Out d = device_parse(whole + part, Opts{0, 0, 0}, true, 0);
	CHECK(d.n == 2 && d.n_not_plain == 1 && d.first_not_plain == 1, "a short last record");
	d = device_parse(whole + part, Opts{0, 0, 0}, false, 0);
	CHECK(d.n == 1 && d.n_not_plain == 0 && d.consumed == whole.size(), "an unfinished record stays unconsumed");
	d = device_parse(whole + "@b\nACGT\n+\nIIII", Opts{0, 0, 0}, false, 0);
	CHECK(d.n == 1 && d.consumed == whole.size(), "a last line without newline is not complete unless the text ends the input");
}

static void check_bits() {
	for(int it = 0; it < 2000; it++) {
		uint8_t b[16];
		for(int k = 0; k < 16; k++) b[k] = rnd_below(3) ? (uint8_t)rnd() : (uint8_t)("\n\x0b\x8a\x09\x0a"[rnd_below(5)]);
		uint32_t w[4];
		memcpy(w, b, 16);
		const uint32_t m = rnd_below(17);
		uint32_t want = 0;
		for(uint32_t k = 0; k < m; k++) if(b[k] == '\n') want |= 1u << k;
		CHECK(nl_mask16(w, m) == want, "nl_mask16");
	}
	for(int it = 0; it < 20000; it++) {      // the four-at-a-time forms against the per-character ones
		alignas(4) char b[12];
		for(int k = 0; k < 12; k++) b[k] = rnd_below(4) ? "ACGTNacgtn.RYKMxz@`[{-/ \r\n\x80\xc1\xe7"[rnd_below(30)] : (char)rnd();
		const uint32_t lo = rnd_below(12), hi = lo + rnd_below(13 - lo);
		bool want = true;
		for(uint32_t k = lo; k < hi; k++) want = want && is_fq_base((unsigned char)b[k]);
		bool got = true;
		for(uint32_t wi = lo >> 2; 4 * wi < hi; wi++) got = got && all_fq_bases(word_of(b, wi, lo, hi, 0x41414141u));
		CHECK(got == want, "all_fq_bases");
		bool want64 = true, got64 = true;
		for(uint32_t k = lo; k < hi; k++) want64 = want64 && (unsigned char)b[k] >= 64 && (unsigned char)b[k] < 128;
		for(uint32_t wi = lo >> 2; 4 * wi < hi; wi++) got64 = got64 && (word_of(b, wi, lo, hi, 0x40404040u) & 0xc0c0c0c0u) == 0x40404040u;
		CHECK(got64 == want64, "phred64 range");
	}
	for(int c = 0; c < 256; c++) {
		const uint8_t tb = h2g_cli::base_tables().fq[c];
		CHECK(is_fq_base((unsigned char)c) == (tb != 0xff), "is_fq_base(%d)", c);
		if(tb != 0xff) CHECK(fq_code((unsigned char)c) == tb, "fq_code(%d)", c);
	}
}

// several files per option: what the parser thread hands on under --h2g-device-parse (Reader::fill in raw mode) is four lines per record whatever lies behind a
// file's last record, the device parses it when it can, and Reader::parse_raw makes of it what the reader makes of the files
static void check_files() {
	Gen g; g.fixed_len = 30;
	const std::string b_text = make_text(40, g);
	static const char* tails[] = {"", "\n", "\n\n", "\r\n\r\n", "\n \n", "@x\n\n", "@x\n\n+\n", "@y\n\n+"};
	static const bool plain[] = {true, true, true, true, true, false, true, true};      // (a record the file ends in after two lines is the host's)
	for(int last_nl = 0; last_nl < 2; last_nl++) for(size_t k = 0; k < sizeof tails / sizeof *tails; k++) {
		Gen ga = g; ga.last_nl = last_nl != 0 || k >= 5;
		std::string a_text = make_text(25, ga);
		if(!ga.last_nl && k) continue;                            // (blank lines follow a line end)
		a_text += tails[k];
		const size_t want_n = 25 + 40 + (k >= 5 ? 1 : 0);
		const std::string fa = tmp_file(a_text), fb = tmp_file(b_text);
		h2g_cli::Batch host, raw;
		{
			h2g_cli::Reader rd(std::vector<std::string>{fa, fb}, h2g_cli::FMT_FASTQ, 1, 2, 3);
			host.clear();
			rd.fill(host, 1000);
			h2g_cli::Reader rr(std::vector<std::string>{fa, fb}, h2g_cli::FMT_FASTQ, 1, 2, 3);
			rr.raw_ = true;
			raw.clear();
			const size_t got = rr.fill(raw, 1000);
			CHECK(got == want_n && raw.raw_n == want_n && host.n() == want_n, "tail %zu: %zu records in raw mode, %zu parsed, %zu wanted", k, got, host.n(), want_n);
			const Out d = device_parse(raw.raw, Opts{2, 3, 0}, true, 0);
			CHECK(d.n == want_n && (d.n_not_plain == 0) == plain[k], "tail %zu: the device sees %llu records, %llu not plain", k, (unsigned long long)d.n, (unsigned long long)d.n_not_plain);
			if(d.n_not_plain == 0) CHECK(d.offs == host.offs && d.noffs == host.noffs && same(d.codes.data(), host.codes.data(), d.nb) && same(d.quals.data(), host.quals.data(), d.nb)
			                             && same(d.names.data(), host.names.data(), d.nn), "tail %zu: the device's arrays differ", k);
			h2g_cli::Batch part = raw;                                // the first records only (a -2 file longer than its -1 file)
			rr.parse_raw(part, 30);
			CHECK(part.n() == 30 && std::equal(part.offs.begin(), part.offs.end(), host.offs.begin()), "tail %zu: parse_raw of the first 30 records", k);
			rr.parse_raw(raw);
			CHECK(raw.offs == host.offs && raw.noffs == host.noffs && raw.codes == host.codes && raw.quals == host.quals && raw.names == host.names, "tail %zu: parse_raw differs from the reader", k);
		}
		unlink(fa.c_str()); unlink(fb.c_str());
	}
}

static int count_plain(const char* fn) {
	std::vector<char> bytes;
	if(!h2g_cli::read_whole_file(fn, bytes)) { printf("cannot read %s\n", fn); return 1; }
	const Out d = device_parse(std::string(bytes.begin(), bytes.end()), Opts{0, 0, 0}, true, 0);
	printf("plain %s %llu %llu\n", fn, (unsigned long long)(d.n - d.n_not_plain), (unsigned long long)d.n);
	return 0;
}

int main(int argc, char** argv) {
	if(argc > 1) { int rc = 0; for(int i = 1; i < argc; i++) rc |= count_plain(argv[i]); return rc; }
	check_bits();
	static const uint32_t trims[] = {0, 3, 200};
	for(int crlf = 0; crlf < 2; crlf++) for(int last_nl = 0; last_nl < 2; last_nl++) {
		Gen g; g.crlf = crlf != 0; g.last_nl = last_nl != 0;
		const uint32_t nrec = 700;      // (several workgroups of text; records straddle lanes, waves and workgroups)
		const std::string t = make_text(nrec, g);
		for(uint32_t t5 : trims) for(uint32_t t3 : trims) compare("ragged", t, Opts{t5, t3, 0}, 0, nrec);
		for(uint64_t mr : {(uint64_t)1, (uint64_t)7, (uint64_t)nrec, (uint64_t)nrec + 5}) compare("max_records", t, Opts{0, 0, 0}, mr, std::min<uint64_t>(mr, nrec));
		Gen p = g; p.phred64 = true;
		const std::string t64 = make_text(300, p);
		compare("phred64", t64, Opts{0, 0, 1}, 0, 300);
		compare("phred64 trimmed", t64, Opts{3, 3, 1}, 0, 300);
		Gen f = g; f.fixed_len = 100;
		compare("100 bases", make_text(300, f), Opts{0, 0, 0}, 0, 300);
		compare("one record", make_text(1, f), Opts{0, 0, 0}, 0, 1);
	}
	compare("empty text", "", Opts{0, 0, 0}, 0, 0);
	compare("empty reads", "@a\n\n+\n\n@b\n\n+\n", Opts{0, 0, 0}, 0, 2);
	check_not_plain();
	check_files();
	printf("fq_check: %d checks, %d failures\n", g_checks, g_fail);
	return g_fail ? 1 : 0;
}
