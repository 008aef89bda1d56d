// h2g_cli.cpp — `hisat2-align-amd`: the reference's `hisat2-align-s -x <index> -U/-1/-2 … -S out.sam` command line for the
// part of HISAT2 that is built here (linear or SNP-graph index; unpaired or paired reads).
// Host code only, over the C ABI of include/h2g.h (HI_Aligner::go on the GPU) and include/h2g_sam.h (the sink + SAM text, N1).  There is no CPU aligner in
// here: without a GPU h2g_index_load fails and so does this program.
//
// main() is the table of contents.  What it runs, each a type or function of its own that owns its state, its synchronisation and its thread:
//   Options / parse_options   the command line; Options::check() holds the refusals that need no device
//   TempInputs                -c / -r: the reads as temporary FASTA files, unlinked on every way out
//   WindowPlan                -F: the window plan over the -U files (the library's planner)
//   parse_only                the test hook --parse-only
//   plan_waves                temporary splice sites: the visibility window and the waves of reads it makes
//   Replicas                  one index per device, shared where streams share a device
//   SpliceSites               the splice-site database: file sites, then the junctions of every completed batch
//   TextWriter                [thread] three text buffers go round; writes them to the output in order
//   ParseStage                [thread] reads windows of records (h2g_cli_reads.h: batched read ingestion) into H host buffer pairs, ahead of the devices
//   FormatStage               [thread, optional] SAM text of a fetched batch, the --un / --al files (h2g_cli_sort.h), the merge of a mixed window, the totals
//   DeviceStage               one stream per device: upload + run batch k on stream k mod G, fetch batches strictly in order (main thread)
// Every variable that two threads see is a member of one stage, guarded by that stage's mutex or handed over under it; the comments at the members say which.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
#include <memory>
#include <time.h>
#include <unistd.h>
#include "../../include/h2g.h"
#include "../../include/h2g_sam.h"
#include "h2g_align.h"      // h2g::Rng (--non-deterministic)
#include "h2g_cli_reads.h"
#include "h2g_cli_sort.h"

namespace {
using namespace h2g_cli;

std::vector<std::string> split_commas(const char* s) {
	std::vector<std::string> v;
	std::string cur;
	for(; *s; s++) { if(*s == ',') { if(!cur.empty()) v.push_back(cur); cur.clear(); } else cur.push_back(*s); }
	if(!cur.empty()) v.push_back(cur);
	return v;
}
[[noreturn]] void die(const char* what) { fprintf(stderr, "hisat2-align-amd: %s (%s)\n", what, h2g_last_error()); exit(1); }
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// `call`, and when it reports a buffer too small (H2G_ERR_ARG) `grow` and `call` once more.  `grow` returns false when the buffers were large enough: the
// error is another one.  Whatever else fails is the end of the run, under the name `what`.  (The format calls used to be repeated on any failure; H2G_ERR_ARG is
// the only status they return, so the two are the same today — a new status of theirs would end the run here without the second call.)
template<class Call, class Grow> void retry_on_small_buffer(const char* what, Call call, Grow grow) {
	const h2g_status rc = call();
	if(rc == H2G_OK) return;
	if(rc != H2G_ERR_ARG || !grow() || call() != H2G_OK) die(what);
}

// text buffer: raw storage, grown without value-initialising hundreds of MB per batch
struct RawBuf {
	char* p = nullptr; size_t n = 0;
	void resize(size_t m) { if(m > n) { free(p); p = (char*)malloc(m); n = m; if(!p) { fprintf(stderr, "out of memory\n"); exit(1); } } }
	char* data() { return p; }
	size_t size() const { return n; }
	RawBuf() = default;
	RawBuf(const RawBuf&) = delete;
	~RawBuf() { free(p); }
};
// what comes back from the device lands in page-locked memory (h2g_host_alloc): the copies run at the link's rate.  The records travel compact
// (h2g_align_*_fetch_compact: 40 bytes + 12 per edit held instead of 424 per record) and are formatted in that layout.
struct Pinned {
	uint8_t* p = nullptr; size_t cap = 0;
	void need(size_t n) { if(n <= cap) return; h2g_host_free(p); cap = n + n / 4 + 4096; p = (uint8_t*)h2g_host_alloc(cap); if(!p) { fprintf(stderr, "hisat2-align-amd: cannot allocate %zu bytes of page-locked memory\n", cap); exit(1); } }
	Pinned() = default;
	Pinned(const Pinned&) = delete;
	~Pinned() { h2g_host_free(p); }
};
struct PinSet { Pinned res, rec1, rec2, o1, o2; std::vector<h2g_edit> long_edits; size_t nlong = 0;
                Pinned text, loffs; /* --h2g-device-sam: the item's SAM text and line starts as the device wrote them */ };

// ---- the command line
struct Options {
	std::string base, outfn, stats_fn;
	bool device_plan = false;                 // --h2g-device-plan (implies --h2g-device-sam): plain reads are planned on the device too, the host plans only the rest
	bool device_parse = false;                // --h2g-device-parse: the FASTQ records are parsed on the device (h2g_set_reads_fastq); the host parses only the items it hands back
	bool device_sam = false;                  // --h2g-device-sam: the SAM text is written on the device from a host-made line plan
	std::vector<std::string> u, m1, m2, m12;
	ReadFormat tab_fmt = FMT_TAB5;
	bool qseq = false, qc_filter = false, from_front_end = false;
	QualCoding qcoding;
	std::string rs_arg[RS_KINDS];
	bool rs_gz[RS_KINDS] = {false, false, false, false, false};
	bool windows = false;                                 // -F <len>,<step>: every <len>-base window, <step> apart, of the -U FASTA records is a read
	uint32_t win_len = 0, win_step = 0;
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
	std::string cmdline;                                  // argv joined by blanks: the header's @PG line
	std::vector<const char*> opts;                        // the alignment options and their arguments, in order: parsed by the library (h2g_align_params_apply_options)
	bool arbitrary_random = false;
	// what check() makes of them
	h2g_align_params P{};                                 // the alignment options; -k and the presets follow with the index type (open_sam)
	h2g_align_presets presets{};
	bool sorting = false;                                 // one of --un / --al ... was given
	ReadFormat fmt = FMT_FASTQ;
	bool have_pairs = false, have_singles = false;
	int check();
};

// the options in command-line order; a faulty one ends the program where it stands, as --version does
Options parse_options(int argc, char** argv) {
	Options o;
	for(int i = 0; i < argc; i++) { if(i) o.cmdline.push_back(' '); o.cmdline += argv[i]; }
	for(int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		auto need = [&](const char* opt) { if(i + 1 >= argc) { fprintf(stderr, "option %s needs an argument\n", opt); exit(1); } return argv[++i]; };
		auto files = [&](std::vector<std::string>& list) { auto v = split_commas(need(a.c_str())); list.insert(list.end(), v.begin(), v.end()); };
		if(a == "-x") o.base = need("-x");
		else if(a == "-U") files(o.u);
		else if(a == "-1") files(o.m1);
		else if(a == "-2") files(o.m2);
		else if(a == "--tab5" || a == "--12") { files(o.m12); o.tab_fmt = FMT_TAB5; }   // hisat2.cpp:1122-1124
		else if(a == "--tab6") { files(o.m12); o.tab_fmt = FMT_TAB6; }
		else if(a == "--qseq") o.qseq = true;
		else if(a == "--wrapper") o.from_front_end = std::string(need("--wrapper")) == "basic-0";   // the front end hisat2-amd announces itself as the reference's script does (hisat2.cpp ARG_WRAPPER)
		else if(a == "--qc-filter") o.qc_filter = true;                          // reads whose QSEQ filter field is '0' are not aligned (hisat2.cpp:3433-3439)
		else if(a == "--solexa-quals") o.qcoding.solexa = true;
		else if(a == "--int-quals" || a == "--integer-quals") o.qcoding.ints = true;
		else if(int rk = read_sink_option(a)) {                                  // --un / --al / --un-conc / --al-conc / --al-conc-disc <path>, each also as -gz
			if(rk < 0) { fprintf(stderr, "hisat2-align-amd: option %s is not built: the -bz2 / -lz4 forms of --un / --al are not (plain and -gz are; see DESIGN.md, scope)\n", a.c_str()); exit(1); }
			const int kind = (rk - 1) / 2;
			o.rs_arg[kind] = need(a.c_str()); o.rs_gz[kind] = (rk - 1) % 2 != 0;
		}
		else if(a == "-S") o.outfn = need("-S");
		else if(a == "-r") o.raw_input = true;                                   // one sequence per line (RawPatternSource pat.h)
		else if(a == "-c") o.cmdline_input = true;                               // -U / -1 / -2 are comma-separated sequences (VectorPatternSource)
		else if(a == "-f") { o.fasta = true; o.windows = false; }                // the last of -f / -q / -F decides (hisat2.cpp:1120-1132)
		else if(a == "-q") { o.fasta = false; o.windows = false; }
		else if(a == "-F") {
			// <len>,<step> as the reference's binary reads it, and the manual's k:<len>,i:<step> (which the binary reads as 0,0: DESIGN.md §8)
			const char* v = need("-F");
			unsigned long L = 0, S = 0;
			char* e = nullptr;
			const char* q = strncmp(v, "k:", 2) == 0 ? v + 2 : v;
			bool ok = *q >= '0' && *q <= '9';
			if(ok) { L = strtoul(q, &e, 10); ok = *e == ','; }
			if(ok) { q = e + 1; if(strncmp(q, "i:", 2) == 0) q += 2; ok = *q >= '0' && *q <= '9'; }
			if(ok) { S = strtoul(q, &e, 10); ok = *e == 0 && S <= 0xffffffffull; }
			if(!ok) { fprintf(stderr, "hisat2-align-amd: -F takes <len>,<step> (or k:<len>,i:<step>), not '%s'\n", v); exit(1); }
			o.windows = true; o.win_len = (uint32_t)std::min<unsigned long>(L, 0xffffffffu); o.win_step = (uint32_t)S;
		}
		else if(a == "-p" || a == "--threads") o.threads = atoi(need("-p"));        // host threads for parsing and SAM formatting
		else if(a == "--ss-window") o.ss_window_opt = (uint32_t)strtoul(need("--ss-window"), nullptr, 10);   // reads a temporary splice site stays invisible for: 1000 x <-p> of the reference (hisat2.cpp:3687), decoupled from this program's host threads
		else if(a == "--rna-strandness") {
			const std::string v = need("--rna-strandness");
			o.strandness = v == "F" ? 1 : v == "R" ? 2 : v == "FR" ? 3 : v == "RF" ? 4 : 0;
			if(!o.strandness) { fprintf(stderr, "Error: should be one of F, R, FR, or RF \n"); exit(1); }
		}
		else if(a == "--known-splicesite-infile") o.known_ss = need("--known-splicesite-infile");
		else if(a == "--novel-splicesite-infile") o.novel_ss = need("--novel-splicesite-infile");
		else if(a == "--novel-splicesite-outfile") o.novel_out = need("--novel-splicesite-outfile");
		else if(a == "--no-templatelen-adjustment") o.tlen_adjust = false;
		else if(a == "--rg-id") o.rg_args.push_back({true, need("--rg-id")});    // hisat2.cpp:1389-1407, in command-line order
		else if(a == "--rg") o.rg_args.push_back({false, need("--rg")});
		else if(a == "--no-sq" || a == "--sam-no-sq" || a == "--sam-nosq" || a == "--sam-noSQ") o.no_sq = true;
		else if(a == "--omit-sec-seq" || a == "--sam-omit-sec-seq") o.omit_sec_seq = true;
		else if(a == "--phred64" || a == "--phred64-quals" || a == "--solexa1.3-quals") o.qcoding.phred64 = true;   // hisat2.cpp ARG_PHRED64
		else if(a == "--phred33" || a == "--phred33-quals") o.qcoding.phred64 = false;
		else if(a == "--remove-chrname") o.chrname_mode |= 1;
		else if(a == "--add-chrname") o.chrname_mode |= 2;
		else if(a == "--new-summary") o.new_summary = true;
		else if(a == "--summary-file") o.summary_file = need("--summary-file");
		else if(a == "--no-mixed") o.report_mixed = false;                       // hisat2.cpp:1162
		else if(a == "--no-discordant") o.report_discordant = false;             // hisat2.cpp:1161
		else if(a == "--non-deterministic" || a == "--nondeterministic") o.arbitrary_random = true;   // hisat2.cpp:1207
		else if(a == "--no-hd" || a == "--no-head") o.nohead = true;
		else if(a == "--batch") { o.batch = (size_t)atoll(need("--batch")); o.saw_batch = true; }
		else if(a == "--device") o.device = atoi(need("--device"));
		else if(a == "--gpus") o.gpus = atoi(need("--gpus"));                        // batches round-robin over <int> devices, output in read order
		else if(a == "-s" || a == "--skip") o.skip = (uint64_t)atoll(need("-s"));     // skip the first <int> reads / pairs (hisat2.cpp:3319)
		else if(a == "-u" || a == "--upto" || a == "--qupto") o.upto = (uint64_t)atoll(need("-u"));
		else if(a == "-5" || a == "--trim5") o.trim5 = (uint32_t)atoi(need("-5"));
		else if(a == "-3" || a == "--trim3") o.trim3 = (uint32_t)atoi(need("-3"));
		else if(a == "--no-unal") o.no_unal = true;
		else if(a == "--quiet") o.quiet = true;                                      // gQuiet: no alignment summary on stderr (hisat2.cpp:4165)
		else if(a == "--version") { printf("hisat2-align-amd (h2g) — output format of HISAT2 2.2.3\n"); exit(0); }
		else if(a == "--reorder" || a == "-t" || a == "--time" || a == "--mm") {}   // output is always in read order; --mm (index mapping) has nothing to act on here
		else if(a == "--h2g-device-sam") o.device_sam = true;
		else if(a == "--h2g-device-plan") o.device_sam = o.device_plan = true;
		else if(a == "--h2g-device-parse") o.device_parse = true;
		else if(a == "--h2g-stats") o.stats_fn = need("--h2g-stats");               // writes {reads, second_pass, overflow, runs, fast, handed_on, device_sam_lines, whole_lines, device_planned, host_planned, device_parsed, host_parsed} as JSON (tests, bench)
		else if(a == "--parse-only") o.parse_only = true;                           // test hook: ingest the reads, print counts + checksums
		else if(const int arity = h2g_align_option_arity(argv[i]); arity >= 0) { o.opts.push_back(argv[i]); if(arity) o.opts.push_back(need(argv[i])); }   // every option that ends in a field of h2g_align_params
		else { fprintf(stderr, "hisat2-align-amd: option %s is not built (see DESIGN.md, scope)\n", a.c_str()); exit(1); }
	}
	return o;
}

// what is refused before anything touches a device, and what the options add up to; 0, or the exit status
int Options::check() {
	if(base.empty() || (m12.empty() && u.empty() && (m1.empty() || m2.empty()))) {
		fprintf(stderr, "usage: hisat2-align-amd -x <ht2-base> {-U <r.fq> | -1 <m1.fq> -2 <m2.fq> | --tab5 <r.tab5> | --tab6 <r.tab6>} [-f|-q|--qseq] --no-spliced-alignment [--bowtie2-dp 0|1|2] [-S out.sam]\n");
		return 1;
	}
	// the alignment options: the library's one parser (h2g_options.cpp)
	h2g_align_params_init(&P, nullptr);
	P.no_spliced_alignment = 0;                           // the command line's default is the reference's: spliced alignment
	{
		char err[512];
		if(h2g_align_params_apply_options(&P, &presets, opts.data(), opts.size(), err, sizeof err) != H2G_OK) { fprintf(stderr, "%s\n", err); return 1; }
	}
	for(int k = 0; k < RS_KINDS; k++) sorting = sorting || !rs_arg[k].empty();
	if(device_parse) {
		// the device parses four-line FASTQ records with character qualities; every other reader, and what needs the host's copy of a record's text, is refused by name
		const char* with = windows ? "-F" : fasta ? "-f" : raw_input ? "-r" : cmdline_input ? "-c" : !m12.empty() ? "--tab5/--tab6/--12" : qseq ? "--qseq" : qcoding.ints ? "--int-quals"
		                   : qcoding.solexa ? "--solexa-quals" : parse_only ? "--parse-only" : nullptr;
		if(with) { fprintf(stderr, "hisat2-align-amd: --h2g-device-parse is not built together with %s: it takes FASTQ files with character qualities (see DESIGN.md, scope)\n", with); return 1; }
		for(int k = 0; k < RS_KINDS; k++) if(!rs_arg[k].empty()) {
			fprintf(stderr, "hisat2-align-amd: --h2g-device-parse is not built together with --%s%s and its kin: they need the host's copy of every record's text (see DESIGN.md, scope)\n", rs_names[k], rs_gz[k] ? "-gz" : "");
			return 1;
		}
	}
	if(windows) {
		// -F cuts its reads out of the -U files and nothing else: what would need another reader or a second mate is refused by name
		const char* with = !m1.empty() || !m2.empty() ? "-1/-2" : !m12.empty() ? "--tab5/--tab6/--12" : qseq ? "--qseq" : cmdline_input ? "-c" : raw_input ? "-r" : nullptr;
		if(with) { fprintf(stderr, "hisat2-align-amd: -F is not built together with %s: it takes -U FASTA files only (see DESIGN.md, scope)\n", with); return 1; }
		if(sorting) { fprintf(stderr, "hisat2-align-amd: -F is not built together with --un / --al and their kin (see DESIGN.md, scope)\n"); return 1; }
		if(win_len == 0) { fprintf(stderr, "hisat2-align-amd: -F %u,%u: a window length of 0 yields no reads\n", win_len, win_step); return 1; }
		if(win_len > 1024) { fprintf(stderr, "hisat2-align-amd: -F %u,%u: windows longer than 1024 bases are beyond the reference's ring (pat.h:1346)\n", win_len, win_step); return 1; }
		if(u.empty()) { fprintf(stderr, "hisat2-align-amd: -F needs -U <fasta>[,<fasta>...]\n"); return 1; }
		// temporary splice sites with a window (-p >= 2 / --ss-window): the window is measured in read ids, and with a step other than 1 the ids have gaps — the
		// reference's own --reorder output stalls there, so there is nothing to equal
		const bool temp_ss = !P.no_spliced_alignment && !P.no_temp_splicesite;
		if(temp_ss && win_step != 1 && (ss_window_opt || threads >= 2)) {
			fprintf(stderr, "hisat2-align-amd: -F %u,%u with -p %d is not built for the temporary-splice-site mode (read ids with gaps: the reference's --reorder output stalls): "
			                "use -p 1, a step of 1, --no-temp-splicesite or --no-spliced-alignment\n", win_len, win_step, threads);
			return 1;
		}
		trim5 = trim3 = 0;                                    // (not applied by this source, as in the reference)
		fasta = true;
	}
	if(sorting && !from_front_end) {
		// as in the reference, where these are options of the `hisat2` script and hisat2-align-s refuses them
		for(int k = 0; k < RS_KINDS; k++) if(!rs_arg[k].empty()) {
			fprintf(stderr, "hisat2-align-amd: option --%s%s is not built into hisat2-align-amd itself: it is an option of the front end, hisat2-amd (the same command line)\n", rs_names[k], rs_gz[k] ? "-gz" : "");
			return 1;
		}
	}
	if(sorting && (cmdline_input || raw_input)) { fprintf(stderr, "hisat2-align-amd: --un / --al and their kin are not built for -c / -r input (see DESIGN.md, scope)\n"); return 1; }
	if(!m12.empty()) { cmdline_input = raw_input = false; }      // the tabbed files are the read set (pat.cpp:438-452)
	fmt = !m12.empty() ? tab_fmt : qseq ? FMT_QSEQ : (fasta || cmdline_input || raw_input) ? FMT_FASTA : FMT_FASTQ;
	have_pairs = m12.empty() && !m1.empty() && !m2.empty();
	have_singles = m12.empty() && !u.empty();
	return 0;
}

// -c / -r: the reads have no names (the reference numbers them, like FASTA records with an empty name) and no qualities ('I'): they are
// handed to the FASTA reader as ">\n<sequence>\n" records through temporary files, which take the place of the option's arguments.
// The files go away on every way out: with this object, and at exit() (die() and the parsers' errors do not return).
class TempInputs {
public:
	explicit TempInputs(Options& o) {
		if(o.cmdline_input || o.raw_input) { as_fasta(o.u, o.cmdline_input); as_fasta(o.m1, o.cmdline_input); as_fasta(o.m2, o.cmdline_input); }
		atexit(unlink_all);
	}
	~TempInputs() { unlink_all(); }
	TempInputs(const TempInputs&) = delete;
private:
	static void unlink_all() { for(const std::string& p : paths_) unlink(p.c_str()); paths_.clear(); }
	static void as_fasta(std::vector<std::string>& list, bool sequences) {
		if(list.empty()) return;
		std::string text;
		for(const std::string& item : list) {
			if(sequences) { text += ">\n"; text += item; text += "\n"; continue; }
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
		paths_.push_back(path);
	}
	inline static std::vector<std::string> paths_;   // (static: the exit handler outlives main's frame)
};

// The reference's two warnings for every read or mate the length filter drops (printMmsSkipMsg / printLenSkipMsg, hisat2.cpp:3017-3052; the worker at :3417-3432:
// length <= the seed mismatches, which are 0, or < 2), in its order: the first message for mate 1 and mate 2, then the second for both.  The length is the trimmed
// one, the name the record's as it was read.  `b`: the second mates when record i is a pair.  --quiet (gQuiet) takes them with the summary.
void warn_length_filtered(const Batch& a, const Batch* b, size_t i) {
	if(a.offs[i + 1] - a.offs[i] >= 2 && (!b || b->offs[i + 1] - b->offs[i] >= 2)) return;   // the common case: nothing to say
	const Batch* m[2] = {&a, b};
	for(int msg = 0; msg < 2; msg++) for(int k = 0; k < (b ? 2 : 1); k++) {
		const Batch& s = *m[k];
		const uint32_t len = s.offs[i + 1] - s.offs[i];
		if(len >= 2) continue;
		std::string w = "Warning: skipping ";
		if(b) { w += "mate #"; w += (char)('1' + k); w += " of "; }
		w += "read '"; w.append(s.names, s.noffs[i], s.noffs[i + 1] - s.noffs[i]);
		if(msg == 0) w += "' because length (" + std::to_string(len) + ") <= # seed mismatches (0)\n";
		else w += "' because it was < 2 characters long\n";
		fwrite(w.data(), 1, w.size(), stderr);
	}
}

// -F: the plan over the -U files (h2g_window_plan_*, the library's planner) and the reads -s / -u leave of it
struct WindowPlan {
	h2g_window_plan* plan = nullptr;
	uint64_t first = 0, n = 0;
	h2g_window_plan_info info{};
	WindowPlan() = default;
	WindowPlan(const WindowPlan&) = delete;
	~WindowPlan() { h2g_window_plan_free(plan); }
	// 0, or the exit status
	int load(const Options& o) {
		// H2G_WINDOW_FIRST_ID=<n> (test hook): the id counter's start, as if records with n windows at step 1 had gone before
		const uint64_t id0 = getenv("H2G_WINDOW_FIRST_ID") ? strtoull(getenv("H2G_WINDOW_FIRST_ID"), nullptr, 10) : 0;
		if(h2g_window_plan_create(o.win_len, o.win_step, id0, &plan) != H2G_OK) { fprintf(stderr, "hisat2-align-amd: -F %u,%u: cannot plan\n", o.win_len, o.win_step); return 1; }
		std::vector<char> bytes;
		for(const std::string& fn : o.u) {
			if(!read_whole_file(fn, bytes)) { fprintf(stderr, "Error: could not open %s\n", fn.c_str()); return 1; }
			if(h2g_window_plan_add_file(plan, bytes.data(), bytes.size()) != H2G_OK) { fprintf(stderr, "hisat2-align-amd: -F: %s holds a record of more than 2^32 windows, or the record names exceed 4 GB\n", fn.c_str()); return 1; }
		}
		h2g_window_plan_get_info(plan, &info);
		const uint64_t hi = o.upto > ~0ull - o.skip ? ~0ull : o.upto + o.skip;      // -u counts from the skipped ids on (hisat2.cpp:1959-1963)
		h2g_window_plan_select(plan, o.skip, hi, &first, &n);
		return 0;
	}
};

// --parse-only (test hook): records, bases and a checksum over every window of <--batch> records (codes, names, qualities and lengths of the unpaired reads and first
// mates, then those of the second mates), then the number of pairs and of unpaired reads; one line per --un / --al option with the file name(s) it would write.
// On stderr: the length-filter warnings of the records, as a run writes them.
// Under -F: after that line, the first and the last read id of every window of <--batch> reads.
int parse_only(const Options& o, Source& src) {
	Win w;
	std::string id_lines;
	uint64_t n = 0, bases = 0, npairs = 0, h = 1469598103934665603ull;
	auto mix = [&](const void* p, size_t len) { const uint8_t* c = (const uint8_t*)p; for(size_t i = 0; i < len; i++) { h ^= c[i]; h *= 1099511628211ull; } };
	while(src.next(w, o.batch)) {
		n += w.n; npairs += w.npairs;
		if(!w.ids64.empty()) id_lines += std::to_string(w.ids64.front()) + " " + std::to_string(w.ids64.back()) + "\n";
		if(!o.quiet) for(size_t i = 0; i < w.n; i++) warn_length_filtered(w.a, (w.kinds.empty() ? w.paired : w.kinds[i] != 0) ? &w.b : nullptr, i);
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
	fputs(id_lines.c_str(), stdout);
	for(int k = 0; k < RS_KINDS; k++) if(!o.rs_arg[k].empty()) {
		std::string f1, f2;
		read_sink_names(k, o.rs_arg[k], &f1, &f2);
		printf("--%s%s\t%s%s%s\n", rs_names[k], o.rs_gz[k] ? "-gz" : "", f1.c_str(), f2.empty() ? "" : "\t", f2.c_str());
	}
	return 0;
}

// Temporary splice sites (the reference's default): a read sees the junctions of reads at least W = 1000 * p ids before it
// (hisat2.cpp:3687; -p 1 means W = 0, every read after the other).  The batches are waves of <= W reads run one after the other.
struct Waves {
	bool temp_ss = false;
	uint32_t window = 0, wave = 0;        // the reference's visibility window, and the reads of one wave here (the window, or ONE read when it is 0)
};
// sizes the waves (then a batch is one wave: *batch); 0, or the exit status
int plan_waves(const Options& o, Waves* w, size_t* batch) {
	w->temp_ss = !o.P.no_spliced_alignment && !o.P.no_temp_splicesite;
	if(w->temp_ss) {
		// -p 1 (and no --ss-window): the reference's window is 0 (hisat2.cpp:3687) — a read sees the junctions of EVERY read before it, a strict
		// chain.  It runs as waves of one read: exact, and as slow as a chain is (a device round trip per read); meant for small inputs — the
		// reference's bare default invocation `hisat2 -x idx -U reads` then simply works.  -p >= 2 / --ss-window are the throughput modes.
		w->window = o.ss_window_opt ? o.ss_window_opt : (o.threads < 2 ? 0u : 1000u * (uint32_t)o.threads);
		w->wave = w->window ? w->window : 1u;
		// a wave sizes the streams and the result rows (one shard per device): bound it — the reference's own window at its largest useful
		// -p (1000 x 256 threads) is far below this, and an absurd value would only be an allocation failure later
		const uint32_t ss_wave_max = 4u * 1024u * 1024u;
		if(w->wave > ss_wave_max) {
			fprintf(stderr, "hisat2-align-amd: --ss-window %u (or 1000 x -p) makes waves of more than %u reads; a wave is one resident batch per device "
			                "(streams and result rows are sized by it, --batch does not apply to the temporary-splice-site mode): use --ss-window <= %u, "
			                "or --no-temp-splicesite with --batch\n", w->wave, ss_wave_max, ss_wave_max);
			return 1;
		}
		*batch = w->wave;   // a wave is exactly one shard per device (ParseStage::run): a smaller --batch would complete shards (and merge their junctions) in the middle of a wave
	}
	if(w->temp_ss && o.have_pairs && o.have_singles) {
		// the reference's read ids restart at the -U reads: which temporary splice sites its window then shows them is not a function of the input
		fprintf(stderr, "hisat2-align-amd: -1/-2 together with -U is not built for the temporary-splice-site mode (the reference's read ids restart at the -U reads, and "
		                "the sites its window shows them depend on thread timing): give --no-temp-splicesite or --no-spliced-alignment\n");
		return 1;
	}
	return 0;
}

// --gpus N: one index replica and one stream per device; batch k runs on device k mod N while the others are in flight, and
// the batches are completed (fetched, formatted, written) strictly in order, so the output is the single-GPU output.
// H2G_GPUS_SHARE_DEVICE=1 (test hook) lets the N streams share the devices that exist: streams of one device share its replica.
class Replicas {
public:
	// 0, or the exit status
	int load(const Options& o, bool temp_ss) {
		int gpus = o.gpus < 1 ? 1 : o.gpus;
		const int ndev = h2g_device_count();
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
		h2g_load_opts lo; h2g_load_opts_init(&lo); lo.load_local = 1;
		ixs_.assign((size_t)gpus, nullptr);
		for(int g = 0; g < gpus; g++) {
			const int dev = (o.device + g % ndevs_asked) % ndev;
			for(int q = 0; q < g; q++) if((o.device + q % ndevs_asked) % ndev == dev) ixs_[(size_t)g] = ixs_[(size_t)q];      // shared device: share the replica
			if(ixs_[(size_t)g]) continue;
			lo.device = dev;
			if(h2g_index_load(o.base.c_str(), &lo, &ixs_[(size_t)g]) != H2G_OK) die("cannot load the index onto the GPU");
		}
		return 0;
	}
	int streams() const { return (int)ixs_.size(); }
	h2g_index* of_stream(int g) const { return ixs_[(size_t)g]; }
	// every replica once, in stream order
	template<class Fn> void for_each_distinct(Fn fn) const {
		for(size_t g = 0; g < ixs_.size(); g++) {
			bool first = true;
			for(size_t q = 0; q < g; q++) if(ixs_[q] == ixs_[g]) first = false;
			if(first) fn(ixs_[g]);
		}
	}
	void free_all() { for_each_distinct([](h2g_index* ix) { h2g_index_free(ix); }); ixs_.clear(); }
private:
	std::vector<h2g_index*> ixs_;     // per stream
};

// The splice-site database: one for go() on every device and for TLEN.  The sites of the files (hisat2.cpp:4100-4120), then the temporary ones by first
// appearance.  Main thread only: merge_novel() runs where a batch is formatted, and with temporary splice sites or a novel-site file that is the main thread.
class SpliceSites {
public:
	// the known and the novel sites of the two files (either may be empty); false: one of them could not be opened
	bool load_files(h2g_sam* sam, const std::string& known_ss, const std::string& novel_ss) {
		for(int pass = 0; pass < 2; pass++) {
			const std::string& fn = pass == 0 ? known_ss : novel_ss;
			if(fn.empty()) continue;
			const size_t n = h2g_sam_read_splice_site_file(sam, fn.c_str(), pass == 0, nullptr, 0);
			if(n == (size_t)-1) { fprintf(stderr, "Error: Could not open %s\n", fn.c_str()); return false; }
			const size_t at = sites_.size();
			sites_.resize(at + n);
			h2g_sam_read_splice_site_file(sam, fn.c_str(), pass == 0, sites_.data() + at, n);
		}
		// SpliceSiteDB::read keeps the first of equal sites (splice_site.cpp:750)
		std::vector<h2g_splice_site> uniq;
		for(const h2g_splice_site& x : sites_) if(site_at_.emplace(key(x), uniq.size()).second) uniq.push_back(x);
		sites_.swap(uniq);
		return true;
	}
	void publish(const Replicas& ix, h2g_sam* sam, uint32_t window) const {
		ix.for_each_distinct([&](h2g_index* i) { if(h2g_index_set_splice_sites(i, sites_.data(), sites_.size(), window) != H2G_OK) die("cannot upload the splice sites"); });
		h2g_sam_set_splice_sites(sam, sites_.data(), sites_.size(), window);
	}
	// the junctions of the lines just formatted leave the sink; with temporary splice sites they join the database (SpliceSiteDB::addSpliceSite: smallest read id per site)
	void merge_novel(const Replicas& ix, h2g_sam* sam, bool temp_ss) {
		const size_t k = h2g_sam_take_novel_sites(sam, nullptr, 0);
		novel_.resize(k);
		if(k) h2g_sam_take_novel_sites(sam, novel_.data(), k);
		// only what is new (or whose smallest read id went down) goes to the devices and the formatter: they merge it into their sorted
		// copies (h2g_index_add_splice_sites) — the cost of a wave is its own junctions, not the database's size
		delta_.clear();
		if(temp_ss) for(const h2g_splice_site& x : novel_) {
			auto it = site_at_.find(key(x));
			if(it == site_at_.end()) { site_at_.emplace(key(x), sites_.size()); sites_.push_back(x); delta_.push_back(x); }
			else if(!sites_[it->second].fromfile && x.readid < sites_[it->second].readid) { sites_[it->second].readid = x.readid; delta_.push_back(sites_[it->second]); }
		}
		if(delta_.empty()) return;
		ix.for_each_distinct([&](h2g_index* i) { if(h2g_index_add_splice_sites(i, delta_.data(), delta_.size()) != H2G_OK) die("cannot upload the splice sites"); });
		h2g_sam_add_splice_sites(sam, delta_.data(), delta_.size());
	}
private:
	typedef std::array<uint32_t, 4> Key;                  // (text, left, right, dir)
	static Key key(const h2g_splice_site& x) { return Key{x.tidx, x.left, x.right, (uint32_t)x.dir}; }
	std::vector<h2g_splice_site> sites_;                  // file sites, then the temporary ones by first appearance
	std::map<Key, size_t> site_at_;                       // -> position in sites_
	std::vector<h2g_splice_site> novel_, delta_;          // merge_novel's scratch
};

// opens the sink and settles what waits for the index type: -k / --max-seeds and the presets (hisat2.cpp:1882-1909, 3903), their ranges, the default batch; 0, or the exit status
int open_sam(const Options& o, const Replicas& ix, const Waves& wv, h2g_align_params* P, h2g_sam** sam, size_t* batch) {
	if(h2g_sam_open(o.base.c_str(), sam) != H2G_OK) die("cannot read reference names");
	if(o.chrname_mode == 3) { fprintf(stderr, "Error: --remove-chrname and --add-chrname cannot be used at the same time\n"); return 1; }   // hisat2.cpp:3958
	if(o.chrname_mode) h2g_sam_set_chrname_mode(*sam, o.chrname_mode);
	h2g_index_info info;
	if(h2g_index_get_info(ix.of_stream(0), &info) != H2G_OK) die("h2g_index_get_info");
	h2g_align_presets presets = o.presets;
	h2g_align_params_presets(P, (int)info.linear, &presets);
	if(!P->no_spliced_alignment && P->max_intronlen > 0xfffffu) {
		fprintf(stderr, "hisat2-align-amd: --max-intronlen %u is beyond the 1048575 bases a splice edit holds here\n", P->max_intronlen);
		return 1;
	}
	if(P->min_intronlen > P->max_intronlen) {   // hisat2.cpp:4278
		fprintf(stderr, "--min-intronlen(%u) should not be greater than --max-intronlen(%u)\n", P->min_intronlen, P->max_intronlen);
		return 1;
	}
	if(P->khits < 1 || P->khits > H2G_KHITS_MAX || P->kseeds > H2G_KSEEDS_MAX || P->kseeds < P->khits) {
		fprintf(stderr, "hisat2-align-amd: -k %u / --max-seeds %u is outside the built range (1 <= -k <= %u, -k <= --max-seeds <= %u)\n", P->khits, P->kseeds,
		        (unsigned)H2G_KHITS_MAX, (unsigned)H2G_KSEEDS_MAX);
		return 1;
	}
	// -k above 32 or --max-seeds above 64 runs on the extra-large units, whose result rows grow with -k (2 k + 4 records of 424 bytes per mate and pair):
	// 64 k reads per batch keep them near 14 GB at -k 128 where the default batch would need 220 GB
	// (not in the temporary-splice-site mode: there a batch is one wave)
	if((P->khits > 32 || P->kseeds > 64) && !o.saw_batch && wv.wave == 0 && *batch > (1u << 16)) *batch = 1u << 16;
	return 0;
}

// the splice sites the run starts with, on every device and in the sink; 0, or the exit status
int start_splice_sites(const Options& o, const h2g_align_params& P, const Waves& wv, const Replicas& ix, h2g_sam* sam, SpliceSites* db) {
	if(!P.no_spliced_alignment && (!o.known_ss.empty() || !o.novel_ss.empty())) {
		if(!db->load_files(sam, o.known_ss, o.novel_ss)) return 1;
		db->publish(ix, sam, wv.window);
	} else if(wv.temp_ss) db->publish(ix, sam, wv.window);      // (the window of the wave scheme; the sites arrive wave after wave)
	if(!wv.temp_ss && !P.no_spliced_alignment && !o.novel_out.empty() && h2g_sam_novel_splice_sites_text(sam, nullptr, 0) > 0) {
		// write (the outfile) + read (a file's or the index's sites) without the temporary-site window: the reference then lets every read see
		// the junctions of whichever reads its threads happened to finish first (window 0, hisat2.cpp:3687, :4092-4093) — not a function of the input
		fprintf(stderr, "hisat2-align-amd: --novel-splicesite-outfile with --no-temp-splicesite and a splice-site database (file or --ss index) "
		        "makes the reference's output depend on thread timing; drop --no-temp-splicesite (output == hisat2 -p <int> --reorder)\n");
		return 1;
	}
	if(wv.temp_ss || (!P.no_spliced_alignment && !o.novel_out.empty())) h2g_sam_collect_novel_sites(sam, 1);   // SpliceSiteDB's `write` (hisat2.cpp:4092)
	return 0;
}

void apply_sam_settings(const Options& o, const h2g_align_params& P, h2g_sam* sam) {
	h2g_sam_set_templatelen_adjustment(sam, o.tlen_adjust);
	h2g_sam_set_report_policy(sam, o.report_discordant, o.report_mixed);
	for(const auto& r : o.rg_args) h2g_sam_add_read_group(sam, r.first ? r.second.c_str() : nullptr, r.first ? nullptr : r.second.c_str());
	h2g_sam_set_header_options(sam, o.no_sq, o.omit_sec_seq);
	h2g_sam_set_new_summary(sam, o.new_summary);
	h2g_sam_set_score_min(sam, P.score_min_type, P.score_min_const, P.score_min_coeff);
	h2g_sam_set_n_ceil(sam, P.n_ceil_type, P.n_ceil_const, P.n_ceil_coeff);
	h2g_sam_set_secondary(sam, (int)P.secondary);
	h2g_sam_set_rna_strandness(sam, o.strandness);
}

// -S (or stdout) with the SAM header in it; null: it could not be opened
FILE* open_output(const Options& o, h2g_sam* sam) {
	FILE* out = o.outfn.empty() ? stdout : fopen(o.outfn.c_str(), "wb");
	if(!out) { fprintf(stderr, "cannot open %s\n", o.outfn.c_str()); return nullptr; }
	if(!o.nohead) {
		const size_t need = h2g_sam_header(sam, o.cmdline.c_str(), nullptr, 0);
		RawBuf buf;
		buf.resize(need + 1);
		h2g_sam_header(sam, o.cmdline.c_str(), buf.data(), buf.size());
		fwrite(buf.data(), 1, need, out);
	}
	return out;
}

// ---- the writer: the text of a batch goes to the output on a thread of its own (6 GB of SAM per 10 M pairs: a third of the run when the main thread wrote it).
// Three text buffers go round; the batches are written in the order they were submitted (one writer, a FIFO).  A buffer belongs to whoever acquire()d it until submit().
class TextWriter {
public:
	explicit TextWriter(FILE* out) : out_(out), thread_(&TextWriter::run, this) {}
	~TextWriter() { finish(); }
	TextWriter(const TextWriter&) = delete;
	int acquire() { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return !free_.empty(); }); const int i = free_.front(); free_.pop_front(); return i; }
	RawBuf& text(int i) { return text_[i]; }
	void submit(int i, size_t used) { { std::lock_guard<std::mutex> lk(m_); used_[i] = used; queue_.push_back(i); } cv_.notify_all(); }
	// writes what is queued and ends the thread
	void finish() { if(!thread_.joinable()) return; { std::lock_guard<std::mutex> lk(m_); done_ = true; } cv_.notify_all(); thread_.join(); }
	bool failed() const { return err_; }
private:
	void run() {
		for(;;) {
			int i;
			{ std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return !queue_.empty() || done_; }); if(queue_.empty()) return; i = queue_.front(); queue_.pop_front(); }
			if(used_[i] && fwrite(text_[i].data(), 1, used_[i], out_) != used_[i]) err_ = true;
			{ std::lock_guard<std::mutex> lk(m_); free_.push_back(i); }
			cv_.notify_all();
		}
	}
	FILE* const out_;                         // the writer thread's, between construction and finish()
	RawBuf text_[3];                          // buffer i: its holder's (acquire() .. submit()), then the writer thread's until it is free again
	size_t used_[3] = {0, 0, 0};              // travels with buffer i; written under m_
	std::mutex m_; std::condition_variable cv_;
	std::deque<int> queue_, free_ = {0, 1, 2};   // guarded by m_
	bool done_ = false;                       // guarded by m_
	bool err_ = false;                        // written by the writer thread, read after finish()
	std::thread thread_;                      // (last: it starts on members that are ready)
};

// What one device run takes: a run of records of one kind.  A window that mixes pairs and unpaired reads (a tabbed file) becomes two items, its pairs (merge 1) and then
// its unpaired reads (merge 2), whose text is put back into record order (`order`: 1 = pair) before it is written: N records in windows of B make at most
// 2 ceil(N / B) device runs however the kinds alternate.  With temporary splice sites the read ids must be exact: the two items carry their records' ids (h2g_set_read_ids), both see the wave's one snapshot of the database and their junctions are merged after the second.
struct Item { std::vector<h2g_window_seg> wsegs; /* -F: the segments of the item's reads; with them ids / ids64 */ size_t n = 0; bool paired = false; uint64_t first_id = 0, skipped = 0; int merge = 0; std::vector<uint8_t> order; std::vector<uint32_t> ids; std::vector<uint64_t> ids64; };   // ids: Read::rdid per read, for the two items of a mixed window

// ---- the parser: item j is read into host buffer pair j mod H as soon as that pair is free (item j - H is formatted), ahead of the main thread.
// H = streams + 2 (+ 1 with a formatter thread): item k + 1 is parsed while item k is uploaded and up to G earlier ones are on the GPUs / being formatted.
// Slot j mod H (its two batches and its Item) is the parser's while it fills it; emit() hands it over under m_, and it stays the consumers' (the main thread from
// wait(j), the formatter after it) until release() has counted item j: the window `j < completed_ + H` is what keeps the parser off it.
class ParseStage {
public:
	ParseStage(Source& src, int H, size_t batch, const Waves& wv, int streams)
		: src_(src), H_(H), batch_(batch), temp_ss_(wv.temp_ss), ss_wave_(wv.wave), streams_((size_t)streams), A_((size_t)H), B_((size_t)H), meta_((size_t)H), thread_(&ParseStage::run, this) {}
	~ParseStage() { { std::lock_guard<std::mutex> lk(m_); stop_ = true; } cv_.notify_all(); finish(); }
	ParseStage(const ParseStage&) = delete;
	// item k, once it is parsed; *short_mates: the parser has met a -2 file shorter than its -1 file.  An item without records (and merge 0) is the end of the input.
	const Item& wait(long k, bool* short_mates) {
		std::unique_lock<std::mutex> lk(m_);
		cv_.wait(lk, [&] { return parsed_ > k; });
		*short_mates = perr_;
		return meta_[(size_t)(k % H_)];
	}
	// the slot of item k, between wait(k) and the release() that counts it
	const Item& item(long k) const { return meta_[(size_t)(k % H_)]; }
	Batch& a(long k) { return A_[(size_t)(k % H_)]; }     // unpaired reads / first mates
	Batch& b(long k) { return B_[(size_t)(k % H_)]; }     // second mates
	// the oldest `count` items are formatted: their slots are the parser's again
	void release(int count) { { std::lock_guard<std::mutex> lk(m_); completed_ += count; } cv_.notify_all(); }
	// the thread ends by itself after the item that ends the input (or names the short file)
	void finish() { if(thread_.joinable()) thread_.join(); }
	double busy() const { return busy_; }
private:
	// hands one item to the main thread: into slot j_ mod H as soon as that slot is free; false: the stage is being destroyed
	bool emit(Batch& a, Batch* b, Item&& it, bool bad) {
		{ std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return stop_ || j_ < completed_ + H_; }); if(stop_) return false; }
		std::swap(A_[(size_t)(j_ % H_)], a);
		if(b) std::swap(B_[(size_t)(j_ % H_)], *b);
		{ std::lock_guard<std::mutex> lk(m_); meta_[(size_t)(j_ % H_)] = std::move(it); perr_ = perr_ || bad; parsed_ = j_ + 1; }
		cv_.notify_all();
		j_++;
		return true;
	}
	// a window of both kinds: its pairs, then its unpaired reads, each read under its record's id
	bool emit_mixed(Win& w, Batch& sa, double tp) {
		Batch pa, pb;
		pa.clear(); pb.clear(); sa.clear();
		pa.have_quals = pb.have_quals = sa.have_quals = true;
		Item ip, is;
		for(size_t i = 0; i < w.n; i++) {
			Item& it = w.kinds[i] ? ip : is;
			if(w.kinds[i]) { pa.take(w.a, i); pb.take(w.b, i); } else sa.take(w.a, i);
			it.ids.push_back((uint32_t)(w.first_id + i)); it.ids64.push_back(w.first_id + i);
		}
		busy_ += now() - tp;
		ip.n = w.npairs; ip.paired = true; ip.first_id = w.first_id; ip.skipped = w.skipped; ip.merge = 1;
		is.n = w.n - w.npairs; is.first_id = w.first_id; is.merge = 2; is.order.swap(w.kinds);
		return emit(pa, &pb, std::move(ip), false) && emit(sa, nullptr, std::move(is), false);
	}
	void run() {
		size_t wave_left = ss_wave_;
		Win w;
		Batch sa;
		for(;;) {
			const double tp = now();
			size_t want = batch_;
			if(temp_ss_) { const size_t shard = (ss_wave_ + streams_ - 1) / streams_; want = std::min(want, std::min(shard, wave_left)); }
			const bool more = src_.next(w, want);
			const bool bad = src_.short_mates();
			if(!more || bad) { busy_ += now() - tp; w.a.clear(); emit(w.a, nullptr, Item(), bad); return; }
			if(temp_ss_) { wave_left -= w.n; if(wave_left == 0) wave_left = ss_wave_; }
			if(!w.kinds.empty()) { if(!emit_mixed(w, sa, tp)) return; continue; }
			busy_ += now() - tp;
			Item it; it.n = w.n; it.paired = w.paired; it.first_id = w.first_id; it.skipped = w.skipped;
			if(!w.wsegs.empty()) { it.wsegs.swap(w.wsegs); it.ids.assign(w.ids64.begin(), w.ids64.end()); it.ids64.swap(w.ids64); }
			if(!emit(w.a, w.paired ? &w.b : nullptr, std::move(it), false)) return;
		}
	}
	Source& src_;                             // the parser thread's
	const int H_;
	const size_t batch_;
	const bool temp_ss_;
	const size_t ss_wave_, streams_;          // temporary splice sites: a wave is cut into one shard per stream
	std::vector<Batch> A_, B_;                // slot j mod H: see above
	std::vector<Item> meta_;                  // slot j mod H: written under m_ by emit(), then as its batches
	std::mutex m_; std::condition_variable cv_;
	long parsed_ = 0, completed_ = 0;         // guarded by m_
	bool perr_ = false, stop_ = false;        // guarded by m_
	long j_ = 0;                              // the parser thread's: the item it is at
	double busy_ = 0;                         // written by the parser thread, read after finish()
	std::thread thread_;                      // (last: it starts on members that are ready)
};

// what the stage has counted: written only by the stage (the thread that formats), read after finish()
struct Totals {
	uint64_t nreads = 0, naligned = 0, novf = 0;
	uint64_t device_planned = 0, host_planned = 0;    // --h2g-device-plan: reads / pairs whose lines the device planned; those handed on to the host planner
	uint64_t device_sam_lines = 0, whole_lines = 0;   // --h2g-device-sam: lines written on the device; of them, those that travelled as text (records beyond H2G_MAX_EDITS)
	std::string ovf_names;                    // the first of the reads / pairs whose lists overflowed, with the bits
	double t_fmt = 0;
	void note_overflow(const char* name, size_t len, uint32_t bits) {
		novf++;
		if(ovf_names.size() < 4096) { ovf_names.append(name, len); ovf_names += " (bits " + std::to_string(bits) + ")\n"; }
	}
};
// one fetched item: its reads lie in the parse stage's slot `batch`, its records in pinned set `set`
struct FmtJob { long batch; size_t n; uint64_t first_id; int set; bool paired; int merge; h2g_stream* st; /* the stream whose buffers still hold the item's compact fetch */ };

// ---- the formatter: SAM text of the fetched items, in fetch order, into the writer's buffers; the --un / --al files; the junctions into the database; the totals.
// On a thread of its own (round 6) the main thread fetches item k + 1's records while item k's text is written — what the device returns goes to one of two sets of
// page-locked buffers, the formatter works through them in order.  Not with temporary splice sites / a novel-site file: there a batch's junctions must be in the database
// before the next wave starts, and submit() formats on the caller's thread.  Either way one thread formats: everything below the queue is that thread's.
class FormatStage {
public:
	struct Config { bool async, qc_filter, drop_unal, temp_ss, merge_sites, warn_short; uint32_t khits; bool device_sam, device_plan; };
	FormatStage(const Config& c, h2g_sam* sam, ParseStage& parse, TextWriter& writer, ReadSorter& sorter, SpliceSites& sites, const Replicas& ix)
		: c_(c), sam_(sam), parse_(parse), writer_(writer), sorter_(sorter), sites_(sites), ix_(ix) { if(c_.async) thread_ = std::thread(&FormatStage::run, this); }
	~FormatStage() { finish(); }
	FormatStage(const FormatStage&) = delete;
	// main thread: the pinned set the next fetch goes to, once the job that used it last is formatted.  It is the caller's until submit().
	int claim_set() {
		const int set = (int)(nclaimed_++ % 2);
		if(c_.async) { std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return !set_busy_[set]; }); set_busy_[set] = true; }
		return set;
	}
	PinSet& set(int i) { return pins_[i]; }
	// main thread: the item is fetched
	void submit(const FmtJob& job) {
		if(c_.async) { { std::lock_guard<std::mutex> lk(m_); queue_.push_back(job); } cv_.notify_all(); }
		else format_job(job);
	}
	// formats what is queued and ends the thread
	void finish() { if(!thread_.joinable()) return; { std::lock_guard<std::mutex> lk(m_); done_ = true; } cv_.notify_all(); thread_.join(); }
	const Totals& totals() const { return tot_; }
private:
	void run() {
		for(;;) {
			FmtJob job;
			{ std::unique_lock<std::mutex> lk(m_); cv_.wait(lk, [&] { return !queue_.empty() || done_; }); if(queue_.empty()) return; job = queue_.front(); queue_.pop_front(); }
			format_job(job);
			{ std::lock_guard<std::mutex> lk(m_); set_busy_[job.set] = false; }
			cv_.notify_all();
		}
	}
	// the SAM text of one item into `buf` (grown as needed); `ends`: where each record's text ends, when asked for
	void format_item(const FmtJob& job, RawBuf& buf, size_t& used, std::vector<uint64_t>* ends) {
		Batch& a = parse_.a(job.batch); Batch& b = parse_.b(job.batch);
		PinSet& ps = pins_[job.set];
		const size_t n = job.n;
		const bool paired = job.paired;
		used = 0;
		h2g_sam_set_first_read_id(sam_, job.first_id);
		const std::vector<uint64_t>& ids64 = parse_.item(job.batch).ids64;
		h2g_sam_set_read_ids(sam_, ids64.empty() ? nullptr : ids64.data());
		h2g_sam_set_long_edits(sam_, ps.nlong ? ps.long_edits.data() : nullptr, ps.nlong);
		if(ends) { ends->resize(n); h2g_sam_set_record_ends(sam_, ends->data()); }
		const bool qc = c_.qc_filter && !a.filt.empty();
		h2g_sam_set_read_filter(sam_, qc ? a.filt.data() : nullptr, qc && paired ? b.filt.data() : nullptr);
		auto grow = [&] { buf.resize(used + 16); return true; };
		if(c_.device_sam) device_text(job, buf, used, ends);
		else if(paired) {
			h2g_pair_result* pres = (h2g_pair_result*)ps.res.p;
			uint64_t *ao1 = (uint64_t*)ps.o1.p, *ao2 = (uint64_t*)ps.o2.p;
			buf.resize(n * 1400 + 6 * (a.codes.size() + b.codes.size()) + 4096);
			retry_on_small_buffer("h2g_sam_format_paired_compact", [&] {
				return h2g_sam_format_paired_compact(sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(),
				                                     b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n,
				                                     pres, ps.rec1.p, ao1, ps.rec2.p, ao2, c_.khits, buf.data(), buf.size(), &used); }, grow);
			for(size_t i = 0; i < n; i++) { tot_.naligned += pres[i].npairs > 0; if(pres[i].overflow) tot_.note_overflow(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i], pres[i].overflow); }
		} else {
			h2g_read_result* res = (h2g_read_result*)ps.res.p;
			uint64_t* ao1 = (uint64_t*)ps.o1.p;
			buf.resize(n * 700 + 3 * a.codes.size() + 4096);
			retry_on_small_buffer("h2g_sam_format_unpaired_compact", [&] {
				return h2g_sam_format_unpaired_compact(sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(), n,
				                                       res, ps.rec1.p, ao1, buf.data(), buf.size(), &used); }, grow);
			for(size_t i = 0; i < n; i++) { tot_.naligned += res[i].nselect > 0; if(res[i].overflow) tot_.note_overflow(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i], res[i].overflow); }
		}
		h2g_sam_set_record_ends(sam_, nullptr);
		h2g_sam_set_read_ids(sam_, nullptr);
		h2g_sam_set_read_filter(sam_, nullptr, nullptr);
	}
	// --h2g-device-sam: the same decisions as a line plan (h2g_sam_plan_*_compact; the handle counts what the format call would), the bytes by the device from the
	// batch and the compact records its stream still holds (h2g_sam_text_*) into the pinned set, and from there into `buf`; `ends` from the line starts.  The caller
	// (format_item) has set the handle up; one thread both fetches and formats in this mode, so nothing has touched the stream since the fetch.
	void device_text(const FmtJob& job, RawBuf& buf, size_t& used, std::vector<uint64_t>* ends) {
		Batch& a = parse_.a(job.batch); Batch& b = parse_.b(job.batch);
		PinSet& ps = pins_[job.set];
		const size_t n = job.n;
		size_t nl = 0, na = 0;
		if(n == 0) { used = 0; return; }
		if(c_.device_plan) {   // --h2g-device-plan: classification, the plain reads' plan and the merge on the device; the host planner sees the handed-on reads only
			ps.loffs.need((2 * n + 17) * 8);
			ps.text.need(n * 1400 + 4096);
			plan_ends_.resize(n + 1);
			auto text = [&] {
				uint64_t* lo = (uint64_t*)ps.loffs.p;
				const size_t lcap = ps.loffs.cap / 8 - 1;
				return job.paired ? h2g_sam_text_paired_planned(job.st, sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(),
				                                                b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n,
				                                                (const h2g_pair_result*)ps.res.p, ps.rec1.p, (const uint64_t*)ps.o1.p, ps.rec2.p, (const uint64_t*)ps.o2.p, c_.khits,
				                                                (char*)ps.text.p, ps.text.cap, &used, lo, lcap, &nl, plan_ends_.data())
				                  : h2g_sam_text_unpaired_planned(job.st, sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(), n,
				                                                  (const h2g_read_result*)ps.res.p, ps.rec1.p, (const uint64_t*)ps.o1.p,
				                                                  (char*)ps.text.p, ps.text.cap, &used, lo, lcap, &nl, plan_ends_.data());
			};
			retry_on_small_buffer("h2g_sam_text_planned", text, [&] {
				const bool small_text = used > ps.text.cap, small_lines = (nl + 1) * 8 > ps.loffs.cap;
				if(small_text) ps.text.need(used + 16);
				if(small_lines) ps.loffs.need((nl + 17) * 8);
				return small_text || small_lines; });
			const uint64_t* loffs = (const uint64_t*)ps.loffs.p;
			buf.resize(used + 16);
			memcpy(buf.data(), ps.text.p, used);
			if(ends) for(size_t i = 0; i < n; i++) (*ends)[i] = nl ? loffs[plan_ends_[i]] : 0;
			h2g_sam_plan_stats pst;
			if(h2g_get_sam_plan_stats(job.st, &pst, nullptr, 0) == H2G_OK) { tot_.device_planned += pst.device_planned; tot_.host_planned += pst.host_planned; tot_.whole_lines += pst.whole_lines; }
			tot_.device_sam_lines += nl;
			count_aligned(job, a, ps);
			return;
		}
		if(plan_lines_.size() < 2 * n + 16) plan_lines_.resize(2 * n + 16);
		if(plan_aux_.size() < 64 * n + 4096) plan_aux_.resize(64 * n + 4096);
		plan_ends_.resize(n + 1);
		auto plan = [&] {
			if(job.paired)
				return h2g_sam_plan_paired_compact(sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(),
				                                   b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n,
				                                   (const h2g_pair_result*)ps.res.p, ps.rec1.p, (const uint64_t*)ps.o1.p, ps.rec2.p, (const uint64_t*)ps.o2.p, c_.khits,
				                                   plan_lines_.data(), plan_lines_.size(), &nl, plan_aux_.data(), plan_aux_.size(), &na, plan_ends_.data());
			return h2g_sam_plan_unpaired_compact(sam_, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, a.names.data(), a.noffs.data(), n,
			                                     (const h2g_read_result*)ps.res.p, ps.rec1.p, (const uint64_t*)ps.o1.p,
			                                     plan_lines_.data(), plan_lines_.size(), &nl, plan_aux_.data(), plan_aux_.size(), &na, plan_ends_.data());
		};
		retry_on_small_buffer("h2g_sam_plan_compact", plan, [&] {
			if(nl <= plan_lines_.size() && na <= plan_aux_.size()) return false;
			if(nl > plan_lines_.size()) plan_lines_.resize(nl);
			if(na > plan_aux_.size()) plan_aux_.resize(na);
			return true; });
		ps.loffs.need((nl + 1) * 8);
		ps.text.need(n * 1400 + 4096);
		uint64_t* loffs = (uint64_t*)ps.loffs.p;
		auto text = [&] {
			return job.paired ? h2g_sam_text_paired(job.st, sam_, plan_lines_.data(), nl, plan_aux_.data(), na, (char*)ps.text.p, ps.text.cap, &used, loffs)
			                  : h2g_sam_text_unpaired(job.st, sam_, plan_lines_.data(), nl, plan_aux_.data(), na, (char*)ps.text.p, ps.text.cap, &used, loffs);
		};
		retry_on_small_buffer("h2g_sam_text", text, [&] { if(used <= ps.text.cap) return false; ps.text.need(used + 16); return true; });
		buf.resize(used + 16);
		memcpy(buf.data(), ps.text.p, used);
		if(ends) for(size_t i = 0; i < n; i++) (*ends)[i] = nl ? loffs[plan_ends_[i]] : 0;
		tot_.device_sam_lines += nl;
		for(size_t j = 0; j < nl; j++) tot_.whole_lines += (plan_lines_[j].bits & H2G_SAM_LINE_WHOLE_LINE) != 0;
		count_aligned(job, a, ps);
	}
	void count_aligned(const FmtJob& job, Batch& a, PinSet& ps) {
		const size_t n = job.n;
		if(job.paired) {
			const h2g_pair_result* pres = (const h2g_pair_result*)ps.res.p;
			for(size_t i = 0; i < n; i++) { tot_.naligned += pres[i].npairs > 0; if(pres[i].overflow) tot_.note_overflow(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i], pres[i].overflow); }
		} else {
			const h2g_read_result* res = (const h2g_read_result*)ps.res.p;
			for(size_t i = 0; i < n; i++) { tot_.naligned += res[i].nselect > 0; if(res[i].overflow) tot_.note_overflow(a.names.data() + a.noffs[i], a.noffs[i + 1] - a.noffs[i], res[i].overflow); }
		}
	}
	// the original text of record i of an item goes to the --un / --al files its lines [t, te) name
	void sort_record(const Batch& a, const Batch* b, size_t i, const char* t, const char* te) {
		sorter_.record(t, te, a.orig.data() + a.ooffs[i], (size_t)(a.ooffs[i + 1] - a.ooffs[i]),
		               b && b->ooffs.size() > i + 1 ? b->orig.data() + b->ooffs[i] : nullptr, b && b->ooffs.size() > i + 1 ? (size_t)(b->ooffs[i + 1] - b->ooffs[i]) : 0);
	}
	// the unpaired reads of a mixed window (merge 2): their text and that of the window's pairs (the item before) into `buf`, in record order
	size_t merge_mixed(const FmtJob& job, RawBuf& buf) {
		format_item(job, mtext_[1], mused_[1], &mends_[1]);
		Batch& a = parse_.a(job.batch);
		Batch& pa = parse_.a(job.batch - 1); Batch& pb = parse_.b(job.batch - 1);
		const size_t used = mused_[0] + mused_[1];
		buf.resize(used + 16);
		size_t at = 0, ip = 0, is = 0;
		for(uint8_t k : parse_.item(job.batch).order) {
			const int m = k ? 0 : 1;
			size_t& i = k ? ip : is;
			const uint64_t t0 = i ? mends_[m][i - 1] : 0, t1 = mends_[m][i];
			memcpy(buf.data() + at, mtext_[m].data() + t0, (size_t)(t1 - t0));
			if(c_.warn_short) warn_length_filtered(k ? pa : a, k ? &pb : nullptr, i);   // (one thread formats, in record order: each warning once, ahead of the summary)
			if(sorter_.on) sort_record(k ? pa : a, k ? &pb : nullptr, i, buf.data() + at, buf.data() + at + (t1 - t0));
			at += (size_t)(t1 - t0);
			i++;
		}
		return used;
	}
	// --no-unal with the read files: the lines with flag 0x4 go, in place; returns what is left of the `used` bytes
	static size_t drop_unaligned(RawBuf& buf, size_t used) {
		char* o = buf.data();
		for(const char* t = buf.data(), *te = buf.data() + used; t < te;) {
			const char* le = (const char*)memchr(t, '\n', (size_t)(te - t));
			le = le ? le + 1 : te;
			if(!(sam_flag_of_line(t, le) & 4u)) { memmove(o, t, (size_t)(le - t)); o += le - t; }
			t = le;
		}
		return (size_t)(o - buf.data());
	}
	// format + hand to the writer: the item whose records lie in pinned set `job.set`
	void format_job(const FmtJob& job) {
		const size_t n = job.n;
		const double tf = now();
		if(job.merge == 1) {                          // the pairs of a mixed window wait for its unpaired reads
			format_item(job, mtext_[0], mused_[0], &mends_[0]);
			tot_.t_fmt += now() - tf;
			tot_.nreads += n;
			return;
		}
		const int wi = writer_.acquire();
		RawBuf& buf = writer_.text(wi);
		size_t used = 0;
		if(job.merge == 2) used = merge_mixed(job, buf);
		else {
			std::vector<uint64_t>& ends = mends_[0];
			format_item(job, buf, used, sorter_.on ? &ends : nullptr);
			Batch& a = parse_.a(job.batch); Batch& b = parse_.b(job.batch);
			if(c_.warn_short) for(size_t i = 0; i < n; i++) warn_length_filtered(a, job.paired ? &b : nullptr, i);
			if(sorter_.on) for(size_t i = 0; i < n; i++) sort_record(a, job.paired ? &b : nullptr, i, buf.data() + (i ? ends[i - 1] : 0), buf.data() + ends[i]);
		}
		if(c_.drop_unal) used = drop_unaligned(buf, used);
		tot_.t_fmt += now() - tf;
		writer_.submit(wi, used);
		if(c_.merge_sites) sites_.merge_novel(ix_, sam_, c_.temp_ss);   // the junctions of the lines just written join the database
		tot_.nreads += n;
		parse_.release(job.merge == 2 ? 2 : 1);       // (its read buffers are free for the parser; a mixed window's pairs were kept for its merge)
	}
	const Config c_;
	h2g_sam* const sam_;                      // the formatting thread's between construction and finish()
	ParseStage& parse_;
	TextWriter& writer_;
	ReadSorter& sorter_;                      // the formatting thread's
	SpliceSites& sites_;                      // (merge_sites, which excludes async: the main thread's)
	const Replicas& ix_;
	Totals tot_;                              // written by the formatting thread, read after finish()
	std::vector<h2g_sam_line> plan_lines_; std::vector<char> plan_aux_; std::vector<uint64_t> plan_ends_;   // --h2g-device-sam: the line plan of the item being formatted
	RawBuf mtext_[2];                         // a mixed window: the text and record ends of its two items, until both are formatted; the formatting thread's
	size_t mused_[2] = {0, 0};
	std::vector<uint64_t> mends_[2];
	PinSet pins_[2];                          // set i: the main thread's from claim_set() to submit(), then the formatting thread's until its job is done
	long nclaimed_ = 0;                       // the main thread's
	std::mutex m_; std::condition_variable cv_;
	std::deque<FmtJob> queue_;                // guarded by m_: jobs in fetch order
	bool set_busy_[2] = {false, false}, done_ = false;   // guarded by m_
	std::thread thread_;                      // (last: it starts on members that are ready)
};

// ---- the devices: G streams, one per device; item k runs on stream k mod G while the others are in flight, and the items are completed (fetched, handed to the
// formatter) strictly in order.  Main thread only.
// Temporary splice sites on G devices: a wave of W reads is cut into G shards that run side by side — a read never sees the junctions of
// its own wave (readid + W > its id), so the shards need nothing from one another; every shard's junctions join the database (on every
// device) before the next wave starts (the exchange between two waves is the junction list, tens of bytes per site).
class DeviceStage {
public:
	struct Config { bool qc_filter, arbitrary_random; size_t batch; const h2g_window_plan* plan; /* -F, or null */
	                const Reader* reader; /* --h2g-device-parse: the reader whose options the items' text is parsed under, or null */ uint32_t trim5, trim3; bool phred64; };
	DeviceStage(const Config& c, const h2g_align_params& P, const Waves& wv, const Replicas& ix, ParseStage& parse, FormatStage& fmt)
		: c_(c), P_(P), wv_(wv), ix_(ix), parse_(parse), fmt_(fmt), G_(ix.streams()), S_((size_t)ix.streams()), wave_left_(wv.wave) {
		// --non-deterministic: every read / pair takes two draws, mate 1's seed then mate 2's, from one RandomSource seeded with time(0) (hisat2.cpp:3273,
		// :3311-3314; the reference keeps one per worker thread), in read order, before the -s test — skipped reads draw too.  H2G_ARB_SEED=<n> (test hook)
		// replaces time(0).
		arb_.init(getenv("H2G_ARB_SEED") ? (uint32_t)strtoul(getenv("H2G_ARB_SEED"), nullptr, 10) : (uint32_t)time(0));
	}
	DeviceStage(const DeviceStage&) = delete;
	// item k (ParseStage::wait(k) has returned it): complete what its stream still carries, upload, run
	void submit(long k, const Item& it) {
		Batch& a = parse_.a(k); Batch& b = parse_.b(k);
		const size_t n = it.n;
		const int g = (int)(k % G_);
		const double tg = now();
		if(wv_.temp_ss) {                              // a wave needs the sites of every earlier one: nothing of them stays in flight when it starts
			if(wave_left_ == wv_.wave) for(long q = k - G_; q < k; q++) if(q >= 0) complete((int)(q % G_));
			wave_left_ -= n;
			if(wave_left_ == 0) wave_left_ = wv_.wave;
		}
		complete(g);                                   // the batch this stream still carries (k - G): the oldest one in flight
		Str& sg = S_[(size_t)g];
		const bool raw = c_.reader && a.raw_n;         // --h2g-device-parse: the item travels as text (its bases are fewer than its bytes)
		size_t bases = raw ? a.raw.size() : a.codes.size();
		if(it.paired && (raw ? b.raw.size() : b.codes.size()) > bases) bases = raw ? b.raw.size() : b.codes.size();
		if(!sg.st || n > sg.reads || bases > sg.bases) {
			if(sg.st) h2g_stream_free(sg.st);
			sg.reads = n > c_.batch ? n : c_.batch; sg.bases = bases + bases / 4 + 1024;
			const double ts = now();
			if(h2g_stream_create(ix_.of_stream(g), sg.reads, sg.bases, &sg.st) != H2G_OK) die("cannot create the device stream");
			t_stream += now() - ts;
		}
		const double tq0 = now();
		const bool on_device = raw && parse_on_device(sg.st, it, a, b);      // (true: the batch is resident and `a` / `b` hold its arrays; no upload call follows)
		if(!it.wsegs.empty()) {
			// -F: the device cuts the windows out of the text itself (codes, names and ids; the host's copies are for the SAM text)
			h2g_window_plan_info pi;
			h2g_window_plan_get_info(c_.plan, &pi);
			if(h2g_set_reads_windows(sg.st, h2g_window_plan_text(c_.plan), pi.n_text, it.wsegs.data(), it.wsegs.size(), pi.len, pi.step, h2g_window_plan_prefixes(c_.plan),
			                         pi.n_prefix_bytes) != H2G_OK) die("h2g_set_reads_windows");
		} else if(!on_device) {
			if(h2g_set_reads(sg.st, a.codes.data(), a.offs.data(), a.have_quals ? a.quals.data() : nullptr, n) != H2G_OK) die("h2g_set_reads");
			if(h2g_set_read_names(sg.st, a.names.data(), a.noffs.data(), n) != H2G_OK) die("h2g_set_read_names");
			// read ids are 32 bits in the splice-site window test (DSpliceSite::readid): past that the temporary sites' visibility would wrap silently
			if(!it.ids.empty() && h2g_set_read_ids(sg.st, it.ids.data()) != H2G_OK) die("h2g_set_read_ids");
		}
		if(wv_.temp_ss && (it.ids.empty() ? it.first_id + n : it.ids64.back() + 1) > 0xffffffffull) die("read ids beyond 2^32 with temporary splice sites (use --no-temp-splicesite or split the input)");
		h2g_align_params P = P_;                       // (this run's: nothing another thread may read is changed)
		P.first_read_id = (uint32_t)it.first_id;
		sg.first_id = it.first_id;
		nsubmitted_ += n;
		warn_of_long_chain(n);
		if(it.paired && !on_device) {
			if(h2g_set_mates(sg.st, b.codes.data(), b.offs.data(), b.have_quals ? b.quals.data() : nullptr, b.names.data(), b.noffs.data(), n) != H2G_OK) die("h2g_set_mates");
		}
		if(c_.arbitrary_random) {                      // this batch's draws, in read order (the batches are submitted in read order whatever the device); the skipped reads draw too
			for(uint64_t r = 0; r < 2 * it.skipped; r++) arb_.nextU32();
			arb1_.resize(n); arb2_.resize(n);
			for(size_t r = 0; r < n; r++) { arb1_[r] = arb_.nextU32(); arb2_[r] = arb_.nextU32(); }
			if(h2g_set_read_seeds(sg.st, arb1_.data(), it.paired ? arb2_.data() : nullptr, n) != H2G_OK) die("h2g_set_read_seeds");
		}
		// --qc-filter: a read whose QSEQ filter field is '0' is not aligned (every other format's reads pass)
		if(c_.qc_filter && !a.filt.empty() && h2g_set_read_filter(sg.st, a.filt.data(), it.paired ? b.filt.data() : nullptr) != H2G_OK) die("h2g_set_read_filter");
		if(it.paired) {
			if(h2g_align_pairs_run(sg.st, &P) != H2G_OK) die("h2g_align_pairs_run");
		} else if(h2g_align_run(sg.st, &P) != H2G_OK) die("h2g_align_run");
		nruns++;
		t_up += now() - tq0;
		sg.batch = k; sg.n = n; sg.paired = it.paired; sg.merge = it.merge;
		t_gpu += now() - tg;
	}
	// the input has ended: what is in flight, oldest first
	void drain() {
		long oldest = -1;
		for(;;) {
			int gi = -1;
			for(int g = 0; g < G_; g++) if(S_[(size_t)g].batch >= 0 && (gi < 0 || S_[(size_t)g].batch < oldest)) { gi = g; oldest = S_[(size_t)g].batch; }
			if(gi < 0) break;
			const double tg = now();
			complete(gi);
			t_gpu += now() - tg;
		}
	}
	void free_streams() { for(Str& sg : S_) if(sg.st) { h2g_stream_free(sg.st); sg.st = nullptr; } }
	uint64_t nsecond = 0, nruns = 0;          // reads that took the second pass; device runs
	uint64_t ndevice_parsed = 0, nhost_parsed = 0;   // --h2g-device-parse: records the device parsed; records of the items it handed back to the host parser
	uint64_t nfast = 0, nhanded = 0;          // reads / pairs the fast pass completed; handed on to the general machine (summed over the runs)
	double t_gpu = 0, t_up = 0, t_fetch = 0, t_stream = 0;
private:
	struct Str { h2g_stream* st = nullptr; size_t reads = 0, bases = 0; long batch = -1; size_t n = 0; uint64_t first_id = 0; bool paired = false; int merge = 0; };
	// --h2g-device-parse: the item's text becomes the stream's batch (h2g_set_reads_fastq) and the arrays the formatter reads are fetched from it; false: a record of the
	// item is not plain — the host parser has filled `a` / `b` from the same text (or ended the run with its message) and the three upload calls follow
	bool parse_on_device(h2g_stream* st, const Item& it, Batch& a, Batch& b) {
		h2g_fastq_opts fo;
		memset(&fo, 0, sizeof fo);
		fo.trim5 = c_.trim5; fo.trim3 = c_.trim3; fo.phred64 = c_.phred64 ? 1 : 0; fo.final1 = fo.final2 = 1;
		h2g_fastq_result fr;
		if(h2g_set_reads_fastq(st, a.raw.data(), a.raw.size(), it.paired ? b.raw.data() : nullptr, it.paired ? b.raw.size() : 0, &fo, &fr) != H2G_OK) die("h2g_set_reads_fastq");
		if(fr.n_not_plain || fr.n_records != it.n) {
			c_.reader->parse_raw(a, it.n);
			if(it.paired) c_.reader->parse_raw(b, it.n);      // (a -2 file with more records than its -1 file: the surplus is nobody's, as without the flag)
			if(a.n() != it.n || (it.paired && b.n() != it.n)) { fprintf(stderr, "hisat2-align-amd: the host parser found %zu records where the record scan found %zu\n", a.n(), it.n); exit(1); }
			nhost_parsed += it.n;
			return false;
		}
		Batch* m[2] = {&a, &b};
		const uint64_t nb[2] = {fr.n_bases1, fr.n_bases2}, nn[2] = {fr.n_name_bytes1, fr.n_name_bytes2};
		for(int k = 0; k < (it.paired ? 2 : 1); k++) {
			Batch& s = *m[k];
			s.have_quals = true;
			s.codes.resize(nb[k]); s.quals.resize(nb[k]); s.names.resize(nn[k]); s.offs.resize(it.n + 1); s.noffs.resize(it.n + 1);
			if(h2g_fetch_read_set(st, k, nullptr, nullptr, nullptr, s.codes.data(), s.offs.data(), &s.quals[0], &s.names[0], s.noffs.data()) != H2G_OK) die("h2g_fetch_read_set");
			s.raw.clear(); s.raw_n = 0;
		}
		ndevice_parsed += it.n;
		return true;
	}
	// fetch the item that stream `g` carries into a pinned set and hand it to the formatter
	void complete(int g) {
		Str& sg = S_[(size_t)g];
		if(sg.batch < 0) return;
		h2g_stream* st = sg.st;
		const size_t n = sg.n;
		const int set = fmt_.claim_set();
		PinSet& ps = fmt_.set(set);
		const double tq0 = now();
		{	// records with more than H2G_MAX_EDITS edits (long deletions: one edit per base) keep their lists in the stream's long-edit area
			size_t nl = 0;
			h2g_status lrc = h2g_align_fetch_long_edits(st, nullptr, 0, &nl);
			if(nl) { ps.long_edits.resize(nl); lrc = h2g_align_fetch_long_edits(st, ps.long_edits.data(), ps.long_edits.size(), &nl); }
			if(lrc != H2G_OK) die("h2g_align_fetch_long_edits");
			ps.nlong = nl;
		}
		// "buffer too small" is H2G_ERR_ARG with the bytes needed in boffs[n] (zeroed first: page-locked memory starts uninitialised)
		if(sg.paired) {
			ps.res.need(n * sizeof(h2g_pair_result)); ps.o1.need((n + 1) * 8); ps.o2.need((n + 1) * 8);
			ps.rec1.need(n * 64 + 4096); ps.rec2.need(n * 64 + 4096);
			h2g_pair_result* pres = (h2g_pair_result*)ps.res.p;
			uint64_t *ao1 = (uint64_t*)ps.o1.p, *ao2 = (uint64_t*)ps.o2.p;
			ao1[n] = 0; ao2[n] = 0;
			retry_on_small_buffer("h2g_align_pairs_fetch_compact",
				[&] { return h2g_align_pairs_fetch_compact(st, pres, ps.rec1.p, ps.rec1.cap, ao1, ps.rec2.p, ps.rec2.cap, ao2, 0, n); },
				[&] { if(ao1[n] <= ps.rec1.cap && ao2[n] <= ps.rec2.cap) return false; ps.rec1.need(ao1[n] + 8); ps.rec2.need(ao2[n] + 8); return true; });
		} else {
			ps.res.need(n * sizeof(h2g_read_result)); ps.o1.need((n + 1) * 8); ps.rec1.need(n * 64 + 4096);
			h2g_read_result* res = (h2g_read_result*)ps.res.p;
			uint64_t* ao1 = (uint64_t*)ps.o1.p;
			ao1[n] = 0;
			retry_on_small_buffer("h2g_align_fetch_compact",
				[&] { return h2g_align_fetch_compact(st, res, ps.rec1.p, ps.rec1.cap, ao1, 0, n); },
				[&] { if(ao1[n] <= ps.rec1.cap) return false; ps.rec1.need(ao1[n] + 8); return true; });
		}
		{ h2g_counters hc; if(h2g_get_counters(st, &hc) == H2G_OK) { nsecond += hc.n_second_pass; nfast += hc.n_fast; nhanded += hc.n_fast_bail; } }
		t_fetch += now() - tq0;
		const FmtJob job{sg.batch, n, sg.first_id, set, sg.paired, sg.merge, st};
		sg.batch = -1;                                  // (the stream's rows are copied: it can take the next batch)
		fmt_.submit(job);
	}
	// the chain mode (window 0: waves of ONE read) is exact and meant for small inputs; an input that turns out not to be small is told so,
	// loudly and once (a small run's stderr stays the reference's summary, byte for byte)
	void warn_of_long_chain(size_t n) const {
		if(wv_.temp_ss && wv_.window == 0 && nsubmitted_ >= 20000 && nsubmitted_ - n < 20000 && !getenv("H2G_QUIET_CHAIN_WARNING"))
			fprintf(stderr, "Warning: hisat2-align-amd: -p 1 with temporary splice sites is the reference's strict read-after-read chain (window 0, hisat2.cpp:3687): "
			                "it runs as waves of ONE read - a device round trip and a database merge per read; 20000 reads in, this input is not small. "
			                "Use -p >= 2 or --ss-window W (output == hisat2 -p W/1000 --reorder), or --no-temp-splicesite, for throughput.\n");
	}
	const Config c_;
	const h2g_align_params P_;
	const Waves wv_;
	const Replicas& ix_;
	ParseStage& parse_;
	FormatStage& fmt_;
	const int G_;
	std::vector<Str> S_;
	size_t wave_left_;                        // reads the current wave still takes
	uint64_t nsubmitted_ = 0;
	h2g::Rng arb_;                            // --non-deterministic
	std::vector<uint32_t> arb1_, arb2_;
};

void write_novel_sites(const std::string& fn, h2g_sam* sam) {   // hisat2.cpp:4189-4197
	FILE* nf = fopen(fn.c_str(), "w");
	if(!nf) return;
	const size_t need = h2g_sam_novel_splice_sites_text(sam, nullptr, 0);
	std::vector<char> tb(need + 1);
	h2g_sam_novel_splice_sites_text(sam, tb.data(), need);
	fwrite(tb.data(), 1, need, nf);
	fclose(nf);
}
// the reference's alignment summary (aln_sink.h:1637), same text
void write_summary(const Options& o, h2g_sam* sam) {
	const size_t need = h2g_sam_summary(sam, nullptr, 0);
	std::vector<char> sb(need + 1);
	h2g_sam_summary(sam, sb.data(), need);
	if(!o.quiet) fwrite(sb.data(), 1, need, stderr);
	if(!o.quiet && !o.summary_file.empty()) { FILE* sf = fopen(o.summary_file.c_str(), "w"); if(sf) { fwrite(sb.data(), 1, need, sf); fclose(sf); } }   // hisat2.cpp:4175
}

}  // namespace

int main(int argc, char** argv) {
	Options o = parse_options(argc, argv);
	if(const int rc = o.check()) return rc;
	TempInputs tmp_inputs(o);
	WindowPlan wp;
	if(o.windows) if(const int rc = wp.load(o)) return rc;
	if(o.parse_only) {
		if(o.windows) { Source src(wp.plan, wp.first, wp.n); return parse_only(o, src); }
		Source src(o.m1, o.m2, o.u, o.m12, o.fmt, o.threads, o.trim5, o.trim3, o.qcoding, false, o.skip, o.upto);
		return parse_only(o, src);
	}
	Waves wv;
	size_t batch = o.batch;
	if(const int rc = plan_waves(o, &wv, &batch)) return rc;
	if(o.windows && wv.temp_ss && wp.info.next_rdid > 0x100000000ull) {
		fprintf(stderr, "hisat2-align-amd: -F %u,%u: the read ids pass 2^32 - 1, beyond what the temporary-splice-site mode compares (use --no-temp-splicesite or split the input)\n", o.win_len, o.win_step);
		return 1;
	}
	const double t0 = now();
	Replicas ix;
	if(const int rc = ix.load(o, wv.temp_ss)) return rc;
	h2g_align_params P = o.P;
	h2g_sam* sam = nullptr;
	if(const int rc = open_sam(o, ix, wv, &P, &sam, &batch)) return rc;
	SpliceSites sites;
	if(const int rc = start_splice_sites(o, P, wv, ix, sam, &sites)) return rc;
	apply_sam_settings(o, P, sam);
	FILE* out = open_output(o, sam);
	if(!out) return 1;
	const double t1 = now();
	h2g_sam_set_threads(sam, o.threads);
	// --no-unal with the read files: the reads are sorted by the flags of every line, the unaligned ones included, so the sink prints them and the formatter stage
	// leaves the lines with flag 0x4 out afterwards, as the reference's script does (it takes --no-unal away from its binary)
	const bool drop_unal = o.sorting && o.no_unal;
	h2g_sam_set_no_unal(sam, o.no_unal && !drop_unal ? 1 : 0);
	// (-s / -u: the record stream skips and counts, Source::next; -u counts the reads after the skipped ones, qUpto += skipReads hisat2.cpp:1959-1963)
	std::unique_ptr<Source> src_owner(o.windows ? new Source(wp.plan, wp.first, wp.n)
	                                            : new Source(o.m1, o.m2, o.u, o.m12, o.fmt, o.threads, o.trim5, o.trim3, o.qcoding, o.sorting, o.skip, o.upto, o.device_parse));
	Source& src = *src_owner;
	ReadSorter sorter;
	for(int k = 0; k < RS_KINDS; k++) if(!o.rs_arg[k].empty()) sorter.open(k, o.rs_arg[k], o.rs_gz[k]);
	const bool merge_sites = wv.temp_ss || !o.novel_out.empty();
	// (--h2g-device-sam: no formatter thread — the SAM handle and the stream would be touched from two threads)
	const bool async_fmt = !merge_sites && !o.device_sam && !(getenv("H2G_CLI_ASYNC_FMT") && atoi(getenv("H2G_CLI_ASYNC_FMT")) == 0);
	const int H = ix.streams() + (async_fmt ? 3 : 2);
	// the stages; their destructors join in the reverse order, whatever way out is taken
	TextWriter writer(out);
	ParseStage parse(src, H, batch, wv, ix.streams());
	FormatStage fmt(FormatStage::Config{async_fmt, o.qc_filter, drop_unal, wv.temp_ss, merge_sites, !o.quiet, P.khits, o.device_sam, o.device_plan}, sam, parse, writer, sorter, sites, ix);
	DeviceStage dev(DeviceStage::Config{o.qc_filter, o.arbitrary_random, batch, wp.plan, o.device_parse ? src.any_reader() : nullptr, o.trim5, o.trim3, o.qcoding.phred64}, P, wv, ix, parse, fmt);
	double t_parse = 0;                                   // what the main thread waited for the parser
	bool short_mates = false;
	for(long k = 0;; k++) {
		const double tp = now();
		const Item& it = parse.wait(k, &short_mates);
		if(short_mates) break;
		t_parse += now() - tp;
		if(it.n == 0 && it.merge == 0) break;
		dev.submit(k, it);
	}
	if(short_mates) fprintf(stderr, "Error, fewer reads in file specified with -2 than in file specified with -1\n");   // (what is in flight is dropped)
	else dev.drain();
	parse.finish();
	fmt.finish();
	writer.finish();
	if(short_mates) return 1;
	if(writer.failed()) { fprintf(stderr, "Error: writing the SAM output failed\n"); return 1; }
	if(out != stdout) fclose(out); else fflush(out);
	if(!sorter.close()) { fprintf(stderr, "Error: writing the --un / --al read files failed\n"); return 1; }
	if(!o.novel_out.empty()) write_novel_sites(o.novel_out, sam);
	const double t2 = now();
	write_summary(o, sam);
	const Totals& tot = fmt.totals();
	// Reads whose lists overflow the default device workspace are re-run on the device with the large one (h2g_align_run's
	// second pass).  What is still flagged after that is NOT known to equal the reference's output: name it and fail.
	if(tot.novf) fprintf(stderr, "Error: %llu %s exceeded even the large device workspace (h2g overflow bit); their SAM records are not verified "
	                     "against hisat2 -- rerun these with the reference aligner:\n%s", (unsigned long long)tot.novf, "reads / pairs", tot.ovf_names.c_str());
	if(getenv("H2G_CLI_TIMING")) fprintf(stderr, "time: index load %.2f s, align+fetch %.2f s (waited for the parser thread %.2f s; it parsed for %.2f s), SAM formatting %.2f s, total %.2f s [stream create %.2f, upload+launch %.2f, wait+fetch %.2f]\n", t1 - t0, dev.t_gpu,
	        t_parse, parse.busy(), tot.t_fmt, t2 - t0, dev.t_stream, dev.t_up, dev.t_fetch);
	if(!o.stats_fn.empty()) {
		FILE* sf = fopen(o.stats_fn.c_str(), "w");
		if(sf) { fprintf(sf, "{\"reads\": %llu, \"second_pass\": %llu, \"overflow\": %llu, \"runs\": %llu, \"fast\": %llu, \"handed_on\": %llu, \"device_sam_lines\": %llu, \"whole_lines\": %llu, \"device_planned\": %llu, \"host_planned\": %llu, \"device_parsed\": %llu, \"host_parsed\": %llu}\n", (unsigned long long)tot.nreads, (unsigned long long)dev.nsecond, (unsigned long long)tot.novf, (unsigned long long)dev.nruns,
		                 (unsigned long long)dev.nfast, (unsigned long long)dev.nhanded, (unsigned long long)tot.device_sam_lines, (unsigned long long)tot.whole_lines,
		                 (unsigned long long)tot.device_planned, (unsigned long long)tot.host_planned, (unsigned long long)dev.ndevice_parsed, (unsigned long long)dev.nhost_parsed); fclose(sf); }
	}
	// (Measured and not shipped, round 6: ending the process here without the frees below saves this run 0.1 s and costs the NEXT process 1.7 s — the driver reclaims 40 GB of
	// device memory of a process that did not return it while the next one is already allocating: profiles/r06_zc_ab.log.)
	dev.free_streams();
	h2g_sam_close(sam);
	ix.free_all();
	return tot.novf ? 3 : 0;
}
