// fastq_host_parse.cpp — times the command line's host parser (Source / Reader, csrc/h2g_cli_reads.h) over a pair of FASTQ files, as its parser thread runs it: the two
// mate files side by side, <threads> threads each, batches of <batch> records.  tools/fastq_upload_bench.py builds it as a shared library and calls
// fastq_host_parse() from its own process, between the device calls it is compared with; as a program:
//   fastq_host_parse <r1.fq> <r2.fq> <threads> <batch> <repeats>   ->   one line per repeat: seconds, records, bases (the first repeat also maps and faults the files in)
#include <chrono>
#include "../hisat2_amd/csrc/h2g_cli_reads.h"

// one pass over the two files -> seconds; *records, *bases: what was parsed
extern "C" __attribute__((visibility("default"))) double fastq_host_parse(const char* f1, const char* f2, int threads, size_t batch, uint64_t* records, uint64_t* bases) {
	const auto t0 = std::chrono::steady_clock::now();
	h2g_cli::Source src({f1}, {f2}, {}, {}, h2g_cli::FMT_FASTQ, threads, 0, 0, h2g_cli::QualCoding(), false, 0, ~0ull);
	h2g_cli::Win w;
	uint64_t n = 0, nb = 0;
	while(src.next(w, batch)) { n += w.n; nb += w.a.codes.size() + w.b.codes.size(); }
	*records = n; *bases = nb;
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
	if(argc != 6) { fprintf(stderr, "usage: fastq_host_parse <r1.fq> <r2.fq> <threads> <batch> <repeats>\n"); return 2; }
	for(int r = 0; r < atoi(argv[5]); r++) {
		uint64_t n = 0, bases = 0;
		const double dt = fastq_host_parse(argv[1], argv[2], atoi(argv[3]), (size_t)atoll(argv[4]), &n, &bases);
		printf("%.6f %llu %llu\n", dt, (unsigned long long)n, (unsigned long long)bases);
	}
	return 0;
}
