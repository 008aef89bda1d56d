// win_check.cpp — stand-alone host check of the -F window expansion's per-read arithmetic (hisat2_amd/csrc/h2g_windows.h): drives the functions the
// expansion kernels call, lane by lane as the kernels do (16 output bytes per lane of the code array, one lane per read for offsets, ids and names),
// over exactly-sized buffers, and compares every array with a naive loop.  Built with -fsanitize=address,undefined by tests/test_windows_cpu.py; it has
// no device code and never runs on a GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../hisat2_amd/csrc/h2g_windows.h"

using h2g_win::DSeg;

struct Seg { uint64_t text_start, name_off0, rdid0; uint32_t n_windows; std::string prefix; };

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while(0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 20); }

static void run_case(const char* what, const std::vector<Seg>& segs, uint32_t len, uint32_t step) {
	// the text the segments touch and nothing more
	uint64_t n_text = 0;
	for(const Seg& s : segs) { const uint64_t e = s.text_start + (uint64_t)(s.n_windows - 1) * step + len; if(e > n_text) n_text = e; }
	std::vector<uint8_t> text(n_text);
	for(uint8_t& c : text) c = (uint8_t)(rnd() % 5);
	std::string prefixes;
	// naive expansion
	std::vector<uint8_t> want_codes;
	std::vector<uint32_t> want_offs(1, 0), want_noffs(1, 0), want_ids;
	std::string want_names;
	std::vector<DSeg> ds;
	uint32_t n = 0;
	for(const Seg& s : segs) {
		DSeg d;
		memset(&d, 0, sizeof d);
		d.name_off0 = s.name_off0; d.text_start = (uint32_t)s.text_start; d.rdid0 = (uint32_t)s.rdid0; d.first_read = n; d.name_first = (uint32_t)want_names.size();
		d.prefix_start = (uint32_t)prefixes.size(); d.prefix_len = (uint32_t)s.prefix.size();
		prefixes += s.prefix;
		ds.push_back(d);
		for(uint32_t j = 0; j < s.n_windows; j++) {
			for(uint32_t k = 0; k < len; k++) want_codes.push_back(text[s.text_start + (uint64_t)j * step + k]);
			want_offs.push_back((uint32_t)want_codes.size());
			want_names += s.prefix + std::to_string(s.name_off0 + (uint64_t)j * step);
			want_noffs.push_back((uint32_t)want_names.size());
			want_ids.push_back((uint32_t)(s.rdid0 + (uint64_t)j * step));
			n++;
		}
	}
	DSeg sentinel;
	memset(&sentinel, 0, sizeof sentinel);
	sentinel.first_read = n; sentinel.name_first = (uint32_t)want_names.size();
	ds.push_back(sentinel);
	const uint32_t n_segs = (uint32_t)segs.size();
	// what the host of h2g_set_reads_windows computes per segment: the name bytes through width_sum
	{
		uint64_t nb = 0;
		for(size_t k = 0; k < segs.size(); k++) {
			CHECK(ds[k].name_first == nb, "%s: name_first of segment %zu", what, k);
			nb += (uint64_t)segs[k].n_windows * segs[k].prefix.size() + h2g_win::width_sum(segs[k].name_off0, step, segs[k].n_windows);
		}
		CHECK(nb == want_names.size(), "%s: name bytes %llu != %zu", what, (unsigned long long)nb, want_names.size());
	}
	// k_win_codes, lane by lane
	const uint64_t n_bytes = (uint64_t)n * len;
	std::vector<uint8_t> codes(n_bytes);
	for(uint64_t c = 0; c < (n_bytes + 15) / 16; c++) {
		const uint64_t b0 = c * 16;
		const uint32_t m = n_bytes - b0 < 16 ? (uint32_t)(n_bytes - b0) : 16u;
		h2g_win::CodeCursor cur;
		cur.seek(ds.data(), n_segs, len, step, b0);
		for(uint32_t k = 0; k < m; k++) {
			const uint32_t src = cur.next();
			if(src >= text.size()) { CHECK(false, "%s: byte %llu reads text[%u] of %zu", what, (unsigned long long)(b0 + k), src, text.size()); return; }
			codes[b0 + k] = text[src];
		}
	}
	CHECK(codes == want_codes, "%s: codes differ", what);
	// k_win_meta, lane by lane
	std::vector<uint32_t> offs(n + 1), noffs(n + 1), ids(n);
	std::string names(want_names.size(), '?');
	for(uint32_t r = 0; r <= n; r++) {
		offs[r] = r * len;
		if(r == n) { noffs[r] = ds[n_segs].name_first; break; }
		const uint32_t si = h2g_win::seg_of(ds.data(), n_segs, r);
		const DSeg s = ds[si];
		const uint32_t j = r - s.first_read;
		ids[r] = s.rdid0 + j * step;
		const uint32_t at = h2g_win::name_start(s, step, j);
		noffs[r] = at;
		char tmp[256 + 24];
		const uint32_t nl = h2g_win::write_name(s, step, j, prefixes.data(), tmp);
		if((uint64_t)at + nl > names.size()) { CHECK(false, "%s: name of read %u ends at %llu of %zu", what, r, (unsigned long long)at + nl, names.size()); return; }
		memcpy(&names[at], tmp, nl);
	}
	CHECK(offs == want_offs, "%s: offs differ", what);
	CHECK(noffs == want_noffs, "%s: name offs differ", what);
	CHECK(ids == want_ids, "%s: ids differ", what);
	CHECK(names == want_names, "%s: names differ", what);
}

int main() {
	const uint32_t lens[] = {1, 3, 30, 33, 128, 129, 512};
	const std::string long_prefix(199, 'p');
	int cases = 0;
	for(uint32_t len : lens) {
		const uint32_t steps[] = {0, 1, 7, len, len + 5};
		for(uint32_t step : steps) {
			char what[96];
			auto name = [&](const char* shape) { snprintf(what, sizeof what, "len %u step %u %s", len, step, shape); cases++; return what; };
			run_case(name("single window"), {Seg{0, 0, 0, 1, "r_"}}, len, step);
			for(uint32_t nw : {63u, 64u, 65u}) run_case(name("63/64/65 windows"), {Seg{2, 5, 1000, nw, "chr1_"}}, len, step);
			{	// 300 segments of 1-3 windows, as the records of a fragmented assembly
				std::vector<Seg> v;
				uint64_t t = 0, id = 17;
				for(int k = 0; k < 300; k++) {
					const uint32_t nw = 1 + rnd() % 3;
					v.push_back(Seg{t, 0, id, nw, "ctg" + std::to_string(k) + "_"});
					t += (uint64_t)(nw - 1) * step + len + rnd() % 4;
					id += (uint64_t)(nw - 1) * step + 1;
				}
				run_case(name("300 segments"), v, len, step);
			}
			{	// printed offsets that straddle a decimal width, an empty and a 200-byte prefix, a batch that begins inside a record
				std::vector<Seg> v;
				uint64_t t = 3;
				const uint64_t edges[] = {9, 99, 999999, 4294967290ull};
				for(uint64_t e : edges) {
					const uint64_t off0 = e >= 3ull * (step ? step : 1) ? e - 3ull * (step ? step : 1) : 0;
					v.push_back(Seg{t, off0, off0 + 12345, 9, e == 99 ? "" : e == 999999 ? long_prefix + "_" : "x_"});
					t += 8ull * step + len;
				}
				run_case(name("width edges"), v, len, step);
			}
		}
	}
	// width_sum against the loop, widths up to 20 digits
	for(uint64_t off0 : {0ull, 1ull, 9ull, 10ull, 95ull, 999999999ull, 4294967290ull, 9999999999999999990ull}) for(uint32_t step : {0u, 1u, 3u, 1000u}) for(uint32_t j : {0u, 1u, 2u, 11u, 1000u}) {
		if(off0 > 1ull << 62 && (uint64_t)step * j > 9) continue;
		uint64_t want = 0;
		for(uint32_t i = 0; i < j; i++) want += std::to_string(off0 + (uint64_t)i * step).size();
		CHECK(h2g_win::width_sum(off0, step, j) == want, "width_sum(%llu, %u, %u)", (unsigned long long)off0, step, j);
	}
	printf("win_check: %d cases, %d failures\n", cases, failures);
	return failures ? 1 : 0;
}
