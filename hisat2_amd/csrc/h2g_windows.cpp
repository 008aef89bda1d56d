// -F <len>,<step>: the planner of the window read source (include/h2g.h, h2g_window_plan_*).  Host only, no device: the command line (h2g_cli.cpp)
// and the Python binding (api.py) both plan through it.  FastaContinuousPatternSource::read, pat.h:1233-1336, restated over whole files:
// the reference emits a window every time its `eat` counter runs out; here a record's windows follow from its base count.
#include "../../include/h2g.h"
#include <cstring>
#include <new>
#include <string>
#include <vector>

struct h2g_window_plan {
	uint32_t len = 0, step = 0;
	uint64_t next_rdid = 0;                   // R0 of the next record that yields reads (BufferedFilePatternSource::readCnt_ at its first window)
	uint64_t n_reads = 0;
	std::vector<uint8_t> text;
	std::string prefixes;
	std::vector<h2g_window_seg> segs;         // one per record that yields reads
	std::vector<uint64_t> first_read;         // per segment: index of its window 0; [n_segs] = n_reads
};

namespace {

// asc2dnacat (alphabet.cpp:36-58) and asc2dna of what FastaContinuousPatternSource keeps: 0xff = not counted; A C G T = 0..3; the IUPAC letters, N and '-' = 4
struct CodeTable {
	uint8_t t[256];
	CodeTable() {
		memset(t, 0xff, sizeof t);
		for(const char* p = "BDHKMNRSVWXYbdhkmnrsvwxy-"; *p; p++) t[(unsigned char)*p] = 4;
		const char* acgt = "ACGT";
		for(int k = 0; k < 4; k++) { t[(unsigned char)acgt[k]] = (uint8_t)k; t[(unsigned char)(acgt[k] | 0x20)] = (uint8_t)k; }
	}
};
bool is_space(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace() in the "C" locale

// the record whose bases are text[t0, text.size()) is over
// (false: it has more windows than a segment counts)
bool close_record(h2g_window_plan* p, size_t t0, uint32_t prefix_start, uint32_t prefix_len) {
	const uint64_t L = p->text.size() - t0;
	if(L < p->len) return true;
	if(p->step && (L - p->len) / p->step >= 0xffffffffull) return false;
	h2g_window_seg s;
	memset(&s, 0, sizeof s);
	s.text_start = t0; s.name_off0 = 0; s.rdid0 = p->next_rdid;
	s.n_windows = p->step == 0 ? 1u : (uint32_t)((L - p->len) / p->step + 1);
	s.prefix_start = prefix_start; s.prefix_len = prefix_len;
	p->first_read.back() = p->n_reads;
	p->segs.push_back(s);
	p->n_reads += s.n_windows;
	p->first_read.push_back(p->n_reads);
	p->next_rdid += L - p->len + 1;
	return true;
}

}  // namespace

extern "C" h2g_status h2g_window_plan_create(uint32_t len, uint32_t step, uint64_t first_rdid, h2g_window_plan** out) {
	if(!out || len == 0 || len > 1024) return H2G_ERR_ARG;
	h2g_window_plan* p = new(std::nothrow) h2g_window_plan;
	if(!p) return H2G_ERR_NOMEM;
	p->len = len; p->step = step; p->next_rdid = first_rdid;
	p->first_read.push_back(0);
	*out = p;
	return H2G_OK;
}

extern "C" h2g_status h2g_window_plan_add_file(h2g_window_plan* p, const char* bytes, size_t n) {
	if(!p || (!bytes && n)) return H2G_ERR_ARG;
	static const CodeTable T;
	// (H2G_ERR_ARG: a record of more than 2^32 - 1 windows does not fit a segment's count, and the prefix pool is addressed with 32 bits)
	try {
		p->text.reserve(p->text.size() + n);
		size_t t0 = p->text.size();
		uint32_t pstart = (uint32_t)p->prefixes.size(), plen = 0;      // text before the first '>': an empty prefix, no underscore
		for(size_t i = 0; i < n;) {
			const unsigned char c = (unsigned char)bytes[i++];
			if(c != '>') { const uint8_t v = T.t[c]; if(v != 0xff) p->text.push_back(v); continue; }
			// any '>' outside a header line starts a record (pat.h:1247): the name up to the first white space, the rest of the line, every line end behind it
			if(!close_record(p, t0, pstart, plen)) return H2G_ERR_ARG;
			t0 = p->text.size();
			if(p->prefixes.size() > 0xfffff000u) return H2G_ERR_ARG;
			pstart = (uint32_t)p->prefixes.size();
			bool saw_space = false;
			for(; i < n && bytes[i] != '\n' && bytes[i] != '\r'; i++) {
				if(!saw_space) saw_space = is_space((unsigned char)bytes[i]);
				if(!saw_space) p->prefixes.push_back(bytes[i]);
			}
			while(i < n && (bytes[i] == '\n' || bytes[i] == '\r')) i++;
			p->prefixes.push_back('_');
			plen = (uint32_t)(p->prefixes.size() - pstart);
		}
		if(!close_record(p, t0, pstart, plen)) return H2G_ERR_ARG;
	} catch(const std::bad_alloc&) { return H2G_ERR_NOMEM; }
	return H2G_OK;
}

extern "C" h2g_status h2g_window_plan_get_info(const h2g_window_plan* p, h2g_window_plan_info* out) {
	if(!p || !out) return H2G_ERR_ARG;
	memset(out, 0, sizeof *out);
	out->n_reads = p->n_reads; out->n_text = p->text.size(); out->n_segs = p->segs.size(); out->n_prefix_bytes = p->prefixes.size();
	out->next_rdid = p->next_rdid; out->len = p->len; out->step = p->step;
	return H2G_OK;
}
extern "C" const uint8_t* h2g_window_plan_text(const h2g_window_plan* p) { return p ? p->text.data() : nullptr; }
extern "C" const char* h2g_window_plan_prefixes(const h2g_window_plan* p) { return p ? p->prefixes.data() : nullptr; }

namespace {
// the segment that holds read r (r < n_reads)
size_t seg_of_read(const h2g_window_plan* p, uint64_t r) {
	size_t lo = 0, hi = p->segs.size();       // first_read[lo] <= r < first_read[hi]
	while(hi - lo > 1) { const size_t mid = lo + (hi - lo) / 2; if(p->first_read[mid] <= r) lo = mid; else hi = mid; }
	return lo;
}
}  // namespace

extern "C" size_t h2g_window_plan_segments(const h2g_window_plan* p, uint64_t first_read, uint64_t n, h2g_window_seg* out, size_t cap) {
	if(!p || first_read >= p->n_reads || n == 0) return 0;
	if(n > p->n_reads - first_read) n = p->n_reads - first_read;
	size_t cnt = 0;
	uint64_t r = first_read;
	for(size_t s = seg_of_read(p, r); n > 0; s++) {
		const uint64_t j = r - p->first_read[s];                       // the range begins inside segment s at window j
		uint64_t take = p->segs[s].n_windows - j;
		if(take > n) take = n;
		if(out && cnt < cap) {
			h2g_window_seg x = p->segs[s];
			x.text_start += j * p->step; x.name_off0 += j * p->step; x.rdid0 += j * p->step;
			x.n_windows = (uint32_t)take;
			out[cnt] = x;
		}
		cnt++;
		r += take; n -= take;
	}
	return cnt;
}

extern "C" void h2g_window_plan_select(const h2g_window_plan* p, uint64_t lo, uint64_t hi, uint64_t* first_read, uint64_t* n) {
	uint64_t a = 0, b = 0;
	if(p) {
		// rdids ascend with the read index (equal never: one window per record at step 0, and a record advances the counter by at least 1)
		auto first_at_or_past = [&](uint64_t id) {
			uint64_t r = p->n_reads;
			for(size_t s = 0; s < p->segs.size(); s++) {            // (linear over records: called once per run)
				const h2g_window_seg& x = p->segs[s];
				const uint64_t last = x.rdid0 + (uint64_t)(x.n_windows - 1) * p->step;
				if(last < id) continue;
				const uint64_t j = x.rdid0 >= id ? 0 : (id - x.rdid0 + p->step - 1) / p->step;
				r = p->first_read[s] + j;
				break;
			}
			return r;
		};
		a = first_at_or_past(lo);
		b = hi <= lo ? a : first_at_or_past(hi);
	}
	if(first_read) *first_read = a;
	if(n) *n = b - a;
}

extern "C" void h2g_window_plan_free(h2g_window_plan* p) { delete p; }
