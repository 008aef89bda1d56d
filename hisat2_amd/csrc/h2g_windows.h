// h2g_windows.h — the per-read arithmetic of the -F <len>,<step> window expansion (include/h2g.h, h2g_set_reads_windows): which segment a read
// belongs to, where its name starts, the bytes of its name, and which text byte an output code byte is a copy of.  The same functions run in the
// expansion kernels (h2g_kernels.hip), on the host where h2g_set_reads_windows sizes the names, and, lane by lane, in the stand-alone checker
// tests/windows/win_check.cpp, which is built with the host sanitizers.  Nothing here touches memory it is not handed.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifndef H2G_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define H2G_HD __host__ __device__ __forceinline__
#else
#define H2G_HD inline
#endif
#endif

namespace h2g_win {

// A segment as the kernels read it (h2g_set_reads_windows derives it from h2g_window_seg): a run of windows of one FASTA record.
struct DSeg {
	uint64_t name_off0;        // the offset window 0 prints
	uint32_t text_start;       // window 0's first base, relative to the uploaded text range
	uint32_t rdid0;            // Read::rdid of window 0 (32 bits, as h2g_set_read_ids)
	uint32_t first_read;       // index of window 0 in the batch: ascending over the table; entry n_segs holds the batch's read count
	uint32_t name_first;       // first name byte of window 0; entry n_segs holds the batch's name bytes
	uint32_t prefix_start, prefix_len;
};
static_assert(sizeof(DSeg) == 32, "DSeg layout");

// the segment of read r: the last one with first_read <= r (segs[n_segs] is the sentinel; r < segs[n_segs].first_read)
H2G_HD uint32_t seg_of(const DSeg* segs, uint32_t n_segs, uint32_t r) {
	uint32_t lo = 0, hi = n_segs;      // invariant: segs[lo].first_read <= r < segs[hi].first_read
	while(hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if(segs[mid].first_read <= r) lo = mid; else hi = mid; }
	return lo;
}
H2G_HD uint32_t dec_width(uint64_t v) { uint32_t w = 1; while(v >= 10) { v /= 10; w++; } return w; }
// Sum of the decimal widths of off0 + i * step for 0 <= i < j: a width is 1 + the number of powers of ten (10, 100, ...) at or below the value, and the
// values ascend, so every power of ten contributes the count of values at or above it — whole decades, at most 19 terms, no loop over the windows.
// (off0 + j * step stays below 2^63: offsets are positions in a FASTA record.)
H2G_HD uint64_t width_sum(uint64_t off0, uint32_t step, uint32_t j) {
	if(j == 0) return 0;
	if(step == 0) return (uint64_t)j * dec_width(off0);
	uint64_t sum = j;
	const uint64_t last = off0 + (uint64_t)(j - 1) * step;
	for(uint64_t p = 10; p <= last; p *= 10) {
		// values below p: i with off0 + i * step < p
		const uint64_t below = off0 >= p ? 0 : (p - off0 + step - 1) / step;      // ceil((p - off0) / step), at most j since last >= p
		sum += j - below;
		if(p > UINT64_MAX / 10) break;
	}
	return sum;
}
// first name byte of window j of segment s
H2G_HD uint32_t name_start(const DSeg& s, uint32_t step, uint32_t j) {
	return s.name_first + j * s.prefix_len + (uint32_t)width_sum(s.name_off0, step, j);
}
// the name of window j of segment s into out[0 .. returned length): the prefix, then the decimal offset
H2G_HD uint32_t write_name(const DSeg& s, uint32_t step, uint32_t j, const char* prefixes, char* out) {
	for(uint32_t k = 0; k < s.prefix_len; k++) out[k] = prefixes[s.prefix_start + k];
	const uint64_t v = s.name_off0 + (uint64_t)j * step;
	const uint32_t w = dec_width(v);
	uint64_t x = v;
	for(uint32_t k = w; k-- > 0;) { out[s.prefix_len + k] = (char)('0' + x % 10); x /= 10; }
	return s.prefix_len + w;
}
// index in the uploaded text of base k of window j of segment s
H2G_HD uint32_t src_index(const DSeg& s, uint32_t step, uint32_t j, uint32_t k) { return s.text_start + j * step + k; }

// Walks consecutive output bytes of the code array: byte b = base (b % len) of read (b / len).  seek() places the cursor (one division and one
// binary search); next() yields the text index of the byte under it and moves on, crossing reads and segments without either.
struct CodeCursor {
	const DSeg* segs; uint32_t n_segs, len, step;
	uint32_t seg, r, k, src;           // segment, read and base of the byte under the cursor; its text index
	H2G_HD void seek(const DSeg* s, uint32_t ns, uint32_t len_, uint32_t step_, uint64_t byte) {
		segs = s; n_segs = ns; len = len_; step = step_;
		r = (uint32_t)(byte / len); k = (uint32_t)(byte % len);
		seg = seg_of(segs, n_segs, r);
		src = src_index(segs[seg], step, r - segs[seg].first_read, k);
	}
	H2G_HD uint32_t next() {
		const uint32_t at = src;
		if(++k < len) { src++; return at; }
		k = 0; r++;
		if(r < segs[n_segs].first_read) {         // (past the last read the cursor is never read again)
			while(segs[seg + 1].first_read <= r) seg++;
			src = src_index(segs[seg], step, r - segs[seg].first_read, 0);
		}
		return at;
	}
};

}  // namespace h2g_win
