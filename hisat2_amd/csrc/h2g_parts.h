// h2g_parts.h — a device area in equal parts: `parts` parts of `cap` elements, part m is [m * cap, (m + 1) * cap), and whoever owns part m fills it from lo(m)
// through a cursor of its own.  The stream's pair-overflow, long-edit and XL-list areas are three of these, one part per lane (h2g_kernels.hip, h2g_stream).
// Where a part's cursor lives, and which streams are waited for before an area is replaced, is the caller's business.
// Plain host C++ over h2g_dev.h: tests/dev/dev_check.cpp drives it over malloc / free.
#pragma once
#include <stdint.h>
#include "h2g_dev.h"

namespace h2g {

template <typename T>
struct PartArea {
	DevBuf<T> buf;
	size_t cap = 0;                // elements per part
	unsigned parts = 0;
	bool fits(unsigned want_parts, size_t want_cap) const { return parts >= want_parts && cap >= want_cap; }
	// frees the area, then allocates want_parts x want_cap; a failed allocation leaves no area (0 parts of 0), so the next call allocates again
	hipError_t reset(unsigned want_parts, size_t want_cap) {
		cap = 0; parts = 0;
		const hipError_t e = buf.reset(want_parts * want_cap);
		if(e == hipSuccess) { cap = want_cap; parts = want_parts; }
		return e;
	}
	size_t lo(unsigned m) const { return m * cap; }
	size_t hi(unsigned m) const { return (m + 1) * cap; }
	explicit operator bool() const { return bool(buf); }
	operator T*() const { return buf; }
};

// What the cursors say is in use: part m holds [lo, end) with end = cur[m] clamped to the part (a cursor runs past hi(m) when a part is full), and nothing when
// bit m of `touched` is clear or the cursor still stands at lo(m).  Fills span[0 .. parts) and returns the elements the used prefix of the area spans: the end of
// the last part that holds anything, 0 when none does.
struct PartSpan { size_t lo, end; };
inline size_t part_spans(const uint32_t* cur, unsigned touched, unsigned parts, size_t cap, PartSpan* span) {
	size_t n = 0;
	for(unsigned m = 0; m < parts; m++) {
		const size_t lo = m * cap, hi = lo + cap;
		size_t end = (touched >> m) & 1u ? cur[m] : lo;
		if(end > hi) end = hi;
		if(end < lo) end = lo;
		span[m].lo = lo; span[m].end = end;
		if(end > lo) n = end;
	}
	return n;
}

}  // namespace h2g
