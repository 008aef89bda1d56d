// dev_check.cpp — the resource handles of csrc/h2g_dev.h and the partitioned areas of csrc/h2g_parts.h over malloc / free, under the host sanitizers
// (tests/test_dev_handles_cpu.py).
// The eight entry points the handles call are defined HERE: they keep a log of calls and a count of live objects, and fail the k-th creation on request.
// No HIP runtime is linked and no GPU is needed.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <set>
#include <string>
#include <utility>
#include <vector>
#include "../../hisat2_amd/csrc/h2g_dev.h"
#include "../../hisat2_amd/csrc/h2g_parts.h"

using namespace h2g;

// ------------------------------------------------------------------------------------------ the runtime underneath
enum Kind { MEM = 0, PIN, EVT, STR };
struct Call { bool create; Kind kind; void* p; size_t bytes; };
static std::vector<Call> g_log;
static std::set<void*> g_live[4];
static long g_creations = 0, g_fail_at = -1;      // the g_fail_at-th creation from now fails (0 = the next one); -1: none
static int g_double_free = 0;

static hipError_t make(Kind k, void** out, size_t bytes) {
	if(g_fail_at >= 0 && g_creations++ == g_fail_at) { *out = (void*)0x1;      // (a handle must not keep what a failed call left in its pointer)
		return k == MEM || k == PIN ? hipErrorOutOfMemory : hipErrorInvalidValue; }
	void* p = malloc(bytes ? bytes : 1);
	g_live[k].insert(p);
	g_log.push_back({true, k, p, bytes});
	*out = p;
	return hipSuccess;
}
static hipError_t unmake(Kind k, void* p) {
	if(!p) return hipSuccess;
	if(!g_live[k].erase(p)) { g_double_free++; return hipErrorInvalidValue; }
	g_log.push_back({false, k, p, 0});
	free(p);
	return hipSuccess;
}
static size_t live() { return g_live[0].size() + g_live[1].size() + g_live[2].size() + g_live[3].size(); }
static void fail_creation(long k) { g_creations = 0; g_fail_at = k; }

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return make(MEM, p, n); }
hipError_t hipFree(void* p) { return unmake(MEM, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return make(PIN, p, n); }
hipError_t hipHostFree(void* p) { return unmake(PIN, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return make(EVT, (void**)e, 8); }
hipError_t hipEventDestroy(hipEvent_t e) { return unmake(EVT, (void*)e); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return make(STR, (void**)s, 8); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { return make(STR, (void**)s, 8); }
hipError_t hipStreamDestroy(hipStream_t s) { return unmake(STR, (void*)s); }
}

// ------------------------------------------------------------------------------------------ the checks
static int g_checks = 0, g_fail = 0;
#define CHECK(cond) do { g_checks++; if(!(cond)) { g_fail++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while(0)

static void check_verbs() {
	g_log.clear();
	{
		DevBuf<uint32_t> b;
		CHECK(!b && b.get() == nullptr && b.size() == 0 && b.bytes() == 0);
		// ensure: once
		CHECK(b.ensure(10) == hipSuccess && b && b.size() == 10 && b.bytes() == 40 && g_log.size() == 1 && g_log[0].bytes == 40);
		uint32_t* const first = b;
		CHECK(b.ensure(1000) == hipSuccess && b.get() == first && b.size() == 10 && g_log.size() == 1);
		b[9] = 7;      // (the last element is inside the allocation: ASan)
		// reserve: at or below the capacity, no call; above, the free comes before the allocation
		CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(0) == hipSuccess && g_log.size() == 1 && b.get() == first);
		CHECK(b.reserve(11) == hipSuccess && b.size() == 11 && g_log.size() == 3);
		CHECK(!g_log[1].create && g_log[1].p == first && g_log[2].create && g_log[2].bytes == 44);
		// reset: always both, smaller or larger
		CHECK(b.reset(4) == hipSuccess && b.size() == 4 && g_log.size() == 5 && !g_log[3].create && g_log[4].create && g_log[4].bytes == 16);
		CHECK(b.reset(4) == hipSuccess && g_log.size() == 7 && !g_log[5].create && g_log[6].create);
		CHECK(live() == 1);
	}
	CHECK(live() == 0 && g_log.size() == 8 && !g_log[7].create);
	{	// reserve(0) and the empty buffer: nothing is called
		g_log.clear();
		DevBuf<uint8_t> e;
		CHECK(e.reserve(0) == hipSuccess && !e && g_log.empty());
	}
	{	// the page-locked twin
		g_log.clear();
		PinnedBuf<uint64_t> h;
		CHECK(!h && h.ensure(3) == hipSuccess && h && h.size() == 3 && h.bytes() == 24 && g_log.size() == 1 && g_log[0].kind == PIN && g_log[0].bytes == 24);
		uint64_t* const first = h;
		h[2] = 1;
		CHECK(h.ensure(9) == hipSuccess && h.get() == first && g_log.size() == 1);
		PinnedBuf<uint64_t> h2(std::move(h));
		CHECK(!h && h.size() == 0 && h2.get() == first && h2.size() == 3);
	}
	CHECK(live() == 0);
}

static void check_failures() {
	{	// a failed reserve / reset: empty, capacity 0, and the next call allocates
		DevBuf<uint16_t> b;
		CHECK(b.ensure(8) == hipSuccess);
		fail_creation(0);
		CHECK(b.reserve(9) == hipErrorOutOfMemory && !b && b.get() == nullptr && b.size() == 0 && live() == 0);
		g_log.clear();
		CHECK(b.reserve(2) == hipSuccess && b && b.size() == 2 && g_log.size() == 1 && g_log[0].create);      // (smaller than what it once held: still allocated)
		fail_creation(0);
		CHECK(b.reset(2) == hipErrorOutOfMemory && !b && b.size() == 0 && live() == 0);
		CHECK(b.reset(2) == hipSuccess && b.size() == 2);
		fail_creation(0);
		DevBuf<uint16_t> c;
		CHECK(c.ensure(5) == hipErrorOutOfMemory && !c && c.size() == 0);
		CHECK(c.ensure(5) == hipSuccess && c.size() == 5);
	}
	{
		PinnedBuf<char> h; DevEvent e; DevStream s, sp;
		fail_creation(0); CHECK(h.ensure(4) != hipSuccess && !h && h.size() == 0);
		fail_creation(0); CHECK(e.create(0) != hipSuccess && !e && e.get() == nullptr);
		fail_creation(0); CHECK(s.create(0) != hipSuccess && !s && s.get() == nullptr);
		fail_creation(0); CHECK(sp.create_with_priority(0, -1) != hipSuccess && !sp);
		CHECK(h.ensure(4) == hipSuccess && e.create(0) == hipSuccess && s.create(0) == hipSuccess && sp.create_with_priority(0, -1) == hipSuccess && live() == 4);
		CHECK(h && e && s && sp && (hipEvent_t)e == e.get() && (hipStream_t)s == s.get());
	}
	g_fail_at = -1;
	CHECK(live() == 0 && g_double_free == 0);
}

template <class H> static void self_move(H& h) { H& same = h; h = std::move(same); }
static void check_moves() {
	{
		DevBuf<int> a;
		CHECK(a.reset(6) == hipSuccess);
		int* const pa = a;
		DevBuf<int> b(std::move(a));                       // move-construction
		CHECK(!a && a.size() == 0 && b.get() == pa && b.size() == 6 && live() == 1);
		DevBuf<int> c;
		CHECK(c.reset(2) == hipSuccess && live() == 2);
		c = std::move(b);                                  // move-assignment: what c held is freed, once
		CHECK(!b && b.size() == 0 && c.get() == pa && c.size() == 6 && live() == 1);
		self_move(c);
		CHECK(c.get() == pa && c.size() == 6 && live() == 1);
		c = DevBuf<int>();                                 // (how a buffer is dropped in place)
		CHECK(!c && live() == 0);
		std::vector<DevBuf<uint8_t>> v;                    // (the index keeps its arrays like this: growth moves them)
		for(int i = 0; i < 20; i++) { DevBuf<uint8_t> x; CHECK(x.reset(16 + i) == hipSuccess); v.push_back(std::move(x)); }
		CHECK(live() == 20);
	}
	CHECK(live() == 0 && g_double_free == 0);
	{	// release: the pointer is the caller's, the destructor frees nothing; adoption is its inverse
		int* p = nullptr;
		{
			DevBuf<int> a;
			CHECK(a.reset(3) == hipSuccess);
			p = a.release();
			CHECK(p != nullptr && !a && a.size() == 0);
		}
		CHECK(live() == 1);
		{ DevBuf<int> back(p, 3); CHECK(back.get() == p && back.size() == 3); }
		CHECK(live() == 0);
	}
	{
		DevEvent e, e2; DevStream s, s2;
		CHECK(e.create(0) == hipSuccess && s.create(0) == hipSuccess);
		const hipEvent_t he = e; const hipStream_t hs = s;
		e2 = std::move(e); s2 = std::move(s);
		CHECK(!e && !s && e2.get() == he && s2.get() == hs && live() == 2);
		self_move(e2); self_move(s2);
		CHECK(e2.get() == he && s2.get() == hs && live() == 2);
		DevEvent e3(std::move(e2)); DevStream s3(std::move(s2));
		CHECK(!e2 && !s2 && e3.get() == he && s3.get() == hs && live() == 2);
		CHECK(e3.create(0) == hipSuccess && live() == 2);   // created again: the former event goes first
	}
	CHECK(live() == 0 && g_double_free == 0);
}

// A context shaped like the library's (h2g_stream): streams declared first, then events, then buffers; built by early-return steps
struct Ctx {
	DevStream st, mst[3], dst;
	DevEvent ev[4];
	PinnedBuf<uint32_t> h_args;
	DevBuf<uint64_t> counters;
	struct Batch { DevBuf<uint8_t> codes; DevBuf<uint32_t> offs; DevBuf<char> names; } batch[2];
	DevBuf<uint8_t> tmp[2];
	DevEvent ev_lazy;
};
#define TRY(call) do { if((call) != hipSuccess) return false; } while(0)
static bool build(Ctx& c) {
	TRY(c.st.create(0));
	for(DevStream& m : c.mst) TRY(m.create(0));
	TRY(c.dst.create_with_priority(0, 0));
	TRY(c.h_args.ensure(18));
	for(DevEvent& e : c.ev) TRY(e.create(0));
	TRY(c.counters.ensure(64));
	for(Ctx::Batch& b : c.batch) { TRY(b.codes.ensure(100)); TRY(b.offs.ensure(11)); TRY(b.names.reserve(50)); TRY(b.names.reserve(80)); }
	for(DevBuf<uint8_t>& t : c.tmp) TRY(t.reset(256));
	TRY(c.ev_lazy.create(0));
	return true;
}
static void check_context() {
	long total = -1;
	for(long k = 0; total < 0 || k <= total; k++) {
		g_log.clear();
		fail_creation(k);
		bool ok;
		{
			Ctx c;
			ok = build(c);
			if(ok) total = g_creations;      // (no creation failed: k is the number of creations)
		}
		CHECK(live() == 0);
		CHECK(ok == (total >= 0 && k >= total));
		// every stream goes after every buffer and event
		size_t first_stream_destroyed = g_log.size(), last_other_destroyed = 0;
		for(size_t i = 0; i < g_log.size(); i++) if(!g_log[i].create) {
			if(g_log[i].kind == STR) { if(i < first_stream_destroyed) first_stream_destroyed = i; }
			else last_other_destroyed = i;
		}
		CHECK(first_stream_destroyed > last_other_destroyed || last_other_destroyed == 0);
	}
	g_fail_at = -1;
	CHECK(total == 5 + 1 + 4 + 1 + 2 * 4 + 2 + 1);      // (names: 50, then 80 — two creations per batch)
	CHECK(g_double_free == 0);
}

// The partitioned areas (h2g_parts.h).  Every expected number below is written out from m * cap by hand
static void check_parts() {
	{
		PartArea<uint32_t> a;
		CHECK(!a && a.cap == 0 && a.parts == 0 && !a.fits(1, 1) && a.fits(0, 0));
		g_log.clear();
		CHECK(a.reset(8, 1000) == hipSuccess && a && a.parts == 8 && a.cap == 1000 && a.buf.size() == 8000 && g_log.size() == 1 && g_log[0].bytes == 32000);
		CHECK(a.lo(0) == 0 && a.hi(0) == 1000);
		CHECK(a.lo(1) == 1000 && a.hi(1) == 2000);
		CHECK(a.lo(7) == 7000 && a.hi(7) == 8000);
		uint32_t* const p = a;
		p[7999] = 1;      // (the last element of the last part is inside the allocation: ASan)
		// fits: both numbers have to be there
		CHECK(a.fits(8, 1000) && a.fits(2, 1000) && a.fits(8, 1) && a.fits(1, 999));
		CHECK(!a.fits(9, 1000) && !a.fits(8, 1001) && !a.fits(9, 1) && !a.fits(1, 1001));
		// a failed allocation: no area, and the next reset allocates
		fail_creation(0);
		CHECK(a.reset(8, 2000) == hipErrorOutOfMemory && !a && a.parts == 0 && a.cap == 0 && !a.fits(1, 1) && live() == 0);
		g_fail_at = -1;
		CHECK(a.reset(2, 2000) == hipSuccess && a && a.parts == 2 && a.cap == 2000 && a.lo(1) == 2000 && a.hi(1) == 4000 && live() == 1);
		// a reset to something smaller is still a new area (the free comes first)
		g_log.clear();
		CHECK(a.reset(1, 10) == hipSuccess && a.parts == 1 && a.cap == 10 && g_log.size() == 2 && !g_log[0].create && g_log[1].create && g_log[1].bytes == 40);
	}
	CHECK(live() == 0 && g_double_free == 0);
	// the spans the cursors describe: 8 parts of 1000
	PartSpan sp[8];
	const auto empty = [&sp](unsigned m, size_t lo) { return sp[m].lo == lo && sp[m].end == lo; };
	{	// nothing touched: whatever the cursors hold (leftovers of an earlier batch), every part is empty
		const uint32_t cur[8] = {500, 1500, 2000, 3999, 4000, 5001, 6000, 7999};
		CHECK(part_spans(cur, 0u, 8, 1000, sp) == 0);
		CHECK(empty(0, 0) && empty(1, 1000) && empty(2, 2000) && empty(3, 3000) && empty(4, 4000) && empty(5, 5000) && empty(6, 6000) && empty(7, 7000));
	}
	{	// one touched part whose cursor still stands at its start: empty
		const uint32_t cur[8] = {0, 1000, 2000, 3000, 4000, 5000, 6000, 7000};
		CHECK(part_spans(cur, 1u << 3, 8, 1000, sp) == 0);
		CHECK(empty(3, 3000) && empty(0, 0) && empty(7, 7000));
	}
	{	// a touched part in the middle; an untouched one with a moved cursor beside it stays empty
		const uint32_t cur[8] = {0, 1000, 2345, 3100, 4000, 5000, 6000, 7000};
		CHECK(part_spans(cur, 1u << 2, 8, 1000, sp) == 2345);
		CHECK(sp[2].lo == 2000 && sp[2].end == 2345 && empty(3, 3000) && empty(1, 1000) && empty(0, 0));
	}
	{	// a cursor beyond its part (the part is full): clamped to the part's end; one below its part (never written by a run): empty
		const uint32_t cur[8] = {0, 2600, 2000, 3000, 4000, 77, 6000, 7000};
		CHECK(part_spans(cur, (1u << 1) | (1u << 5), 8, 1000, sp) == 2000);
		CHECK(sp[1].lo == 1000 && sp[1].end == 2000 && empty(5, 5000) && empty(2, 2000));
	}
	{	// the last part touched, and the first: the span reaches into the last
		const uint32_t cur[8] = {12, 1000, 2000, 3000, 4000, 5000, 6000, 7001};
		CHECK(part_spans(cur, (1u << 0) | (1u << 7), 8, 1000, sp) == 7001);
		CHECK(sp[0].lo == 0 && sp[0].end == 12 && sp[7].lo == 7000 && sp[7].end == 7001 && empty(4, 4000));
	}
	{	// fewer parts than cursors: the ones beyond `parts` are nobody's
		const uint32_t cur[8] = {1, 1001, 2002, 3003, 0, 0, 0, 0};
		sp[2].lo = sp[2].end = 99;
		CHECK(part_spans(cur, 0xffu, 2, 1000, sp) == 1001);
		CHECK(sp[0].end == 1 && sp[1].lo == 1000 && sp[1].end == 1001 && sp[2].lo == 99 && sp[2].end == 99);
	}
}

int main() {
	check_parts();
	printf("dev_check: the areas in parts, %d checks\n", g_checks);
	check_verbs();
	check_failures();
	check_moves();
	check_context();
	CHECK(live() == 0 && g_double_free == 0);
	printf("dev_check: %d checks, %d failures\n", g_checks, g_fail);
	return g_fail ? 1 : 0;
}
