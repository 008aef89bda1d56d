// dev_check.cpp — the resource handles of csrc/h2g_dev.h over malloc / free, under the host sanitizers (tests/test_dev_handles_cpu.py).
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

int main() {
	check_verbs();
	check_failures();
	check_moves();
	check_context();
	CHECK(live() == 0 && g_double_free == 0);
	printf("dev_check: %d checks, %d failures\n", g_checks, g_fail);
	return g_fail ? 1 : 0;
}
