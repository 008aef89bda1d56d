// h2g_dev.h — the owners of what the HIP runtime hands out: device memory, page-locked host memory, events, streams.
//
// One rule: whoever holds the handle owns the resource, and the handle's destructor gives it back.  All four are move-only, none throws, and every
// operation that can fail returns hipError_t (HIPCHK(buf.reserve(n)) at the call site).  A handle converts to its raw HIP type, so launches, copies and
// event calls read as they do with bare pointers; a pointer that does NOT own what it points to stays a raw pointer and says so where it is declared.
// Nothing here zeroes memory: which stream first writes a fresh buffer is the caller's choice (a visible hipMemset[Async]).
// Plain host C++ over <hip/hip_runtime_api.h>: tests/dev/dev_check.cpp drives it over malloc / free.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace h2g {

// Device memory as T* and its capacity in elements (DevBuf<uint8_t>: bytes).  Three verbs:
//   ensure(n)   nothing there yet: allocate n.  Otherwise nothing (first use).
//   reserve(n)  fewer than n: free, THEN allocate n (growth; old and new are never held together).  Otherwise nothing.
//   reset(n)    free, then allocate n (whatever was there).
// A failed allocation leaves the buffer empty with capacity 0, so the next call allocates again.
template <typename T>
class DevBuf {
	T* p_ = nullptr;
	size_t n_ = 0;
	void drop() { if(p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
public:
	DevBuf() = default;
	DevBuf(T* p, size_t n) : p_(p), n_(n) {}      // adopts memory the caller allocated (hipMalloc or hipExtMallocWithFlags)
	DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
	DevBuf& operator=(DevBuf&& o) noexcept { if(this != &o) { drop(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { drop(); }
	hipError_t ensure(size_t n) { return p_ ? hipSuccess : reset(n); }
	hipError_t reserve(size_t n) { return n_ >= n ? hipSuccess : reset(n); }
	hipError_t reset(size_t n) {
		drop();
		const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
		if(e != hipSuccess) p_ = nullptr; else n_ = n;
		return e;
	}
	T* release() { T* p = p_; p_ = nullptr; n_ = 0; return p; }      // the memory is the caller's from here on
	T* get() const { return p_; }
	size_t size() const { return n_; }
	size_t bytes() const { return n_ * sizeof(T); }
	explicit operator bool() const { return p_ != nullptr; }
	operator T*() const { return p_; }
};

// Page-locked host memory, allocated once
template <typename T>
class PinnedBuf {
	T* p_ = nullptr;
	size_t n_ = 0;
	void drop() { if(p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
public:
	PinnedBuf() = default;
	PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
	PinnedBuf& operator=(PinnedBuf&& o) noexcept { if(this != &o) { drop(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	~PinnedBuf() { drop(); }
	hipError_t ensure(size_t n) {
		if(p_) return hipSuccess;
		const hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault);
		if(e != hipSuccess) p_ = nullptr; else n_ = n;
		return e;
	}
	T* get() const { return p_; }
	size_t size() const { return n_; }
	size_t bytes() const { return n_ * sizeof(T); }
	explicit operator bool() const { return p_ != nullptr; }
	operator T*() const { return p_; }
};

// An event.  Created by an explicit call, never by a constructor: when an event comes to exist is the caller's business (some are created lazily)
class DevEvent {
	hipEvent_t e_ = nullptr;
	void drop() { if(e_) (void)hipEventDestroy(e_); e_ = nullptr; }
public:
	DevEvent() = default;
	DevEvent(DevEvent&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
	DevEvent& operator=(DevEvent&& o) noexcept { if(this != &o) { drop(); e_ = o.e_; o.e_ = nullptr; } return *this; }
	DevEvent(const DevEvent&) = delete;
	DevEvent& operator=(const DevEvent&) = delete;
	~DevEvent() { drop(); }
	hipError_t create(unsigned flags = hipEventDefault) {
		drop();
		const hipError_t e = hipEventCreateWithFlags(&e_, flags);
		if(e != hipSuccess) e_ = nullptr;
		return e;
	}
	hipEvent_t get() const { return e_; }
	explicit operator bool() const { return e_ != nullptr; }
	operator hipEvent_t() const { return e_; }
};

// A stream.  Created by an explicit call: the ORDER in which a process creates its streams decides their hardware queues (h2g_stream_create).
// The destructor does not wait: a struct that owns streams declares them first, so that they go last, and waits for them in its own destructor.
class DevStream {
	hipStream_t s_ = nullptr;
	void drop() { if(s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
public:
	DevStream() = default;
	DevStream(DevStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
	DevStream& operator=(DevStream&& o) noexcept { if(this != &o) { drop(); s_ = o.s_; o.s_ = nullptr; } return *this; }
	DevStream(const DevStream&) = delete;
	DevStream& operator=(const DevStream&) = delete;
	~DevStream() { drop(); }
	hipError_t create(unsigned flags) {
		drop();
		const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
		if(e != hipSuccess) s_ = nullptr;
		return e;
	}
	hipError_t create_with_priority(unsigned flags, int priority) {
		drop();
		const hipError_t e = hipStreamCreateWithPriority(&s_, flags, priority);
		if(e != hipSuccess) s_ = nullptr;
		return e;
	}
	hipStream_t get() const { return s_; }
	explicit operator bool() const { return s_ != nullptr; }
	operator hipStream_t() const { return s_; }
};

}  // namespace h2g
