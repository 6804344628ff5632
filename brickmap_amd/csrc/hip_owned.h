// hip_owned.h -- move-only owners of HIP resources: device memory, pinned host memory, an event, a turn, the events around a launch's stages, a stream.  Each frees what it holds
// in its destructor (on whatever device is current: the owner's destructor body selects it) and allocates through a method that
// returns the project's int error.  A default-constructed owner holds nothing, so an object whose init() failed halfway destructs cleanly.
// None of them synchronises: a buffer that work in flight may still use is waited for by the caller before reserve() / alloc().
#pragma once
#include <cstddef>
#include <utility>

#include "error.h"

namespace bm {

// what DeviceBuffer and PinnedBuffer share; use those two
template <typename T>
class HipBuffer {
public:
	HipBuffer(HipBuffer&& o) noexcept : pinned_(o.pinned_) { swap(o); }
	HipBuffer& operator=(HipBuffer&& o) noexcept { swap(o); return *this; } // (what this held goes with `o`)
	~HipBuffer() { (void)release(); }
	int release() {
		T* const p = p_;
		p_ = nullptr;
		bytes_ = 0;
		if (p) BM_HIP(pinned_ ? hipHostFree(p) : hipFree(p));
		return 0;
	}
	int alloc(size_t bytes) { // contents undefined; whatever was held is freed first
		if (int e = release()) return e;
		void** const at = reinterpret_cast<void**>(&p_);
		BM_HIP(pinned_ ? hipHostMalloc(at, bytes, hipHostMallocDefault) : hipMalloc(at, bytes));
		bytes_ = bytes;
		return 0;
	}
	int reserve(size_t bytes) { return bytes <= bytes_ ? 0 : alloc(bytes); } // grows without keeping the contents
	T* get() const { return p_; }
	operator T*() const { return p_; }
	size_t bytes() const { return bytes_; }

protected:
	explicit HipBuffer(bool pinned) : pinned_(pinned) {}

private:
	void swap(HipBuffer& o) { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); }
	const bool pinned_;
	T* p_ = nullptr;
	size_t bytes_ = 0;
};
template <typename T>
struct DeviceBuffer : HipBuffer<T> {
	DeviceBuffer() : HipBuffer<T>(false) {}
};
template <typename T>
struct PinnedBuffer : HipBuffer<T> {
	PinnedBuffer() : HipBuffer<T>(true) {}
};

class Event {
public:
	Event() = default;
	Event(Event&& o) noexcept { std::swap(e_, o.e_); }
	Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
	~Event() { if (e_) (void)hipEventDestroy(e_); }
	int create(unsigned flags = hipEventDefault) { // no-op when the event exists already (events made on first use)
		if (!e_) BM_HIP(hipEventCreateWithFlags(&e_, flags));
		return 0;
	}
	operator hipEvent_t() const { return e_; }

private:
	hipEvent_t e_ = nullptr;
};

// Whose turn it is with something one call at a time may use (a scratch buffer, a staging area): the call that uses it passes the turn on its
// stream behind its work, and the next one orders its stream behind that -- or, before it rewrites or grows the thing from the host, waits.
class Turn {
public:
	bool pending() const { return pending_; }
	int order(hipStream_t stream) const { // `stream` goes on once the call before has finished
		if (pending_) BM_HIP(hipStreamWaitEvent(stream, ev_, 0));
		return 0;
	}
	int wait() { // the host does
		if (pending_) BM_HIP(hipEventSynchronize(ev_));
		pending_ = false;
		return 0;
	}
	int pass(hipStream_t stream) { // behind what this call has queued on `stream`
		if (int e = ev_.create(hipEventDisableTiming)) return e;
		BM_HIP(hipEventRecord(ev_, stream));
		pending_ = true;
		return 0;
	}
	void clear() { pending_ = false; } // the device has just been waited for

private:
	Event ev_; // made on first use
	bool pending_ = false;
};

// N timing events around the stages of one launch: what the launch_* functions of kernels.h take as `marks` -- mark i is recorded before
// stage i, mark `stages` behind the last one
template <int N>
class StageMarks {
public:
	int create(int count = N) { // the first `count` events, made on first use
		for (int i = 0; i < count; ++i) {
			if (int e = ev_[i].create(hipEventDefault)) return e;
			raw_[i] = ev_[i];
		}
		return 0;
	}
	hipEvent_t* marks() { return raw_; }
	// waits for mark first + stages, then ms[i] = the time from mark first + i to the mark after it
	int read(int stages, float* ms, int first = 0) const {
		BM_HIP(hipEventSynchronize(raw_[first + stages]));
		for (int i = 0; i < stages; ++i) BM_HIP(hipEventElapsedTime(&ms[i], raw_[first + i], raw_[first + i + 1]));
		return 0;
	}

private:
	Event ev_[N];
	hipEvent_t raw_[N] = {};
};

// a launch of `stages` (< N) stages, as launch(marks) issues it.  kernel_ms null: launched without marks.  Otherwise the call waits for
// the launch and kernel_ms[0 ... stages) are the stages' durations
template <int N, class Launch>
int launch_staged(int stages, float* kernel_ms, Launch&& launch) {
	if (!kernel_ms) {
		launch(nullptr);
		BM_HIP(hipGetLastError());
		return 0;
	}
	StageMarks<N> marks;
	if (int e = marks.create(stages + 1)) return e;
	launch(marks.marks());
	BM_HIP(hipGetLastError());
	return marks.read(stages, kernel_ms);
}

class Stream {
public:
	Stream() = default;
	Stream(const Stream&) = delete;
	Stream& operator=(const Stream&) = delete;
	~Stream() { if (s_) (void)hipStreamDestroy(s_); }
	int create(unsigned flags) {
		BM_HIP(hipStreamCreateWithFlags(&s_, flags));
		return 0;
	}
	operator hipStream_t() const { return s_; }

private:
	hipStream_t s_ = nullptr;
};

} // namespace bm
