// frame_order.h -- the one owner of the ordering between what reads a scene's world (frames, and the queries issued like frames, on any
// stream) and what rewrites it on the load stream (brick uploads, edits, region writes, plane builds).  A wrong decision here lets an
// upload rewrite index words, pool bases or bricks under a frame in flight, so the decisions are taken by a book without HIP
// (launch_book.h StreamTable, scripted on the CPU by tests/launch_book_check.cpp) and this class only holds the events and makes the calls:
//   - a frame on `stream` must see every batch queued so far: begin() lets the stream wait for the upload event unless it already has
//     (per stream, not per scene), end() records the stream's "done" event behind the frame;
//   - work that rewrites what frames read is queued on the load stream behind every "done" event (load_behind_frames) and published as an
//     upload batch (published): every frame begun later waits for it;
//   - the pinned staging of a brick upload belongs to it until the upload event has passed (wait_upload_on_host).
// Scene holds it as one member and forwards begin_frame / end_frame to it.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "error.h"
#include "hip_owned.h"
#include "launch_book.h"

namespace bm {

class FrameOrder {
public:
	int init(hipStream_t load_stream) {
		load_stream_ = load_stream;
		if (int e = ev_upload_.create(hipEventDisableTiming)) return e;
		return ev_caller_.create(hipEventDisableTiming);
	}
	// ---- frames
	int begin(hipStream_t stream) {
		const StreamTable::Begin b = table_.begin(stream);
		if (b.retired >= 0) {
			BM_HIP(hipEventSynchronize(done_[b.retired]));
			for (int i = b.retired; i < b.entry; ++i) std::swap(done_[i], done_[i + 1]); // (the event serves the new entry)
		}
		if (b.made) { if (int e = done_[b.entry].create(hipEventDisableTiming)) return e; }
		bool wait = b.wait;
		if (b.ask) {
			// (only the query's own "not ready" status is cleared -- never a sticky error of the caller's that happens to be pending on this thread)
			const bool ready = hipEventQuery(ev_upload_) != hipErrorNotReady;
			if (!ready) (void)hipGetLastError();
			wait = table_.upload_asked(b.entry, ready);
		}
		if (wait) BM_HIP(hipStreamWaitEvent(stream, ev_upload_, 0));
		return 0;
	}
	int end(hipStream_t stream) {
		const int entry = table_.find(stream);
		if (entry < 0) { set_error("frame_end without frame_begin"); return BM_ESTATE; }
		BM_HIP(hipEventRecord(done_[entry], stream));
		return 0;
	}
	// a frame that has begun is ended on every return path: end() where the path that fails nowhere ends it, else when the guard goes
	class Ending {
	public:
		Ending(FrameOrder& order, hipStream_t stream) : order_(order), stream_(stream) {}
		Ending(const Ending&) = delete;
		Ending& operator=(const Ending&) = delete;
		~Ending() { if (open_) (void)order_.end(stream_); }
		int end() { open_ = false; return order_.end(stream_); }

	private:
		FrameOrder& order_;
		hipStream_t stream_;
		bool open_ = true;
	};
	int wait_frames_on_host() {
		for (int i = 0; i < table_.size(); ++i) BM_HIP(hipEventSynchronize(done_[i]));
		return 0;
	}
	// ---- the load stream
	int load_behind_frames() {
		for (int i = 0; i < table_.size(); ++i) BM_HIP(hipStreamWaitEvent(load_stream_, done_[i], 0));
		return 0;
	}
	int load_behind_caller(hipStream_t stream) { // what the load stream is about to read is whatever the caller's stream has written by now
		BM_HIP(hipEventRecord(ev_caller_, stream));
		BM_HIP(hipStreamWaitEvent(load_stream_, ev_caller_, 0));
		return 0;
	}
	// what has been queued on the load stream is an upload batch from here on; staging: its pinned staging is free again once it has run
	int published(bool staging = false) {
		BM_HIP(hipEventRecord(ev_upload_, load_stream_));
		table_.published();
		staging_busy_ = staging_busy_ || staging;
		return 0;
	}
	// work that rewrites what frames read: queue() issues it on the load stream behind every frame in flight, and it is published
	template <class Queue> int publish_behind_frames(Queue&& queue) {
		if (int e = load_behind_frames()) return e;
		if (int e = queue()) return e;
		return published();
	}
	int wait_upload_on_host() {
		if (staging_busy_) {
			BM_HIP(hipEventSynchronize(ev_upload_));
			staging_busy_ = false;
		}
		return 0;
	}
	void residency_rebuilt() { // (the device has been waited for)
		staging_busy_ = false;
		table_.residency_rebuilt();
	}

private:
	hipStream_t load_stream_ = nullptr;
	StreamTable table_;
	Event done_[StreamTable::kMaxStreams];
	Event ev_upload_, ev_caller_;
	bool staging_busy_ = false; // the pinned staging buffers belong to an upload that may still be copying
};

} // namespace bm
