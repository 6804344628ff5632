// launch_book.h -- who waits for whom among the launches of a scene, decided without HIP: the book holds no event and no stream (frame_order.h
// owns the events of the stream table and keeps it; Scene keeps the rings beside the events they index).  It is told what is about to be
// issued and answers what has to be waited for first.  tests/launch_book_check.cpp scripts it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

namespace bm {

// ---- frames against uploads.  Frames may be issued on any number of streams (bench.py --pipeline, the multi-stream tests); uploads, edits and
// plane builds run on the load stream and end with the upload event.  Every stream a frame was issued on has an entry: the owner keeps a "done"
// event per entry, recorded behind the stream's most recent frame (the load stream is ordered behind ALL of them before it rewrites what frames
// read), and `upload_seen` is the upload batch the stream has already been ordered behind.  Streams are opaque keys.
class StreamTable {
public:
	static constexpr int kMaxStreams = 16;
	struct Begin {
		int entry = 0;     // the stream's entry, once the retired one has gone: entries stay in the order they were made
		bool made = false; // by this call
		int retired = -1;  // the entry that went to make room (the one idle longest): the caller waits on the host for its "done" -- its last frame must have
		                   // finished before the entry, and with it the ordering of the load stream behind that frame, can go -- and moves its event behind the others
		bool wait = false; // the stream has not been ordered behind the latest batch: it waits for the upload event
		bool ask = false;  // ... it has, as far as the book knows: the caller asks the upload event and reports what it said (upload_asked)
	};
	// a frame is about to be issued on `key`.  An entry that claims to have seen the latest batch is only trusted once that batch has completed
	// (a stream handle can be recycled by the runtime after its owner destroyed it), so the event is asked -- but only for an entry that was not
	// made by this call, and only when there is a batch at all
	Begin begin(const void* key) {
		Begin b;
		b.entry = find(key);
		if (b.entry < 0) {
			b.made = true;
			if (size_ == kMaxStreams) {
				int lru = 0;
				for (int i = 1; i < size_; ++i) if (e_[i].last_use < e_[lru].last_use) lru = i;
				for (int i = lru; i + 1 < size_; ++i) e_[i] = e_[i + 1];
				b.retired = lru;
				size_--;
			}
			b.entry = size_++;
			e_[b.entry] = Entry{key, 0, 0};
		}
		Entry& e = e_[b.entry];
		b.wait = e.upload_seen < upload_seq_;
		b.ask = !b.wait && upload_seq_ > 0 && !b.made;
		if (b.wait) e.upload_seen = upload_seq_; // (the upload event is re-recorded behind every batch: waiting for it covers all earlier ones)
		e.last_use = ++frame_seq_;
		return b;
	}
	// the upload event has been asked for `entry`: whether the stream waits for it after all
	bool upload_asked(int entry, bool ready) {
		if (!ready) e_[entry].upload_seen = upload_seq_;
		return !ready;
	}
	int find(const void* key) const { // the entry of a stream a frame was begun on, -1: none
		for (int i = 0; i < size_; ++i) if (e_[i].key == key) return i;
		return -1;
	}
	int size() const { return size_; }
	// ---- what happens on the load stream
	void published() { upload_seq_++; } // a batch was queued and the upload event recorded behind it: every frame issued later waits for it
	void residency_rebuilt() {          // the device has been waited for and the index grid rewritten: no batch is pending, no stream has anything to see
		upload_seq_ = 0;
		for (int i = 0; i < size_; ++i) e_[i].upload_seen = 0;
	}
	uint64_t batches() const { return upload_seq_; }

private:
	struct Entry {
		const void* key;
		uint64_t upload_seen, last_use;
	};
	Entry e_[kMaxStreams] = {};
	int size_ = 0;
	uint64_t upload_seq_ = 0, frame_seq_ = 0; // upload batches queued on the load stream / frames issued
};

// ---- a ring of kSlots clocks (an event, or a pair), one per launch in turn: launch n takes slot n % kSlots and first waits for launch
// n - kSlots, which used it last.  The ray queries' ticket ring is one of 64; the frames' timing ring one of 256.
template <int kSlots>
class ClockRing {
public:
	long long launches() const { return n_; }
	int slot() const { return static_cast<int>(n_ % kSlots); } // of the launch about to be issued
	bool reused() const { return n_ >= kSlots; }               // ... which waits for the slot's previous user
	void issued() { n_++; }
	int last_slot() const { return static_cast<int>((n_ - 1) % kSlots); } // of the last launch issued (launches() > 0)
	// the most recent launches whose clocks still stand, at most `capacity` of them: how many, and the slot of the k-th, oldest first
	int recent(long long capacity) const {
		return static_cast<int>(std::max(0ll, std::min({n_, static_cast<long long>(kSlots), capacity})));
	}
	int recent_slot(int count, int k) const { return static_cast<int>((n_ - count + k) % kSlots); }

private:
	long long n_ = 0;
};

// ---- the frame ring: kEntries entries (constants + ticket counters of a frame in flight) of which a launch takes `count` consecutive ones,
// and the launches' clocks.  An entry is free once the launch that used it last has finished: launches older than the clock ring have been
// waited for when their clock was recycled, in their turn; a younger one is waited for by the launch that takes the entry -- a caller that
// queues thousands of frames without a synchronisation would otherwise overwrite constants whose copy has not run yet.
template <int kEntries, int kSlots, int kMaxCount>
class FrameRing {
public:
	FrameRing() { for (long long& o : owner_) o = -1; }
	struct Launch {
		bool ok = false;             // count is 1 ... kMaxCount
		int first = 0, count = 0;    // the entries first ... first + count - 1
		int slot = 0;                // the clock slot
		int waits = 0;               // the launches to wait for on the host, in this order, and their clock slots
		long long wait_launch[kMaxCount + 1];
		int wait_slot[kMaxCount + 1];
	};
	Launch plan(int count) const {
		Launch l;
		if (count < 1 || count > kMaxCount) return l;
		l.ok = true;
		l.count = count;
		l.first = next_ + count > kEntries ? 0 : next_; // a run does not wrap: the tail entries it skips keep their owners
		l.slot = clock_.slot();
		const long long now = clock_.launches();
		auto wait_for = [&l](long long launch) {
			l.wait_launch[l.waits] = launch;
			l.wait_slot[l.waits++] = static_cast<int>(launch % kSlots);
		};
		if (clock_.reused()) wait_for(now - kSlots); // (almost always done)
		long long waited = -1;
		for (int e = l.first; e < l.first + count; ++e) {
			const long long owner = owner_[e];
			if (owner >= 0 && owner != waited && now - owner < kSlots) {
				wait_for(owner);
				waited = owner;
			}
		}
		return l;
	}
	// the launch was issued (one that could not be is not reported: the ring stays as it was)
	void issued(const Launch& l) {
		if (!l.ok) return;
		for (int e = l.first; e < l.first + l.count; ++e) owner_[e] = clock_.launches();
		next_ = l.first + l.count;
		clock_.issued();
	}
	const ClockRing<kSlots>& clock() const { return clock_; }
	long long owner(int entry) const { return owner_[entry]; } // the launch that used the entry last, -1: none
	int next() const { return next_; }

private:
	long long owner_[kEntries];
	int next_ = 0;
	ClockRing<kSlots> clock_;
};

} // namespace bm
