// launch_book_check.cpp -- a program with its own main around csrc/launch_book.h alone (no HIP, no scene), built plain and with
// -fsanitize=address,undefined by tests/test_launch_book.py.  It scripts frames, upload batches and residency resets on the stream table, and
// launches on the frame ring and the clock rings, and after every step compares the book's answer -- who waits for whom -- with values
// written out here by hand from the rules of launch_book.h.  prints "steps N" and "failures N".
#include <cstdint>
#include <cstdio>

#include "../brickmap_amd/csrc/launch_book.h"

namespace {

using bm::ClockRing;
using bm::StreamTable;
using Ring = bm::FrameRing<1024, 256, 256>; // what a scene holds: 1024 entries, 256 clocks, at most 256 frames per launch

long failures = 0, steps = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		++steps;                                                                     \
		if (!(cond)) {                                                               \
			if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

// streams are opaque keys: the addresses of these
char keys[32];
const void* key(int i) { return &keys[i]; }

bool is(const StreamTable::Begin& b, int entry, bool made, int retired, bool wait, bool ask) {
	return b.entry == entry && b.made == made && b.retired == retired && b.wait == wait && b.ask == ask;
}

// (a) one stream: nothing to wait for or to ask before the first batch; behind a batch it waits, once; afterwards the event is asked
void one_stream() {
	StreamTable t;
	CHECK(is(t.begin(key(0)), 0, true, -1, false, false));
	CHECK(is(t.begin(key(0)), 0, false, -1, false, false)); // no batch yet: nothing to ask either
	t.published();
	CHECK(t.batches() == 1);
	CHECK(is(t.begin(key(0)), 0, false, -1, true, false));
	StreamTable::Begin b = t.begin(key(0));
	CHECK(is(b, 0, false, -1, false, true));
	CHECK(t.upload_asked(b.entry, false)); // not ready: the stream waits after all
	b = t.begin(key(0));
	CHECK(is(b, 0, false, -1, false, true)); // ... and is asked again the next time
	CHECK(!t.upload_asked(b.entry, true));   // ready: nothing
	t.published();
	t.published();
	CHECK(is(t.begin(key(0)), 0, false, -1, true, false)); // two batches: one wait covers both
	CHECK(is(t.begin(key(0)), 0, false, -1, false, true));
	CHECK(t.size() == 1 && t.find(key(0)) == 0 && t.find(key(1)) == -1);
}

// (b) an entry made after batches exist waits, and is not asked
void late_stream() {
	StreamTable t;
	CHECK(is(t.begin(key(0)), 0, true, -1, false, false));
	t.published();
	t.published();
	CHECK(is(t.begin(key(1)), 1, true, -1, true, false));
	CHECK(is(t.begin(key(1)), 1, false, -1, false, true));
	CHECK(is(t.begin(key(0)), 0, false, -1, true, false)); // the first stream has not seen them either
}

// (c) 16 streams, then a 17th: the entry idle longest goes, the others move up, the table stays at 16
void seventeenth_stream() {
	StreamTable t;
	for (int i = 0; i < 16; ++i) CHECK(is(t.begin(key(i)), i, true, -1, false, false));
	CHECK(t.size() == 16);
	CHECK(is(t.begin(key(0)), 0, false, -1, false, false)); // stream 0 was used again: stream 1 is the one idle longest
	t.published();
	CHECK(is(t.begin(key(16)), 15, true, 1, true, false));
	CHECK(t.size() == 16 && t.find(key(1)) == -1);
	CHECK(t.find(key(0)) == 0 && t.find(key(2)) == 1 && t.find(key(15)) == 14 && t.find(key(16)) == 15); // in the order they were made
	CHECK(is(t.begin(key(1)), 15, true, 1, true, false)); // the retired stream comes back as a new entry (a wait, no question); stream 2 goes
	CHECK(t.size() == 16 && t.find(key(2)) == -1 && t.find(key(3)) == 1 && t.find(key(16)) == 14 && t.find(key(1)) == 15);
	CHECK(is(t.begin(key(0)), 0, false, -1, true, false)); // stream 0 kept its entry, and what it had seen
	CHECK(is(t.begin(key(17)), 15, true, 1, true, false)); // stream 3 goes: 0 has been used since
	CHECK(t.find(key(3)) == -1 && t.find(key(4)) == 1 && t.find(key(1)) == 14);
}

// (d) the residency was rebuilt: every stream starts over, as if no batch had ever been published
void residency_rebuilt() {
	StreamTable t;
	CHECK(is(t.begin(key(0)), 0, true, -1, false, false));
	t.published();
	CHECK(is(t.begin(key(0)), 0, false, -1, true, false));
	CHECK(is(t.begin(key(1)), 1, true, -1, true, false));
	t.published(); // neither stream has seen this one
	t.residency_rebuilt();
	CHECK(t.batches() == 0 && t.size() == 2);
	CHECK(is(t.begin(key(0)), 0, false, -1, false, false));
	CHECK(is(t.begin(key(1)), 1, false, -1, false, false));
	CHECK(is(t.begin(key(2)), 2, true, -1, false, false));
	t.published();
	CHECK(is(t.begin(key(1)), 1, false, -1, true, false)); // and the rule goes on from there
}

bool waits_are(const Ring::Launch& l, int n, long long a = -1, long long b = -1, long long c = -1) {
	const long long want[3] = {a, b, c};
	if (l.waits != n) return false;
	for (int i = 0; i < n; ++i)
		if (l.wait_launch[i] != want[i] || l.wait_slot[i] != static_cast<int>(want[i] % 256)) return false;
	return true;
}
Ring::Launch launch(Ring& r, int count) {
	const Ring::Launch l = r.plan(count);
	r.issued(l);
	return l;
}

// (e), (f) the frame ring, plain and wrapping
void frame_ring() {
	static Ring r;
	CHECK(!r.plan(0).ok && !r.plan(257).ok && r.plan(256).ok);
	// launches 0 ... 7, of 128 frames each, fill the ring exactly; nobody used these entries before
	for (int n = 0; n < 8; ++n) {
		const Ring::Launch l = launch(r, 128);
		CHECK(l.ok && l.first == 128 * n && l.count == 128 && l.slot == n && waits_are(l, 0));
	}
	CHECK(r.next() == 1024 && r.clock().launches() == 8 && r.owner(0) == 0 && r.owner(127) == 0 && r.owner(128) == 1 && r.owner(1023) == 7);
	// launch 8, one frame: the run would pass entry 1024, so it starts over at 0 and waits for launch 0
	Ring::Launch l = launch(r, 1);
	CHECK(l.first == 0 && l.slot == 8 && waits_are(l, 1, 0));
	// launch 9, seven frames: entries 1 ... 7, all of launch 0 -- equal owners in a row are waited for once
	l = launch(r, 7);
	CHECK(l.first == 1 && l.slot == 9 && waits_are(l, 1, 0));
	// (f) launch 10, 128 frames, entries 8 ... 135 (8 ... 127 of launch 0, 128 ... 135 of launch 1): planned, but not issued -- nothing changes
	l = r.plan(128);
	CHECK(l.first == 8 && l.slot == 10 && waits_are(l, 2, 0, 1));
	CHECK(r.next() == 8 && r.clock().launches() == 10 && r.owner(8) == 0 && r.owner(135) == 1);
	l = r.plan(128);
	CHECK(l.first == 8 && l.slot == 10 && waits_are(l, 2, 0, 1));
	r.issued(l);
	CHECK(r.next() == 136 && r.clock().launches() == 11 && r.owner(8) == 10 && r.owner(135) == 10 && r.owner(136) == 1);
	// launches 11 ... 16, 128 frames each: entries 136 + 128 k ..., each over the ends of two of the first eight launches
	for (int n = 11; n <= 16; ++n) {
		l = launch(r, 128);
		CHECK(l.first == 136 + 128 * (n - 11) && l.slot == n && waits_are(l, 2, n - 10, n - 9));
	}
	CHECK(r.next() == 904);
	// launch 17, 128 frames: 904 + 128 passes the end, so entries 0 ... 127 (launch 8, launch 9, launch 10); the tail 904 ... 1023 keeps launch 7
	l = launch(r, 128);
	CHECK(l.first == 0 && l.slot == 17 && waits_are(l, 3, 8, 9, 10));
	CHECK(r.owner(903) == 16 && r.owner(904) == 7 && r.owner(1023) == 7 && r.owner(0) == 17 && r.next() == 128);
	// launches 18 ... 255, one frame each: entries 128 ... 365, of launch 10 (up to 135), 11 (up to 263) and 12
	for (int n = 18; n <= 255; ++n) {
		l = launch(r, 1);
		const int entry = 128 + (n - 18);
		CHECK(l.first == entry && l.slot == n && waits_are(l, 1, entry < 136 ? 10 : entry < 264 ? 11 : 12));
	}
	CHECK(r.next() == 366 && r.clock().launches() == 256);
	// launch 256: the clock slots come round -- slot 0's previous user, launch 0, first; then entry 366's owner
	l = launch(r, 1);
	CHECK(l.first == 366 && l.slot == 0 && waits_are(l, 2, 0, 12));
	// launch 257, 128 frames: entries 367 ... 494 (launch 12 up to 391, then launch 13), behind slot 1's previous user
	l = launch(r, 128);
	CHECK(l.first == 367 && l.slot == 1 && waits_are(l, 3, 1, 12, 13));
	// launches 258 ... 268, one frame each on entries 495 ... 505 of launch 13, which is 245 ... 255 launches old: waited for
	for (int n = 258; n <= 268; ++n) {
		l = launch(r, 1);
		CHECK(l.first == 495 + (n - 258) && l.slot == n - 256 && waits_are(l, 2, n - 256, 13));
	}
	// launch 269: entry 506's owner, launch 13, is 256 launches old -- it is waited for as slot 13's previous user, in its turn, and not again
	l = launch(r, 1);
	CHECK(l.first == 506 && l.slot == 13 && waits_are(l, 1, 13));
	// launch 270: entry 507's owner is older than the clock ring and not waited for
	l = launch(r, 1);
	CHECK(l.first == 507 && l.slot == 14 && waits_are(l, 1, 14));
	// launch 271, 128 frames: entries 508 ... 635 of launches 13 and 14, both too old
	l = launch(r, 128);
	CHECK(l.first == 508 && l.slot == 15 && waits_are(l, 1, 15));
	CHECK(r.clock().last_slot() == 15 && r.clock().launches() == 272);
}

// (g) the slots of the most recent launches, oldest first
void recent_launches() {
	ClockRing<256> c;
	CHECK(c.recent(4) == 0 && c.launches() == 0 && !c.reused());
	for (int i = 0; i < 3; ++i) c.issued();
	CHECK(c.last_slot() == 2);
	CHECK(c.recent(2) == 2 && c.recent_slot(2, 0) == 1 && c.recent_slot(2, 1) == 2);                             // capacity below the launches
	CHECK(c.recent(3) == 3 && c.recent_slot(3, 0) == 0 && c.recent_slot(3, 2) == 2);                             // at
	CHECK(c.recent(10) == 3 && c.recent_slot(3, 1) == 1);                                                        // above
	CHECK(c.recent(0) == 0 && c.recent(-1) == 0);
	for (int i = 3; i < 300; ++i) c.issued(); // 300 launches: the clocks of 44 ... 299 stand
	CHECK(c.last_slot() == 43 && c.reused() && c.slot() == 44);
	CHECK(c.recent(2) == 2 && c.recent_slot(2, 0) == 42 && c.recent_slot(2, 1) == 43);
	CHECK(c.recent(256) == 256 && c.recent_slot(256, 0) == 44 && c.recent_slot(256, 255) == 43);
	CHECK(c.recent(1000) == 256 && c.recent_slot(256, 211) == 255 && c.recent_slot(256, 212) == 0);
}

// (h) the query ring: no wait before query 64; from then on the slot's previous user
void query_ring() {
	ClockRing<64> q;
	for (int i = 0; i < 64; ++i) {
		CHECK(!q.reused() && q.slot() == i);
		q.issued();
	}
	CHECK(q.reused() && q.slot() == 0); // query 64 waits for query 0's event
	for (int i = 64; i < 70; ++i) q.issued();
	CHECK(q.reused() && q.slot() == 6 && q.launches() == 70);
}

} // namespace

int main() {
	one_stream();
	late_stream();
	seventeenth_stream();
	residency_rebuilt();
	frame_ring();
	recent_launches();
	query_ring();
	std::printf("steps %ld\nfailures %ld\n", steps, failures);
	return failures ? 1 : 0;
}
