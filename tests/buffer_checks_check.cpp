// buffer_checks_check.cpp -- a program with its own main around csrc/buffer_checks.h alone (no HIP, no scene), built plain and with
// -fsanitize=address,undefined by tests/test_buffer_checks.py.  Every helper against brute force:
//   1. overlap: every pair of spans with start 0 ... 40 and length 0 ... 12 inside a 64-byte array overlaps exactly when their byte
//      sets intersect (an empty span has no byte);
//   2. alignment: the 4, 8 and 16 tests on every start 0 ... 63 of a 16-byte aligned array equal start % a == 0;
//   3. the OR form on every triple of such starts equals "all three aligned";
//   4. the top of the address space: spans within 16 bytes of UINTPTR_MAX and spans at address 0 ... 4, as numbers (no pointer is
//      formed).  An empty span overlaps nothing; two non-empty ones overlap when either ends beyond the address space, and otherwise
//      exactly when they share a byte (128-bit arithmetic here).  A span whose last byte is UINTPTR_MAX does not end beyond it.
// prints "name count" pairs and "failures N".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../brickmap_amd/csrc/buffer_checks.h"

namespace {

long failures = 0;
#define CHECK(cond)                                                                  \
	do {                                                                             \
		if (!(cond)) {                                                               \
			if (++failures <= 10) std::printf("line %d: %s\n", __LINE__, #cond);     \
		}                                                                            \
	} while (0)

alignas(16) unsigned char bytes[64];

long check_overlap() {
	long cases = 0;
	for (int s0 = 0; s0 <= 40; ++s0)
		for (int n0 = 0; n0 <= 12; ++n0)
			for (int s1 = 0; s1 <= 40; ++s1)
				for (int n1 = 0; n1 <= 12; ++n1) {
					bool shared = false;
					for (int b = 0; b < 64; ++b) shared = shared || (s0 <= b && b < s0 + n0 && s1 <= b && b < s1 + n1);
					CHECK(bm::spans_overlap(bm::span_of(bytes + s0, n0), bm::span_of(bytes + s1, n1)) == shared);
					++cases;
				}
	return cases;
}

long check_aligned() {
	long cases = 0;
	for (size_t a : {4, 8, 16})
		for (int s = 0; s < 64; ++s) {
			CHECK(bm::aligned(bytes + s, a) == (s % a == 0));
			++cases;
		}
	CHECK(bm::aligned(nullptr, 16));
	return cases;
}

long check_all_aligned() {
	long cases = 0;
	for (size_t a : {4, 8, 16})
		for (int s0 = 0; s0 < 64; ++s0)
			for (int s1 = 0; s1 < 64; ++s1)
				for (int s2 = 0; s2 < 64; ++s2) {
					// (pointers of different types, as the operators pass them)
					const bool got = bm::all_aligned(a, bytes + s0, static_cast<const void*>(bytes + s1), reinterpret_cast<const char*>(bytes + s2));
					CHECK(got == (s0 % a == 0 && s1 % a == 0 && s2 % a == 0));
					++cases;
				}
	CHECK(bm::all_aligned(16, bytes, static_cast<const void*>(nullptr)));
	return cases;
}

long check_top_of_address_space(long* beyond_cases) {
	std::vector<bm::Span> spans;
	for (uintptr_t back = 0; back <= 16; ++back)
		for (size_t n = 0; n <= 32; ++n) spans.push_back({UINTPTR_MAX - back, n});
	for (uintptr_t addr = 0; addr <= 4; ++addr)
		for (size_t n = 0; n <= 4; ++n) spans.push_back({addr, n});
	typedef unsigned __int128 u128;
	const u128 top = u128{1} << (8 * sizeof(uintptr_t));
	long cases = 0;
	for (const bm::Span& x : spans)
		for (const bm::Span& y : spans) {
			const u128 xe = u128{x.addr} + x.bytes, ye = u128{y.addr} + y.bytes;
			bool want;
			if (x.bytes == 0 || y.bytes == 0) want = false;
			else if (xe > top || ye > top) { want = true; ++*beyond_cases; }
			else want = (x.addr > y.addr ? u128{x.addr} : u128{y.addr}) < (xe < ye ? xe : ye);
			CHECK(bm::spans_overlap(x, y) == want);
			++cases;
		}
	return cases;
}

} // namespace

int main() {
	long beyond = 0;
	std::printf("overlap %ld\n", check_overlap());
	std::printf("aligned %ld\n", check_aligned());
	std::printf("all_aligned %ld\n", check_all_aligned());
	const long top = check_top_of_address_space(&beyond);
	std::printf("top %ld\nbeyond %ld\n", top, beyond);
	std::printf("failures %ld\n", failures);
	return failures ? 1 : 0;
}
