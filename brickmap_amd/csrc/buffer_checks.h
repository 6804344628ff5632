// buffer_checks.h -- the arithmetic on a caller's buffers that every device operator checks before it launches: alignment and overlap.
// Host code on integers alone; needs no HIP header: tests/buffer_checks_check.cpp builds it with a host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bm {

// [addr, addr + bytes): an address and a byte count; an empty span holds no byte, wherever it is
struct Span {
	uintptr_t addr;
	size_t bytes;
};
inline Span span_of(const void* p, size_t bytes) { return {reinterpret_cast<uintptr_t>(p), bytes}; }

// both hold a byte, and one of them holds a byte of the other.  A span that ends beyond the address space overlaps every non-empty span
// (no allocation gives one; sums are never formed, so nothing wraps)
inline bool spans_overlap(const Span& a, const Span& b) {
	if (a.bytes == 0 || b.bytes == 0) return false;
	if (a.bytes - 1 > UINTPTR_MAX - a.addr || b.bytes - 1 > UINTPTR_MAX - b.addr) return true;
	return a.addr <= b.addr + (b.bytes - 1) && b.addr <= a.addr + (a.bytes - 1); // last bytes: addr + bytes - 1 is representable
}

// a = 4, 8 or 16 (a power of two)
inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// every pointer is aligned: the OR of the addresses is
template <class... P>
inline bool all_aligned(size_t a, const P*... p) {
	return ((... | reinterpret_cast<uintptr_t>(p)) & (a - 1)) == 0;
}

} // namespace bm
