// arena.cpp -- see arena.h
#include "arena.h"

#include <algorithm>
#include <cstdlib>

#include "error.h"
#include "world.h"

namespace bm {

// ---- the arena's address range.  Reserved once per world for the worst case -- every pool is a power of two >= its
// supercell's brick count, and a pool that doubles its way up leaves regions of every smaller size behind (reused only by
// pools of that size) -- i.e. below 4 x the world's bricks + 32 per supercell; address space costs nothing.
int BrickArena::open(int device, uint64_t max_bricks) {
	close();
	device_ = device;
	int vmm = 0;
	if (hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, device_) != hipSuccess) vmm = 0;
	if (const char* e = std::getenv("BM_ARENA_VMM")) vmm = vmm && std::atoi(e) != 0; // experiment knob: 0 = reallocate + copy
	if (!vmm) { (void)hipGetLastError(); virtual_ = false; return 0; }
	hipMemAllocationProp prop{};
	prop.type = hipMemAllocationTypePinned;
	prop.location.type = hipMemLocationTypeDevice;
	prop.location.id = device_;
	size_t gran = 0;
	BM_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
	if (gran == 0) gran = 2u << 20;
	granularity_ = gran;
	uint64_t bytes = std::min<uint64_t>(max_bricks, (1ull << 32) - 1) * sizeof(Brick);
	bytes = (std::max<uint64_t>(bytes, 1ull << 22) + gran - 1) / gran * gran;
	void* va = nullptr;
	BM_HIP(hipMemAddressReserve(&va, bytes, 0, nullptr, 0));
	base_ = static_cast<uint32_t*>(va);
	va_bytes_ = bytes;
	virtual_ = true;
	capacity_ = 0;
	return 0;
}

int BrickArena::unmap_all() {
	// every chunk is taken off the list as it is processed (a chunk that failed to unmap must not be unmapped and released a
	// second time by a later call); the first error is reported after all of them have been tried
	hipError_t first = hipSuccess;
	const char* what = "";
	while (!chunks_.empty()) {
		const Chunk c = chunks_.back();
		chunks_.pop_back();
		if (hipError_t e = hipMemUnmap(reinterpret_cast<char*>(base_) + c.offset, c.bytes); e != hipSuccess && first == hipSuccess) { first = e; what = "hipMemUnmap"; }
		if (hipError_t e = hipMemRelease(c.handle); e != hipSuccess && first == hipSuccess) { first = e; what = "hipMemRelease"; }
	}
	capacity_ = 0;
	if (first != hipSuccess) return hip_fail(first, what, __FILE__, __LINE__);
	return 0;
}

void BrickArena::close() {
	if (virtual_) {
		// unlike hipFree, unmapping does not wait for work that still uses the range
		if (!chunks_.empty()) (void)hipDeviceSynchronize();
		const int unmap_error = unmap_all();
		// (a range that may still hold a mapping is not handed back: leaking address space is harmless, freeing a mapped range is not)
		if (base_ && unmap_error == 0) (void)hipMemAddressFree(base_, va_bytes_);
	} else if (base_) {
		(void)hipFree(base_);
	}
	base_ = nullptr;
	virtual_ = false;
	va_bytes_ = 0;
	capacity_ = 0;
	regions_.reset();
	chunks_.clear();
}

// Make the arena at least `bricks` large, keeping what it holds.  Virtual arena: map one more physical chunk behind the
// mapped part (the mapped size doubles) -- no copy, no synchronisation, nothing moves, so frames in flight and upload
// batches already queued are not disturbed (the reference grows one pool at a time with a blocking cudaMemcpy,
// Scene.cpp:242-247).  exact: (re)size an EMPTY arena to fit a known residency (callers have synchronised the device).
int BrickArena::reserve(uint64_t bricks, bool exact, bool* left_unmapped) {
	const uint64_t top = regions_.top();
	if (bricks <= capacity_ && !(exact && top == 0 && capacity_ > 2 * std::max<uint64_t>(bricks, 1ull << 16))) return 0;
	if (bricks >= (1ull << 32)) { set_error("brick arena would exceed 2^32 bricks"); return BM_EINVAL; }
	if (virtual_) {
		const size_t gran = granularity_;
		auto round_up = [gran](uint64_t b) { return (b + gran - 1) / gran * gran; };
		uint64_t want_bytes;
		bool remapping_empty_arena = false;
		// (when the arena was unmapped for an exact re-size, any failure below is reported as *left_unmapped: the owner refuses frames
		// until the residency has been rebuilt -- the device index words may still carry loaded bits)
		auto fail = [&](int code) { if (remapping_empty_arena && left_unmapped) *left_unmapped = true; return code; };
		if (exact && top == 0) {
			if (!chunks_.empty()) BM_HIP(hipDeviceSynchronize()); // (callers have synchronised already; unmapping itself does not wait)
			remapping_empty_arena = true; // from here on a failure leaves base() pointing at an unmapped range
			if (int e = unmap_all()) return fail(e);
			want_bytes = round_up(std::max<uint64_t>(bricks, 1ull << 16) * sizeof(Brick));
		} else {
			want_bytes = round_up(std::max<uint64_t>(capacity_, 1ull << 16) * sizeof(Brick)); // 4 MiB to start with
			while (want_bytes < bricks * sizeof(Brick)) want_bytes *= 2;
		}
		if (want_bytes > va_bytes_) want_bytes = va_bytes_;
		if (want_bytes < bricks * sizeof(Brick)) { set_error("brick arena: reserved address range exhausted"); return fail(BM_ESTATE); }
		const size_t have = static_cast<size_t>(capacity_) * sizeof(Brick);
		if (want_bytes > have) {
			hipMemAllocationProp prop{};
			prop.type = hipMemAllocationTypePinned;
			prop.location.type = hipMemLocationTypeDevice;
			prop.location.id = device_;
			Chunk c{};
			c.offset = have;
			c.bytes = want_bytes - have;
			if (hipError_t e = hipMemCreate(&c.handle, c.bytes, &prop, 0); e != hipSuccess) return fail(hip_fail(e, "hipMemCreate", __FILE__, __LINE__));
			char* at = reinterpret_cast<char*>(base_) + c.offset;
			if (hipError_t e = hipMemMap(at, c.bytes, 0, c.handle, 0); e != hipSuccess) { (void)hipMemRelease(c.handle); return fail(hip_fail(e, "hipMemMap", __FILE__, __LINE__)); }
			hipMemAccessDesc access{};
			access.location = prop.location;
			access.flags = hipMemAccessFlagsProtReadWrite;
			// access is (re)declared for the WHOLE mapped range, from the base: on this runtime (ROCm 7.2) hipMemSetAccess on a
			// chunk at an offset fails sporadically with "invalid argument" when the chunks differ in size
			// (tools/ubench/vmm_probe2.hip: 33 of 144 growths; 0 of 144 this way, with kernels in flight over the range)
			if (hipError_t e = hipMemSetAccess(base_, want_bytes, &access, 1); e != hipSuccess) {
				(void)hipMemUnmap(at, c.bytes); (void)hipMemRelease(c.handle);
				return fail(hip_fail(e, "hipMemSetAccess", __FILE__, __LINE__));
			}
			chunks_.push_back(c);
			if (capacity_ > 0) growths_++;
			capacity_ = want_bytes / sizeof(Brick);
		}
		return 0;
	}
	// ---- no virtual memory management on this device: reallocate + copy.  Synchronises the device: frames in flight may
	// still read the old allocation, and the copy must see every upload.
	uint64_t cap = bricks;
	if (!exact) { // growth by residency: double
		cap = std::max<uint64_t>(capacity_, 1ull << 16); // 4 MiB to start with
		while (cap < bricks) cap *= 2;
	} else if (top == 0) {
		cap = std::max<uint64_t>(bricks, 1ull << 16); // (re)sized for a known residency: exact fit, shrinking an oversized arena
	}
	if (cap >= (1ull << 32)) { set_error("brick arena would exceed 2^32 bricks"); return BM_EINVAL; }
	BM_HIP(hipDeviceSynchronize());
	uint32_t* fresh = nullptr;
	BM_HIP(hipMalloc(reinterpret_cast<void**>(&fresh), cap * sizeof(Brick)));
	if (base_ && top > 0) {
		BM_HIP(hipMemcpy(fresh, base_, top * sizeof(Brick), hipMemcpyDeviceToDevice));
		growths_++; copy_growths_++;
	}
	if (base_) BM_HIP(hipFree(base_));
	base_ = fresh;
	capacity_ = cap;
	return 0;
}

int BrickArena::region_alloc(uint32_t bricks, uint32_t* offset) {
	if (regions_.take_free(bricks, offset)) return 0;
	if (int e = reserve(regions_.top() + bricks)) return e;
	*offset = regions_.claim_top(bricks);
	return 0;
}

} // namespace bm
