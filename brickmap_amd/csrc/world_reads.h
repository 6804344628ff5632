// world_reads.h -- the calls that only read the world, with one owner: bm_scene_read_region, the three label calls, bm_scene_cast_rays and
// bm_scene_query_volumes.  Four of them are issued like a frame -- the stream is ordered behind pending uploads and changes, and
// process_load_queue orders itself behind the call -- and each takes the Turn of the scratch it uses (the table in read_book.h).  Every
// decision that needs no device is read_book.h's (host only, scripted on the CPU by tests/read_book_check.cpp); this class holds the scratch
// buffers, their Turns and the label clocks and makes the calls.  A Scene holds one and forwards; `ready` is its state check (on device,
// not failed, device selected), which every call here makes after its argument refusals and before it looks at a pointer's allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "../../include/brickmap.h"
#include "error.h"
#include "frame_order.h"
#include "hip_owned.h"
#include "launch_book.h"
#include "read_book.h"
#include "residency.h"
#include "world.h"

namespace bm {

class WorldReads {
public:
	// view: the scene's device view, copied when a call is issued; compute_units: read after the scene's init
	WorldReads(int device, World* world, Residency* residency, FrameOrder* order, const DeviceScene* view, const int* compute_units, std::function<int()> ready)
		: device_(device), world_(world), residency_(residency), order_(order), view_(view), compute_units_(compute_units), ready_(std::move(ready)) {}

	// a region that has passed Scene::check_region (pitches filled in, `ready` made), not empty.  The host world is authoritative, so a host
	// read is World::store_region.  A device read: the unpack kernel reads the device words and bricks; bricks that are not resident (a
	// streaming scene) are staged from the host world and written by a second small launch; what lies outside the world is zeroed.
	int read_region(const bm_region& r, uint8_t* voxels, int where, hipStream_t stream);
	// connected components (label.hip).  label_region is issued like a device read of the same box: zero what lies outside the world, label
	// the cells the device holds and then the staged ones, merge across cell faces, flatten and count.  Only the caller's volume is written.
	int label_region(const int32_t lo[3], const int32_t hi[3], uint32_t flags, int32_t* labels, uint64_t* count, hipStream_t stream);
	// These two read the label volume alone, so they are not frames: ordered on their stream, and behind the label call before them (the
	// root counts are one buffer, which grows only once that call has finished).
	int label_components(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, bm_component* comps, int64_t capacity, hipStream_t stream);
	int label_mask(const int32_t lo[3], const int32_t hi[3], const int32_t* labels, const bm_component* comps, int64_t n, const uint8_t* chosen, uint8_t* mask,
				   hipStream_t stream);
	int last_label_ms(float* local_ms, float* merge_ms, float* flatten_ms);
	// ray queries (query.hip).  The kernel only reads the world, apart from the request atomics, so it may run beside frames.
	int cast_rays(int64_t n, const bm_ray* rays, bm_ray_hit* hits, uint32_t flags, const float* lod_origin, hipStream_t stream);
	// volume queries (volume.hip).  The item offsets are one buffer, so a query is ordered behind the previous one (on whatever stream that
	// ran), and the buffer grows only once that has finished.
	int query_volumes(int64_t n, const bm_volume* volumes, bm_volume_result* results, uint32_t flags, hipStream_t stream);

private:
	// ray queries: a ring of slot counters (one 128-byte line each); a query that reuses an entry waits for the one that used it last.  Taken
	// like a Turn: order() before the query's work on the stream, pass() behind it.
	class TicketRing {
	public:
		int create(); // on first use
		uint32_t* ticket() const { return tickets_ + ring_.slot() * 32; } // of the query about to be issued
		int order(hipStream_t stream) const;
		int pass(hipStream_t stream);

	private:
		static constexpr int kQueryRing = 64;
		DeviceBuffer<uint32_t> tickets_;
		Event ev_[kQueryRing];
		ClockRing<kQueryRing> ring_;
	};
	// THE way a read is issued as a frame: begin (state check, `stream` behind pending uploads and changes), the frame ended on every path
	// from there, the Turn ordered, launch(view) queues the work on `stream`, the Turn passed behind it.  turn: a Turn, a TicketRing or null.
	template <class T, class Launch> int issue_frame(hipStream_t stream, T* turn, Launch&& launch);
	// a scratch that one call at a time uses (turn) holds `bytes`: it grows only after the call that uses it has finished
	template <class B> int reserve_behind(Turn& turn, B& scratch, size_t bytes);
	// the patch list of the clipped box [lo, hi), staged in h_patch_ with room in d_patch_ (nothing to do for an empty list)
	int stage_patches(const PatchList& list);
	int check_label_box(const char* who, const int32_t lo[3], const int32_t hi[3], LabelDims* d, bool* empty);

	int device_;
	World* world_;
	Residency* residency_;
	FrameOrder* order_;
	const DeviceScene* view_;
	const int* compute_units_;
	std::function<int()> ready_;
	// the patch list of read_region and label_region (pinned + device), the call's until its launch has used it (patches_)
	DeviceBuffer<char> d_patch_;
	PinnedBuffer<char> h_patch_;
	Turn patches_;
	TicketRing tickets_;
	int query_blocks_per_cu_[2] = {0, 0};
	// volume queries: the item offsets of one launch (volume_tmp_bytes); a query waits for the one before it, which used them
	DeviceBuffer<uint64_t> d_volume_tmp_;
	Turn volume_;
	int volume_blocks_per_cu_[2] = {0, 0};
	// connected components: the root counts of one bm_scene_label_components (label_tmp_bytes); label calls of a scene run one after another,
	// each waits for the one before it.  The stage clock of label_region: made on first use, marks 0 ... 3 (read_book.h LabelClock)
	DeviceBuffer<uint64_t> d_label_tmp_;
	Turn label_;
	StageMarks<4> label_marks_;
	LabelClock label_clock_;
};

} // namespace bm
