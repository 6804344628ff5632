// kernels.h -- host-callable launchers implemented in trace.hip, edit.hip, escape.hip, sunfield.hip, viewfield.hip, load.hip, region.hip, query.hip, volume.hip, label.hip, voxelize.hip, mesh.hip, distance.hip, travel.hip, settle.hip, foot.hip, water.hip, denoise.hip, reproject.hip and wavefront.hip.
// What those kernel files share on the device side: device_types.h (argument blocks, the index word and a cell's place), global_mem.h
// (plain global accesses), voxel_bits.h (voxel bytes <-> brick bits), brick_rows.h (a run of 16 bricks through LDS), traverse.h (the walk).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "reproject.h"
#include "shadowheight.h"
#include "sunfield.h"
#include "viewfield.h"

namespace bm {
// resident workgroups of `threads` threads per compute unit of a kernel, at least 1 (host code of the file that defines the kernel)
template <class K>
int resident_blocks_per_cu(K kernel, int threads = 256) {
	int n = 0;
	const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0);
	return e == hipSuccess && n > 0 ? n : 1;
}

constexpr size_t kWorkCounterBytes = 64 * 32 * sizeof(uint32_t); // up to 64 chunk counters, one 128-byte line each
int trace_blocks_per_cu(bool instrumented, bool xcd_handout, bool helpers, int ring = 0); // resident workgroups per CU of that instantiation (ring: 0 = a launch of one frame, 1 = of several, 2 = of several uniform ones)
// fc_dev[0], fc_dev[1], ... are the constants of the frames of this launch (the frame ring, trace.hip; the last entry has frames_after == 0): each
// names its own accumulation / hit-record buffers; work_counter is the first of as many zeroed blocks of kWorkCounterBytes (a uniform launch uses one per GROUP of frames, FrameConstants::ring_group).
// instrumented ... ring name the instantiation and `workgroups` is the grid, both as planned (frame_plan.h LaunchPlan), the grid capped here by what the
// device keeps resident; blocks_per_cu_cap: 0 = as many workgroups per CU as the instantiation keeps resident; > 0 = at most that many (tuning runs)
void launch_trace(const DeviceScene& sc, const FrameConstants* fc_dev, DeviceCounters* counters, uint32_t* work_counter, bool instrumented, bool xcd_handout, bool helpers,
				  int ring, long long workgroups, int compute_units, int blocks_per_cu_cap, hipStream_t stream);
void launch_upload(const DeviceScene& sc, const uint32_t* bricks_queue, const uint32_t* indices_queue, uint32_t* arena, uint32_t count,
				   hipStream_t stream);
void launch_pool_moves(const PoolMove* moves, uint32_t count, uint32_t* arena, uint32_t* pool_base, hipStream_t stream);
void launch_snapshot_ring(const int* queue, const uint32_t* count, int* host_positions, uint32_t* host_count, uint32_t capacity, hipStream_t stream);
void launch_resolve(const float* accum, float* out, long long n, hipStream_t stream);
void launch_debug_sincos(int n, const float* x, float* s, float* c, hipStream_t stream);
void launch_debug_sky(const FrameConstants& fc, int n, const float* v, float* sun, float* sky, float* sunsky, hipStream_t stream);

// voxel edits (edit.hip).  FieldUpdate: the box of the octant cube field an edit batch recomputes, in bordered cell coordinates
// (1 ... cells, half-open ranges): r* = the cells written (the changed cells' bounding box grown by 254, clipped); ay = the rows the x
// pass covers for the y pass, bz = the slices the x and y passes cover for the z pass (the r ranges grown by 254, clipped)
struct FieldUpdate {
	int rx0, rx1, ry0, ry1, rz0, rz1;
	int ay0, ay1, bz0, bz1;
	int cells, cells_height, sg_xy, sg_xy2;
	int cf_shift;
	uint32_t cf_pxy, cf_plane;
};
size_t field_update_tmp_bytes(const FieldUpdate& u); // intermediate planes of the passes
// dirty cell i: index word words[i] at index_grid[cells[i]]; brick bricks[16 i ...] at arena slot slots[i] unless that is 0xFFFFFFFF
void launch_edit_scatter(const uint32_t* cells, const uint32_t* words, const uint32_t* slots, const uint32_t* bricks, uint32_t count,
						 uint32_t* index_grid, uint32_t* arena, hipStream_t stream);
void launch_field_update(const uint32_t* index_grid, uint8_t* field, uint8_t* tmp, const FieldUpdate& u, hipStream_t stream);

// escape heights (escape.hip; escape.h has the rule): the table the walk reads -- escape_entries() words -- rebuilt from the index grid.
// [x0, x1) x [y0, y1): the columns (unbordered cells) whose tops and bottoms are scanned again; the quadrant passes always cover the whole table.
// cols: escape_columns_bytes() bytes that keep every column's top and bottom between updates.
struct EscapeUpdate {
	int x0, x1, y0, y1;
	int cells, cells_height, sg_xy, sg_xy2;
	int cf_shift;
	uint32_t cf_pxy, cf_plane;
};
size_t escape_columns_bytes(int cells);
void launch_escape_update(const uint32_t* index_grid, int32_t* cols, uint32_t* table, const EscapeUpdate& u, hipStream_t stream);

// the sun plane (sunfield.hip; sunfield.h has the rules): plane 8 of `field`, every interior byte, rebuilt from the index grid, the column
// tops in `cols` and the escape table (both as launch_escape_update leaves them).  nd / n1 / n2: cells along the plan's dominant and minor
// axes.  tmp: sun_build_tmp_bytes() bytes that no other launch uses until this one has finished.
// The shadow heights (shadowheight.h) are built on the same occasion, by the clear-heights kernel of every slab: slice 8 of the escape
// table, from a scan of the columns' full bricks (index words, pool bases and the arena as they stand on the stream); where the plan has
// none (shadow.valid == 0) the slice is zeroed.  field = false: the slice alone, the plane stands (bricks changed, no cell's occupancy did).
struct SunBuild {
	SunPlan plan; // valid
	ShadowPlan shadow;
	int fx0, fx1, fy0, fy1; // the columns (unbordered cells, half-open, inside the grid) whose full tops are scanned again; the others keep what tmp_shadow holds
	int cells, cells_height, sg_xy, sg_xy2;
	int nd, n1, n2;
	int cf_shift;
	uint32_t cf_pxy, cf_plane;
};
size_t sun_build_tmp_bytes(const SunBuild& u);
size_t shadow_build_tmp_bytes(const SunBuild& u); // tmp_shadow: the scratch of the shadow heights, under the same condition
void launch_sun_build(const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, const int32_t* cols, uint32_t* escape, uint8_t* field, uint8_t* tmp,
					  uint8_t* tmp_shadow, const SunBuild& u, bool with_field, hipStream_t stream);

// the view plane (viewfield.hip; viewfield.h has the rule): plane 9 of `field`, every interior byte, rebuilt for the camera position of
// `plan` from the octant planes of `field` and the escape table (both as the field and escape updates leave them on the stream)
struct ViewBuild {
	ViewPlan plan; // valid
	int cells, cells_height;
	int cf_shift;
	uint32_t cf_pxy, cf_plane;
};
void launch_view_build(const uint32_t* escape, uint8_t* field, const ViewBuild& u, hipStream_t stream);

// dense voxels -> scene (load.hip): the volume is V[z][y][x], one byte per voxel, in device memory.  classify leaves lod << 12 in every
// cell's index word; number turns the words into slot | loaded | lod << 12 (slots in local cell order), fills counts[supercells] and
// pool_base[supercells] (exclusive scan of the counts) and total[2] (the 64-bit brick total, low word first); pack writes the bricks
// to arena[pool_base[sc] + slot] -- the arena must hold `total` bricks by then
struct LoadDims {
	uint32_t grid_size;      // voxels along x and y
	uint32_t sg_xy, sg_xy2;  // supercells per axis, squared
	uint32_t supercells;
};
void launch_load_classify(const uint8_t* voxels, uint32_t* index_grid, const LoadDims& d, hipStream_t stream);
void launch_load_number(uint32_t* index_grid, uint32_t* counts, uint32_t* pool_base, uint32_t* total, const LoadDims& d, hipStream_t stream);
void launch_load_pack(const uint8_t* voxels, const uint32_t* index_grid, const uint32_t* pool_base, uint32_t* arena, const LoadDims& d, hipStream_t stream);

// dense regions (region.hip): a box of voxels as a volume V[z][y][x] in device memory, x contiguous (RegionDims: device_types.h)
// bricks[16 i ...] = the box's part of its cell i (cells in x-fastest order over c0 ... c0 + nc), bits outside the box 0
void launch_region_pack(const uint8_t* voxels, uint32_t* bricks, const RegionDims& d, hipStream_t stream);
// the box's voxels as bytes 0 / 1 from the device world: 0 where a cell is empty or its brick is not resident
void launch_region_unpack(uint8_t* voxels, const uint32_t* index_grid, const uint32_t* pool_base, const uint32_t* arena, const RegionDims& d, hipStream_t stream);
// the box's part of `count` (> 0) listed cells: cells[3 i ...] = brick cell (x, y, z), bricks[16 i ...] = its bits
void launch_region_patch(uint8_t* voxels, const int* cells, const uint32_t* bricks, uint32_t count, const RegionDims& d, hipStream_t stream);
// nz slices of ny rows of nx bytes from `voxels` on, set to 0 (all > 0)
void launch_region_zero(uint8_t* voxels, int64_t row_pitch, int64_t slice_pitch, int64_t nx, int64_t ny, int64_t nz, hipStream_t stream);

// ray queries (query.hip): n bm_ray records in, n bm_ray_hit records out; ticket = a zeroed word; campos = the LoD centre in brick cells
int query_blocks_per_cu(bool request);
void launch_query(const DeviceScene& sc, const int campos[3], const void* rays, void* hits, uint32_t n, uint32_t* ticket, int resident_blocks,
				  bool request, hipStream_t stream);

// volume queries (volume.hip): n bm_volume records in, n bm_volume_result records out (every byte written).  tmp: volume_tmp_bytes(n) bytes --
// one 64-bit word per record and one per 256 records, plus one -- that no other launch uses until this one has finished
int volume_blocks_per_cu(bool any);
size_t volume_tmp_bytes(uint32_t n);
void launch_volume_query(const DeviceScene& sc, const void* volumes, void* results, uint32_t n, bool any, uint64_t* tmp, int resident_blocks, hipStream_t stream);

// connected components (label.hip; label.h has the rules, device_types.h LabelDims)
// local, merge, flatten over the clipped box (not empty; the voxels outside the world are zeroed by the caller): labels as the contract
// of bm_scene_label_region has them, and the number of components added to *count.  patch_cells / patch_bricks: `patches` listed cells
// (as launch_region_patch takes them) whose bricks the device does not hold.  marks: null, or 4 events around local, merge and flatten.
void launch_label_region(const DeviceScene& sc, uint32_t* labels, uint64_t* count, const LabelDims& d, const int* patch_cells, const uint32_t* patch_bricks,
						 uint32_t patches, hipStream_t stream, hipEvent_t* marks = nullptr);
// tmp of launch_label_components: one 64-bit word per 1024 voxels, plus one, that no other launch uses until this one has finished
size_t label_tmp_bytes(uint32_t voxels);
void launch_label_components(const uint32_t* labels, void* comps, uint64_t capacity, const LabelDims& d, uint64_t* tmp, hipStream_t stream);
void launch_label_mask(const uint32_t* labels, uint32_t voxels, const void* comps, uint64_t records, const uint8_t* chosen, uint8_t* mask, hipStream_t stream);

// meshes -> voxels (voxelize.hip; voxelize.h has the rules and VoxelizeDims): n triangles of 9 floats fill the volume V[z][y][x] of extent voxels at the
// given pitches.  workspace: voxelize_workspace_bytes() bytes, 16-byte aligned, that no other launch uses until this one has finished
// (zeroed here); result: null, or the 16 bytes of a bm_voxelize_result.  resident_blocks: the grids of the surface and the solid items.
// marks: null, or 6 events around zeroing, plan + scan, surface, solid and the dense pass.
struct VoxelizeDims;
size_t voxelize_workspace_bytes(const VoxelizeDims& d, uint32_t n);
int voxelize_blocks_per_cu(bool solid);
void launch_voxelize(const VoxelizeDims& d, const float* triangles, uint32_t n, uint8_t* volume, void* result, void* workspace, const int resident_blocks[2],
					 hipStream_t stream, hipEvent_t* marks = nullptr);

// block_off[g * (nblocks + 1) + (0 ... nblocks)), g < groups: sums -> 64-bit exclusive offsets, entry nblocks = the total (voxelize.hip's
// scan of workgroup sums, also the last step of mesh.hip's)
void launch_offsets_scan(uint64_t* block_off, uint32_t nblocks, uint32_t groups, hipStream_t stream);

// voxels -> quads (mesh.hip; mesh.h has the rules and MeshDims): the volume's surface as 16-byte quads, the first `capacity` of them
// written (capacity 0: none), the totals in the 16 bytes of `result`.  workspace: mesh_workspace_bytes() bytes, 16-byte aligned, that no
// other launch uses until this one has finished.  marks: null, or 4 events around count, scan and emit.
struct MeshDims;
void launch_mesh_quads(const MeshDims& d, const uint8_t* volume, void* quads, uint64_t capacity, void* result, void* workspace, hipStream_t stream,
					   hipEvent_t* marks = nullptr);
// n quads -> 2 n triangles of 9 floats
void launch_mesh_triangles(const void* quads, uint64_t n, float* triangles, hipStream_t stream);

// voxels -> their squared distance to the nearest source (distance.hip; distance.h has the rules and DistanceDims): the tight field of
// d.voxels words and the 32 bytes of `result`.  workspace: distance_workspace_bytes() bytes, 16-byte aligned, that no other launch uses
// until this one has finished (its tail is zeroed here).  marks: null, or 4 events around the x pass, the y pass and the z pass + finish.
struct DistanceDims;
void launch_distance_field(const DistanceDims& d, const uint8_t* volume, uint32_t* field, void* result, void* workspace, hipStream_t stream,
						   hipEvent_t* marks = nullptr);
// out[i] = field[i] <= limit_sq (above: the opposite), i < n; out at any address
void launch_distance_mask(const uint32_t* field, uint64_t n, uint32_t limit_sq, uint32_t above, uint8_t* out, hipStream_t stream);

// voxels + seeds -> shortest face-step distances (travel.hip; travel.h has the rules, TravelDims and the workspace's layout).  The caller
// (device_ops.cpp) enqueues the set-up, then rounds in batches -- between batches it reads the next list's count from the tail and stops
// at 0 -- then the finish.  workspace: travel_workspace_bytes() bytes, 16-byte aligned, that no other launch uses until the finish has
// run (its stamps and tail are zeroed by the set-up).  Rounds count from 1.
struct TravelDims;
void launch_travel_setup(const TravelDims& d, const uint8_t* volume, const int32_t* seeds, uint32_t n, uint32_t* field, void* workspace, hipStream_t stream);
void launch_travel_rounds(const TravelDims& d, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream);
void launch_travel_finish(const TravelDims& d, const uint32_t* field, void* result, void* workspace, hipStream_t stream);
// n starts -> n paths of at most `capacity` voxels down the field, and their lengths
void launch_travel_paths(const TravelDims& d, const uint32_t* field, const int32_t* starts, uint32_t n, int32_t capacity, int32_t* path, int32_t* lengths, hipStream_t stream);

// labels + chosen records -> the settled volume (settle.hip; settle.h has the rules, SettleDims and the workspace's layout).  The caller
// (device_ops.cpp) enqueues the set-up, then rounds in batches -- between batches it reads the last round's count of changes from the
// tail and stops at 0 -- then the move with the finish.  workspace: settle_workspace_bytes() bytes, 4-byte aligned, that no other launch
// uses until the move has run (its tail is zeroed by the set-up).  Rounds count from 1.  records, chosen, drops: unused when d.n is 0.
struct SettleDims;
void launch_settle_setup(const SettleDims& d, const uint8_t* chosen, void* workspace, hipStream_t stream);
void launch_settle_rounds(const SettleDims& d, const int32_t* labels, const void* records, const uint8_t* chosen, void* workspace, uint32_t first_round, uint32_t rounds,
						  hipStream_t stream);
void launch_settle_move(const SettleDims& d, const int32_t* labels, const void* records, const uint8_t* chosen, uint8_t* out, int32_t* drops, void* result, void* workspace,
						hipStream_t stream);

// a byte volume -> room bytes, room bytes + seeds -> walk distances and paths (foot.hip; foot.h has the rules, FootDims and the workspace's
// layout).  The caller (device_ops.cpp) enqueues the set-up, then rounds in batches -- between batches it reads the size of the next front
// from the tail and stops at 0 -- then the finish with the number of rounds enqueued.  workspace: foot_workspace_bytes() bytes, 16-byte
// aligned, that no other launch uses until the finish has run (its tail is zeroed by the set-up).  Rounds count from 1.
struct FootDims;
void launch_foot_room(const FootDims& d, const uint8_t* volume, uint8_t* room, hipStream_t stream);
void launch_foot_setup(const FootDims& d, const uint8_t* room, const int32_t* seeds, uint32_t n, uint32_t* field, void* workspace, hipStream_t stream);
void launch_foot_rounds(const FootDims& d, const uint8_t* room, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream);
void launch_foot_finish(const FootDims& d, const uint32_t* field, void* result, void* workspace, uint32_t done, hipStream_t stream);
void launch_foot_paths(const FootDims& d, const uint8_t* room, const uint32_t* field, const int32_t* starts, uint32_t n, int32_t capacity, int32_t* path, int32_t* lengths,
					   hipStream_t stream);

// a byte volume + drains -> spill levels, and a field -> the mask of its pools (water.hip; water.h has the rules; the dims, the workspace
// and the rounds are those of the travel field).  The caller (device_ops.cpp) enqueues the set-up, reads the first list's count, then
// enqueues rounds in batches -- between batches it reads the next list's count from the tail and stops at 0 -- then the finish.
// workspace: travel_workspace_bytes() bytes, 16-byte aligned, that no other launch uses until the finish has run.  Rounds count from 1.
void launch_water_setup(const TravelDims& d, uint32_t sea, uint32_t faces, const uint8_t* volume, const int32_t* drains, uint32_t n, uint32_t* field, void* workspace,
						hipStream_t stream);
void launch_water_rounds(const TravelDims& d, uint32_t* field, void* workspace, uint32_t first_round, uint32_t rounds, hipStream_t stream);
void launch_water_finish(const TravelDims& d, const uint32_t* field, void* result, void* workspace, hipStream_t stream);
// mask[i] = the voxel is wet and at least min_depth deep; mask at any address
void launch_water_mask(const int32_t extent[3], const uint32_t* field, uint32_t min_depth, uint8_t* mask, hipStream_t stream);

// the a-trous filter (denoise.hip; denoise.h has the rules): accum and hits in, out = (c, 1) per pixel; workspace: denoise_workspace_bytes()
// bytes that no other launch uses until this one has finished.  iterations 0 ... 8, every pointer 16-byte aligned; out may be accum.
// tiled_max_step: a-trous passes up to this stride (1, 2; 0 = none) stage their taps in LDS, the others read them from global memory.
// marks: null, or 2 + max(iterations, 1) events, recorded before the first kernel and after every kernel (prepare, moments, the passes).
constexpr int kDenoiseTiledMaxStep = 2;
void launch_denoise(int width, int height, int iterations, float sigma_l, const float* accum, const void* hits, float* out, void* workspace,
					int tiled_max_step, hipStream_t stream, hipEvent_t* marks = nullptr);
// pixel-centre rays of a width x height frame (denoise.hip): width * height bm_ray records; the basis is that of fill_frame_constants
struct PixelRayBasis {
	float right[3], up[3], dir[3], origin[3];
	int width, height;
};
void launch_pixel_rays(const PixelRayBasis& basis, void* rays, hipStream_t stream);
// temporal accumulation (reproject.hip; reproject.h has the rules): accum and hits of the frame of camera `cur`, the history of the frame
// of camera `prev` (history_prev, or null: no history) -> history_out; a history is history_bytes() bytes, every pointer 16-byte aligned,
// history_out overlaps no input.  Both bases travel by value as a kernel argument.
struct ReprojectCameras {
	CameraBasis cur;
	RpPrevCamera prev;
	int width, height;
};
void launch_reproject(const ReprojectCameras& cams, float max_history, const float* accum, const void* hits, const void* history_prev, void* history_out,
					  hipStream_t stream);

// wavefront mode (wavefront.hip)
int wavefront_blocks_per_cu(bool connect, bool instrumented);
void launch_wf_primary(WfState* st, WfRay* work, const FrameConstants* fc_dev, uint32_t queue_size, uint32_t pixels, hipStream_t stream);
void launch_wf_trace(bool connect, const DeviceScene& sc, const FrameConstants* fc_dev, WfState* st, WfRay* work, const WfShadow* shadow, float* accum,
					 DeviceCounters* counters, uint32_t queue_size, int resident_blocks, void* cold_scratch, hipStream_t stream);
void launch_wf_shade(const WfRay* work, WfRay* next, WfShadow* shadow, float* accum, void* block_counts, WfState* st, const FrameConstants* fc_dev,
					 uint32_t queue_size, hipStream_t stream);
} // namespace bm
