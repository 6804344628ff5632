"""brickmap_amd -- MI355X-native voxel brickmap path tracer (hot path of stijnherfst/BrickMap).

The package is a thin host-side mirror of the reference's Scene / Camera / State /
launch_kernels interface over the C-ABI of libbrickmap_hip.so (include/brickmap.h); all
rendering happens in hand-written HIP kernels for gfx950 (brickmap_amd/csrc/trace.hip).
"""
from ._lib import (BM_EDIT_BOX, BM_EDIT_CLEAR, BM_EDIT_SET, BM_EDIT_SPHERE, BM_REGION_REPLACE, bm_region, BM_FLAG_COUNTERS, BM_FLAG_ORDERED, BM_FLAG_PRIMARY_ONLY, BM_FLAG_RAY_DIGEST, BM_FLAG_SAMPLE_ITEMS, BM_DISTANCE_MASK_ABOVE, BM_DISTANCE_NONE, BM_DISTANCE_OUTSIDE, BM_DISTANCE_TO_EMPTY, BM_TRAVEL_NONE, BM_MESH_HALO, BM_MESH_UNIT_FACES, BM_QUERY_LOD, BM_QUERY_NO_REQUESTS, BM_VOLUME_ANY, BM_VOXELIZE_KEEP, BM_VOXELIZE_SOLID, BM_VOXELIZE_SURFACE, BM_VOXELS_DEVICE, BM_VOXELS_HOST, BRICK_INDEX_BITS, BRICK_LOADED_BIT, BRICK_LOD_BITS,  # noqa: F401
                   BRICK_REQUESTED_BIT, BRICK_UNLOADED_BIT, BrickmapError, load)
from .host import (FLYTHROUGH_VIEWS, RAY_DTYPE, RAY_HIT_DTYPE, RAY_QUEUE_DTYPE, SHADOW_QUEUE_DTYPE, Camera, FrameParams, RayHit, RayHits, Scene, State, Wavefront, camera_pixel_rays, denoise_workspace_bytes, host_denoise, host_label_volume, host_voxelize, voxelize_workspace_bytes, host_mesh_quads, host_mesh_triangles, mesh_workspace_bytes, QUAD_DTYPE, MESH_RESULT_DTYPE, Quads, DISTANCE_NONE, DISTANCE_RESULT_DTYPE, DistanceField, distance_workspace_bytes, host_distance_field, host_distance_mask, TRAVEL_NONE, TRAVEL_RESULT_DTYPE, TravelField, travel_workspace_bytes, host_travel_field, host_travel_paths, VOXELIZE_RESULT_DTYPE, VoxelizeResult, COMPONENT_DTYPE, Components, history_bytes, host_reproject, History, TemporalAccumulator, edit_box, edit_sphere, flythrough_camera, frame_plan, launch_plan, host_column_heights, host_cube_field,  # noqa: F401
                   host_edit_supercell, host_generate_supercell, host_load_supercell, host_write_region_supercell, region_of, launch_kernels, local_rows, pack_rays, probe_streams, release_streams, trace_waves_per_simd, tuning_overrides, volume_dims, VOLUME_DTYPE, VOLUME_RESULT_DTYPE, VolumeResults, volume_box, volume_sphere)
from . import dist  # noqa: F401

__all__ = ["Scene", "Camera", "State", "FrameParams", "Wavefront", "launch_kernels", "local_rows", "dist", "load", "BrickmapError"]
