"""Loader for libbrickmap_hip.so (the C-ABI in include/brickmap.h).

There is deliberately no CPU fallback: if the HIP library is missing or fails to load, every
entry point of this package raises.  torch is imported first so that the library binds to the
same libamdhip64.so.7 torch already loaded (torch is plumbing here: device memory, streams,
torch.distributed).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbrickmap_hip.so")

BM_FLAG_PRIMARY_ONLY = 1
BM_FLAG_SAMPLE_ITEMS = 4
BM_FLAG_COUNTERS = 2
BM_FLAG_ORDERED = 16
BM_FLAG_RAY_DIGEST = 32
BM_QUERY_LOD = 1
BM_QUERY_NO_REQUESTS = 2
BM_VOLUME_ANY = 1
BM_VOXELS_HOST = 0
BM_VOXELS_DEVICE = 1
BRICK_INDEX_BITS = 0x00000FFF
BRICK_LOD_BITS = 0x000FF000
BRICK_REQUESTED_BIT = 0x20000000
BRICK_UNLOADED_BIT = 0x40000000
BRICK_LOADED_BIT = 0x80000000


class BrickmapError(RuntimeError):
    pass


class bm_camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("direction", C.c_float * 3), ("up", C.c_float * 3),
                ("focal_distance", C.c_float), ("lens_radius", C.c_float)]


class bm_frame_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("sample_base", C.c_int32),
                ("max_bounces", C.c_int32), ("base_frame", C.c_uint32), ("flags", C.c_uint32),
                ("band_rows", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("sun_position", C.c_float * 2)]


class bm_frame_plan(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("ordered", C.c_int32), ("helpers", C.c_int32), ("sample_items", C.c_int32), ("xcd_handout", C.c_int32),
                ("refill_min", C.c_int32), ("refill_min_in_ring", C.c_int32), ("instrumented", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("local_rows", C.c_int32), ("ring_group", C.c_int32)]


class bm_launch_plan(C.Structure):
    _fields_ = [("ring_mode", C.c_int32), ("ring_group", C.c_int32), ("sample_stride", C.c_int32), ("pixel_stride", C.c_uint32), ("shared_digest", C.c_int32),
                ("instrumented", C.c_int32), ("counter_blocks", C.c_int32), ("refill_min", C.c_int32), ("workgroups", C.c_int64)]


BM_EDIT_SET = 1
BM_EDIT_CLEAR = 2
BM_EDIT_BOX = 1
BM_EDIT_SPHERE = 2


class bm_edit(C.Structure):
    _fields_ = [("op", C.c_int32), ("shape", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("center", C.c_int32 * 3),
                ("radius", C.c_int32)]


BM_REGION_REPLACE = 0


class bm_region(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64)]


class bm_ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("direction", C.c_float * 3), ("tmax", C.c_float), ("reserved", C.c_uint32)]


class bm_ray_hit(C.Structure):
    _fields_ = [("distance", C.c_float), ("normal", C.c_float * 3), ("voxel", C.c_int32 * 3), ("level", C.c_int32)]


class bm_reproject_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_history", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_denoise_params(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("sigma_l", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_component(C.Structure):
    _fields_ = [("label", C.c_int32), ("faces", C.c_uint32), ("voxels", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


BM_VOXELIZE_SURFACE = 1
BM_VOXELIZE_SOLID = 2
BM_VOXELIZE_KEEP = 1


class bm_voxelize_params(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64), ("mode", C.c_uint32), ("flags", C.c_uint32)]


class bm_voxelize_result(C.Structure):
    _fields_ = [("rejected", C.c_uint32), ("degenerate", C.c_uint32), ("open_columns", C.c_uint64)]


BM_MESH_HALO = 1
BM_MESH_UNIT_FACES = 2


class bm_mesh_params(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("extent", C.c_int32 * 3), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_quad(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("z", C.c_int32), ("shape", C.c_uint32)]


class bm_mesh_result(C.Structure):
    _fields_ = [("quads", C.c_uint64), ("faces", C.c_uint64)]


BM_DISTANCE_TO_EMPTY = 1
BM_DISTANCE_OUTSIDE = 2
BM_DISTANCE_MASK_ABOVE = 1
BM_DISTANCE_NONE = 0x7FFFFFFF


class bm_distance_params(C.Structure):
    _fields_ = [("extent", C.c_int32 * 3), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_distance_result(C.Structure):
    _fields_ = [("sources", C.c_uint64), ("max_sq", C.c_uint32), ("reserved0", C.c_uint32), ("max_at", C.c_uint64), ("reserved1", C.c_uint64)]


BM_TRAVEL_NONE = 0x7FFFFFFF


class bm_travel_params(C.Structure):
    _fields_ = [("extent", C.c_int32 * 3), ("max_steps", C.c_uint32), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_travel_result(C.Structure):
    _fields_ = [("reached", C.c_uint64), ("farthest", C.c_uint32), ("seeds_rejected", C.c_uint32), ("farthest_at", C.c_uint64), ("reserved", C.c_uint64)]


class bm_settle_result(C.Structure):
    _fields_ = [("moved_voxels", C.c_uint64), ("chosen_pieces", C.c_uint32), ("moved_pieces", C.c_uint32), ("largest_drop", C.c_uint32), ("reserved", C.c_uint32),
                ("contacts", C.c_uint64)]


BM_FOOT_NONE, BM_FOOT_TOWARD, BM_FOOT_NO_FLOOR = 0x7FFFFFFF, 1, 2


class bm_foot_params(C.Structure):  # begins with the fields of bm_travel_params: dense_layout fills that part unchanged
    _fields_ = bm_travel_params._fields_ + [("height", C.c_int32), ("climb", C.c_int32), ("drop", C.c_int32), ("reserved2", C.c_int32)]


class bm_foot_result(C.Structure):
    _fields_ = [("reached", C.c_uint64), ("farthest", C.c_uint32), ("seeds_rejected", C.c_uint32), ("farthest_at", C.c_uint64), ("standable", C.c_uint64)]


BM_WATER_NONE = 0x7FFFFFFF
BM_WATER_FACES = {"-x": 1, "+x": 2, "-y": 4, "+y": 8, "-z": 16, "+z": 32}   # the bits of bm_component.faces


class bm_water_params(C.Structure):  # a bm_travel_params with sea_level where max_steps is: dense_layout fills the rest unchanged
    _fields_ = [("extent", C.c_int32 * 3), ("sea_level", C.c_uint32), ("row_pitch", C.c_int64), ("slice_pitch", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class bm_water_result(C.Structure):
    _fields_ = [("wet", C.c_uint64), ("deepest", C.c_uint32), ("drains_rejected", C.c_uint32), ("deepest_at", C.c_uint64), ("closed", C.c_uint64)]


class bm_volume(C.Structure):
    _fields_ = [("shape", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("center", C.c_int32 * 3), ("radius", C.c_int32), ("reserved", C.c_uint32)]


class bm_volume_result(C.Structure):
    _fields_ = [("solid", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("unresolved", C.c_uint32), ("status", C.c_uint32)]


class bm_scene_info(C.Structure):
    _fields_ = [("grid_size", C.c_int32), ("grid_height", C.c_int32), ("supergrid_xy", C.c_int32),
                ("supergrid_z", C.c_int32), ("supercells", C.c_int32), ("queue_capacity", C.c_int32),
                ("lod_distance_8x8x8", C.c_int32), ("lod_distance_2x2x2", C.c_int32),
                ("generated", C.c_int32), ("on_device", C.c_int32),
                ("total_bricks", C.c_uint64), ("resident_bricks", C.c_uint64),
                ("index_bytes", C.c_uint64), ("brick_bytes", C.c_uint64),
                ("pool_bytes", C.c_uint64), ("cube_field_bytes", C.c_uint64),
                ("arena_growths", C.c_uint64), ("arena_copy_growths", C.c_uint64), ("arena_virtual", C.c_int32), ("failed", C.c_int32),
                ("stream_batches", C.c_uint64), ("stream_host_ns", C.c_uint64), ("escape_bytes", C.c_uint64), ("sun_plane_bytes", C.c_uint64)]


COUNTER_NAMES = ("index_loads", "brick_tests", "byte_tests", "voxel_steps", "extend_rays",
                 "shadow_rays", "requests", "paths")


class bm_counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_NAMES]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_NAMES}


SCHED_NAMES = ("step_runs", "step_lanes", "candidate_runs", "candidate_lanes", "shade_runs", "shade_lanes", "connect_runs", "connect_lanes",
               "step_cycles", "candidate_cycles", "shade_cycles", "drain_cycles", "total_cycles", "jump_runs", "jump_lanes", "waves")


class bm_sched_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in SCHED_NAMES]


# The records as numpy sees them, each derived from its structure above (tests/test_binding_surface.py keeps an independent second copy)
RAY_DTYPE, RAY_HIT_DTYPE = np.dtype(bm_ray), np.dtype(bm_ray_hit)                                   # 32 bytes each
VOLUME_DTYPE, VOLUME_RESULT_DTYPE = np.dtype(bm_volume), np.dtype(bm_volume_result)                 # 48 bytes in, 40 bytes out
COMPONENT_DTYPE = np.dtype(bm_component)                                                            # 40 bytes
VOXELIZE_RESULT_DTYPE = np.dtype(bm_voxelize_result)                                                # 16 bytes
QUAD_DTYPE, MESH_RESULT_DTYPE = np.dtype(bm_quad), np.dtype(bm_mesh_result)                         # 16 bytes each; a quad's shape = d | w << 4 | h << 8
DISTANCE_RESULT_DTYPE, TRAVEL_RESULT_DTYPE = np.dtype(bm_distance_result), np.dtype(bm_travel_result)  # 32 bytes each
SETTLE_RESULT_DTYPE = np.dtype(bm_settle_result)                                                    # 32 bytes
FOOT_RESULT_DTYPE = np.dtype(bm_foot_result)                                                        # 32 bytes
WATER_RESULT_DTYPE = np.dtype(bm_water_result)                                                      # 32 bytes
# the queue records (variables.h:43-52 RayQueue, :54-59 ShadowQueue), which the header does not declare
RAY_QUEUE_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("throughput", "<f4", 3), ("normal", "<f4", 3),
                            ("distance", "<f4"), ("identifier", "<i4"), ("bounces", "<i4"), ("pixel_index", "<u4")])
SHADOW_QUEUE_DTYPE = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3), ("pixel_index", "<u4")])

# every symbol include/brickmap.h declares: name -> (restype, argtypes)
_vp, _i, _u32p = C.c_void_p, C.c_int, C.POINTER(C.c_uint32)
SIGNATURES = {
    "bm_last_error_string": (C.c_char_p, []),
    "bm_device_count": (_i, [C.POINTER(C.c_int)]),
    "bm_device_name": (_i, [_i, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]),
    "bm_scene_create": (_i, [_i, _i, _i, C.POINTER(_vp)]),
    "bm_scene_destroy": (None, [_vp]),
    "bm_scene_set_lod": (_i, [_vp, _i, _i]),
    "bm_scene_set_queue_capacity": (_i, [_vp, _i]),
    "bm_scene_set_streaming_mode": (_i, [_vp, _i]),
    "bm_scene_generate": (_i, [_vp, _i]),
    "bm_scene_generate_supercell": (_i, [_vp, _i, _i, _i]),
    "bm_scene_preload_all": (_i, [_vp]),
    "bm_scene_reset_residency": (_i, [_vp]),
    "bm_scene_process_load_queue": (_i, [_vp, _u32p]),
    "bm_scene_dump": (_i, [_vp, C.c_char_p]),
    "bm_scene_get_info": (_i, [_vp, C.POINTER(bm_scene_info)]),
    "bm_scene_host_supercell": (_i, [_vp, _i, _vp, _u32p, _vp, C.c_uint32]),
    "bm_scene_device_indices": (_i, [_vp, _i, _vp]),
    "bm_scene_device_brick": (_i, [_vp, _i, C.c_uint32, _vp]),
    "bm_scene_column_heights": (_i, [_vp, _i, _i, _vp]),
    "bm_scene_edit": (_i, [_vp, _i, C.POINTER(bm_edit), _vp]),
    "bm_scene_set_voxels": (_i, [_vp, _i, _vp, _vp, _vp]),
    "bm_scene_device_cube_field": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bm_scene_host_cube_field": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bm_scene_escape_table": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bm_scene_sun_plane": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "bm_scene_shadow_heights": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), _vp]),
    "bm_scene_sun_plane_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    "bm_scene_view_plane": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "bm_scene_view_plane_stats": (_i, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]),
    "bm_scene_last_edit_ms": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "bm_scene_load_voxels": (_i, [_vp, _vp, C.c_size_t, _i, _vp]),
    "bm_scene_host_voxels": (_i, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bm_scene_last_load_ms": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "bm_scene_write_region": (_i, [_vp, C.POINTER(bm_region), _i, _vp, _i, _vp]),
    "bm_scene_read_region": (_i, [_vp, C.POINTER(bm_region), _vp, _i, _vp]),
    "bm_scene_last_region_ms": (_i, [_vp] + [C.POINTER(C.c_float)] * 4),
    "bm_scene_cast_rays": (_i, [_vp, C.c_int64, _vp, _vp, C.c_uint32, _vp, _vp]),
    "bm_scene_query_volumes": (_i, [_vp, C.c_int64, _vp, _vp, C.c_uint32, _vp]),
    "bm_scene_label_region": (_i, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_int32 * 3), C.c_uint32, _vp, _vp, _vp]),
    "bm_scene_label_components": (_i, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_int32 * 3), _vp, _vp, C.c_int64, _vp]),
    "bm_scene_label_mask": (_i, [_vp, C.POINTER(C.c_int32 * 3), C.POINTER(C.c_int32 * 3), _vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "bm_scene_last_label_ms": (_i, [_vp] + [C.POINTER(C.c_float)] * 3),
    "bm_host_label_volume": (_i, [_vp, C.c_int64, C.c_int64, C.c_int64, _vp, C.POINTER(C.c_uint64)]),
    "bm_voxelize_workspace_bytes": (_i, [C.POINTER(bm_voxelize_params), C.c_int64, C.POINTER(C.c_size_t)]),
    "bm_voxelize": (_i, [_vp, C.POINTER(bm_voxelize_params), C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_voxelize_times": (_i, [_vp, C.POINTER(bm_voxelize_params), C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_float)]),
    "bm_host_voxelize": (_i, [C.POINTER(bm_voxelize_params), C.c_int64, _vp, _vp, C.POINTER(bm_voxelize_result)]),
    "bm_mesh_workspace_bytes": (_i, [C.POINTER(bm_mesh_params), C.POINTER(C.c_size_t)]),
    "bm_mesh_quads": (_i, [_vp, C.POINTER(bm_mesh_params), _vp, _vp, C.c_uint64, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_mesh_times": (_i, [_vp, C.POINTER(bm_mesh_params), _vp, _vp, C.c_uint64, _vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_float)]),
    "bm_mesh_triangles": (_i, [_vp, _vp, C.c_int64, _vp, _vp]),
    "bm_host_mesh_quads": (_i, [C.POINTER(bm_mesh_params), _vp, _vp, C.c_uint64, C.POINTER(bm_mesh_result)]),
    "bm_host_mesh_triangles": (_i, [_vp, C.c_int64, _vp]),
    "bm_distance_workspace_bytes": (_i, [C.POINTER(bm_distance_params), C.POINTER(C.c_size_t)]),
    "bm_distance_field": (_i, [_vp, C.POINTER(bm_distance_params), _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_distance_times": (_i, [_vp, C.POINTER(bm_distance_params), _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_float)]),
    "bm_distance_mask": (_i, [_vp, C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp, _vp]),
    "bm_host_distance_field": (_i, [C.POINTER(bm_distance_params), _vp, _vp, C.POINTER(bm_distance_result)]),
    "bm_host_distance_mask": (_i, [C.c_uint64, _vp, C.c_uint32, C.c_uint32, _vp]),
    "bm_travel_workspace_bytes": (_i, [C.POINTER(bm_travel_params), C.POINTER(C.c_size_t)]),
    "bm_travel_field": (_i, [_vp, C.POINTER(bm_travel_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_travel_times": (_i, [_vp, C.POINTER(bm_travel_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "bm_travel_paths": (_i, [_vp, C.POINTER(C.c_int32), _vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp]),
    "bm_host_travel_field": (_i, [C.POINTER(bm_travel_params), _vp, _vp, C.c_int64, _vp, C.POINTER(bm_travel_result)]),
    "bm_host_travel_paths": (_i, [C.POINTER(C.c_int32), _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    "bm_settle_workspace_bytes": (_i, [C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_size_t)]),
    "bm_settle": (_i, [_vp, C.POINTER(C.c_int32), _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_uint32, _vp]),
    "bm_debug_settle_times": (_i, [_vp, C.POINTER(C.c_int32), _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_uint32, _vp, C.c_uint32, C.POINTER(C.c_float),
                                   C.POINTER(C.c_uint32)]),
    "bm_host_settle": (_i, [C.POINTER(C.c_int32), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.POINTER(bm_settle_result)]),
    "bm_foot_workspace_bytes": (_i, [C.POINTER(bm_foot_params), C.POINTER(C.c_size_t)]),
    "bm_foot_room": (_i, [_vp, C.POINTER(bm_foot_params), _vp, _vp, _vp]),
    "bm_foot_field": (_i, [_vp, C.POINTER(bm_foot_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_foot_times": (_i, [_vp, C.POINTER(bm_foot_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "bm_foot_paths": (_i, [_vp, C.POINTER(bm_foot_params), _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp]),
    "bm_host_foot_room": (_i, [C.POINTER(bm_foot_params), _vp, _vp]),
    "bm_host_foot_field": (_i, [C.POINTER(bm_foot_params), _vp, _vp, C.c_int64, _vp, C.POINTER(bm_foot_result)]),
    "bm_host_foot_paths": (_i, [C.POINTER(bm_foot_params), _vp, _vp, _vp, C.c_int64, C.c_int32, _vp, _vp]),
    "bm_water_workspace_bytes": (_i, [C.POINTER(bm_water_params), C.POINTER(C.c_size_t)]),
    "bm_water_field": (_i, [_vp, C.POINTER(bm_water_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_water_times": (_i, [_vp, C.POINTER(bm_water_params), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "bm_water_mask": (_i, [_vp, C.POINTER(C.c_int32), _vp, C.c_uint32, _vp, _vp]),
    "bm_host_water_field": (_i, [C.POINTER(bm_water_params), _vp, _vp, C.c_int64, _vp, C.POINTER(bm_water_result)]),
    "bm_host_water_mask": (_i, [C.POINTER(C.c_int32), _vp, C.c_uint32, _vp]),
    "bm_camera_pixel_rays": (_i, [C.POINTER(bm_camera), _i, _i, C.c_int64, _vp, _vp, _vp]),
    "bm_camera_pixel_rays_device": (_i, [_vp, C.POINTER(bm_camera), _i, _i, _vp, _vp]),
    "bm_denoise_workspace_bytes": (_i, [_i, _i, C.POINTER(C.c_size_t)]),
    "bm_denoise": (_i, [_vp, C.POINTER(bm_denoise_params), _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bm_debug_denoise_times": (_i, [_vp, C.POINTER(bm_denoise_params), _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.POINTER(C.c_float)]),
    "bm_host_denoise": (_i, [C.POINTER(bm_denoise_params), _vp, _vp, _vp]),
    "bm_history_bytes": (_i, [_i, _i, C.POINTER(C.c_size_t)]),
    "bm_reproject": (_i, [_vp, C.POINTER(bm_reproject_params), C.POINTER(bm_camera), C.POINTER(bm_camera), _vp, _vp, _vp, _vp, _vp]),
    "bm_host_reproject": (_i, [C.POINTER(bm_reproject_params), C.POINTER(bm_camera), C.POINTER(bm_camera), _vp, _vp, _vp, _vp]),
    "bm_host_column_heights": (_i, [_i, _i, _i, _i, _vp]),
    "bm_host_generate_supercell": (_i, [_i, _i, _i, _i, _i, _vp, _u32p, _vp, C.c_uint32]),
    "bm_host_edit_supercell": (_i, [_i, _i, _i, _i, _i, _vp, _u32p, _vp, C.c_uint32, _i, C.POINTER(bm_edit)]),
    "bm_host_write_region_supercell": (_i, [_i, _i, _i, _i, _i, _vp, _u32p, _vp, C.c_uint32, C.POINTER(bm_region), _i, _vp]),
    "bm_host_load_supercell": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _u32p]),
    "bm_host_cube_field": (_i, [_i, _i, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "bm_buffer_alloc": (_i, [_i, C.c_size_t, C.POINTER(_vp)]),
    "bm_buffer_free": (_i, [_i, _vp]),
    "bm_buffer_zero": (_i, [_i, _vp, C.c_size_t, _vp]),
    "bm_buffer_read": (_i, [_i, _vp, _vp, C.c_size_t]),
    "bm_buffer_write": (_i, [_i, _vp, _vp, C.c_size_t]),
    "bm_local_rows": (_i, [C.POINTER(bm_frame_params)]),
    "bm_render_frame": (_i, [_vp, C.POINTER(bm_camera), C.POINTER(bm_frame_params), _vp, _vp, _vp]),
    "bm_render_frames": (_i, [_vp, _i, C.POINTER(bm_camera), C.POINTER(bm_frame_params), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "bm_frame_plan_of": (_i, [C.POINTER(bm_frame_params), _i, C.POINTER(bm_frame_plan)]),
    "bm_launch_plan_of": (_i, [_i, C.POINTER(bm_camera), C.POINTER(bm_frame_params), _vp, _vp, _i, _i, C.POINTER(bm_launch_plan)]),
    "bm_trace_waves_per_simd": (_i, [_i, _i, _i, _i, C.POINTER(C.c_int)]),
    "bm_tuning_overrides": (_i, [C.c_char_p, C.c_size_t]),
    "bm_resolve": (_i, [_vp, _vp, _vp, C.c_int64, _vp]),
    "bm_synchronize": (_i, [_vp]),
    "bm_last_render_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "bm_render_times": (_i, [_vp, _vp, _i, C.POINTER(C.c_int)]),
    "bm_counters_read": (_i, [_vp, C.POINTER(bm_counters)]),
    "bm_counters_reset": (_i, [_vp]),
    "bm_sched_stats_read": (_i, [_vp, C.POINTER(bm_sched_stats)]),
    "bm_sched_detail_read": (_i, [_vp, _vp]),
    "bm_wavefront_create": (_i, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "bm_wavefront_destroy": (None, [_vp]),
    "bm_wavefront_reset": (_i, [_vp]),
    "bm_wavefront_frame": (_i, [_vp, C.POINTER(bm_camera), C.POINTER(bm_frame_params), _vp, _vp]),
    "bm_wavefront_stats": (_i, [_vp, _u32p]),
    "bm_wavefront_read_queue": (_i, [_vp, _i, C.c_uint32, C.c_uint32, _vp]),
    "bm_wavefront_times": (_i, [_vp, C.POINTER(C.c_float)]),
    "bm_wavefront_counters_read": (_i, [_vp, _i, C.POINTER(bm_counters)]),
    "bm_wavefront_counters_reset": (_i, [_vp]),
    "bm_wavefront_sched_stats_read": (_i, [_vp, _i, C.POINTER(C.c_uint64)]),
    "bm_comm_unique_id": (_i, [_vp]),
    "bm_comm_create": (_i, [_i, _i, _i, _vp, C.POINTER(_vp)]),
    "bm_comm_destroy": (None, [_vp]),
    "bm_comm_info": (_i, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bm_comm_available": (_i, []),
    "bm_debug_division_magic": (_i, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "bm_gather_frame": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "bm_gather_frames": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bm_reduce_frame": (_i, [_vp, _vp, _vp, C.c_int64, _i, _vp]),
    "bm_probe_streams": (_i, [_i, _i, C.POINTER(_vp)]),
    "bm_release_streams": (None, [_i, C.POINTER(_vp)]),
    "bm_comm_barrier": (_i, [_vp, _vp]),
    "bm_comm_selftest": (_i, [_vp, _vp]),
    "bm_debug_assemble_frame": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "bm_debug_sincos": (_i, [_i, _i, _vp, _vp, _vp]),
    "bm_debug_sky": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp]),
}

_lib = None


def load():
    """dlopen libbrickmap_hip.so and bind every C-ABI symbol.  Raises BrickmapError when the HIP
    extension is missing -- the product path never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BrickmapError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C brickmap_amd/csrc`. There is no CPU fallback.")
    import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first; see module docstring)
    try:
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise BrickmapError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(code):
    if code != 0:
        msg = load().bm_last_error_string()
        raise BrickmapError(f"brickmap error {code}: {msg.decode() if msg else ''}")


def size_call(name, *args):
    """the size_t that the library's `name`(*args, &size) reports"""
    out = C.c_size_t(0)
    check(getattr(load(), name)(*args, C.byref(out)))
    return int(out.value)


def stage_call(plain, timed, args, stages=None, before=(), after=()):
    """Issue an operator: plain(*args), or with `stages` its stage-timing twin timed(*args, *before, ms, *after), where ms is a float array
    of that many stages.  Returns the stage times in ms as a list, or None for the plain call."""
    if stages is None:
        return check(plain(*args))
    ms = (C.c_float * stages)()
    check(timed(*args, *before, ms, *after))
    return [float(v) for v in ms]
