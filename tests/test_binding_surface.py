"""The surface of the Python binding, pinned without a GPU and without loading the library: the public names of brickmap_amd and
brickmap_amd.host, the signature of every public callable, the record dtypes against their former hand-written spelling, and the one
layout of a dense volume in the four params structs.  The literal lists and tables were produced by running public_names() and surface()
below on the commit before the binding was split by subject (one host.py of 2 251 lines), so the split can be seen to have changed none.

public_names: every name of the module's namespace that does not start with an underscore, is not a module, and is not a class or
function of the standard library or numpy (dataclass, field, replace).  Signatures are str(inspect.signature(...)) with the module path
of the package's own annotations removed ("brickmap_amd.host.Camera" reads "Camera"): where a class lives is not part of its surface."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import brickmap_amd
from brickmap_amd import _lib, host
from brickmap_amd.volumes import _distance_params, _mesh_params, _travel_params, _voxelize_params, dense_layout


def public_names(mod):
    out = []
    for n, v in vars(mod).items():
        if n.startswith("_") or inspect.ismodule(v):
            continue
        if (inspect.isclass(v) or inspect.isroutine(v)) and not v.__module__.startswith("brickmap_amd"):
            continue
        out.append(n)
    return sorted(out)


def sig(f):
    return re.sub(r"brickmap_amd\.\w+\.", "", str(inspect.signature(f)))


CLASSES = ("Scene", "Components", "VoxelizeResult", "Quads", "DistanceField", "TravelField", "History", "TemporalAccumulator", "Wavefront", "State")


def class_surface(cls):
    out = {}
    for n, v in inspect.getmembers(cls):
        if n.startswith("_") and n != "__init__":
            continue
        if isinstance(inspect.getattr_static(cls, n), property):
            out[n] = "property"
        elif callable(v):
            out[n] = sig(v)
    return out


def surface(mod):
    table = {c: class_surface(getattr(mod, c)) for c in CLASSES}
    table["functions"] = {n: sig(getattr(mod, n)) for n in public_names(mod) if inspect.isfunction(getattr(mod, n))}
    return table


PACKAGE_NAMES = [
    'BM_DISTANCE_MASK_ABOVE', 'BM_DISTANCE_NONE', 'BM_DISTANCE_OUTSIDE', 'BM_DISTANCE_TO_EMPTY', 'BM_EDIT_BOX', 'BM_EDIT_CLEAR', 'BM_EDIT_SET',
    'BM_EDIT_SPHERE', 'BM_FLAG_COUNTERS', 'BM_FLAG_ORDERED', 'BM_FLAG_PRIMARY_ONLY', 'BM_FLAG_RAY_DIGEST', 'BM_FLAG_SAMPLE_ITEMS', 'BM_MESH_HALO',
    'BM_MESH_UNIT_FACES', 'BM_QUERY_LOD', 'BM_QUERY_NO_REQUESTS', 'BM_REGION_REPLACE', 'BM_TRAVEL_NONE', 'BM_VOLUME_ANY', 'BM_VOXELIZE_KEEP',
    'BM_VOXELIZE_SOLID', 'BM_VOXELIZE_SURFACE', 'BM_VOXELS_DEVICE', 'BM_VOXELS_HOST', 'BRICK_INDEX_BITS', 'BRICK_LOADED_BIT', 'BRICK_LOD_BITS',
    'BRICK_REQUESTED_BIT', 'BRICK_UNLOADED_BIT', 'BrickmapError', 'COMPONENT_DTYPE', 'Camera', 'Components', 'DISTANCE_NONE', 'DISTANCE_RESULT_DTYPE',
    'DistanceField', 'FLYTHROUGH_VIEWS', 'FrameParams', 'History', 'MESH_RESULT_DTYPE', 'QUAD_DTYPE', 'Quads', 'RAY_DTYPE', 'RAY_HIT_DTYPE',
    'RAY_QUEUE_DTYPE', 'RayHit', 'RayHits', 'SHADOW_QUEUE_DTYPE', 'Scene', 'State', 'TRAVEL_NONE', 'TRAVEL_RESULT_DTYPE', 'TemporalAccumulator',
    'TravelField', 'VOLUME_DTYPE', 'VOLUME_RESULT_DTYPE', 'VOXELIZE_RESULT_DTYPE', 'VolumeResults', 'VoxelizeResult', 'Wavefront', 'bm_region',
    'camera_pixel_rays', 'denoise_workspace_bytes', 'distance_workspace_bytes', 'edit_box', 'edit_sphere', 'flythrough_camera', 'frame_plan',
    'history_bytes', 'host_column_heights', 'host_cube_field', 'host_denoise', 'host_distance_field', 'host_distance_mask', 'host_edit_supercell',
    'host_generate_supercell', 'host_label_volume', 'host_load_supercell', 'host_mesh_quads', 'host_mesh_triangles', 'host_reproject',
    'host_travel_field', 'host_travel_paths', 'host_voxelize', 'host_write_region_supercell', 'launch_kernels', 'launch_plan', 'load', 'local_rows',
    'mesh_workspace_bytes', 'pack_rays', 'probe_streams', 'region_of', 'release_streams', 'trace_waves_per_simd', 'travel_workspace_bytes',
    'tuning_overrides', 'volume_box', 'volume_dims', 'volume_sphere', 'voxelize_workspace_bytes']
PACKAGE_ALL = ['BrickmapError', 'Camera', 'FrameParams', 'Scene', 'State', 'Wavefront', 'dist', 'launch_kernels', 'load', 'local_rows']
HOST_NAMES = [
    'BM_EDIT_BOX', 'BM_EDIT_CLEAR', 'BM_EDIT_SET', 'BM_EDIT_SPHERE', 'BM_QUERY_LOD', 'BM_QUERY_NO_REQUESTS', 'BM_REGION_REPLACE', 'BM_VOLUME_ANY',
    'BM_VOXELS_DEVICE', 'BM_VOXELS_HOST', 'COMPONENT_DTYPE', 'Camera', 'Components', 'DISTANCE_NONE', 'DISTANCE_RESULT_DTYPE', 'DistanceField',
    'FACE_BITS', 'FLYTHROUGH_VIEWS', 'FrameParams', 'History', 'MESH_RESULT_DTYPE', 'QUAD_DTYPE', 'Quads', 'RAY_DTYPE', 'RAY_HIT_DTYPE',
    'RAY_QUEUE_DTYPE', 'RayHit', 'RayHits', 'SHADOW_QUEUE_DTYPE', 'Scene', 'State', 'TRAVEL_NONE', 'TRAVEL_RESULT_DTYPE', 'TemporalAccumulator',
    'TravelField', 'VOLUME_DTYPE', 'VOLUME_RESULT_DTYPE', 'VOXELIZE_RESULT_DTYPE', 'VolumeResults', 'VoxelizeResult', 'Wavefront', 'bm_camera',
    'bm_counters', 'bm_edit', 'bm_frame_params', 'bm_region', 'bm_scene_info', 'camera_pixel_rays', 'check', 'denoise_workspace_bytes',
    'distance_workspace_bytes', 'edit_box', 'edit_sphere', 'flythrough_camera', 'frame_plan', 'history_bytes', 'host_column_heights', 'host_cube_field',
    'host_denoise', 'host_distance_field', 'host_distance_mask', 'host_edit_supercell', 'host_generate_supercell', 'host_label_volume',
    'host_load_supercell', 'host_mesh_quads', 'host_mesh_triangles', 'host_reproject', 'host_travel_field', 'host_travel_paths', 'host_voxelize',
    'host_write_region_supercell', 'launch_kernels', 'launch_plan', 'local_rows', 'mesh_workspace_bytes', 'pack_rays', 'probe_streams', 'region_of',
    'release_streams', 'trace_waves_per_simd', 'travel_workspace_bytes', 'tuning_overrides', 'volume_box', 'volume_dims', 'volume_sphere',
    'voxelize_workspace_bytes']
SURFACE = {
    'Components': {'__init__': '(self, scene, lo, hi, labels, records, table)',
                   'floating': "(self, anchor=('-x', '+x', '-y', '+y', '-z'), stream=None)",
                   'loose': "(self, anchor=('-x', '+x', '-y', '+y', '-z'))",
                   'mask': '(self, chosen, stream=None)'},
    'DistanceField': {'__init__': '(self, scene, field, result)',
                      'largest': '(self)',
                      'mask': '(self, radius_sq, above=False, out=None, stream=None)',
                      'record': 'property',
                      'sources': 'property'},
    'History': {'__init__': '(self, buffer, width, height)'},
    'Quads': {'__init__': '(self, scene, packed, result, record=None)',
              'count': 'property',
              'faces': 'property',
              'record': 'property',
              'records': 'property',
              'triangles': '(self, stream=None)'},
    'Scene': {'__init__': '(self, grid_size=4096, grid_height=512, device=0)',
              'carve_sphere': '(self, center, radius, stream=None)',
              'cast_rays': '(self, origins, directions=None, tmax=None, lod_origin=None, request=True, stream=None)',
              'cast_rays_raw': '(self, n, rays_ptr, hits_ptr, flags=0, lod_origin=None, stream=None)',
              'clear_box': '(self, lo, hi, stream=None)',
              'clearance': '(self, lo, hi, stream=None)',
              'close': '(self)',
              'column_heights': '(self, sx, sy)',
              'components': '(self, lo, hi, stream=None)',
              'count_box': '(self, lo, hi)',
              'count_sphere': '(self, center, radius)',
              'counters': '(self)',
              'counters_reset': '(self)',
              'denoise': '(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None)',
              'denoise_times': '(self, accum, hits, width, height, iterations=5, sigma_l=4.0, out=None, stream=None)',
              'device_brick': '(self, sc, device_slot)',
              'device_cube_field': '(self)',
              'device_indices': '(self, sc)',
              'distance_field': "(self, volume, to='solid', outside=False, out=None, stream=None)",
              'distance_field_times': "(self, volume, to='solid', outside=False, out=None, stream=None)",
              'dump': "(self, path='dump.txt')",
              'edit': '(self, edits, stream=None)',
              'escape_table': '(self)',
              'extract_mesh': '(self, lo, hi, closed=True, unit=False, stream=None)',
              'fill_box': '(self, lo, hi, stream=None)',
              'fill_sphere': '(self, center, radius, stream=None)',
              'find_path': '(self, start, goal, lo=None, hi=None, clearance_sq=0, max_steps=0, stream=None)',
              'from_voxels': '(volume, device=0)',
              'generate': '(self, threads=None)',
              'generate_supercell': '(self, start_x, start_y, start_z)',
              'grow': '(self, lo, hi, radius_sq, stream=None)',
              'host_cube_field': '(self)',
              'host_supercell': '(self, sc)',
              'info': '(self)',
              'is_free': '(self, lo, hi)',
              'label_components_raw': '(self, lo, hi, labels_ptr, comps_ptr, capacity, stream=None)',
              'label_mask_raw': '(self, lo, hi, labels_ptr, comps_ptr, n, chosen_ptr, mask_ptr, stream=None)',
              'label_region': '(self, lo, hi, out=None, stream=None)',
              'label_region_raw': '(self, lo, hi, labels_ptr, count_ptr, flags=0, stream=None)',
              'last_edit_ms': '(self)',
              'last_label_ms': '(self)',
              'last_load_ms': '(self)',
              'last_region_ms': '(self)',
              'last_render_ms': '(self)',
              'load_voxels': '(self, volume, stream=None)',
              'mesh_quads': '(self, volume, lo=(0, 0, 0), halo=False, unit=False, capacity=None, stream=None)',
              'mesh_quads_times': '(self, volume, lo=(0, 0, 0), halo=False, unit=False, capacity=None, stream=None)',
              'pick': '(self, camera, x, y, width, height, lod_origin=None)',
              'pixel_hits': "(self, camera, width, height, lod_origin='camera', stream=None)",
              'pixel_rays': '(self, camera, width, height, stream=None)',
              'preload_all': '(self)',
              'process_load_queue': '(self)',
              'query_volumes': '(self, volumes, any=False, stream=None)',
              'query_volumes_raw': '(self, n, volumes_ptr, results_ptr, flags=0, stream=None)',
              'reach': '(self, lo, hi, seeds, clearance_sq=0, max_steps=0, stream=None)',
              'read_region': '(self, lo, hi, out=None, device=False, stream=None)',
              'remove_floating': "(self, lo, hi, anchor=('-x', '+x', '-y', '+y', '-z'))",
              'render': '(self, camera: Camera, params: FrameParams, accum, debug=None, stream=None)',
              'render_frames': '(self, cameras, params, accums, debugs=None, stream=None)',
              'render_times': '(self, capacity=256)',
              'reproject': '(self, accum, hits, camera, prev_camera, history_prev, width, height, max_history=32.0, out=None, stream=None)',
              'reset_residency': '(self)',
              'resolve': '(self, accum, out=None, stream=None)',
              'sched_detail': '(self)',
              'sched_stats': '(self)',
              'set_lod': '(self, lod_distance_8x8x8=600000, lod_distance_2x2x2=100000)',
              'set_queue_capacity': '(self, capacity)',
              'set_streaming_mode': '(self, overlapped)',
              'set_voxels': '(self, coords, values, stream=None)',
              'shadow_heights': '(self)',
              'shrink': '(self, lo, hi, radius_sq, stream=None)',
              'sun_plane': '(self)',
              'sun_plane_stats': '(self)',
              'sweep_box': '(self, lo, hi, axis, sign, max_distance)',
              'synchronize': '(self)',
              'travel_field': '(self, volume, seeds, max_steps=0, out=None, stream=None)',
              'travel_field_times': '(self, volume, seeds, max_steps=0, out=None, stream=None, batch=0)',
              'view_plane': '(self)',
              'view_plane_stats': '(self)',
              'voxelize': "(self, triangles, lo, shape=None, mode='solid+surface', keep=False, out=None, stream=None)",
              'voxelize_times': "(self, triangles, lo, shape=None, mode='solid+surface', keep=False, out=None, stream=None)",
              'voxels': '(self)',
              'write_mesh': "(self, triangles, op='set', mode='solid+surface', stream=None)",
              'write_region': "(self, lo, volume, op='replace', stream=None)"},
    'State': {'__init__': '(self, screen_width, screen_height, device=0, band_rows=0, shard_rank=0, shard_count=1)',
              'screen_resize': '(self, screen_width, screen_height)'},
    'TemporalAccumulator': {'__init__': '(self, scene, width, height, max_history=32.0)',
                            'add': '(self, camera, accum, hits=None)',
                            'history': 'property',
                            'reset': '(self)'},
    'TravelField': {'__init__': '(self, scene, field, result)',
                    'path': '(self, start)',
                    'paths': '(self, starts, capacity, stream=None)',
                    'reached': 'property',
                    'record': 'property'},
    'VoxelizeResult': {'__init__': '(self, packed)', 'degenerate': 'property', 'open_columns': 'property', 'record': 'property', 'rejected': 'property'},
    'Wavefront': {'__init__': '(self, scene: Scene, queue_size=2097152)',
                  'close': '(self)',
                  'counters': "(self, which='both')",
                  'counters_reset': '(self)',
                  'frame': '(self, camera: Camera, params: FrameParams, accum, stream=None)',
                  'read_queue': '(self, which, first=0, count=None)',
                  'reset': '(self)',
                  'sched_stats': "(self, which='extend')",
                  'stats': '(self)',
                  'times': '(self)'},
    'functions': {'camera_pixel_rays': '(camera, width, height, px, py)',
                  'check': '(code)',
                  'denoise_workspace_bytes': '(width, height)',
                  'distance_workspace_bytes': '(shape)',
                  'edit_box': '(op, lo, hi)',
                  'edit_sphere': '(op, center, radius)',
                  'flythrough_camera': '(i)',
                  'frame_plan': '(params: FrameParams, hit_records=False)',
                  'history_bytes': '(width, height)',
                  'host_column_heights': '(grid_size, grid_height, sx, sy)',
                  'host_cube_field': '(grid_size, grid_height)',
                  'host_denoise': '(accum, hits, width=None, height=None, iterations=5, sigma_l=4.0, flags=0, reserved=0)',
                  'host_distance_field': "(volume, to='solid', outside=False)",
                  'host_distance_mask': '(field, limit_sq, above=False)',
                  'host_edit_supercell': '(grid_size, grid_height, sx, sy, sz, indices, bricks, edits)',
                  'host_generate_supercell': '(grid_size, grid_height, sx, sy, sz)',
                  'host_label_volume': '(volume)',
                  'host_load_supercell': '(volume, sx, sy, sz)',
                  'host_mesh_quads': '(volume, lo=(0, 0, 0), halo=False, unit=False)',
                  'host_mesh_triangles': '(quads)',
                  'host_reproject': '(accum, hits, camera, prev_camera=None, history_prev=None, width=None, height=None, max_history=32.0, flags=0, '
                                    'reserved=0)',
                  'host_travel_field': '(volume, seeds, max_steps=0)',
                  'host_travel_paths': '(field, starts, capacity)',
                  'host_voxelize': "(triangles, lo, shape=None, mode='solid+surface', keep=False, out=None)",
                  'host_write_region_supercell': "(grid_size, grid_height, sx, sy, sz, indices, bricks, lo, volume, op='replace')",
                  'launch_kernels': '(state: State, blit_buffer, gpuScene: Scene, camera: Camera, spp=1, max_bounces=3, flags=0, sun_position=None, '
                                    "statics=None, queues: 'Wavefront' = None)",
                  'launch_plan': '(cameras, params, accum_ptrs, debug_ptrs=None, grid_size=256, grid_height=256)',
                  'local_rows': '(params: FrameParams) -> int',
                  'mesh_workspace_bytes': '(shape, halo=False, lo=(0, 0, 0))',
                  'pack_rays': '(origins, directions, tmax=None)',
                  'probe_streams': '(count, device=0)',
                  'region_of': "(lo, volume, name='volume')",
                  'release_streams': '(handles)',
                  'trace_waves_per_simd': '(instrumented=False, xcd_handout=False, helpers=True, device=0)',
                  'travel_workspace_bytes': '(shape)',
                  'tuning_overrides': '()',
                  'volume_box': '(lo, hi)',
                  'volume_dims': '(volume, grid_size=None, grid_height=None)',
                  'volume_sphere': '(center, radius)',
                  'voxelize_workspace_bytes': "(shape, n, mode='solid+surface')"}}

# the former hand-written spelling of every record dtype that is now derived from its ctypes structure
FORMER_DTYPES = {
    "RAY_DTYPE": ("bm_ray", [("origin", "<f4", 3), ("direction", "<f4", 3), ("tmax", "<f4"), ("reserved", "<u4")]),
    "RAY_HIT_DTYPE": ("bm_ray_hit", [("distance", "<f4"), ("normal", "<f4", 3), ("voxel", "<i4", 3), ("level", "<i4")]),
    "VOLUME_DTYPE": ("bm_volume", [("shape", "<i4"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("center", "<i4", 3), ("radius", "<i4"), ("reserved", "<u4")]),
    "VOLUME_RESULT_DTYPE": ("bm_volume_result", [("solid", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("unresolved", "<u4"), ("status", "<u4")]),
    "COMPONENT_DTYPE": ("bm_component", [("label", "<i4"), ("faces", "<u4"), ("voxels", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3)]),
    "VOXELIZE_RESULT_DTYPE": ("bm_voxelize_result", [("rejected", "<u4"), ("degenerate", "<u4"), ("open_columns", "<u8")]),
    "QUAD_DTYPE": ("bm_quad", [("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("shape", "<u4")]),
    "MESH_RESULT_DTYPE": ("bm_mesh_result", [("quads", "<u8"), ("faces", "<u8")]),
    "DISTANCE_RESULT_DTYPE": ("bm_distance_result", [("sources", "<u8"), ("max_sq", "<u4"), ("reserved0", "<u4"), ("max_at", "<u8"), ("reserved1", "<u8")]),
    "TRAVEL_RESULT_DTYPE": ("bm_travel_result", [("reached", "<u8"), ("farthest", "<u4"), ("seeds_rejected", "<u4"), ("farthest_at", "<u8"), ("reserved", "<u8")]),
}
FORMER_SIZES = {"RAY_DTYPE": 32, "RAY_HIT_DTYPE": 32, "VOLUME_DTYPE": 48, "VOLUME_RESULT_DTYPE": 40, "COMPONENT_DTYPE": 40, "VOXELIZE_RESULT_DTYPE": 16,
                "QUAD_DTYPE": 16, "MESH_RESULT_DTYPE": 16, "DISTANCE_RESULT_DTYPE": 32, "TRAVEL_RESULT_DTYPE": 32}


def test_public_names_are_those_before_the_split():
    assert public_names(brickmap_amd) == PACKAGE_NAMES
    assert sorted(brickmap_amd.__all__) == PACKAGE_ALL
    assert public_names(host) == HOST_NAMES


def test_signatures_are_those_before_the_split():
    got = surface(host)
    assert sorted(got) == sorted(SURFACE)
    for owner, table in SURFACE.items():
        assert got[owner] == table, owner
    for name in PACKAGE_NAMES:   # the package offers the very objects of brickmap_amd.host
        if hasattr(host, name):
            assert getattr(brickmap_amd, name) is getattr(host, name), name


@pytest.mark.parametrize("name", sorted(FORMER_DTYPES))
def test_derived_dtype_equals_its_former_spelling(name):
    struct, fields = FORMER_DTYPES[name]
    derived, former = getattr(host, name), np.dtype(fields)
    assert derived == former
    assert derived.names == former.names and [derived.fields[n][1] for n in derived.names] == [former.fields[n][1] for n in former.names]
    assert derived.itemsize == former.itemsize == FORMER_SIZES[name] == ctypes.sizeof(getattr(_lib, struct))


def four_params(lo, volume):
    return {"voxelize": _voxelize_params(lo, volume, "solid", False)[0], "mesh": _mesh_params(lo, volume, False, False)[0],
            "distance": _distance_params(volume, "solid", False)[0], "travel": _travel_params(volume, 0)[0]}


LAYOUT_VOLUMES = {"slice": np.zeros((6, 7, 9), np.uint8)[1:4, 2:6, 3:8], "1x1x1": np.zeros((1, 1, 1), np.uint8), "1x4x1": np.zeros((1, 4, 1), np.bool_),
                  "3x1x5": np.zeros((3, 1, 5), np.uint8), "empty": np.zeros((0, 4, 5), np.uint8)}


@pytest.mark.parametrize("case", sorted(LAYOUT_VOLUMES))
def test_one_layout_in_the_four_params_structs(case):
    volume, lo = LAYOUT_VOLUMES[case], (3, -5, 7)
    nz, ny, nx = volume.shape
    region, ptr, cuda = brickmap_amd.region_of(lo, volume)
    assert not cuda and tuple(region.lo) == lo and tuple(region.hi) == (3 + nx, -5 + ny, 7 + nz)
    if case == "slice":
        assert (region.row_pitch, region.slice_pitch) == (9, 63) and ptr == volume.ctypes.data
    for name, par in four_params(lo, volume).items():
        assert tuple(par.extent) == (nx, ny, nz), name
        assert (par.row_pitch, par.slice_pitch) == (region.row_pitch, region.slice_pitch), name
        assert hasattr(par, "lo") == (name in ("voxelize", "mesh")), name
        if hasattr(par, "lo"):
            assert tuple(par.lo) == lo, name
        again = dense_layout(type(par)(), region)   # the function itself, on an empty struct: nothing but the layout is filled
        assert (tuple(again.extent), again.row_pitch, again.slice_pitch) == ((nx, ny, nz), region.row_pitch, region.slice_pitch), name
        assert again.flags == 0 and (not hasattr(again, "lo") or tuple(again.lo) == lo), name


def test_layout_near_the_end_of_32_bits():
    """hi = lo + extent wraps in the region's 32-bit fields; the extent that reaches the params struct does not"""
    volume = np.zeros((2, 3, 5), np.uint8)
    for par in four_params((2**31 - 2, 2**31 - 1, -2**31), volume).values():
        assert tuple(par.extent) == (5, 3, 2)


@pytest.mark.parametrize("bad", ["x_strided", "negative_y", "negative_z"])
def test_layouts_that_are_refused_stay_refused(bad):
    base = np.zeros((6, 7, 10), np.uint8)
    volume = {"x_strided": base[:, :, ::2], "negative_y": base[:, ::-1, :], "negative_z": base[::-1]}[bad]
    with pytest.raises(ValueError):
        brickmap_amd.region_of((0, 0, 0), volume)
    for make in (lambda: _voxelize_params((0, 0, 0), volume, "solid", False), lambda: _mesh_params((0, 0, 0), volume, False, False),
                 lambda: _distance_params(volume, "solid", False), lambda: _travel_params(volume, 0)):
        with pytest.raises(ValueError):
            make()
