"""octree_slam_amd -- Python front end of libsvoslam_hip.so (include/svoslam.h).

The product is the C-ABI shared library built from csrc/*.hip for gfx950; this
package only binds it with ctypes and moves pointers of torch CUDA tensors
across the boundary (PyTorch = device memory, streams, torch.distributed).
There is NO CPU fallback: every compute entry point raises SvoslamError when
the library or a gfx950 device is missing.

The directory is called ``octree-slam_amd`` (not importable by name); load it
with ``svoslam_pkg.load()`` from the repo root, which registers it as the module
``octree_slam_amd``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsvoslam_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "svoslam.h")

MAX_DEPTH = 16
FLAG_CHILDREN = 0x40000000
CHILD_MASK = 0x3FFFFFFF
RENDER_REFERENCE = 0
RENDER_CARRY = 1
PYRAMID_ITERS = (10, 5, 4)  # rgbd_camera.cpp:19, index = pyramid level
DELTA_FLOATS = 20  # SVOSLAM_DELTA_FLOATS: update_trans[16], levels lost (int32 bits), 3 x padding


class SvoslamError(RuntimeError):
    pass


def build(verbose=False, force=False):
    """Compile csrc/*.hip for gfx950 into libsvoslam_hip.so (hipcc, in tree)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_svoslam_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=verbose, force=force)


class _PoolStruct(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("size", C.c_int32), ("capacity", C.c_int32), ("d_size", C.c_void_p),
                ("pending", C.c_int32), ("pending_bound", C.c_int64), ("tracker", C.c_void_p)]


class _ReachStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("tile_runs", C.c_int32), ("seeds_used", C.c_int32)]


class _OwnerStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("tile_runs", C.c_int32), ("seeds_used", C.c_int32), ("owner_rounds", C.c_int32),
                ("owner_tile_runs", C.c_int32)]


class _PlanStats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("tile_runs", C.c_int32), ("seeds_used", C.c_int32), ("max_weight", C.c_int32)]


class _GroundStats(C.Structure):
    _fields_ = [("footholds", C.c_int32), ("seeds_used", C.c_int32), ("rounds", C.c_int32), ("tile_runs", C.c_int32)]


class _ComponentStats(C.Structure):
    _fields_ = [("components", C.c_int32), ("largest", C.c_int32), ("tile_passes", C.c_int32), ("unions", C.c_int32)]


class MeshStruct(C.Structure):
    _fields_ = [("vbo", C.POINTER(C.c_float)), ("tbo", C.POINTER(C.c_float)), ("n_tris", C.c_int32), ("tbosize", C.c_int32),
                ("bbox0", C.c_float * 3), ("bbox1", C.c_float * 3)]


class TextureStruct(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("width", C.c_int32), ("height", C.c_int32)]


class FuseStats(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("num_split", C.c_int32), ("pass_sizes", C.c_int32 * (MAX_DEPTH + 1)),
                ("pool_size_before", C.c_int32), ("pool_size_after", C.c_int32)]


class CompactStats(C.Structure):
    _fields_ = [("size_before", C.c_int32), ("size_after", C.c_int32), ("capacity_before", C.c_int32), ("capacity_after", C.c_int32),
                ("levels", C.c_int32), ("tiles_dropped", C.c_int32)]


class AccelView(C.Structure):
    """include/svoslam.h svoslam_accel_view"""
    _fields_ = ([("grid", C.c_void_p), ("bricks", C.c_void_p), ("brick_touched", C.c_void_p), ("dirty", C.c_void_p * 2)] +
                [(n, C.c_int32) for n in ("valid", "bricks_valid", "brick_shift", "mip_consistent", "max_depth", "deferred_pending",
                                          "bricks_failed")] +
                [("epoch", C.c_uint32), ("node0_served", C.c_uint32), ("brick_served", C.c_uint32 * 2)] +
                [(n, C.c_int32) for n in ("dirty_words", "list_offset", "count_offset", "node0_offset", "brick_count_offset",
                                          "brick_list_offset", "brick_list_cap", "brick_bits_offset", "brick_bits_words",
                                          "sib_count_offset", "sib_list_offset", "sib_list_cap", "state_words")])


class SurfaceStats(C.Structure):
    _fields_ = [("cells", C.c_int32), ("faces", C.c_int32), ("vertices", C.c_int32)]


_lib = None
_vp, _i32, _f32 = C.c_void_p, C.c_int32, C.c_float
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); this table is also what tests/test_abi_symbols.py checks against include/svoslam.h
SIGNATURES = {
    "svoslam_abi_version": (C.c_int, []),
    "svoslam_config_get": (C.c_int, [C.c_void_p]),
    "svoslam_config_set": (C.c_int, [C.c_void_p]),
    "svoslam_status_string": (C.c_char_p, [C.c_int]),
    "svoslam_last_error": (C.c_char_p, []),
    "svoslam_device_arch": (C.c_char_p, []),
    "svoslam_pool_init": (C.c_int, [C.POINTER(_PoolStruct), _i32, _vp]),
    "svoslam_pool_reserve": (C.c_int, [C.POINTER(_PoolStruct), _i32, _vp]),
    "svoslam_pool_free": (C.c_int, [C.POINTER(_PoolStruct)]),
    "svoslam_pool_sync": (C.c_int, [C.POINTER(_PoolStruct), _vp]),
    "svoslam_pool_reset": (C.c_int, [C.POINTER(_PoolStruct), _vp]),
    "svoslam_pool_expand": (C.c_int, [C.POINTER(_PoolStruct), _fp, C.POINTER(_f32), _fp, _vp]),
    "svoslam_camera_reset": (C.c_int, [_vp]),
    "svoslam_pool_save": (C.c_int, [C.POINTER(_PoolStruct), C.c_char_p, _fp, _f32, _i32, _vp]),
    "svoslam_pool_touch": (C.c_int, [C.POINTER(_PoolStruct)]),
    "svoslam_pool_march_accel": (C.c_int, [C.POINTER(_PoolStruct), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "svoslam_pool_accel_view": (C.c_int, [C.POINTER(_PoolStruct), C.POINTER(AccelView)]),
    "svoslam_pool_set_nodes": (C.c_int, [C.POINTER(_PoolStruct), C.POINTER(C.c_uint32), _i32, _vp]),
    "svoslam_pool_evict_subtree": (C.c_int, [C.POINTER(_PoolStruct), C.POINTER(C.c_uint8), _i32, C.c_char_p, _vp]),
    "svoslam_pool_restore_subtree": (C.c_int, [C.POINTER(_PoolStruct), C.c_char_p, _vp]),
    "svoslam_pool_graft_subtree": (C.c_int, [C.POINTER(_PoolStruct), C.c_char_p, _vp]),
    "svoslam_pool_compact": (C.c_int, [C.POINTER(_PoolStruct), _i32, _vp, C.POINTER(CompactStats), _vp]),
    "svoslam_subtree_file_nodes": (C.c_int, [C.c_char_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(_i32)]),
    "svoslam_pool_copy": (C.c_int, [C.POINTER(_PoolStruct), C.POINTER(_PoolStruct), _vp]),
    "svoslam_pool_load": (C.c_int, [C.POINTER(_PoolStruct), C.c_char_p, _fp, C.POINTER(_f32), C.POINTER(_i32), _vp]),
    "svoslam_svo_from_point_cloud_async": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _fp, _f32, _vp]),
    "svoslam_svo_fuse_sort": (C.c_int, [_vp, _vp, _i32, _i32, _fp, _f32, _vp]),
    "svoslam_svo_fuse_sort_frame": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _f32, _f32, _i32, _fp, _f32, _vp, _vp]),
    "svoslam_svo_fuse_plan": (C.c_int, [_vp, _i32, _i32, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_commit": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_split_early": (C.c_int, [_vp, _i32, _i32, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_plan_structure": (C.c_int, [_vp, _i32, _i32, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_adopt_sorted": (C.c_int, [_vp, _vp, _vp, _i32, _i32]),
    "svoslam_svo_fuse_sort_frame_band": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _f32, _f32, _i32, _fp, _f32, _i32, _i32, _vp]),
    "svoslam_svo_fuse_merge_sorted": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), _i32, _vp, _vp, _vp]),
    "svoslam_svo_fuse_export_sorted": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "svoslam_pool_structure_begin": (C.c_int, [C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_commit_deferred": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_apply": (C.c_int, [_vp, C.POINTER(_PoolStruct), _vp]),
    "svoslam_svo_fuse_keyrange_commit": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _i32, _i32, _vp, C.c_int64, _vp]),
    "svoslam_svo_fuse_keyrange_apply": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), C.POINTER(C.c_void_p), _i32, _vp]),
    "svoslam_svo_fuse_keyrange_status": (C.c_int, [_vp, C.POINTER(C.c_int32), _vp]),
    "svoslam_svo_fuse_keyrange_discard": (C.c_int, [_vp, C.POINTER(_PoolStruct)]),
    "svoslam_frame_reader_open": (C.c_int, [C.POINTER(_vp), C.c_char_p, _f32]),
    "svoslam_frame_reader_close": (C.c_int, [_vp]),
    "svoslam_frame_reader_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "svoslam_frame_reader_rewind": (C.c_int, [_vp]),
    "svoslam_frame_reader_next_host": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_longlong), C.POINTER(_i32)]),
    "svoslam_frame_reader_next": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_longlong), C.POINTER(_i32), _vp]),
    "svoslam_focal_from_fov": (C.c_int, [_i32, _i32, _f32, _f32, _fp, _fp]),
    "svoslam_image_load": (C.c_int, [C.c_char_p, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "svoslam_workspace_create": (C.c_int, [C.POINTER(_vp)]),
    "svoslam_workspace_destroy": (C.c_int, [_vp]),
    "svoslam_svo_from_point_cloud": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _fp, _f32,
                                                C.POINTER(FuseStats), _vp]),
    "svoslam_svo_from_voxel_grid": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.POINTER(_PoolStruct), _fp, _f32,
                                               C.POINTER(FuseStats), _vp]),
    "svoslam_extract_voxel_grid": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, _fp, _f32, C.POINTER(_vp),
                                              C.POINTER(_vp), C.POINTER(_i32), _vp]),
    "svoslam_mesh_load_obj": (C.c_int, [C.c_char_p, C.POINTER(MeshStruct)]),
    "svoslam_mesh_free": (C.c_int, [C.POINTER(MeshStruct)]),
    "svoslam_texture_load_bmp": (C.c_int, [C.c_char_p, C.POINTER(TextureStruct)]),
    "svoslam_texture_free": (C.c_int, [C.POINTER(TextureStruct)]),
    "svoslam_mesh_to_voxel_grid": (C.c_int, [_vp, C.POINTER(MeshStruct), C.POINTER(TextureStruct), _i32, _i32, C.POINTER(_vp),
                                             C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), _fp, _vp]),
    "svoslam_mesh_last_fragments": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "svoslam_voxel_grid_to_mesh": (C.c_int, [_vp, _vp, _vp, _i32, _f32, _fp, _i32, C.POINTER(C.c_int32), _i32, _fp, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t]),
    "svoslam_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t]),
    "svoslam_runner_run_model": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_longlong), _fp, _i32, _vp, _i32, _i32, _vp,
                                           _f32, C.POINTER(_i32), _vp]),
    "svoslam_runner_create": (C.c_int, [C.POINTER(_vp), _vp, C.POINTER(_PoolStruct), _i32, _i32, _i32, _fp, _f32, _f32, _f32, _i32]),
    "svoslam_runner_destroy": (C.c_int, [_vp]),
    "svoslam_runner_timeline": (C.c_int, [_vp, _fp, _i32, C.POINTER(_i32)]),
    "svoslam_runner_run": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_longlong), _fp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "svoslam_runner_bbox": (C.c_int, [_vp, _fp]),
    "svoslam_runner_run_sharded": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_longlong), _fp, _i32, C.POINTER(_vp),
                                             C.POINTER(_vp), C.POINTER(C.c_uint8), C.POINTER(_vp), _i32, _i32, _vp, _vp]),
    "svoslam_runner_run_sharded_presorted": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_longlong), _fp, _i32, C.POINTER(_vp),
                                                       C.POINTER(_vp), C.POINTER(C.c_uint8), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                                       C.POINTER(_vp), _i32, _i32, _vp, _vp]),
    "svoslam_mailbox_create": (C.c_int, [C.POINTER(_vp), _i32, _i32]),
    "svoslam_mailbox_destroy": (C.c_int, [_vp]),
    "svoslam_mailbox_handle": (C.c_int, [_vp, _vp]),
    "svoslam_mailbox_connect": (C.c_int, [_vp, _vp]),
    "svoslam_mailbox_connect_local": (C.c_int, [_vp, C.POINTER(_vp)]),
    "svoslam_mailbox_all_gather": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "svoslam_mailbox_all_reduce_f64": (C.c_int, [_vp, _vp, _i32, _vp]),
    "svoslam_mailbox_failed": (C.c_int, [_vp, C.POINTER(_i32)]),
    "svoslam_mailbox_set_wait_limit": (C.c_int, [_vp, C.c_uint32]),
    "svoslam_mailbox_post": (C.c_int, [_vp, _vp, _i32, _vp]),
    "svoslam_mailbox_collect": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_scene_create": (C.c_int, [C.POINTER(_vp)]),
    "svoslam_scene_destroy": (C.c_int, [_vp]),
    "svoslam_scene_load_obj": (C.c_int, [_vp, C.c_char_p]),
    "svoslam_scene_load_bmp": (C.c_int, [_vp, C.c_char_p]),
    "svoslam_scene_set_octree": (C.c_int, [_vp, _f32, _fp, _f32, _i32]),
    "svoslam_scene_voxelize_meshes": (C.c_int, [_vp, _i32, _i32, _vp]),
    "svoslam_scene_extract_voxel_grid": (C.c_int, [_vp, _vp]),
    "svoslam_scene_add_point_cloud": (C.c_int, [_vp, _fp, _vp, _vp, _i32, _fp, _fp, _vp]),
    "svoslam_scene_voxel_grid": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), _fp]),
    "svoslam_scene_svo": (C.c_int, [_vp, C.POINTER(_vp), _fp, _fp, C.POINTER(_i32), C.POINTER(_i32)]),
    "svoslam_free": (C.c_int, [_vp]),
    "svoslam_extract_surface_mesh": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, _fp, _f32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                                C.POINTER(SurfaceStats), _vp]),
    "svoslam_mesh_write_ply": (C.c_int, [C.c_char_p, _fp, _i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _i32, _i32]),
    "svoslam_pool_cast_rays": (C.c_int, [C.POINTER(_PoolStruct), _i32, _fp, _f32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_pool_query_points": (C.c_int, [C.POINTER(_PoolStruct), _i32, _fp, _f32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_pool_count_boxes": (C.c_int, [C.POINTER(_PoolStruct), _i32, _fp, _f32, _vp, C.c_int64, _i32, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_pool_nearest_occupied": (C.c_int, [C.POINTER(_PoolStruct), _i32, _fp, _f32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_pool_distance_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _vp]),
    "svoslam_pool_distance_field_profile": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _fp, _vp]),
    "svoslam_box_to_cells": (C.c_int, [_i32, _fp, _f32, _fp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "svoslam_workspace_field_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_reach_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _i32, _vp,
                                           C.POINTER(_ReachStats), _vp]),
    "svoslam_workspace_reach_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_owner_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _i32, _vp, _vp, _vp,
                                           C.POINTER(_OwnerStats), _vp]),
    "svoslam_pool_label_components": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _vp, _vp,
                                                C.POINTER(_ComponentStats), _vp]),
    "svoslam_workspace_component_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_nearest_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _vp, _vp, _vp,
                                             _vp, _vp]),
    "svoslam_workspace_nearest_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_visibility_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _i32, _vp, _vp,
                                                _vp]),
    "svoslam_workspace_visibility_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_cover_views": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _vp, _vp, _i32, _i32,
                                           _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_workspace_cover_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_field_observe_rays": (C.c_int, [_vp, _vp, _i32, _fp, _f32, C.POINTER(_i32), C.POINTER(_i32), _vp, _i32, _vp, _i32, _i32, _i32, _vp,
                                             _vp]),
    "svoslam_workspace_observe_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_frontier_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _vp, _vp, _vp, _vp, _vp]),
    "svoslam_workspace_frontier_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_score_poses": (C.c_int, [_vp, _vp, _i32, _fp, _f32, C.POINTER(_i32), C.POINTER(_i32), _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "svoslam_workspace_score_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_pool_cost_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, C.POINTER(_i32), _vp,
                                          _i32, _vp, C.POINTER(_PlanStats), _vp]),
    "svoslam_field_trace_paths": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), _vp, _i32, _i32, _vp, _vp, _vp]),
    "svoslam_workspace_plan_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_field_segment_clearance": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), _vp, _i32, _vp, _vp, _vp]),
    "svoslam_field_shorten_paths": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "svoslam_pool_ground_field": (C.c_int, [_vp, C.POINTER(_PoolStruct), _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32,
                                            _i32, _vp, _i32, _vp, C.POINTER(_GroundStats), _vp]),
    "svoslam_field_trace_ground_paths": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp,
                                                   _vp]),
    "svoslam_workspace_ground_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "svoslam_sort_words": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "svoslam_exclusive_scan_u32": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "svoslam_malloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "svoslam_cone_trace_svo": (C.c_int, [_vp, _i32, _i32, _f32, _fp, _vp, _fp, _f32, _i32, _vp, _vp]),
    "svoslam_cone_trace_svo_band": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _fp, _vp, _fp, _f32, _i32, _vp, _vp]),
    "svoslam_cone_trace_release": (C.c_int, [_vp, _i32]),
    "svoslam_cone_trace_timing": (C.c_int, [_i32]),
    "svoslam_cone_trace_timing_read": (C.c_int, [_fp, C.POINTER(_i32)]),
    "svoslam_stage_timing": (C.c_int, [C.c_uint32]),
    "svoslam_stage_timing_read": (C.c_int, [_i32, _fp, C.POINTER(_i32)]),
    "svoslam_generate_vertex_map": (C.c_int, [_vp, _vp, _i32, _i32, _f32, _f32, _i32, _i32, _vp]),
    "svoslam_generate_vertex_map_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _i32, _i32, _vp]),
    "svoslam_generate_normal_map": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_bilateral_filter": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_subsample_depth_u16": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_subsample_depth_f32": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_subsample_f32": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_subsample_rgb8": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_color_to_intensity": (C.c_int, [_vp, _vp, _i32, _vp]),
    "svoslam_transform_vertex_map": (C.c_int, [_vp, _fp, _i32, _vp]),
    "svoslam_transform_normal_map": (C.c_int, [_vp, _fp, _i32, _vp]),
    "svoslam_transform_vertex_map_dmat": (C.c_int, [_vp, _vp, _i32, _vp]),
    "svoslam_point_cloud_bbox": (C.c_int, [_vp, _i32, _fp, _fp, _vp]),
    "svoslam_point_cloud_bbox_device": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "svoslam_gradient": (C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    "svoslam_difference": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "svoslam_rgbd_cost": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _f32, _i32, _i32, _fp, _fp, _vp]),
    "svoslam_camera_set_rgbd": (C.c_int, [_vp, _i32]),
    "svoslam_camera_set_strict_reference": (C.c_int, [_vp, _i32]),
    "svoslam_raycast_model_depth": (C.c_int, [_vp, _i32, _i32, _f32, _f32, _fp, _vp, _vp, _fp, _f32, _vp, _vp]),
    "svoslam_camera_set_model_depth": (C.c_int, [_vp, _vp, _vp]),
    "svoslam_camera_set_frame_to_model": (C.c_int, [_vp, _i32]),
    "svoslam_icp_cost2": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _fp, _fp, _vp]),
    "svoslam_icp_cost": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _fp, _fp, C.POINTER(_i32), _vp]),
    "svoslam_icp_accumulate": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "svoslam_camera_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _f32, _f32]),
    "svoslam_camera_destroy": (C.c_int, [_vp]),
    "svoslam_camera_set_band": (C.c_int, [_vp, _i32, _i32]),
    "svoslam_camera_set_acc": (C.c_int, [_vp, _vp]),
    "svoslam_camera_update": (C.c_int, [_vp, _vp, _vp, C.c_longlong, C.POINTER(_i32), _vp]),
    "svoslam_camera_begin": (C.c_int, [_vp, _vp, _vp, C.c_longlong, C.POINTER(_i32), _vp]),
    "svoslam_camera_prepare": (C.c_int, [_vp, _vp, _vp, C.c_longlong, C.POINTER(_i32), _vp]),
    "svoslam_camera_track": (C.c_int, [_vp, _vp]),
    "svoslam_camera_pair_delta": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "svoslam_camera_apply_delta": (C.c_int, [_vp, _vp, C.c_longlong, C.POINTER(_i32), _vp]),
    "svoslam_camera_icp_iters": (C.c_int, [_i32]),
    "svoslam_camera_icp_accumulate": (C.c_int, [_vp, _i32, _i32, _vp]),
    "svoslam_camera_acc": (_vp, [_vp]),
    "svoslam_camera_icp_solve": (C.c_int, [_vp, _i32, _i32, _vp]),
    "svoslam_camera_end": (C.c_int, [_vp, _vp]),
    "svoslam_camera_pose": (C.c_int, [_vp, _fp, _fp, _vp]),
    "svoslam_camera_fusion_transform_device": (_vp, [_vp]),
    "svoslam_camera_last_system": (C.c_int, [_vp, _fp, _fp, _fp, _vp]),
    "svoslam_camera_last_vertex": (_vp, [_vp, _i32]),
    "svoslam_camera_last_normal": (_vp, [_vp, _i32]),
    "svoslam_camera_tracking_lost_count": (C.c_int, [_vp, C.POINTER(_i32), _vp]),
    "svoslam_camera_last_track_plan": (C.c_int, [_vp, C.POINTER(_i32)]),
    "svoslam_camera_latest_timestamp": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(C.c_longlong)]),
    "svoslam_camera_track_profile": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), _vp]),
    "svoslam_timer_start": (C.c_int, [_vp]),
    "svoslam_timer_stop": (C.c_int, [_vp, _fp]),
}


def lib():
    """Load libsvoslam_hip.so; raises SvoslamError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SvoslamError("%s is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                           "There is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime: whichever of the two is mapped first serves the whole process, and torch finds no
    # device when this library's (/opt/rocm) came first -- e.g. __graft_entry__.build() followed by smoke() in one process.
    # torch is the device-memory / stream provider of every caller of this binding, so it goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status):
    if status != 0:
        L = lib()
        raise SvoslamError("svoslam status %d (%s): %s" % (status, L.svoslam_status_string(status).decode(),
                                                          L.svoslam_last_error().decode()))


_raw_stream = None


def _stream():
    """torch's current HIP stream as a raw handle (the C call, not the Stream object: this runs ~20x per frame)"""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or False
    if _raw_stream:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _fa(values, n):
    a = (C.c_float * n)(*[float(v) for v in np.asarray(values, dtype=np.float32).reshape(-1)])
    return a


class ConfigStruct(C.Structure):
    """include/svoslam.h svoslam_config"""
    _fields_ = [(n, C.c_int32) for n in ("march_bricks", "track_mode", "track_workers", "track_stream", "runner_deferred", "runner_lead",
                                         "runner_prio", "runner_replicas", "runner_timeline", "sort_pairs", "graphs", "march_ahead")] + [("reserved", C.c_int32 * 4)]


def get_config():
    """the library's settings as a dict (include/svoslam.h svoslam_config)"""
    c = ConfigStruct()
    check(lib().svoslam_config_get(C.byref(c)))
    return {n: int(getattr(c, n)) for n, _ in ConfigStruct._fields_ if n != "reserved"}


def configure(**settings):
    """svoslam_config_set: e.g. configure(track_mode=1, runner_deferred=0); takes effect for cameras / runners created afterwards and
    for the next render / fusion call.  Returns the settings as they were."""
    c = ConfigStruct()
    check(lib().svoslam_config_get(C.byref(c)))
    before = {n: int(getattr(c, n)) for n, _ in ConfigStruct._fields_ if n != "reserved"}
    for k, v in settings.items():
        if k not in before:
            raise KeyError("svoslam_config has no field %r" % (k,))
        setattr(c, k, int(v))
    check(lib().svoslam_config_set(C.byref(c)))
    return before


def config_env(**settings):
    """{"SVOSLAM_CONFIG": "name=value,..."}: the same settings for a child process (read once when its library starts)"""
    return {"SVOSLAM_CONFIG": ",".join("%s=%d" % (k, int(v)) for k, v in settings.items())}


def device_arch():
    a = lib().svoslam_device_arch()
    return a.decode() if a else None


# ----------------------------------------------------------------------------- pool / fusion
class Workspace:
    def __init__(self):
        self._h = C.c_void_p()
        check(lib().svoslam_workspace_create(C.byref(self._h)))

    def close(self):
        if self._h:
            lib().svoslam_workspace_destroy(self._h)
            self._h = C.c_void_p()

    def field_buffers(self):
        """svoslam_workspace_field_buffers: [(device pointer, bytes)] of the three distance-field slots (diagnostics)"""
        ptrs, sizes = (_vp * 3)(), (C.c_uint64 * 3)()
        check(lib().svoslam_workspace_field_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(3)]

    def reach_buffers(self):
        """svoslam_workspace_reach_buffers: [(device pointer, bytes)] of the two reach-field slots (diagnostics)"""
        ptrs, sizes = (_vp * 2)(), (C.c_uint64 * 2)()
        check(lib().svoslam_workspace_reach_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(2)]

    def plan_buffers(self):
        """svoslam_workspace_plan_buffers: [(device pointer, bytes)] of the three cost-field slots (diagnostics)"""
        ptrs, sizes = (_vp * 3)(), (C.c_uint64 * 3)()
        check(lib().svoslam_workspace_plan_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(3)]

    def ground_buffers(self):
        """svoslam_workspace_ground_buffers: [(device pointer, bytes)] of the six ground-field slots (diagnostics)"""
        ptrs, sizes = (_vp * 6)(), (C.c_uint64 * 6)()
        check(lib().svoslam_workspace_ground_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(6)]

    def component_buffers(self):
        """svoslam_workspace_component_buffers: [(device pointer, bytes)] of the two component slots (diagnostics)"""
        ptrs, sizes = (_vp * 2)(), (C.c_uint64 * 2)()
        check(lib().svoslam_workspace_component_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(2)]

    def nearest_buffers(self):
        """svoslam_workspace_nearest_buffers: [(device pointer, bytes)] of the three nearest-cell slots (diagnostics)"""
        ptrs, sizes = (_vp * 3)(), (C.c_uint64 * 3)()
        check(lib().svoslam_workspace_nearest_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(3)]

    def visibility_buffers(self):
        """svoslam_workspace_visibility_buffers: [(device pointer, bytes)] of the visibility field's one slot (diagnostics)"""
        ptrs, sizes = (_vp * 1)(), (C.c_uint64 * 1)()
        check(lib().svoslam_workspace_visibility_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[0] or 0), int(sizes[0]))]

    def cover_buffers(self):
        """svoslam_workspace_cover_buffers: [(device pointer, bytes)] of the view cover's four slots -- the bit rows, the flags / ranks
        and the target list, the matrix, the covered words and round records (diagnostics)"""
        ptrs, sizes = (_vp * 4)(), (C.c_uint64 * 4)()
        check(lib().svoslam_workspace_cover_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(4)]

    def observe_buffers(self):
        """svoslam_workspace_observe_buffers: [(device pointer, bytes)] of the ray observation's one slot, the two bit planes (diagnostics)"""
        ptrs, sizes = (_vp * 1)(), (C.c_uint64 * 1)()
        check(lib().svoslam_workspace_observe_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[0] or 0), int(sizes[0]))]

    def frontier_buffers(self):
        """svoslam_workspace_frontier_buffers: [(device pointer, bytes)] of the frontier field's one slot, the bit rows (diagnostics)"""
        ptrs, sizes = (_vp * 1)(), (C.c_uint64 * 1)()
        check(lib().svoslam_workspace_frontier_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[0] or 0), int(sizes[0]))]

    def score_buffers(self):
        """svoslam_workspace_score_buffers: [(device pointer, bytes)] of the pose scoring's one slot (diagnostics)"""
        ptrs, sizes = (_vp * 1)(), (C.c_uint64 * 1)()
        check(lib().svoslam_workspace_score_buffers(self._h, ptrs, sizes))
        return [(int(ptrs[0] or 0), int(sizes[0]))]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pool:
    """Device node pool (svoslam_pool).  words() copies it to the host as uint32."""

    def __init__(self, capacity_nodes=8):
        self._p = _PoolStruct(None, 0, 0, None, 0, 0)
        check(lib().svoslam_pool_init(C.byref(self._p), capacity_nodes, _stream()))

    @property
    def size(self):
        if self._p.pending > 0:   # asynchronous fusion calls in flight: fetch the exact size (blocking)
            check(lib().svoslam_pool_sync(C.byref(self._p), _stream()))
        return int(self._p.size)

    @property
    def capacity(self):
        return int(self._p.capacity)

    @property
    def data_ptr(self):
        return int(self._p.d_data)

    def reserve(self, capacity_nodes):
        check(lib().svoslam_pool_reserve(C.byref(self._p), capacity_nodes, _stream()))

    def words(self):
        import torch
        torch.cuda.synchronize()
        n = 2 * self.size
        out = np.empty(n, dtype=np.uint32)
        hip = _hip()
        r = hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.data_ptr), C.c_size_t(n * 4), 2)
        if r != 0:
            raise SvoslamError("hipMemcpy D2H failed: %d" % r)
        return out

    def set_words(self, words):
        """replace the pool's contents (svoslam_pool_set_nodes: validates child pointers, resets the device-resident size
        and the reservations of asynchronous fusions, so fusing into the loaded tree allocates after it)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        check(lib().svoslam_pool_set_nodes(C.byref(self._p), words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size // 2, _stream()))

    def evict_subtree(self, path, file):
        """page the sub-tree below the node reached by the octant `path` out to `file` (svoslam_pool_evict_subtree)"""
        p = (C.c_uint8 * len(path))(*[int(o) for o in path])
        check(lib().svoslam_pool_evict_subtree(C.byref(self._p), p, len(path), str(file).encode(), _stream()))

    def restore_subtree(self, file):
        check(lib().svoslam_pool_restore_subtree(C.byref(self._p), str(file).encode(), _stream()))

    def graft_subtree(self, file):
        """bring a paged-out sub-tree back as new tiles at the end of the pool (svoslam_pool_graft_subtree): independent of node
        numbering, so it works after compact() where restore_subtree refuses"""
        check(lib().svoslam_pool_graft_subtree(C.byref(self._p), str(file).encode(), _stream()))

    def compact(self, capacity_nodes=0, want_map=False):
        """re-index the pool to the tiles reachable from the root, in canonical breadth-first order (svoslam_pool_compact).
        capacity_nodes <= 0 keeps the capacity, otherwise the new one is max(capacity_nodes, size after): 1 shrinks to fit.
        Returns the stats as a dict; with want_map also an int32 device tensor, entry k = old first-node index of new tile k."""
        st = CompactStats()
        old_tile, ptr = None, None
        if want_map:
            import torch
            # the call writes size_before / 8 entries, size_before being the size AFTER its own sync: take the same one here
            # (every commit in flight reports through the pool's tracker, which the sync drains), not a host-side size that lags
            check(lib().svoslam_pool_sync(C.byref(self._p), _stream()))
            old_tile = torch.zeros(max(int(self._p.size) // 8, 1), dtype=torch.int32, device="cuda")
            ptr = C.c_void_p(old_tile.data_ptr())
        check(lib().svoslam_pool_compact(C.byref(self._p), int(capacity_nodes), ptr, C.byref(st), _stream()))
        stats = {n: int(getattr(st, n)) for n, _ in CompactStats._fields_}
        if want_map:
            return stats, old_tile[:stats["size_after"] // 8]
        return stats

    def copy_from(self, other):
        """become a byte-identical replica of `other` (blocking)"""
        check(lib().svoslam_pool_copy(C.byref(self._p), C.byref(other._p), _stream()))

    def reset(self):
        """empty map (8 zeroed root children), same allocation"""
        check(lib().svoslam_pool_reset(C.byref(self._p), _stream()))

    def march_accel(self):
        """what the ray march of this pool runs on: {grid: bool, bricks: 1 in use / 0 not built / -1 allocation failed (tree march),
        brick_shift}"""
        g, b, sh = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        check(lib().svoslam_pool_march_accel(C.byref(self._p), C.byref(g), C.byref(b), C.byref(sh)))
        return {"grid": bool(g.value), "bricks": int(b.value), "brick_shift": int(sh.value)}

    def accel_view(self):
        """svoslam_pool_accel_view: the march's tables and their upkeep state as the library holds them right now, as a dict of
        device addresses (0: none), host flags and word offsets into a dirty state.  Launches nothing and changes nothing."""
        v = AccelView()
        check(lib().svoslam_pool_accel_view(C.byref(self._p), C.byref(v)))
        out = {n: getattr(v, n) for n, _ in AccelView._fields_ if n not in ("dirty", "brick_served")}
        for n in ("grid", "bricks", "brick_touched"):
            out[n] = int(out[n] or 0)
        for n in ("valid", "bricks_valid", "mip_consistent", "deferred_pending", "bricks_failed"):
            out[n] = bool(out[n])
        out["dirty"] = [int(v.dirty[k] or 0) for k in range(2)]
        out["brick_served"] = [int(v.brick_served[k]) for k in range(2)]
        out["bricks_in_use"] = bool(out["bricks"]) and out["bricks_valid"] and out["brick_shift"] >= 0
        return out

    def accel_grid(self, view=None):
        """the level-8 grid and the pyramid behind it as host words: (uint32 [2^24, 2], uint32 [pyramid entries, 2]); None
        before the first render"""
        v = view or self.accel_view()
        if not v["grid"]:
            return None
        n8, npyr = 1 << 24, ((1 << 24) - 8) // 7
        both = copy_from_device(v["grid"], (n8 + npyr, 2), np.uint32)
        return both[:n8], both[n8:]

    def accel_brick_group(self, group, view=None):
        """one 64 KB group of the brick field (8^3 bricks of 64 entries) as host uint16 [32768]"""
        v = view or self.accel_view()
        if not v["bricks"] or not 0 <= int(group) < (1 << 18):
            raise SvoslamError("no brick field, or no such group")
        return copy_from_device(v["bricks"] + int(group) * 65536, (32768,), np.uint16)

    def accel_dirty_words(self, state, offset, count, view=None):
        """`count` words of dirty state `state` from word `offset` on (uint32)"""
        v = view or self.accel_view()
        if not v["dirty"][state] or offset < 0 or offset + count > v["state_words"]:
            raise SvoslamError("no such dirty state, or words outside it")
        return copy_from_device(v["dirty"][state] + 4 * int(offset), (int(count),), np.uint32)

    def expand(self, center, edge_length, toward):
        """doubles the root cube towards `toward` (re-rooting); returns the new (center, edge_length)"""
        c = _fa(center, 3)
        e = C.c_float(float(edge_length))
        check(lib().svoslam_pool_expand(C.byref(self._p), c, C.byref(e), _fa(toward, 3), _stream()))
        return tuple(float(v) for v in c), float(e.value)

    def save(self, path, center, edge_length, max_depth):
        """checkpoint: linear tree + root parameters (svoslam_pool_save)"""
        check(lib().svoslam_pool_save(C.byref(self._p), str(path).encode(), _fa(center, 3), float(edge_length), int(max_depth),
                                      _stream()))

    def load(self, path):
        """resume from a checkpoint; returns (center, edge_length, max_depth)"""
        c, e, d = (C.c_float * 3)(), C.c_float(0), C.c_int32(0)
        check(lib().svoslam_pool_load(C.byref(self._p), str(path).encode(), c, C.byref(e), C.byref(d), _stream()))
        return tuple(float(v) for v in c), float(e.value), int(d.value)

    def close(self):
        if self._p.d_data:
            lib().svoslam_pool_free(C.byref(self._p))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_hiplib = None


def _hip():
    global _hiplib
    if _hiplib is None:
        _hiplib = C.CDLL("libamdhip64.so")
        _hiplib.hipMemcpy.restype = C.c_int
        _hiplib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hiplib


def svo_from_point_cloud(ws, points, colors, max_depth, pool, center, edge_length):
    """svo::svoFromPointCloud.  points: cuda float32 [n,3]; colors: cuda uint8 [n,3]."""
    n = int(points.shape[0]) if points is not None else 0
    stats = FuseStats()
    check(lib().svoslam_svo_from_point_cloud(ws._h, _ptr(points), _ptr(colors), n, max_depth, C.byref(pool._p),
                                             _fa(center, 3), float(edge_length), C.byref(stats), _stream()))
    return stats


def svo_from_point_cloud_async(ws, points, colors, max_depth, pool, center, edge_length):
    """svoFromPointCloud without any host round trip (size stays on the device until pool.size is read)."""
    n = int(points.shape[0]) if points is not None else 0
    check(lib().svoslam_svo_from_point_cloud_async(ws._h, _ptr(points), _ptr(colors), n, max_depth, C.byref(pool._p),
                                                   _fa(center, 3), float(edge_length), _stream()))


def svo_fuse_sort(ws, points, max_depth, center, edge_length):
    """phase 1 of the asynchronous fusion: keys + sort (workspace only)."""
    n = int(points.shape[0]) if points is not None else 0
    check(lib().svoslam_svo_fuse_sort(ws._h, _ptr(points), n, max_depth, _fa(center, 3), float(edge_length), _stream()))


def svo_fuse_sort_frame(ws, depth_image, pose_ptr, fx, fy, max_depth, center, edge_length, bbox7=None):
    """sort phase straight from a depth frame and a device-resident pose (vertex map + transform + bbox + keys in one launch)"""
    h, w = depth_image.shape[-2], depth_image.shape[-1]
    check(lib().svoslam_svo_fuse_sort_frame(ws._h, _ptr(depth_image), C.c_void_p(int(pose_ptr)), w, h, float(fx), float(fy),
                                            int(max_depth), _fa(center, 3), float(edge_length), _ptr(bbox7), _stream()))


def svo_fuse_sort_frame_band(ws, depth_image, pose_ptr, fx, fy, max_depth, center, edge_length, first_row, rows):
    """svo_fuse_sort_frame for one row band of the frame; the sorted point indices are whole-image indices"""
    h, w = depth_image.shape[-2], depth_image.shape[-1]
    check(lib().svoslam_svo_fuse_sort_frame_band(ws._h, _ptr(depth_image), C.c_void_p(int(pose_ptr)), w, h, float(fx), float(fy),
                                                 int(max_depth), _fa(center, 3), float(edge_length), int(first_row), int(rows), _stream()))


def svo_fuse_merge_sorted(keys_lists, idx_lists, keys_out, idx_out):
    """merge sorted (key, index) lists with ascending, disjoint index ranges (row bands in order) -> keys_out, idx_out"""
    n = len(keys_lists)
    kp = (C.c_void_p * n)(*[k.data_ptr() for k in keys_lists])
    ip = (C.c_void_p * n)(*[k.data_ptr() for k in idx_lists])
    cn = (C.c_int32 * n)(*[int(k.shape[0]) for k in keys_lists])
    check(lib().svoslam_svo_fuse_merge_sorted(kp, ip, cn, n, _ptr(keys_out), _ptr(idx_out), _stream()))


def svo_fuse_export_sorted(ws, n, keys_out, idx_out):
    """the outcome of the workspace's sort phase -> keys_out (int64 cuda tensor [n]), idx_out (int32 cuda tensor [n])"""
    check(lib().svoslam_svo_fuse_export_sorted(ws._h, int(n), _ptr(keys_out), _ptr(idx_out), _stream()))


def sort_words(ws, words, key_bits, idx_bits, digit_bits=0, want_vals=True, vals=None, keys_out=None, vals_out=None):
    """svoslam_sort_words: the library's stable radix sort on `words` (int64 cuda tensor [n]).  idx_bits >= 0: the packed form
    (key << idx_bits | index; digit_bits 1..11, 0 = by size); idx_bits == -1: the pair form carrying `vals` (int32 cuda tensor
    [n]; None: 0..n-1).  -> (keys, vals) as int64 / int32 cuda tensors (vals None when want_vals is false)"""
    import torch
    n = int(words.shape[0])
    if keys_out is None:
        keys_out = torch.empty(n, dtype=torch.int64, device=words.device)
    if vals_out is None and want_vals:
        vals_out = torch.empty(n, dtype=torch.int32, device=words.device)
    check(lib().svoslam_sort_words(ws._h, _ptr(words), _ptr(vals), n, int(key_bits), int(idx_bits), int(digit_bits), 1 if want_vals else 0,
                                   _ptr(keys_out), _ptr(vals_out), _stream()))
    return keys_out, vals_out


def exclusive_scan_u32(ws, data, total=None):
    """svoslam_exclusive_scan_u32: `data` (int32 cuda tensor [n], read as uint32) becomes its exclusive prefix sums mod 2^32, in
    place.  -> total (int32 cuda tensor [1]: the sum mod 2^32)"""
    import torch
    if total is None:
        total = torch.empty(1, dtype=torch.int32, device=data.device)
    check(lib().svoslam_exclusive_scan_u32(ws._h, _ptr(data), int(data.shape[0]), _ptr(total), _stream()))
    return total


def svo_fuse_adopt_sorted(ws, keys, idx, max_depth):
    """sorted keys / point indices from elsewhere become the outcome of the workspace's sort phase (they must stay alive
    until the commit has run)"""
    check(lib().svoslam_svo_fuse_adopt_sorted(ws._h, _ptr(keys), _ptr(idx), int(keys.shape[0]), int(max_depth)))


def svo_fuse_plan(ws, n, max_depth, pool):
    """phase 2: split planning against the pool's current tree (reads the pool)."""
    check(lib().svoslam_svo_fuse_plan(ws._h, int(n), max_depth, C.byref(pool._p), _stream()))


def pool_structure_begin(pool):
    """before a sequence of svo_fuse_plan_structure calls: the structure-side size := the pool's size"""
    check(lib().svoslam_pool_structure_begin(C.byref(pool._p), _stream()))


def svo_fuse_plan_structure(ws, n, max_depth, pool):
    """plan + every split with its links, independent of the previous frame's commit (colour words)"""
    check(lib().svoslam_svo_fuse_plan_structure(ws._h, int(n), int(max_depth), C.byref(pool._p), _stream()))


def svo_fuse_split_early(ws, n, max_depth, pool):
    """between plan and commit: the planned splits' child tiles, written where no ray march can see them yet"""
    check(lib().svoslam_svo_fuse_split_early(ws._h, int(n), int(max_depth), C.byref(pool._p), _stream()))


def svo_fuse_commit(ws, colors, max_depth, pool):
    """phase 3: splits, leaf blend, mip levels (writes the pool)."""
    n = int(colors.shape[0]) if colors is not None else 0
    check(lib().svoslam_svo_fuse_commit(ws._h, _ptr(colors), n, max_depth, C.byref(pool._p), _stream()))


def svo_fuse_commit_deferred(ws, colors, max_depth, pool):
    """phase 3 without a store a concurrent render of the pool's present state can see; svo_fuse_apply publishes it"""
    n = int(colors.shape[0]) if colors is not None else 0
    check(lib().svoslam_svo_fuse_commit_deferred(ws._h, _ptr(colors), n, max_depth, C.byref(pool._p), _stream()))


def svo_fuse_apply(ws, pool):
    check(lib().svoslam_svo_fuse_apply(ws._h, C.byref(pool._p), _stream()))


KEYRANGE_OVERFLOW, KEYRANGE_MISMATCH, KEYRANGE_USED_WORD = 2, 4, 10
KEYRANGE_FIXED_WORDS = 11264    # header + fixed-size lists of a delta; its tiles, links and words follow


def svo_fuse_keyrange_commit(ws, sorted_keys, sorted_idx, colors, max_depth, pool, rank, world, delta):
    """key-range sharded fusion, first half: plan + (invisible) commit of rank's slice of the frame's sorted keys, its delta into `delta`
    (a uint32 / int32 device tensor with room: 64 bytes per key of the slice is ample)"""
    n = int(sorted_keys.shape[0])
    check(lib().svoslam_svo_fuse_keyrange_commit(ws._h, _ptr(sorted_keys), _ptr(sorted_idx), _ptr(colors), n, int(max_depth), C.byref(pool._p),
                                                 int(rank), int(world), _ptr(delta), int(delta.numel() * delta.element_size()), _stream()))


def svo_fuse_keyrange_apply(ws, sorted_keys, max_depth, pool, deltas):
    """second half, after the all-gather: every rank's delta (rank order, the own one included) into this replica"""
    n = int(sorted_keys.shape[0])
    arr = (C.c_void_p * len(deltas))(*[int(d.data_ptr()) for d in deltas])
    check(lib().svoslam_svo_fuse_keyrange_apply(ws._h, _ptr(sorted_keys), n, int(max_depth), C.byref(pool._p), arr, len(deltas), _stream()))


def svo_fuse_keyrange_discard(ws, pool):
    """the delta of the last keyrange_commit was all that was wanted: no apply follows on this pool"""
    check(lib().svoslam_svo_fuse_keyrange_discard(ws._h, C.byref(pool._p)))


def svo_fuse_keyrange_status(ws):
    """flags of the last apply on this workspace (blocking): 0 = applied"""
    f = C.c_int32(0)
    check(lib().svoslam_svo_fuse_keyrange_status(ws._h, C.byref(f), _stream()))
    return int(f.value)


def svo_from_voxel_grid(ws, centers, colors, max_depth, pool, center, edge_length):
    """svo::svoFromVoxelGrid.  centers, colors: cuda float32 [n,4]."""
    n = int(centers.shape[0]) if centers is not None else 0
    stats = FuseStats()
    check(lib().svoslam_svo_from_voxel_grid(ws._h, _ptr(centers), _ptr(colors), n, max_depth, C.byref(pool._p),
                                            _fa(center, 3), float(edge_length), C.byref(stats), _stream()))
    return stats


def extract_voxel_grid(ws, pool, max_depth, center, edge_length):
    """svo::extractVoxelGridFromSVO -> (centers[n,4], colors[n,4]) numpy float32."""
    import torch
    pc, pk, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    check(lib().svoslam_extract_voxel_grid(ws._h, C.byref(pool._p), max_depth, _fa(center, 3), float(edge_length),
                                           C.byref(pc), C.byref(pk), C.byref(n), _stream()))
    torch.cuda.synchronize()
    ce = np.zeros((n.value, 4), np.float32)
    co = np.zeros((n.value, 4), np.float32)
    if n.value > 0:
        _hip().hipMemcpy(C.c_void_p(ce.ctypes.data), pc, C.c_size_t(ce.nbytes), 2)
        _hip().hipMemcpy(C.c_void_p(co.ctypes.data), pk, C.c_size_t(co.nbytes), 2)
        lib().svoslam_free(pc)
        lib().svoslam_free(pk)
    return ce, co


def extract_surface_mesh(ws, pool, max_depth, center, edge_length):
    """svoslam_extract_surface_mesh: the surface of the occupied cells at max_depth as a welded quad mesh ->
    (vertices[n,3] float32, quads[m,4] uint32, colors[m] uint32 (the cells' colour words), stats dict) as numpy arrays"""
    pv, pq, pc, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), SurfaceStats()
    check(lib().svoslam_extract_surface_mesh(ws._h, C.byref(pool._p), max_depth, _fa(center, 3), float(edge_length),
                                             C.byref(pv), C.byref(pq), C.byref(pc), C.byref(st), _stream()))
    stats = {n: int(getattr(st, n)) for n, _ in SurfaceStats._fields_}
    try:
        vertices = copy_from_device(pv.value, (stats["vertices"], 3), np.float32) if pv.value else np.zeros((0, 3), np.float32)
        quads = copy_from_device(pq.value, (stats["faces"], 4), np.uint32) if pq.value else np.zeros((0, 4), np.uint32)
        colors = copy_from_device(pc.value, (stats["faces"],), np.uint32) if pc.value else np.zeros(0, np.uint32)
    finally:
        for p in (pv, pq, pc):
            if p.value:
                lib().svoslam_free(p)
    return vertices, quads, colors, stats


def write_ply(path, vertices, quads, colors, triangulate=False):
    """svoslam_mesh_write_ply: binary little-endian PLY of a mesh held in numpy arrays (needs no device)"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 4)
    c = np.ascontiguousarray(colors, dtype=np.uint32).reshape(-1)
    if c.shape[0] != q.shape[0]:
        raise ValueError("one colour per quad: %d colours, %d quads" % (c.shape[0], q.shape[0]))
    u32p = C.POINTER(C.c_uint32)
    check(lib().svoslam_mesh_write_ply(os.fsencode(str(path)), v.ctypes.data_as(_fp), v.shape[0], q.ctypes.data_as(u32p),
                                       c.ctypes.data_as(u32p), q.shape[0], 1 if triangulate else 0))


def _query(inputs, width, fields, outputs, call):
    """shared by cast_rays / query_points / count_boxes / nearest_occupied: numpy or cuda-tensor input [n, width] -> dict of the requested outputs, of the same kind.
    uint32 / uint64 results are computed in int32 / int64 tensors and viewed as unsigned on the way out (numpy) or left signed
    bit patterns (torch, which has no arithmetic on unsigned 32 / 64-bit)."""
    import torch
    as_torch = isinstance(inputs, torch.Tensor)
    t_in = inputs if as_torch else torch.from_numpy(np.ascontiguousarray(inputs, dtype=np.float32))
    if as_torch and not t_in.is_cuda:
        raise ValueError("a tensor input has to be a cuda tensor (pass numpy arrays for host data)")
    t_in = t_in.to(device="cuda", dtype=torch.float32).reshape(-1, width).contiguous()
    n = int(t_in.shape[0])
    names = tuple(fields) if outputs is None else tuple(outputs)
    for name in names:
        if name not in fields:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(fields)))
    bufs = {name: torch.empty(n, dtype=fields[name][0], device="cuda") for name in names}
    call(t_in, n, [_ptr(bufs.get(name)) for name in fields])
    if as_torch:
        return bufs
    return {name: b.cpu().numpy().view(fields[name][1]) for name, b in bufs.items()}


def cast_rays(pool, max_depth, center, edge_length, rays, t_max=None, outputs=None):
    """svoslam_pool_cast_rays: the first occupied cell at max_depth along each ray (rays[n, 6]: origin, direction; t_max[n] or None).
    -> {"t": float32, "node": int32, "cell": uint64 (x | y << 16 | z << 32 | face << 48), "color": uint32, "steps": uint32} as numpy
    arrays, or as torch tensors (cell int64, color / steps int32: the same bits) when `rays` is a cuda tensor, in which case nothing
    is synchronised.  `outputs`: the subset of those names to compute (the others are passed as NULL)."""
    import torch
    fields = {"t": (torch.float32, np.float32), "node": (torch.int32, np.int32), "cell": (torch.int64, np.uint64),
              "color": (torch.int32, np.uint32), "steps": (torch.int32, np.uint32)}
    tm = None
    if t_max is not None:
        tm = t_max if isinstance(t_max, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t_max, dtype=np.float32))
        tm = tm.to(device="cuda", dtype=torch.float32).reshape(-1).contiguous()

    def call(t_in, n, ptrs):
        if tm is not None and int(tm.shape[0]) != n:
            raise ValueError("one t_max per ray: %d values, %d rays" % (int(tm.shape[0]), n))
        check(lib().svoslam_pool_cast_rays(C.byref(pool._p), int(max_depth), _fa(center, 3), float(edge_length), _ptr(t_in), _ptr(tm), n,
                                           *ptrs, _stream()))
    return _query(rays, 6, fields, outputs, call)


def query_points(pool, max_depth, center, edge_length, points, outputs=None):
    """svoslam_pool_query_points: the node that holds each point (points[n, 3]), by the fusion's own descent to max_depth or the first
    childless node.  -> {"node": int32 (-1 outside), "level": int32, "key": uint64, "color": uint32}, numpy or torch as cast_rays."""
    import torch
    fields = {"node": (torch.int32, np.int32), "level": (torch.int32, np.int32), "key": (torch.int64, np.uint64),
              "color": (torch.int32, np.uint32)}

    def call(t_in, n, ptrs):
        check(lib().svoslam_pool_query_points(C.byref(pool._p), int(max_depth), _fa(center, 3), float(edge_length), _ptr(t_in), n, *ptrs,
                                              _stream()))
    return _query(points, 3, fields, outputs, call)


def count_boxes(pool, max_depth, center, edge_length, boxes, stop_after=0, outputs=None):
    """svoslam_pool_count_boxes: the occupied cells at max_depth in each axis-aligned box (boxes[n, 6]: min xyz, max xyz; infinities
    allowed).  stop_after > 0 ends a box's walk at that count (1: the any-hit collision test).  -> {"count": uint64, "first_cell":
    uint64 (x | y << 16 | z << 32 of the lowest occupied cell in Morton order; all ones: none), "first_node": int32, "steps": uint32},
    numpy or torch as cast_rays."""
    import torch
    fields = {"count": (torch.int64, np.uint64), "first_cell": (torch.int64, np.uint64), "first_node": (torch.int32, np.int32),
              "steps": (torch.int32, np.uint32)}

    def call(t_in, n, ptrs):
        check(lib().svoslam_pool_count_boxes(C.byref(pool._p), int(max_depth), _fa(center, 3), float(edge_length), _ptr(t_in),
                                             int(stop_after), n, *ptrs, _stream()))
    return _query(boxes, 6, fields, outputs, call)


def nearest_occupied(pool, max_depth, center, edge_length, points, radius_cells, outputs=None):
    """svoslam_pool_nearest_occupied: the nearest occupied cell at max_depth within radius_cells of each point's cell (points[n, 3]).
    -> {"dist2": int32 (squared distance in cells; -1: none within the radius, -2: the point is outside the root or NaN; metres =
    sqrt(dist2) * 2 * edge_length / 2^max_depth), "cell": uint64 (x | y << 16 | z << 32), "node": int32, "color": uint32, "steps":
    uint32}, numpy or torch as cast_rays."""
    import torch
    fields = {"dist2": (torch.int32, np.int32), "cell": (torch.int64, np.uint64), "node": (torch.int32, np.int32),
              "color": (torch.int32, np.uint32), "steps": (torch.int32, np.uint32)}

    def call(t_in, n, ptrs):
        check(lib().svoslam_pool_nearest_occupied(C.byref(pool._p), int(max_depth), _fa(center, 3), float(edge_length), _ptr(t_in),
                                                  int(radius_cells), n, *ptrs, _stream()))
    return _query(points, 3, fields, outputs, call)


def distance_field(ws, pool, max_depth, origin, dims, radius_cells, as_tensor=False, launch_ms=None):
    """svoslam_pool_distance_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the squared
    distance in cells to the nearest occupied cell of the map within radius_cells, -1 where there is none: an exact Euclidean
    distance transform truncated at the radius.  -> int32 [nz, ny, nx] (metres = sqrt(dist2) * 2 * edge_length / 2^max_depth), a
    numpy array, or with as_tensor a cuda tensor, in which case nothing is synchronised.  `launch_ms`: a list that receives the
    milliseconds of the four launches (raster, x, y, z pass): svoslam_pool_distance_field_profile, which blocks."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    out = torch.empty([max(v, 0) for v in reversed(n)], dtype=torch.int32, device="cuda")
    if launch_ms is None:
        check(lib().svoslam_pool_distance_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(radius_cells),
                                                _ptr(out), _stream()))
    else:
        ms = (C.c_float * 4)()
        check(lib().svoslam_pool_distance_field_profile(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n),
                                                        int(radius_cells), _ptr(out), ms, _stream()))
        launch_ms[:] = [float(v) for v in ms]
    return out if as_tensor else out.cpu().numpy()


def reach_field(ws, pool, max_depth, origin, dims, clearance_cells, seeds, as_tensor=False, stats=None):
    """svoslam_pool_reach_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the number of
    face-neighbour moves of the shortest path from any of `seeds` ([n, 3] absolute cells: an array, or an int32 cuda tensor) that
    stays in the region and in cells with no occupied cell within clearance_cells (those where distance_field with that radius is
    -1); 0 at a seed that counts, -1 where no path leads, -2 where the cell is blocked.  -> int32 [nz, ny, nx] (metres along the
    path = steps * 2 * edge_length / 2^max_depth), a numpy array, or with as_tensor a cuda tensor.  The call blocks either way:
    the host reads a convergence record per round.  `stats`: a dict that receives rounds, tile_runs and seeds_used."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    if isinstance(seeds, torch.Tensor):
        if not seeds.is_cuda or seeds.dtype != torch.int32:
            raise ValueError("a seeds tensor is int32 on the device")
        t_seeds = seeds.reshape(-1, 3).contiguous()
    else:
        t_seeds = torch.from_numpy(np.ascontiguousarray(np.asarray(seeds, np.int32).reshape(-1, 3))).cuda()
    count = int(t_seeds.shape[0])
    out = torch.empty([max(v, 0) for v in reversed(n)], dtype=torch.int32, device="cuda")
    st = _ReachStats()
    check(lib().svoslam_pool_reach_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(clearance_cells),
                                         _ptr(t_seeds) if count else None, count, _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(rounds=int(st.rounds), tile_runs=int(st.tile_runs), seeds_used=int(st.seeds_used))
    return out if as_tensor else out.cpu().numpy()


MAX_RING_COST = 65534                                                   # include/svoslam.h SVOSLAM_MAX_RING_COST


def _cells_tensor(cells, what):
    """[n, 3] absolute cells, an array or an int32 cuda tensor -> a contiguous int32 cuda tensor"""
    import torch
    if isinstance(cells, torch.Tensor):
        if not cells.is_cuda or cells.dtype != torch.int32:
            raise ValueError("a %s tensor is int32 on the device" % what)
        return cells.reshape(-1, 3).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(cells, np.int32).reshape(-1, 3))).cuda()


def owner_field(ws, pool, max_depth, origin, dims, clearance_cells, seeds=None, seed_field=None, as_tensor=False, stats=None, owner=None):
    """svoslam_pool_owner_field: reach_field's steps and, with them, which seed is nearest by path.  Seeds are given one of two ways:
    `seeds` ([n, 3] absolute cells: an array, or an int32 cuda tensor; the label of entry k is k), or `seed_field` (int32 [nz, ny,
    nx]: an array or a cuda tensor; a traversable cell with a value 0 <= v < 2^31 - 1 is a seed with label v -- the labels of
    label_components, say).  -> (steps, owner), int32 [nz, ny, nx] each: steps as reach_field gives them for the seeds that count
    (-1 no path, -2 blocked); owner, at a cell with steps >= 0, the smallest label among the seeds whose shortest path to the cell
    has exactly that many moves, elsewhere the value of steps.  numpy arrays, or with as_tensor cuda tensors.  `owner`: a
    contiguous int32 cuda tensor of the region's shape that receives the owners; it may be the seed_field tensor itself, which is
    then grown IN PLACE (otherwise a seed_field tensor is left as it is).  The call blocks either way.  `stats`: a dict that
    receives rounds, tile_runs, seeds_used, owner_rounds and owner_tile_runs."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    if (seeds is None) == (seed_field is None):
        raise ValueError("give the seeds as a list (seeds) or as a field of labels (seed_field), one of the two")
    shape = [max(v, 0) for v in reversed(n)]
    steps = torch.empty(shape, dtype=torch.int32, device="cuda")
    if owner is None:
        owner = torch.empty(shape, dtype=torch.int32, device="cuda")
    elif not (isinstance(owner, torch.Tensor) and owner.is_cuda and owner.dtype == torch.int32 and owner.is_contiguous()
              and list(owner.shape) == shape):
        raise ValueError("owner is a contiguous int32 cuda tensor of the region's shape, [nz, ny, nx]")
    if seed_field is None:
        t_seeds = _cells_tensor(seeds, "seeds")
        count = int(t_seeds.shape[0])
        seed_args = (_ptr(t_seeds) if count else None, count, None)
    else:
        if isinstance(seed_field, torch.Tensor):
            if not seed_field.is_cuda or seed_field.dtype != torch.int32:
                raise ValueError("a seed_field tensor is int32 on the device")
            t_field = seed_field if seed_field is owner else seed_field.contiguous()
        else:
            t_field = torch.from_numpy(np.ascontiguousarray(np.asarray(seed_field, np.int32))).cuda()
        if list(t_field.shape) != shape:
            raise ValueError("seed_field has the shape of the region, [nz, ny, nx]")
        if not t_field.numel():                                         # no cell to point at; the pointer only says which form this is
            t_field = torch.zeros(1, dtype=torch.int32, device="cuda")
        seed_args = (None, 0, _ptr(t_field))
    st = _OwnerStats()
    check(lib().svoslam_pool_owner_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(clearance_cells),
                                         *seed_args, _ptr(steps), _ptr(owner), C.byref(st), _stream()))
    if stats is not None:
        stats.update(rounds=int(st.rounds), tile_runs=int(st.tile_runs), seeds_used=int(st.seeds_used),
                     owner_rounds=int(st.owner_rounds), owner_tile_runs=int(st.owner_tile_runs))
    return (steps, owner) if as_tensor else (steps.cpu().numpy(), owner.cpu().numpy())


def segment_rooms(ws, pool, max_depth, origin, dims, clearance_cells, door_cells, min_core=1):
    """The rooms of a region, and the doors between them: free space is eroded to the cells at least door_cells clear of every
    occupied cell, the components of what remains (label_components) are the cores, cores of fewer than min_core cells are dropped,
    and owner_field grows every core back through the cells at least clearance_cells clear (door_cells >= clearance_cells): a cell
    belongs to the core nearest by path, the smaller label on a tie.  Everything stays on the device until the end.  -> a dict of
    numpy arrays: rooms int32 [nz, ny, nx] (a room's label is its core's smallest output index; -1 = free but reached by no core,
    -2 = blocked), steps (moves to the room's core), cores (the seed field: the core's label, else -1), labels [k] ascending with
    core_sizes [k] and room_sizes [k] in cells, and doors [m, 3] int64: (a, b, faces) for every pair a < b of room labels that are
    face neighbours, faces the cell faces between them, sorted by (a, b)."""
    import torch
    if int(door_cells) < int(clearance_cells):
        raise ValueError("door_cells is at least clearance_cells: a core is part of the space it grows back through")
    cores, sizes = label_components(ws, pool, max_depth, origin, dims, int(door_cells), sizes=True, as_tensor=True)
    cores = torch.where(sizes >= max(int(min_core), 1), cores, torch.full_like(cores, -1))
    rooms = cores.clone()                                               # grown in place
    steps, rooms = owner_field(ws, pool, max_depth, origin, dims, clearance_cells, seed_field=rooms, as_tensor=True, owner=rooms)
    cells = rooms.numel()
    # every kept core reaches itself, so the rooms' labels are the kept cores' labels
    labels, room_sizes = torch.unique(rooms[rooms >= 0], return_counts=True)
    core_sizes = torch.unique(cores[cores >= 0], return_counts=True)[1]
    pairs = []
    for axis in range(3):
        if rooms.shape[axis] < 2:
            continue
        a, b = rooms.narrow(axis, 0, rooms.shape[axis] - 1).reshape(-1).long(), rooms.narrow(axis, 1, rooms.shape[axis] - 1).reshape(-1).long()
        meet = (a >= 0) & (b >= 0) & (a != b)
        a, b = a[meet], b[meet]
        pairs.append(torch.minimum(a, b) * cells + torch.maximum(a, b))
    doors = torch.zeros((0, 3), dtype=torch.int64, device=rooms.device)
    if pairs:
        keys, faces = torch.unique(torch.cat(pairs), return_counts=True)          # sorted: by a, then by b
        doors = torch.stack([keys // max(cells, 1), keys % max(cells, 1), faces], 1)
    return dict(rooms=rooms.cpu().numpy(), steps=steps.cpu().numpy(), cores=cores.cpu().numpy(), labels=labels.cpu().numpy().astype(np.int32),
                core_sizes=core_sizes.cpu().numpy(), room_sizes=room_sizes.cpu().numpy(), doors=doors.cpu().numpy())


def cost_field(ws, pool, max_depth, origin, dims, clearance_cells, comfort_cells, ring_cost, seeds, as_tensor=False, stats=None):
    """svoslam_pool_cost_field: reach_field with a weight per cell.  Entering a traversable cell costs 1 + ring_cost[j - clearance_cells
    - 1] when its nearest occupied cell is in ring j ((j - 1)^2 < dist2 <= j^2, clearance_cells < j <= comfort_cells), and 1 beyond
    comfort_cells; `ring_cost` holds comfort_cells - clearance_cells integers in 0 .. MAX_RING_COST.  The value of a cell is the
    cheapest sum over a path from any of `seeds` ([n, 3] absolute cells: an array, or an int32 cuda tensor), the seed's own weight
    left out: 0 at a seed that counts, -1 where no path leads, -2 where the cell is blocked.  With all ring costs 0 it is
    reach_field.  -> int32 [nz, ny, nx], a numpy array, or with as_tensor a cuda tensor.  The call blocks either way.  `stats`: a
    dict that receives rounds, tile_runs, seeds_used and max_weight."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    ring = [int(v) for v in np.asarray(ring_cost if ring_cost is not None else [], np.int64).reshape(-1)]
    if len(ring) != max(int(comfort_cells) - int(clearance_cells), 0):
        raise ValueError("ring_cost holds comfort_cells - clearance_cells entries")
    if any(v < 0 or v > MAX_RING_COST for v in ring):
        raise ValueError("a ring cost lies in 0 .. %d" % MAX_RING_COST)
    t_seeds = _cells_tensor(seeds, "seeds")
    count = int(t_seeds.shape[0])
    out = torch.empty([max(v, 0) for v in reversed(n)], dtype=torch.int32, device="cuda")
    st = _PlanStats()
    check(lib().svoslam_pool_cost_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(clearance_cells),
                                        int(comfort_cells), (_i32 * len(ring))(*ring) if ring else None, _ptr(t_seeds) if count else None,
                                        count, _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(rounds=int(st.rounds), tile_runs=int(st.tile_runs), seeds_used=int(st.seeds_used), max_weight=int(st.max_weight))
    return out if as_tensor else out.cpu().numpy()


def trace_paths(field, origin, dims, starts, max_cells, as_tensor=False):
    """svoslam_field_trace_paths: from every start ([n, 3] absolute cells: an array, or an int32 cuda tensor) down `field` (int32 [nz,
    ny, nx] over origin[3] .. origin + dims[3], as cost_field and reach_field return it: an array or a cuda tensor), always to the
    face neighbour in the region with the smallest value below the cell's own, the first of -x +x -y +y -z +z on a tie, until a cell
    of value 0.  -> (paths int32 [n, max_cells, 3], lengths int32 [n]): lengths[i] counts the cells of the whole path, start and
    final cell included, even beyond max_cells; only the first min(length, max_cells) rows of paths[i] are written, the rest are
    -1 here.  Length 0: the start is outside the region or on a negative value; a negative length: the array is not a cost-to-go
    field, the walk stopped after that many cells.  numpy arrays, or with as_tensor cuda tensors and nothing is synchronised."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    if isinstance(field, torch.Tensor):
        if not field.is_cuda or field.dtype != torch.int32:
            raise ValueError("a field tensor is int32 on the device")
        t_field = field.contiguous()
    else:
        t_field = torch.from_numpy(np.ascontiguousarray(np.asarray(field, np.int32))).cuda()
    if t_field.numel() != max(n[0], 0) * max(n[1], 0) * max(n[2], 0):
        raise ValueError("the field holds dims[0] * dims[1] * dims[2] values")
    t_starts = _cells_tensor(starts, "starts")
    count, cap = int(t_starts.shape[0]), int(max_cells)
    paths = torch.full((count, max(cap, 0), 3), -1, dtype=torch.int32, device="cuda")
    lengths = torch.zeros(count, dtype=torch.int32, device="cuda")
    check(lib().svoslam_field_trace_paths(_ptr(t_field) if t_field.numel() else None, (_i32 * 3)(*o), (_i32 * 3)(*n),
                                          _ptr(t_starts) if count else None, count, cap, _ptr(paths) if paths.numel() else None,
                                          _ptr(lengths) if count else None, _stream()))
    if as_tensor:
        return paths, lengths
    return paths.cpu().numpy(), lengths.cpu().numpy()


def _field_tensor(field, n):
    """a field over dims n, an array or an int32 cuda tensor -> a contiguous int32 cuda tensor"""
    import torch
    if isinstance(field, torch.Tensor):
        if not field.is_cuda or field.dtype != torch.int32:
            raise ValueError("a field tensor is int32 on the device")
        t_field = field.contiguous()
    else:
        t_field = torch.from_numpy(np.ascontiguousarray(np.asarray(field, np.int32))).cuda()
    if t_field.numel() != max(n[0], 0) * max(n[1], 0) * max(n[2], 0):
        raise ValueError("the field holds dims[0] * dims[1] * dims[2] values")
    return t_field


def segment_clearance(field, origin, dims, segments, want_cell=False, as_tensor=False):
    """svoslam_field_segment_clearance: for every segment ([n, 6] absolute cells, a xyz then b xyz: an array, or an int32 cuda
    tensor) the smallest value of `field` (int32 [nz, ny, nx] over origin[3] .. origin + dims[3], as distance_field returns it: an
    array or a cuda tensor) over a, the cells whose closed cube the centre-to-centre segment meets, and b; -1 counts as infinite
    and a cell outside the region as 0.  -> int32 [n]: 0 = the segment touches an occupied cell or leaves the region, -1 = nothing
    within the field's radius of it; with want_cell the pair (minimum, cells int32 [n, 3]): the first cell in walk order that
    attains it.  numpy arrays, or with as_tensor cuda tensors and nothing is synchronised."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    t_field = _field_tensor(field, n)
    if isinstance(segments, torch.Tensor):
        if not segments.is_cuda or segments.dtype != torch.int32:
            raise ValueError("a segments tensor is int32 on the device")
        t_seg = segments.reshape(-1, 6).contiguous()
    else:
        t_seg = torch.from_numpy(np.ascontiguousarray(np.asarray(segments, np.int32).reshape(-1, 6))).cuda()
    count = int(t_seg.shape[0])
    low = torch.zeros(count, dtype=torch.int32, device="cuda")
    at = torch.zeros((count, 3), dtype=torch.int32, device="cuda") if want_cell else None
    check(lib().svoslam_field_segment_clearance(_ptr(t_field) if t_field.numel() else None, (_i32 * 3)(*o), (_i32 * 3)(*n),
                                                _ptr(t_seg) if count else None, count, _ptr(low) if count else None,
                                                _ptr(at) if want_cell and count else None, _stream()))
    if not as_tensor:
        low, at = low.cpu().numpy(), at.cpu().numpy() if want_cell else None
    return (low, at) if want_cell else low


def shorten_paths(field, origin, dims, clearance_cells, paths, lengths, max_lookahead=0, max_vertices=None, as_tensor=False):
    """svoslam_field_shorten_paths: prune every path (paths int32 [n, max_cells, 3], lengths int32 [n], as trace_paths returns them:
    arrays or cuda tensors) into vertices joined by straight segments.  From vertex a the next one is the largest j within
    max_lookahead (0: unlimited) whose segment p_a .. p_j keeps more than clearance_cells from every occupied cell and comes no
    nearer to one than the path between a and j did, by `field` (int32 [nz, ny, nx] as distance_field returns it, WITH A RADIUS >=
    clearance_cells -- the call cannot check that); j = a + 1 always qualifies.  -> (vertices int32 [n, max_vertices], counts int32
    [n]): indices into each path, counts[i] even beyond max_vertices, unwritten entries -1 here.  max_vertices=None: two passes,
    the first for the counts alone (it blocks).  Unlimited lookahead costs O(length^2) segment walks per path in the worst case.
    numpy arrays, or with as_tensor cuda tensors."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    t_field = _field_tensor(field, n)

    def on_device(a, what):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda or a.dtype != torch.int32:
                raise ValueError("a %s tensor is int32 on the device" % what)
            return a.contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32))).cuda()
    t_paths, t_lengths = on_device(paths, "paths"), on_device(lengths, "lengths").reshape(-1)
    count = int(t_lengths.shape[0])
    if t_paths.dim() != 3 or t_paths.shape[0] != count or t_paths.shape[2] != 3:
        raise ValueError("paths is [n, max_cells, 3] for lengths [n]")
    cap = int(t_paths.shape[1])

    def run(room):
        vertices = torch.full((count, max(room, 0)), -1, dtype=torch.int32, device="cuda")
        counts = torch.zeros(count, dtype=torch.int32, device="cuda")
        check(lib().svoslam_field_shorten_paths(_ptr(t_field) if t_field.numel() else None, (_i32 * 3)(*o), (_i32 * 3)(*n),
                                                int(clearance_cells), _ptr(t_paths) if t_paths.numel() else None,
                                                _ptr(t_lengths) if count else None, count, cap, int(max_lookahead), room,
                                                _ptr(vertices) if vertices.numel() else None, _ptr(counts) if count else None,
                                                _stream()))
        return vertices, counts
    if max_vertices is None:
        _, counts = run(0)                                              # the counts alone: the room the longest result needs
        vertices, counts = run(int(counts.max()) if count else 0)
    else:
        vertices, counts = run(int(max_vertices))
    if as_tensor:
        return vertices, counts
    return vertices.cpu().numpy(), counts.cpu().numpy()


def plan_paths(ws, pool, max_depth, center, edge_length, box, goal, starts, clearance_cells, comfort_cells, ring_cost, max_cells=None,
               straighten=False, max_lookahead=0):
    """From every start to the goal (metres) through the box (metres: min xyz, max xyz) of the map, keeping clearance_cells from
    every occupied cell and paying ring_cost nearer than comfort_cells (cost_field).  The cells of the box are box_to_cells', the
    goal and the starts the cells that hold them by the same rule; the cost field is seeded at the goal's cell, computed once, and
    every start is traced down it (trace_paths).  -> None for an empty box, else a dict: cost (the field), origin, dims, cell_size,
    goal_cell (None outside the root cube), and paths, one dict per start: cell (None outside the root cube), cost and length (None
    without a path: the start or the goal is outside the box or blocked, or no path joins them), cells int32 [length, 3] from the
    start to the goal and polyline float64 [length, 3], their centres in metres (both None without a path).  max_cells: at most
    that many cells of each path are kept (length still counts them all); default: every path whole.  straighten: the kept cells
    of every path are also pruned by shorten_paths against distance_field with radius comfort_cells, at clearance_cells and
    max_lookahead (0: unlimited, O(length^2) segment walks per path in the worst case), and every path dict gains vertices (int32
    indices into cells), waypoints (int32 [k, 3], the cells at them), waypoint_polyline (float64 [k, 3], metres) and
    straight_length (the Euclidean length of that polyline in metres); all None without a path."""
    cells = box_to_cells(max_depth, center, edge_length, box)
    if cells is None:
        return None
    lo, hi = cells
    dims = hi - lo + 1

    def cell_of(point):
        at = box_to_cells(max_depth, center, edge_length, [float(v) for v in point] * 2)
        return None if at is None else at[0]
    goal_cell = cell_of(goal)
    start_cells = [cell_of(s) for s in np.asarray(starts, np.float64).reshape(-1, 3)]
    outside = lo - 1                                                    # a cell that is not in the region, for points outside the root
    cost = cost_field(ws, pool, max_depth, lo, dims, clearance_cells, comfort_cells, ring_cost,
                      [goal_cell if goal_cell is not None else outside], as_tensor=True)
    stand_ins = [c if c is not None else outside for c in start_cells]
    _, lengths = trace_paths(cost, lo, dims, stand_ins, 0)              # the lengths alone: the room the longest path needs
    room = int(lengths.max()) if len(stand_ins) else 0
    paths, lengths = trace_paths(cost, lo, dims, stand_ins, room if max_cells is None else min(room, int(max_cells)))
    cell_size = 2.0 * float(edge_length) / (1 << int(max_depth))
    corner = np.asarray(center, np.float64) - float(edge_length)
    cost = cost.cpu().numpy()
    if straighten:
        comfort = distance_field(ws, pool, max_depth, lo, dims, comfort_cells, as_tensor=True)
        vertices, counts = shorten_paths(comfort, lo, dims, clearance_cells, paths, lengths, max_lookahead=max_lookahead)
    out = []
    for k, c in enumerate(start_cells):
        n = int(lengths[k])
        if n <= 0:
            out.append(dict(cell=c, cost=None, length=None, cells=None, polyline=None))
            if straighten:
                out[-1].update(vertices=None, waypoints=None, waypoint_polyline=None, straight_length=None)
            continue
        kept = paths[k, :min(n, paths.shape[1])].copy()
        rel = c - lo
        out.append(dict(cell=c, cost=int(cost[rel[2], rel[1], rel[0]]), length=n, cells=kept,
                        polyline=corner + (kept.astype(np.float64) + 0.5) * cell_size))
        if straighten:
            at = vertices[k, :int(counts[k])].copy()
            line = corner + (kept[at].astype(np.float64) + 0.5) * cell_size
            out[-1].update(vertices=at, waypoints=kept[at], waypoint_polyline=line,
                           straight_length=float(np.sqrt((np.diff(line, axis=0) ** 2).sum(1)).sum()))
    return dict(cost=cost, origin=lo, dims=dims, cell_size=cell_size, goal_cell=goal_cell, paths=out)


UP_PLUS_Y, UP_MINUS_Y, UP_PLUS_Z, UP_MINUS_Z = 2, 3, 4, 5                # include/svoslam.h: the `up` of the ground calls
MAX_STEP_CELLS, MAX_HEIGHT_CELLS, MAX_SNAP_CELLS = 4, 256, 256          # include/svoslam.h SVOSLAM_MAX_{STEP,HEIGHT,SNAP}_CELLS
_UP_NAMES = {"+y": 2, "-y": 3, "+z": 4, "-z": 5}


def _up_code(up):
    """2..5, or one of "+y", "-y", "+z", "-z" -> the integer the library takes (another integer goes through for it to refuse)"""
    if isinstance(up, str):
        if up not in _UP_NAMES:
            raise ValueError("up is one of %s, or 2 .. 5" % ", ".join(sorted(_UP_NAMES)))
        return _UP_NAMES[up]
    return int(up)


def ground_field(ws, pool, max_depth, origin, dims, up, radius_cells, height_cells, step_cells, climb_cost, seeds, snap_cells=0,
                 as_tensor=False, stats=None):
    """svoslam_pool_ground_field: the cost-to-go field of a robot that stands on surfaces, over the region origin[3] .. origin +
    dims[3] (cells at max_depth, x y z).  `up`: 2 or "+y" (the project's convention), 3 "-y", 4 "+z", 5 "-z".  A cell is a foothold
    iff the cell under it is occupied, height_cells cells from it upwards are free, and from step_cells above it upwards no occupied
    cell of the same layer lies within radius_cells horizontally.  A move goes one cell horizontally and at most step_cells (<=
    min(height_cells - 1, MAX_STEP_CELLS)) up or down, between footholds in the region, and costs 1 + climb_cost * cells climbed.
    `seeds` ([n, 3] absolute cells: an array, or an int32 cuda tensor) are snapped downwards by at most snap_cells to their
    foothold.  -> int32 [nz, ny, nx]: 0 at a counted seed's foothold, the cheapest chain of moves from one elsewhere, -1 without a
    chain, -2 where the cell is no foothold; a numpy array, or with as_tensor a cuda tensor.  The call blocks either way.  `stats`:
    a dict that receives footholds, seeds_used, rounds and tile_runs."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    t_seeds = _cells_tensor(seeds, "seeds")
    count = int(t_seeds.shape[0])
    out = torch.empty([max(v, 0) for v in reversed(n)], dtype=torch.int32, device="cuda")
    st = _GroundStats()
    check(lib().svoslam_pool_ground_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), _up_code(up),
                                          int(radius_cells), int(height_cells), int(step_cells), int(climb_cost), int(snap_cells),
                                          _ptr(t_seeds) if count else None, count, _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(footholds=int(st.footholds), seeds_used=int(st.seeds_used), rounds=int(st.rounds), tile_runs=int(st.tile_runs))
    return out if as_tensor else out.cpu().numpy()


def trace_ground_paths(field, origin, dims, up, step_cells, climb_cost, starts, max_cells, snap_cells=0, as_tensor=False):
    """svoslam_field_trace_ground_paths: from every start ([n, 3] absolute cells: an array, or an int32 cuda tensor), snapped
    downwards by at most snap_cells to the first cell whose value is not -2, down `field` (int32 [nz, ny, nx] over origin[3] ..
    origin + dims[3], as ground_field returns it with the same up, step_cells and climb_cost: an array or a cuda tensor): from a
    cell of value v > 0 to the first cell one step away horizontally and j cells up or down whose value v' >= 0 has v' + 1 +
    climb_cost * |j| == v, the horizontal directions in the order -x, +x, then - and + along the other horizontal axis, and j = 0,
    -1, +1, -2, +2, ... within each; until a cell of value 0.  -> (paths int32 [n, max_cells, 3], lengths int32 [n]) as trace_paths
    returns them: lengths[i] counts the whole path even beyond max_cells, unwritten rows are -1 here, length 0 = no foothold under
    the start or no way from it, a negative length = not such a field.  numpy arrays, or with as_tensor cuda tensors and nothing is
    synchronised."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    t_field = _field_tensor(field, n)
    t_starts = _cells_tensor(starts, "starts")
    count, cap = int(t_starts.shape[0]), int(max_cells)
    paths = torch.full((count, max(cap, 0), 3), -1, dtype=torch.int32, device="cuda")
    lengths = torch.zeros(count, dtype=torch.int32, device="cuda")
    check(lib().svoslam_field_trace_ground_paths(_ptr(t_field) if t_field.numel() else None, (_i32 * 3)(*o), (_i32 * 3)(*n), _up_code(up),
                                                 int(step_cells), int(climb_cost), int(snap_cells), _ptr(t_starts) if count else None,
                                                 count, cap, _ptr(paths) if paths.numel() else None,
                                                 _ptr(lengths) if count else None, _stream()))
    if as_tensor:
        return paths, lengths
    return paths.cpu().numpy(), lengths.cpu().numpy()


def plan_ground_paths(ws, pool, max_depth, center, edge_length, box, goal, starts, up, radius_cells, height_cells, step_cells, climb_cost,
                      snap_cells, max_cells=None):
    """From every start to the goal (metres) over the ground of the box (metres: min xyz, max xyz) of the map, for a robot of
    radius_cells and height_cells that climbs step_cells at climb_cost a cell (ground_field).  Shaped as plan_paths: the cells of
    the box are box_to_cells', the goal and the starts the cells that hold them, each snapped downwards by at most snap_cells to
    its foothold; the field is seeded at the goal, computed once, and every start is traced down it (trace_ground_paths) twice,
    for the lengths and then for the cells.  -> None for an empty box, else a dict: cost (the field), origin, dims, cell_size,
    goal_cell (None outside the root cube), footholds, and paths, one dict per start: cell (None outside the root cube), cost,
    length and climb (None without a path), cells int32 [length, 3] from the start's foothold to the goal's and polyline float64
    [length, 3], their centres in metres (both None without a path); climb is the total of cells climbed or descended.  max_cells:
    at most that many cells of each path are kept (length still counts them all; climb then covers the kept cells)."""
    cells = box_to_cells(max_depth, center, edge_length, box)
    if cells is None:
        return None
    lo, hi = cells
    dims = hi - lo + 1
    code = _up_code(up)

    def cell_of(point):
        at = box_to_cells(max_depth, center, edge_length, [float(v) for v in point] * 2)
        return None if at is None else at[0]
    goal_cell = cell_of(goal)
    start_cells = [cell_of(s) for s in np.asarray(starts, np.float64).reshape(-1, 3)]
    outside = lo - 1                                                    # a cell that is not in the region, for points outside the root
    stats = {}
    cost = ground_field(ws, pool, max_depth, lo, dims, code, radius_cells, height_cells, step_cells, climb_cost,
                        [goal_cell if goal_cell is not None else outside], snap_cells=snap_cells, as_tensor=True, stats=stats)
    stand_ins = [c if c is not None else outside for c in start_cells]
    _, lengths = trace_ground_paths(cost, lo, dims, code, step_cells, climb_cost, stand_ins, 0, snap_cells=snap_cells)
    room = int(lengths.max()) if len(stand_ins) else 0
    paths, lengths = trace_ground_paths(cost, lo, dims, code, step_cells, climb_cost, stand_ins,
                                        room if max_cells is None else min(room, int(max_cells)), snap_cells=snap_cells)
    cell_size = 2.0 * float(edge_length) / (1 << int(max_depth))
    corner = np.asarray(center, np.float64) - float(edge_length)
    cost = cost.cpu().numpy()
    out = []
    for k, c in enumerate(start_cells):
        n = int(lengths[k])
        if n <= 0:
            out.append(dict(cell=c, cost=None, length=None, climb=None, cells=None, polyline=None))
            continue
        kept = paths[k, :min(n, paths.shape[1])].copy()
        value = None
        if len(kept):
            rel = kept[0] - lo
            value = int(cost[rel[2], rel[1], rel[0]])
        out.append(dict(cell=c, cost=value, length=n, climb=int(np.abs(np.diff(kept[:, code >> 1])).sum()), cells=kept,
                        polyline=corner + (kept.astype(np.float64) + 0.5) * cell_size))
    return dict(cost=cost, origin=lo, dims=dims, cell_size=cell_size, goal_cell=goal_cell, footholds=stats["footholds"], paths=out)


COMPONENTS_FREE, COMPONENTS_SOLID = 0, 1                                # include/svoslam.h SVOSLAM_COMPONENTS_*


def label_components(ws, pool, max_depth, origin, dims, clearance_cells, solid=False, sizes=False, as_tensor=False, stats=None):
    """svoslam_pool_label_components: the 6-connected components, inside the region origin[3] .. origin + dims[3] (cells at max_depth,
    x y z), of the cells with no occupied cell within clearance_cells (those where distance_field with that radius is -1), or with
    `solid` of the region's other cells (at clearance 0 the occupied cells).  -> int32 [nz, ny, nx]: -1 where the cell is not in the
    set, otherwise the smallest output index ((z * ny + y) * nx + x) of any cell of its component; with `sizes` the pair (labels,
    sizes), sizes the cells of the component at every cell of the set and 0 elsewhere.  numpy arrays, or with as_tensor cuda tensors,
    in which case nothing is synchronised -- unless `stats` is given: a dict that receives components, largest (0 without `sizes`),
    tile_passes and unions, for which the call blocks on one readback."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    shape = [max(v, 0) for v in reversed(n)]
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    count = torch.empty(shape, dtype=torch.int32, device="cuda") if sizes else None
    st = _ComponentStats()
    check(lib().svoslam_pool_label_components(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(clearance_cells),
                                              COMPONENTS_SOLID if solid else COMPONENTS_FREE, _ptr(out), _ptr(count),
                                              C.byref(st) if stats is not None else None, _stream()))
    if stats is not None:
        stats.update(components=int(st.components), largest=int(st.largest), tile_passes=int(st.tile_passes), unions=int(st.unions))
    if not as_tensor:
        out, count = out.cpu().numpy(), count.cpu().numpy() if sizes else None
    return (out, count) if sizes else out


NEAREST_OCCUPIED, NEAREST_FREE = 0, 1                                   # include/svoslam.h SVOSLAM_NEAREST_*


def nearest_field(ws, pool, max_depth, origin, dims, radius_cells, which=0, want=("dist2", "cell"), as_tensor=False):
    """svoslam_pool_nearest_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the nearest
    cell within radius_cells of the occupied cells (which = NEAREST_OCCUPIED) or of the root's cells that are not occupied
    (NEAREST_FREE); among equally near cells the one with the smallest z, then y, then x.  `want`: the subset of "dist2" (int32,
    squared cells, -1 = none), "cell" (uint64 x | y << 16 | z << 32, all ones = none), "node" (int32, -1) and "color" (uint32, 0) to
    compute -- node and color only for NEAREST_OCCUPIED; the others are passed as NULL.  -> a dict of [nz, ny, nx] arrays; with
    "cell" also "cell_xyz", int32 [nz, ny, nx, 3], -1 where there is none.  numpy arrays, or with as_tensor cuda tensors (cell int64,
    color int32: the same bits), in which case nothing is synchronised."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    fields = {"dist2": (torch.int32, np.int32), "cell": (torch.int64, np.uint64), "node": (torch.int32, np.int32),
              "color": (torch.int32, np.uint32)}
    names = tuple(want)
    for name in names:
        if name not in fields:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(fields)))
    shape = [max(v, 0) for v in reversed(n)]
    bufs = {name: torch.empty(shape, dtype=fields[name][0], device="cuda") for name in names}
    check(lib().svoslam_pool_nearest_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(radius_cells),
                                           int(which), *[_ptr(bufs.get(name)) for name in fields], _stream()))
    if "cell" in bufs:
        c = bufs["cell"]
        xyz = torch.stack([c & 0xFFFF, (c >> 16) & 0xFFFF, (c >> 32) & 0xFFFF], -1).to(torch.int32)
        bufs["cell_xyz"] = torch.where((c < 0).unsqueeze(-1), torch.full_like(xyz, -1), xyz)
    if as_tensor:
        return bufs
    return {name: b.cpu().numpy().view(fields[name][1]) if name in fields else b.cpu().numpy() for name, b in bufs.items()}


MAX_VIEWS_MASK = 32                                                     # include/svoslam.h SVOSLAM_MAX_VIEWS_MASK


def visibility_field(ws, pool, max_depth, origin, dims, range_cells, views, want=("mask",), as_tensor=False):
    """svoslam_pool_visibility_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the
    viewpoints that see it: `views` is [n, 3] absolute cells (an array, or an int32 cuda tensor); viewpoint k counts iff it lies in
    the root, and sees cell q iff |q - k|^2 <= range_cells^2 and no occupied cell other than the two themselves touches the segment
    between their centres (edges and corners block).  `want`: the subset of "mask" (uint32, bit k = viewpoint k sees the cell; at
    most MAX_VIEWS_MASK viewpoints) and "count" (int32, the viewpoint entries that see the cell) to compute; the other is passed as
    NULL.  -> a dict of [nz, ny, nx] arrays: numpy, or with as_tensor cuda tensors (mask int32: the same bits), in which case
    nothing is synchronised."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    fields = {"mask": (torch.int32, np.uint32), "count": (torch.int32, np.int32)}
    names = tuple(want)
    for name in names:
        if name not in fields:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(fields)))
    if isinstance(views, torch.Tensor):
        if not views.is_cuda or views.dtype != torch.int32:
            raise ValueError("a views tensor is int32 on the device")
        t_views = views.reshape(-1, 3).contiguous()
    else:
        t_views = torch.from_numpy(np.ascontiguousarray(np.asarray(views, np.int32).reshape(-1, 3))).cuda()
    count = int(t_views.shape[0])
    shape = [max(v, 0) for v in reversed(n)]
    bufs = {name: torch.empty(shape, dtype=fields[name][0], device="cuda") for name in names}
    check(lib().svoslam_pool_visibility_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(range_cells),
                                              _ptr(t_views) if count else None, count, *[_ptr(bufs.get(name)) for name in fields],
                                              _stream()))
    if as_tensor:
        return bufs
    return {name: b.cpu().numpy().view(fields[name][1]) for name, b in bufs.items()}


COVER_SURFACE, COVER_FREE, COVER_ALL = 0, 1, 2                          # include/svoslam.h SVOSLAM_COVER_*
COVER_TARGETS = {"surface": COVER_SURFACE, "free": COVER_FREE, "all": COVER_ALL}
MAX_COVER_VIEWS = 1024                                                  # include/svoslam.h SVOSLAM_MAX_COVER_VIEWS
COVER_OUTPUTS = ("seen", "chosen", "gain", "round", "summary")


def cover_views(ws, pool, max_depth, origin, dims, range_cells, candidates, k_max, min_gain=1, targets="surface", select=None,
                want=COVER_OUTPUTS, as_tensor=False):
    """svoslam_pool_cover_views: which of the `candidates` ([n, 3] absolute cells at max_depth: an array, or an int32 cuda tensor)
    see the most of the target cells of the region origin[3] .. origin + dims[3], by svoslam_pool_visibility_field's sight rule
    within range_cells, and a greedy set cover of at most k_max rounds over them: each round takes the candidate that sees the most
    targets not yet covered, the lowest index among equals, until that gain is below min_gain.  `targets`: "surface" (occupied
    cells with a free face neighbour in the root), "free" or "all", or a COVER_* value; `select`: None, or one byte per region cell
    ([nz, ny, nx]: an array, or a uint8 / bool cuda tensor) -- only cells with a non-zero byte are targets.  `want`: the subset of
    "seen" (int32 [n]: the targets each candidate sees), "chosen" and "gain" (int32 [k_max]: -1 / 0 past the end), "round" (int32
    [nz, ny, nx]: -1 not a target, -2 a target no chosen candidate sees, else the round that first covered it) and "summary"
    (int32 [4]: targets, chosen, covered, coverable) to return.  -> a dict: numpy, or with as_tensor cuda tensors.  The call itself
    reads the number of targets back once."""
    import torch
    o, n = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    names = tuple(want)
    for name in names:
        if name not in COVER_OUTPUTS:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(COVER_OUTPUTS)))
    mode = COVER_TARGETS[targets] if isinstance(targets, str) else int(targets)
    t_cands = _device_array(candidates, torch.int32, np.int32, 3, "candidates")
    count, k = int(t_cands.shape[0]), int(k_max)
    shape = [max(v, 0) for v in reversed(n)]
    t_select = None
    if select is not None:
        if isinstance(select, torch.Tensor):
            if not select.is_cuda or select.dtype not in (torch.uint8, torch.bool):
                raise ValueError("a select tensor is uint8 or bool on the device")
            t_select = select.contiguous().view(torch.uint8)
        else:
            t_select = torch.from_numpy(np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)).cuda()
        if t_select.numel() != shape[0] * shape[1] * shape[2]:
            raise ValueError("select has one byte per region cell")
    bufs = {"summary": torch.empty(4, dtype=torch.int32, device="cuda")}
    if "seen" in names:
        bufs["seen"] = torch.zeros(count, dtype=torch.int32, device="cuda")      # a region without cells leaves it unwritten
    if k > 0 or "chosen" in names or "gain" in names:
        bufs["chosen"] = torch.empty(max(k, 0), dtype=torch.int32, device="cuda")
        bufs["gain"] = torch.empty(max(k, 0), dtype=torch.int32, device="cuda")
    if "round" in names:
        bufs["round"] = torch.empty(shape, dtype=torch.int32, device="cuda")
    check(lib().svoslam_pool_cover_views(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n), int(range_cells), mode,
                                         _ptr(t_select), _ptr(t_cands) if count else None, count, k, int(min_gain),
                                         *[_ptr(bufs.get(name)) if name not in ("chosen", "gain") or k > 0 else None
                                           for name in COVER_OUTPUTS], _stream()))
    out = {name: bufs[name] for name in names}
    return out if as_tensor else {name: b.cpu().numpy() for name, b in out.items()}


OBS_THROUGH, OBS_END = 1, 2                                             # include/svoslam.h SVOSLAM_OBS_*
STATE_UNKNOWN, STATE_FREE, STATE_FRONTIER, STATE_OCCUPIED, STATE_VACATED, STATE_UNMAPPED = range(6)   # include/svoslam.h SVOSLAM_STATE_*
STATE_NAMES = ("unknown", "free", "frontier", "occupied", "vacated", "unmapped")
FRONTIER_OUTPUTS = ("state", "frontier", "summary")


def observe_rays(ws, obs, max_depth, center, edge_length, origin, dims, points, poses, range_cells=0, accumulate=False, as_tensor=False):
    """svoslam_field_observe_rays: what the sensor rays of `poses` ([F, 16] float32, sensor to world, the layout of every trans[16])
    and `points` ([F, n, 3] float32 in the sensor frame, frame f's points with pose f; e.g. vertex maps) have seen of the region
    origin[3] .. origin + dims[3] (cells at max_depth, x y z): per cell bit OBS_THROUGH, a ray passed through it, and bit OBS_END, a
    ray ended in it.  A point that is not finite is void; a ray with an end outside the root is outside; with range_cells > 0 a ray
    longer than that many cells is far, and skipped whole.  `obs`: None for a new array, or the uint8 [nz, ny, nx] to write (an
    array, or a uint8 cuda tensor, which is written in place); with `accumulate` the marks are ORed into it and its bits 2..7 are
    kept, else it is overwritten.  points and poses may be cuda tensors (used in place) or arrays (uploaded).  -> (obs, summary):
    summary is int64 [6] = rays void, outside, far, marked, then the region cells with THROUGH and with END after the call.  numpy,
    or with as_tensor cuda tensors, in which case nothing is synchronised."""
    import torch
    o, n3 = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n3) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    shape = [max(v, 0) for v in reversed(n3)]
    t_poses = _device_array(poses, torch.float32, np.float32, 16, "poses")
    t_points = _device_array(points, torch.float32, np.float32, 3, "points")
    frames = int(t_poses.shape[0])
    rows = int(t_points.shape[0])
    if (frames == 0 and rows != 0) or (frames > 0 and rows % frames != 0):
        raise ValueError("%d points are not %d frames of equally many" % (rows, frames))
    n = rows // frames if frames else 0
    if obs is None:
        if accumulate:
            raise ValueError("accumulate needs the obs to add to")
        t_obs = torch.empty(shape, dtype=torch.uint8, device="cuda")
    elif isinstance(obs, torch.Tensor):
        if not obs.is_cuda or obs.dtype != torch.uint8 or not obs.is_contiguous():
            raise ValueError("an obs tensor is contiguous uint8 on the device")
        t_obs = obs
    else:
        t_obs = torch.from_numpy(np.ascontiguousarray(np.asarray(obs, np.uint8))).cuda()
    if t_obs.numel() != shape[0] * shape[1] * shape[2]:
        raise ValueError("obs has one byte per region cell")
    t_obs = t_obs.view(shape)
    summary = torch.empty(6, dtype=torch.int64, device="cuda")
    check(lib().svoslam_field_observe_rays(ws._h, _ptr(t_obs) if t_obs.numel() else None, int(max_depth), _fa(center, 3), float(edge_length),
                                           (_i32 * 3)(*o), (_i32 * 3)(*n3), _ptr(t_points) if n * frames else None, n,
                                           _ptr(t_poses) if n * frames else None, frames, int(range_cells), 1 if accumulate else 0,
                                           _ptr(summary), _stream()))
    if as_tensor:
        return t_obs, summary
    return t_obs.cpu().numpy(), summary.cpu().numpy()


def frontier_field(ws, pool, max_depth, origin, dims, obs, want=FRONTIER_OUTPUTS, as_tensor=False):
    """svoslam_pool_frontier_field: observe_rays' `obs` (uint8 [nz, ny, nx]: an array, or a uint8 cuda tensor) held against the map
    over the region origin[3] .. origin + dims[3]: "state" (uint8 [nz, ny, nx]: STATE_UNKNOWN, STATE_FREE, STATE_FRONTIER -- free
    with a face neighbour in the region that is unknown --, STATE_OCCUPIED, STATE_VACATED -- occupied, rays passed through it and
    none ended in it --, STATE_UNMAPPED -- a ray ended where the map has nothing), "frontier" (uint8 [nz, ny, nx]: 1 where the state
    is STATE_FRONTIER; cover_views' select) and "summary" (int32 [6]: the cells per state).  `want`: the subset to compute; the
    others are passed as NULL.  -> a dict: numpy, or with as_tensor cuda tensors, in which case nothing is synchronised."""
    import torch
    o, n3 = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n3) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    names = tuple(want)
    for name in names:
        if name not in FRONTIER_OUTPUTS:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(FRONTIER_OUTPUTS)))
    shape = [max(v, 0) for v in reversed(n3)]
    if isinstance(obs, torch.Tensor):
        if not obs.is_cuda or obs.dtype != torch.uint8:
            raise ValueError("an obs tensor is uint8 on the device")
        t_obs = obs.contiguous()
    else:
        t_obs = torch.from_numpy(np.ascontiguousarray(np.asarray(obs, np.uint8))).cuda()
    if t_obs.numel() != shape[0] * shape[1] * shape[2]:
        raise ValueError("obs has one byte per region cell")
    bufs = {name: torch.empty(6, dtype=torch.int32, device="cuda") if name == "summary" else torch.empty(shape, dtype=torch.uint8, device="cuda")
            for name in names}
    check(lib().svoslam_pool_frontier_field(ws._h, C.byref(pool._p), int(max_depth), (_i32 * 3)(*o), (_i32 * 3)(*n3),
                                            _ptr(t_obs) if t_obs.numel() else None, *[_ptr(bufs.get(name)) for name in FRONTIER_OUTPUTS],
                                            _stream()))
    return bufs if as_tensor else {name: b.cpu().numpy() for name, b in bufs.items()}


def explore_views(ws, pool, max_depth, origin, dims, obs, candidates, range_cells, k_max, min_gain=1):
    """Where to look next: frontier_field of `obs`, then cover_views of the region's free cells selected by the frontier bytes --
    which few of the `candidates` ([n, 3] absolute cells) see the most of the boundary between the observed free space and the
    unknown within range_cells.  The frontier stays on the device between the two calls.  -> (frontier_field's dict, cover_views'
    dict), numpy."""
    field = frontier_field(ws, pool, max_depth, origin, dims, obs, as_tensor=True)
    cover = cover_views(ws, pool, max_depth, origin, dims, range_cells, candidates, k_max, min_gain, "free", field["frontier"])
    return {name: b.cpu().numpy() for name, b in field.items()}, cover


MAX_MISS_COST = 1 << 30                                                 # include/svoslam.h SVOSLAM_MAX_MISS_COST
SCORE_OUTPUTS = ("cost", "near", "far", "outside", "best")


def _device_array(a, torch_dtype, np_dtype, width, what):
    """a cuda tensor of that type as it is, anything else uploaded: -> a contiguous [rows, width] cuda tensor"""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_cuda or a.dtype != torch_dtype:
            raise ValueError("a %s tensor is %s on the device" % (what, str(torch_dtype).replace("torch.", "")))
        return a.reshape(-1, width).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np_dtype).reshape(-1, width))).cuda()


def score_poses(ws, field, max_depth, center, edge_length, origin, dims, points, poses, miss_cost, min_near=0, want=("cost", "near"),
                as_tensor=False):
    """svoslam_score_poses: every one of `points` ([n, 3] float32 in the sensor frame, e.g. a vertex map; a non-finite point counts
    nowhere) moved by every one of `poses` ([P, 16] float32, sensor to world, the layout of every trans[16]) and looked up in
    `field`, the int32 [nz, ny, nx] distance field of the region origin[3] .. origin + dims[3] (distance_field's or nearest_field's
    dist2 with the same max_depth, origin and dims).  Per pose: "cost" int64 = the sum of the field's values where it has one +
    miss_cost * the pairs where it has none or that fall outside the region, and the counts "near", "far", "outside" (int32).
    "best": int64 (cost, index) of the cheapest pose with near >= min_near, the lowest index among equals, (-1, -1) if none.
    field, points and poses may be cuda tensors (used in place) or arrays (uploaded).  `want`: the subset to compute; the others are
    passed as NULL.  -> a dict of numpy arrays, or with as_tensor cuda tensors, in which case nothing is synchronised."""
    import torch
    o, n3 = [int(v) for v in origin], [int(v) for v in dims]
    if len(o) != 3 or len(n3) != 3:
        raise ValueError("origin and dims are three cells each (x, y, z)")
    names = tuple(want)
    for name in names:
        if name not in SCORE_OUTPUTS:
            raise KeyError("no output %r (have: %s)" % (name, ", ".join(SCORE_OUTPUTS)))
    t_field = _device_array(field, torch.int32, np.int32, 1, "field")
    cells = max(n3[0], 0) * max(n3[1], 0) * max(n3[2], 0)
    if int(t_field.shape[0]) != cells:
        raise ValueError("the field has %d values, the region %d cells" % (int(t_field.shape[0]), cells))
    t_points = _device_array(points, torch.float32, np.float32, 3, "points")
    t_poses = _device_array(poses, torch.float32, np.float32, 16, "poses")
    n, count = int(t_points.shape[0]), int(t_poses.shape[0])
    bufs = {name: torch.empty(2 if name == "best" else count, dtype=torch.int64 if name in ("cost", "best") else torch.int32, device="cuda")
            for name in names}
    check(lib().svoslam_score_poses(ws._h, _ptr(t_field) if cells else None, int(max_depth), _fa(center, 3), float(edge_length),
                                    (_i32 * 3)(*o), (_i32 * 3)(*n3), _ptr(t_points) if n else None, n, _ptr(t_poses) if count else None,
                                    count, int(miss_cost), int(min_near), *[_ptr(bufs.get(name)) for name in SCORE_OUTPUTS], _stream()))
    if as_tensor:
        return bufs
    return {name: b.cpu().numpy() for name, b in bufs.items()}


def _rotation(axis, angle):
    """Rodrigues' rotation about the unit vector along `axis`, float64 [3, 3]; exactly the identity at angle 0"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _symmetric_steps(half, steps):
    """`steps` evenly spaced values from -half to half: exactly symmetric, the middle one of an odd number exactly 0"""
    steps = int(steps)
    if steps < 1:
        raise ValueError("at least one step per axis")
    if steps == 1:
        return np.zeros(1)
    return (np.arange(steps, dtype=np.float64) - (steps - 1) / 2.0) * (2.0 * float(half) / (steps - 1))


def pose_grid(prior, half_extent, steps, yaw_half, yaw_steps, up=(0, 1, 0)):
    """A grid of candidate poses around `prior` (16 floats, sensor to world, the layout of every trans[16]) for score_poses: host only.
    Candidate = T(dx, dy, dz) . prior . R_up(yaw): the sensor moved by (dx, dy, dz) in the world and turned by yaw (radians) about
    its own `up` axis.  Offsets run over steps[a] evenly spaced values in [-half_extent[a], half_extent[a]] per world axis, yaws over
    yaw_steps values in [-yaw_half, yaw_half]; both symmetric about 0, a single step is 0.  ORDER: z slowest, then y, then x, yaw
    fastest: index = ((iz * steps[1] + iy) * steps[0] + ix) * yaw_steps + iyaw.  Computed in float64 and rounded once; with odd step
    counts the middle candidate is `prior` bit for bit.  -> float32 [steps[0] * steps[1] * steps[2] * yaw_steps, 16]."""
    prior32 = np.asarray(prior, np.float32).reshape(16)
    M = prior32.astype(np.float64).reshape(4, 4).T                      # column-major storage -> M[row, col]
    offs = [_symmetric_steps(half_extent[a], steps[a]) for a in range(3)]
    yaws = _symmetric_steps(yaw_half, yaw_steps)
    turned = np.empty((len(yaws), 4, 4))
    for k, yaw in enumerate(yaws):
        R = np.eye(4)
        R[:3, :3] = _rotation(up, yaw)
        turned[k] = M @ R
    dz, dy, dx = np.meshgrid(offs[2], offs[1], offs[0], indexing="ij")
    shift = np.stack([dx, dy, dz], -1).reshape(-1, 1, 3)               # z slowest, x fastest
    out = np.broadcast_to(turned, (shift.shape[0],) + turned.shape).copy()
    out[:, :, :3, 3] += shift
    grid = np.ascontiguousarray(out.transpose(0, 1, 3, 2)).reshape(-1, 16).astype(np.float32)
    still = (np.broadcast_to(shift == 0.0, out.shape[:2] + (3,)).all(-1) & (yaws == 0.0)[None, :]).reshape(-1)
    grid[still] = prior32                                               # -0.0 + 0.0 is +0.0: the unmoved candidate is the prior's own bits
    return grid


def relocalize(ws, pool, max_depth, center, edge_length, points, prior, half_extent, yaw_half, radius_cells, steps=(9, 9, 9), yaw_steps=9,
               rounds=3, min_near_fraction=0.5, up=(0, 1, 0)):
    """Where in this map were these points seen?  A coarse-to-fine search with score_poses around `prior` (16 floats, sensor to world):
    `points` ([n, 3] float32 in the sensor frame, a cuda tensor or an array; non-finite = no measurement), half_extent[3] in metres
    per world axis and yaw_half in radians about the sensor's `up` axis are the first round's pose_grid; every round scores its
    grid, re-centres on the best pose if that is strictly cheaper than the centre it came from, and halves extents and yaw.  The
    distance field (radius_cells, miss cost radius_cells^2 + 1) is built once, over the box of cells the search can reach, and
    stays on the device; every round reads back only the two words of `best`.  A pose qualifies with near >= ceil(min_near_fraction
    * the finite points).  -> {"pose": float32 [16], "cost": int, "near": int, "rounds": [(cost, index) per round]}, or None when
    no pose of some round qualifies (the rounds so far are then lost: nothing was found)."""
    import torch
    t_points = _device_array(points, torch.float32, np.float32, 3, "points")
    prior32 = np.asarray(prior, np.float32).reshape(16)
    finite = torch.isfinite(t_points).all(1)
    n_finite = int(finite.sum().item())
    if n_finite == 0:
        return None
    # the box the search can reach: the points under the prior, moved by at most the sum of all rounds' extents (< 2 x the first)
    # and turned by at most the sum of all rounds' yaws about the sensor's origin (a chord of the farthest point's circle)
    live = t_points[finite].double()
    M = torch.from_numpy(prior32.astype(np.float64).reshape(4, 4).T.copy()).cuda()
    world = live @ M[:3, :3].T + M[:3, 3]
    chord = 2.0 * float(live.norm(dim=1).max().item()) * np.sin(min(2.0 * abs(float(yaw_half)), np.pi) / 2.0)
    cell = 2.0 * float(edge_length) / (1 << int(max_depth))
    slack = np.array([2.0 * abs(float(e)) for e in half_extent]) + chord + cell
    box = np.concatenate([world.min(0).values.cpu().numpy() - slack, world.max(0).values.cpu().numpy() + slack]).astype(np.float32)
    cells = box_to_cells(max_depth, center, edge_length, box)
    if cells is None:
        return None                                                     # the search cannot reach the root
    origin, dims = cells[0], cells[1] - cells[0] + 1
    field = distance_field(ws, pool, max_depth, origin, dims, radius_cells, as_tensor=True)
    miss, min_near = int(radius_cells) * int(radius_cells) + 1, int(np.ceil(float(min_near_fraction) * n_finite))
    pose, extent, yaw, found, best_cost = prior32, np.asarray(half_extent, np.float64), float(yaw_half), [], None
    for _ in range(int(rounds)):
        grid = pose_grid(pose, extent, steps, yaw, yaw_steps, up)
        best = score_poses(ws, field, max_depth, center, edge_length, origin, dims, t_points, grid, miss, min_near, want=("best",))["best"]
        cost, index = int(best[0]), int(best[1])
        if index < 0:
            return None
        found.append((cost, index))
        if best_cost is None or cost < best_cost:                       # an equally cheap neighbour does not move the centre
            pose, best_cost = grid[index], cost
        extent, yaw = extent / 2.0, yaw / 2.0
    last = score_poses(ws, field, max_depth, center, edge_length, origin, dims, t_points, pose.reshape(1, 16), miss, 0, want=("cost", "near"))
    return {"pose": pose.copy(), "cost": int(last["cost"][0]), "near": int(last["near"][0]), "rounds": found}


def box_to_cells(max_depth, center, edge_length, box):
    """svoslam_box_to_cells (host only): the inclusive cell range (lo[3], hi[3]) at max_depth of the axis-aligned box[6] (min xyz, max
    xyz; infinities allowed) exactly as count_boxes takes it, or None for an empty box (a NaN, min > max, outside the root).  The
    field of that box: distance_field(ws, pool, max_depth, lo, hi - lo + 1, radius_cells)."""
    lo, hi, empty = (_i32 * 3)(), (_i32 * 3)(), _i32(0)
    check(lib().svoslam_box_to_cells(int(max_depth), _fa(center, 3), float(edge_length), _fa(box, 6), lo, hi, C.byref(empty)))
    if empty.value:
        return None
    return np.array(lo[:], np.int32), np.array(hi[:], np.int32)


# ----------------------------------------------------------------------------- mesh path
class Mesh:
    """Host mesh as Scene::loadObjFile builds it (recentred, non-indexed)."""

    def __init__(self, path=None):
        self._m = MeshStruct()
        if path is not None:
            check(lib().svoslam_mesh_load_obj(str(path).encode(), C.byref(self._m)))

    @property
    def n_tris(self):
        return int(self._m.n_tris)

    def vbo(self):
        return np.ctypeslib.as_array(self._m.vbo, shape=(self.n_tris, 3, 3)).copy() if self.n_tris else np.zeros((0, 3, 3), np.float32)

    def tbo(self):
        n = int(self._m.tbosize)
        return np.ctypeslib.as_array(self._m.tbo, shape=(n // 6, 3, 2)).copy() if n else None

    def bbox(self):
        return np.array(list(self._m.bbox0), np.float32), np.array(list(self._m.bbox1), np.float32)

    def __del__(self):
        try:
            lib().svoslam_mesh_free(C.byref(self._m))
        except Exception:
            pass


class Texture:
    def __init__(self, path=None):
        self._t = TextureStruct()
        if path is not None:
            check(lib().svoslam_texture_load_bmp(str(path).encode(), C.byref(self._t)))

    def data(self):
        h, w = int(self._t.height), int(self._t.width)
        return np.ctypeslib.as_array(self._t.data, shape=(h, w, 3)).copy()

    def __del__(self):
        try:
            lib().svoslam_texture_free(C.byref(self._t))
        except Exception:
            pass


def mesh_to_voxel_grid(ws, mesh, tex, log_n, log_t=3, want_indices=True):
    """voxelization::meshToVoxelGrid -> (centers cuda [n,4], colors cuda [n,4], indices numpy or None, scale)."""
    import torch
    pc, pk, pi, n, scale = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_float(0)
    check(lib().svoslam_mesh_to_voxel_grid(ws._h, C.byref(mesh._m), C.byref(tex._t) if tex is not None else None, log_n, log_t,
                                           C.byref(pc), C.byref(pk), C.byref(pi) if want_indices else None, C.byref(n),
                                           C.byref(scale), _stream()))
    torch.cuda.synchronize()
    cnt = n.value
    ce = torch.empty((cnt, 4), dtype=torch.float32, device="cuda")
    co = torch.empty((cnt, 4), dtype=torch.float32, device="cuda")
    idx = None
    if cnt > 0:
        _hip().hipMemcpy(C.c_void_p(ce.data_ptr()), pc, C.c_size_t(cnt * 16), 3)
        _hip().hipMemcpy(C.c_void_p(co.data_ptr()), pk, C.c_size_t(cnt * 16), 3)
        lib().svoslam_free(pc); lib().svoslam_free(pk)
        if want_indices:
            idx = np.empty(cnt, np.uint64)
            _hip().hipMemcpy(C.c_void_p(idx.ctypes.data), pi, C.c_size_t(cnt * 8), 2)
            lib().svoslam_free(pi)
    return ce, co, idx, float(scale.value)


def mesh_last_fragments(ws):
    """(cell, triangle) fragments of the workspace's last mesh_to_voxel_grid (measurement aid)"""
    n = C.c_int64(0)
    check(lib().svoslam_mesh_last_fragments(ws._h, C.byref(n)))
    return int(n.value)


def voxel_grid_to_mesh(ws, centers, colors, scale_factor, cube_vbo, cube_ibo, cube_nbo):
    """voxelization::voxelGridToMesh: centers, colors cuda float32 [n,4]; cube arrays numpy -> cuda (vbo, ibo, nbo, cbo)."""
    import torch
    cv = np.ascontiguousarray(cube_vbo, np.float32).reshape(-1)
    cn = np.ascontiguousarray(cube_nbo, np.float32).reshape(-1)
    ci = np.ascontiguousarray(cube_ibo, np.int32).reshape(-1)
    if cv.size != cn.size:
        raise ValueError("cube vbo and nbo have different sizes")
    n = int(centers.shape[0])
    vbo, nbo, cbo = (torch.empty(n * cv.size, dtype=torch.float32, device="cuda") for _ in range(3))
    ibo = torch.empty(n * ci.size, dtype=torch.int32, device="cuda")
    check(lib().svoslam_voxel_grid_to_mesh(ws._h, _ptr(centers), _ptr(colors), n, float(scale_factor),
                                           cv.ctypes.data_as(_fp), cv.size, ci.ctypes.data_as(C.POINTER(C.c_int32)), ci.size,
                                           cn.ctypes.data_as(_fp), _ptr(vbo), _ptr(ibo), _ptr(nbo), _ptr(cbo), _stream()))
    return vbo, ibo, nbo, cbo


class Runner:
    """Native frame scheduler (csrc/runner.hip): track -> back-project -> fuse -> raycast of a list of frames on four
    HIP streams, enqueued by ONE call."""

    def __init__(self, cam, pool, width, height, max_depth, center, edge, fx, fy, render_mode):
        self._h = C.c_void_p()
        self._cam, self._pool = cam, pool          # keep the handles alive
        check(lib().svoslam_runner_create(C.byref(self._h), cam._h, C.byref(pool._p), width, height, max_depth, _fa(center, 3),
                                          float(edge), float(fx), float(fy), int(render_mode)))

    def run(self, depths, rgbs, timestamps, views, image, row_first, rows, counters=None):
        n = len(timestamps)
        dp = (C.c_void_p * n)(*[d.data_ptr() for d in depths])
        rp = (C.c_void_p * n)(*[r.data_ptr() for r in rgbs])
        ts = (C.c_longlong * n)(*[int(t) for t in timestamps])
        vw = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(16) for v in views]), np.float32)
        check(lib().svoslam_runner_run(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, _ptr(image), int(row_first), int(rows),
                                       _ptr(counters), _stream()))

    def run_sharded(self, depths, rgbs, timestamps, views, deltas, delta_events, march, images, row_first, rows, counters=None):
        """one rank of a frame-sharded session (svoslam_runner_run_sharded): deltas = per-frame tensors (or None) of
        DELTA_FLOATS floats, delta_events = per-frame torch.cuda.Event (recorded) or None, march = per-frame bool,
        images = per-frame output tensor (or None where march is False)"""
        n = len(timestamps)
        dp = (C.c_void_p * n)(*[d.data_ptr() for d in depths])
        rp = (C.c_void_p * n)(*[r.data_ptr() for r in rgbs])
        ts = (C.c_longlong * n)(*[int(t) for t in timestamps])
        vw = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(16) for v in views]), np.float32)
        dl = (C.c_void_p * n)(*[(d.data_ptr() if d is not None else None) for d in deltas])
        ev = (C.c_void_p * n)(*[(e.cuda_event if e is not None else None) for e in delta_events]) if delta_events is not None else None
        mf = (C.c_uint8 * n)(*[1 if m else 0 for m in march])
        im = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in images])
        self._keep = (depths, rgbs, deltas, delta_events, images)   # alive until the next call (the work is asynchronous)
        check(lib().svoslam_runner_run_sharded(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, dl, ev, mf, im, int(row_first), int(rows),
                                               _ptr(counters), _stream()))

    def run_sharded_presorted(self, depths, rgbs, timestamps, views, deltas, delta_events, march, images, sorted_keys, sorted_idx,
                              sorted_events, row_first, rows, counters=None):
        """run_sharded with every frame's sorted keys / point indices supplied (svoslam_runner_run_sharded_presorted):
        sorted_keys / sorted_idx = per-frame int64 / int32 cuda tensors, sorted_events = per-frame torch.cuda.Event or None"""
        n = len(timestamps)
        dp = (C.c_void_p * n)(*[d.data_ptr() for d in depths])
        rp = (C.c_void_p * n)(*[r.data_ptr() for r in rgbs])
        ts = (C.c_longlong * n)(*[int(t) for t in timestamps])
        vw = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(16) for v in views]), np.float32)
        dl = (C.c_void_p * n)(*[(d.data_ptr() if d is not None else None) for d in deltas])
        ev = (C.c_void_p * n)(*[(e.cuda_event if e is not None else None) for e in delta_events]) if delta_events is not None else None
        mf = (C.c_uint8 * n)(*[1 if m else 0 for m in march])
        im = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in images])
        sk = (C.c_void_p * n)(*[k.data_ptr() for k in sorted_keys])
        si = (C.c_void_p * n)(*[k.data_ptr() for k in sorted_idx])
        se = (C.c_void_p * n)(*[(e.cuda_event if e is not None else None) for e in sorted_events]) if sorted_events is not None else None
        self._keep = (depths, rgbs, deltas, delta_events, images, sorted_keys, sorted_idx, sorted_events)
        check(lib().svoslam_runner_run_sharded_presorted(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, dl, ev, mf, im, sk, si, se,
                                                         int(row_first), int(rows), _ptr(counters), _stream()))

    def run_model(self, depths, rgbs, timestamps, views, image, row_first, rows, min_coverage=0.5, counters=None):
        """the frame loop with frame-to-model tracking inside the library (svoslam_runner_run_model); returns the number of frames
        whose ray-cast model was accepted.  Blocking."""
        n = len(timestamps)
        dp = (C.c_void_p * n)(*[d.data_ptr() for d in depths])
        rp = (C.c_void_p * n)(*[r.data_ptr() for r in rgbs])
        ts = (C.c_longlong * n)(*[int(t) for t in timestamps])
        vw = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(16) for v in views]), np.float32)
        used = C.c_int32(0)
        check(lib().svoslam_runner_run_model(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, _ptr(image), int(row_first), int(rows),
                                             _ptr(counters), float(min_coverage), C.byref(used), _stream()))
        return int(used.value)

    def bbox(self):
        """{min xyz, max xyz, any} of the last frame's point cloud (main.cpp:43)"""
        b = (C.c_float * 7)()
        check(lib().svoslam_runner_bbox(self._h, b))
        return np.array(list(b), np.float32)

    def timeline(self, max_frames=4096):
        """[frames, 10] stage times in ms of the last run (svoslam_config.runner_timeline = 1 when the runner was created)"""
        out = np.full((max_frames, 10), -1.0, np.float32)
        n = _i32(0)
        check(lib().svoslam_runner_timeline(self._h, out.ctypes.data_as(_fp), max_frames, C.byref(n)))
        return out[: n.value]

    def close(self):
        if self._h:
            lib().svoslam_runner_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mailbox:
    """One-shot peer-to-peer exchange of small records between the ranks of a node (csrc/mailbox.hip): all_gather of up to
    2 KB per rank, all_reduce of up to 256 float64 added in rank order; enqueued on the current stream, no host round trip."""

    def __init__(self, rank, world):
        self._h = C.c_void_p()
        self.rank, self.world = int(rank), int(world)
        check(lib().svoslam_mailbox_create(C.byref(self._h), self.rank, self.world))

    def handle(self):
        """64 bytes (numpy uint8) that the other PROCESSES need to map this rank's inbox"""
        buf = (C.c_uint8 * 64)()
        check(lib().svoslam_mailbox_handle(self._h, buf))
        return np.frombuffer(bytes(buf), dtype=np.uint8).copy()

    def connect(self, handles):
        """handles: uint8 array [world, 64], row r from rank r (this rank's own row is ignored)"""
        h = np.ascontiguousarray(handles, dtype=np.uint8)
        assert h.shape == (self.world, 64)
        check(lib().svoslam_mailbox_connect(self._h, h.ctypes.data_as(C.c_void_p)))

    def connect_local(self, boxes):
        """all mailboxes of the session live in this process (tests; one process driving several devices)"""
        arr = (C.c_void_p * self.world)(*[b._h for b in boxes])
        check(lib().svoslam_mailbox_connect_local(self._h, arr))

    def all_gather(self, src, dst):
        """dst[world, ...] <- every rank's src (same byte count on every rank, a multiple of 4, <= 2048)"""
        nbytes = src.numel() * src.element_size()
        assert dst.numel() * dst.element_size() == nbytes * self.world
        check(lib().svoslam_mailbox_all_gather(self._h, _ptr(src), nbytes, _ptr(dst), _stream()))

    def all_reduce_f64(self, values):
        """values (float64 cuda tensor, <= 256 entries) <- sum over ranks, added in rank order: the same bits everywhere"""
        check(lib().svoslam_mailbox_all_reduce_f64(self._h, _ptr(values), int(values.numel()), _stream()))

    def post(self, src):
        """first half of a collective: this rank's record into every inbox"""
        check(lib().svoslam_mailbox_post(self._h, _ptr(src), src.numel() * src.element_size(), _stream()))

    def collect(self, dst, nbytes, reduce_f64=False):
        """second half: every rank's record of the epoch just posted -> dst[world, ...] (or their rank-ordered float64 sum)"""
        check(lib().svoslam_mailbox_collect(self._h, _ptr(dst), int(nbytes), 1 if reduce_f64 else 0, _stream()))

    def set_wait_limit(self, polls):
        check(lib().svoslam_mailbox_set_wait_limit(self._h, int(polls)))

    def failed(self):
        f = _i32(0)
        check(lib().svoslam_mailbox_failed(self._h, C.byref(f)))
        return bool(f.value)

    def close(self):
        if self._h:
            lib().svoslam_mailbox_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """Mirror of world::Scene (include/octree_slam/world/scene.h)."""

    def __init__(self):
        self._h = C.c_void_p()
        check(lib().svoslam_scene_create(C.byref(self._h)))

    def load_obj(self, path):
        check(lib().svoslam_scene_load_obj(self._h, str(path).encode()))

    def load_bmp(self, path):
        check(lib().svoslam_scene_load_bmp(self._h, str(path).encode()))

    def set_octree(self, resolution, center, size, depth_override=0):
        check(lib().svoslam_scene_set_octree(self._h, float(resolution), _fa(center, 3), float(size), int(depth_override)))

    def voxelize_meshes(self, octree=False, log_n=0):
        check(lib().svoslam_scene_voxelize_meshes(self._h, 1 if octree else 0, int(log_n), _stream()))

    def extract_voxel_grid_from_octree(self):
        check(lib().svoslam_scene_extract_voxel_grid(self._h, _stream()))

    def add_point_cloud_to_octree(self, origin, points, colors, bbox0, bbox1):
        check(lib().svoslam_scene_add_point_cloud(self._h, _fa(origin, 3), _ptr(points), _ptr(colors), int(points.numel() // 3),
                                                  _fa(bbox0, 3), _fa(bbox1, 3), _stream()))

    def voxel_grid(self):
        pc, pk, n, sc = C.c_void_p(), C.c_void_p(), C.c_int32(0), C.c_float(0)
        check(lib().svoslam_scene_voxel_grid(self._h, C.byref(pc), C.byref(pk), C.byref(n), C.byref(sc)))
        ce = copy_from_device(pc.value, (n.value, 4), np.float32) if n.value else np.zeros((0, 4), np.float32)
        co = copy_from_device(pk.value, (n.value, 4), np.float32) if n.value else np.zeros((0, 4), np.float32)
        return ce, co, float(sc.value)

    def svo(self):
        """-> dict(data_ptr, center, size, num_nodes, max_depth): the SVO view of Scene::svo()."""
        pd, c, sz, nn, md = C.c_void_p(), (C.c_float * 3)(), C.c_float(0), C.c_int32(0), C.c_int32(0)
        check(lib().svoslam_scene_svo(self._h, C.byref(pd), c, C.byref(sz), C.byref(nn), C.byref(md)))
        return {"data_ptr": int(pd.value or 0), "center": np.array(list(c), np.float32), "size": float(sz.value),
                "num_nodes": int(nn.value), "max_depth": int(md.value)}

    def pool_words(self):
        v = self.svo()
        return copy_from_device(v["data_ptr"], (2 * v["num_nodes"],), np.uint32)

    def close(self):
        if self._h:
            lib().svoslam_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- rendering
def cone_trace_svo(out, fov, view, pool_ptr, center, size, mode=RENDER_REFERENCE, counters=None):
    """rendering::coneTraceSVO into `out` (cuda uint8 [h,w,4])."""
    h, w = int(out.shape[0]), int(out.shape[1])
    check(lib().svoslam_cone_trace_svo(_ptr(out), w, h, float(fov), _fa(view, 16), C.c_void_p(int(pool_ptr)),
                                       _fa(center, 3), float(size), int(mode), _ptr(counters), _stream()))
    return out


def raycast_model_depth(out, fx, fy, pool_ptr, center, size, cam_to_world=None, cam_to_world_ptr=None, counters=None):
    """the map ray-cast into a depth image in the sensor's pixel grid (`out`: cuda uint16 [h, w]); the pose as a host matrix
    (16 floats, column-major: the fusion transform) or as a device pointer (Camera.fusion_transform_ptr()).  Own
    specification: include/svoslam.h, svoslam_raycast_model_depth."""
    h, w = int(out.shape[0]), int(out.shape[1])
    if (cam_to_world is None) == (cam_to_world_ptr is None):
        raise ValueError("exactly one of cam_to_world / cam_to_world_ptr")
    host = _fa(cam_to_world, 16) if cam_to_world is not None else None
    check(lib().svoslam_raycast_model_depth(_ptr(out), w, h, float(fx), float(fy), host,
                                            C.c_void_p(int(cam_to_world_ptr)) if cam_to_world_ptr is not None else C.c_void_p(0),
                                            C.c_void_p(int(pool_ptr)), _fa(center, 3), float(size), _ptr(counters), _stream()))
    return out


def cone_trace_svo_band(out, row_first, rows, fov, view, pool_ptr, center, size, mode=RENDER_REFERENCE, counters=None):
    """rows [row_first, row_first+rows) of the same render into the full-frame buffer `out`."""
    h, w = int(out.shape[0]), int(out.shape[1])
    check(lib().svoslam_cone_trace_svo_band(_ptr(out), w, h, int(row_first), int(rows), float(fov), _fa(view, 16),
                                            C.c_void_p(int(pool_ptr)), _fa(center, 3), float(size), int(mode),
                                            _ptr(counters), _stream()))
    return out


def cone_trace_timing(enable):
    """HIP events around every trace kernel from now on (on its launch stream)"""
    check(lib().svoslam_cone_trace_timing(1 if enable else 0))


def cone_trace_timing_read():
    """(summed kernel ms, launches) since the last read; blocking"""
    ms, n = C.c_float(0), C.c_int32(0)
    check(lib().svoslam_cone_trace_timing_read(C.byref(ms), C.byref(n)))
    return float(ms.value), int(n.value)


(STAGE_MARCH, STAGE_TRACKER, STAGE_FUSE_SORT, STAGE_FUSE_PLAN, STAGE_FUSE_COMMIT, STAGE_MAPS, STAGE_MESH_RASTER, STAGE_MESH_SORT,
 STAGE_MESH_EMIT, STAGE_SURFACE_BFS, STAGE_SURFACE_FACES, STAGE_SURFACE_WELD, STAGE_QUERY) = range(13)   # SVOSLAM_STAGE_*
STAGE_NAMES = ("march", "tracker", "fuse_sort", "fuse_plan", "fuse_commit", "maps", "mesh_raster", "mesh_sort", "mesh_emit", "surface_bfs",
               "surface_faces", "surface_weld", "query")


def stage_timing(stages):
    """HIP events around the launches of the given stages (iterable of STAGE_*) from now on; clears every log"""
    mask = 0
    for s in stages:
        mask |= 1 << int(s)
    check(lib().svoslam_stage_timing(mask))


def stage_timing_read(stage):
    """(summed ms, bracketed launches / launch groups) of one stage since the last read; blocking"""
    ms, n = C.c_float(0), C.c_int32(0)
    check(lib().svoslam_stage_timing_read(int(stage), C.byref(ms), C.byref(n)))
    return float(ms.value), int(n.value)


# ----------------------------------------------------------------------------- recorded sensor
def image_load(path):
    """PNG / PGM / PPM -> numpy array [h, w] uint16 or [h, w, 3] uint8 (host side, no device needed)"""
    data, w, h, ch, bits = _vp(), _i32(0), _i32(0), _i32(0), _i32(0)
    check(lib().svoslam_image_load(str(path).encode(), C.byref(data), C.byref(w), C.byref(h), C.byref(ch), C.byref(bits)))
    try:
        n = w.value * h.value * ch.value
        if bits.value == 16:
            a = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint16)), shape=(n,)).copy()
        else:
            a = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), shape=(n,)).copy()
    finally:
        C.CDLL(None).free(data)
    return a.reshape(h.value, w.value) if ch.value == 1 else a.reshape(h.value, w.value, ch.value)


def focal_from_fov(width, height, hfov_rad, vfov_rad):
    fx, fy = C.c_float(0), C.c_float(0)
    check(lib().svoslam_focal_from_fov(width, height, float(hfov_rad), float(vfov_rad), C.byref(fx), C.byref(fy)))
    return float(fx.value), float(fy.value)


class FrameReader:
    """sensor::OpenNIDevice replaced by a TUM-style association list of depth / colour images"""

    def __init__(self, association_file, depth_units_per_metre=1000.0):
        self._h = _vp()
        check(lib().svoslam_frame_reader_open(C.byref(self._h), str(association_file).encode(), float(depth_units_per_metre)))
        w, h, n = _i32(0), _i32(0), _i32(0)
        check(lib().svoslam_frame_reader_info(self._h, C.byref(w), C.byref(h), C.byref(n)))
        self.width, self.height, self.num_frames = w.value, h.value, n.value

    def rewind(self):
        check(lib().svoslam_frame_reader_rewind(self._h))

    def next_host(self):
        """(depth uint16 [h,w] in mm, rgb uint8 [h,w,3], timestamp_us) or None at the end"""
        d = np.empty((self.height, self.width), np.uint16)
        c = np.empty((self.height, self.width, 3), np.uint8)
        ts, got = C.c_longlong(0), _i32(0)
        check(lib().svoslam_frame_reader_next_host(self._h, C.c_void_p(d.ctypes.data), C.c_void_p(c.ctypes.data), C.byref(ts),
                                                   C.byref(got)))
        return (d, c, int(ts.value)) if got.value else None

    def next_device(self, depth_out, rgb_out):
        """uploads the next frame into cuda tensors (int16/uint16 [h,w], uint8 [h,w,3]); returns the timestamp or None"""
        ts, got = C.c_longlong(0), _i32(0)
        check(lib().svoslam_frame_reader_next(self._h, _ptr(depth_out), _ptr(rgb_out), C.byref(ts), C.byref(got), _stream()))
        return int(ts.value) if got.value else None

    def close(self):
        if self._h:
            lib().svoslam_frame_reader_close(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- sensor
def generate_vertex_map(depth, out, fx, fy, img_w, img_h):
    h, w = int(depth.shape[0]), int(depth.shape[1])
    check(lib().svoslam_generate_vertex_map(_ptr(depth), _ptr(out), w, h, float(fx), float(fy), img_w, img_h, _stream()))
    return out


def generate_vertex_map_rows(depth, out, first_row, rows, fx, fy, img_w, img_h):
    h, w = int(depth.shape[0]), int(depth.shape[1])
    check(lib().svoslam_generate_vertex_map_rows(_ptr(depth), _ptr(out), w, h, int(first_row), int(rows), float(fx), float(fy),
                                                 img_w, img_h, _stream()))
    return out


def generate_normal_map(vmap, out):
    h, w = int(vmap.shape[0]), int(vmap.shape[1])
    check(lib().svoslam_generate_normal_map(_ptr(vmap), _ptr(out), w, h, _stream()))
    return out


def bilateral_filter(depth, out):
    h, w = int(depth.shape[0]), int(depth.shape[1])
    check(lib().svoslam_bilateral_filter(_ptr(depth), _ptr(out), w, h, _stream()))
    return out


def subsample_depth(data, tmp, w, h):
    import torch
    fn = lib().svoslam_subsample_depth_u16 if data.dtype in (torch.uint16, torch.int16) else lib().svoslam_subsample_depth_f32
    check(fn(_ptr(data), _ptr(tmp), w, h, _stream()))


def subsample(data, tmp, w, h):
    import torch
    fn = lib().svoslam_subsample_rgb8 if data.dtype == torch.uint8 else lib().svoslam_subsample_f32
    check(fn(_ptr(data), _ptr(tmp), w, h, _stream()))


def color_to_intensity(rgb, out):
    check(lib().svoslam_color_to_intensity(_ptr(rgb), _ptr(out), int(out.numel()), _stream()))
    return out


def transform_vertex_map(v, trans):
    check(lib().svoslam_transform_vertex_map(_ptr(v), _fa(trans, 16), int(v.numel() // 3), _stream()))


def transform_normal_map(v, trans):
    check(lib().svoslam_transform_normal_map(_ptr(v), _fa(trans, 16), int(v.numel() // 3), _stream()))


def transform_vertex_map_dmat(v, d_trans_ptr):
    check(lib().svoslam_transform_vertex_map_dmat(_ptr(v), C.c_void_p(int(d_trans_ptr)), int(v.numel() // 3), _stream()))


def point_cloud_bbox(points, bbox0=(0, 0, 0), bbox1=(0, 0, 0)):
    b0, b1 = _fa(bbox0, 3), _fa(bbox1, 3)
    check(lib().svoslam_point_cloud_bbox(_ptr(points), int(points.numel() // 3), b0, b1, _stream()))
    return np.array(list(b0), np.float32), np.array(list(b1), np.float32)


def point_cloud_bbox_device(ws, points, out7):
    check(lib().svoslam_point_cloud_bbox_device(ws._h, _ptr(points), int(points.numel() // 3), _ptr(out7), _stream()))
    return out7


def gradient(intensity, out):
    """Sobel / 8 of a float image [h, w] into out [h, w, 2] (own specification, see svoslam.h)"""
    h, w = int(intensity.shape[0]), int(intensity.shape[1])
    check(lib().svoslam_gradient(_ptr(intensity), _ptr(out), w, h, _stream()))
    return out


def difference(a, b, out):
    check(lib().svoslam_difference(_ptr(a), _ptr(b), _ptr(out), int(out.numel()), _stream()))
    return out


def rgbd_cost(last_i, last_g, last_v, cur_i, cur_v, fx, fy, img_w, img_h):
    """photometric normal equations (computeRGBDCost, own specification) -> (A [6,6], b [6])"""
    h, w = int(last_i.shape[0]), int(last_i.shape[1])
    A, b = (C.c_float * 36)(), (C.c_float * 6)()
    check(lib().svoslam_rgbd_cost(_ptr(last_i), _ptr(last_g), _ptr(last_v), _ptr(cur_i), _ptr(cur_v), w, h, float(fx), float(fy),
                                  int(img_w), int(img_h), A, b, _stream()))
    return np.array(list(A), np.float32).reshape(6, 6), np.array(list(b), np.float32)


def icp_cost2(last_v, last_n, cur_v, cur_n):
    h, w = int(last_v.shape[0]), int(last_v.shape[1])
    A, b = (C.c_float * 36)(), (C.c_float * 6)()
    check(lib().svoslam_icp_cost2(_ptr(last_v), _ptr(last_n), _ptr(cur_v), _ptr(cur_n), w, h, A, b, _stream()))
    return np.array(list(A), np.float32).reshape(6, 6), np.array(list(b), np.float32)


def icp_cost(last_v, last_n, cur_v, cur_n, A0=None, b0=None):
    """sensor::computeICPCost (correspondence variant).  Returns (A, b, num_correspondences); without correspondences
    A and b keep A0 / b0 (zeros by default), as the reference leaves its outputs untouched."""
    h, w = int(last_v.shape[0]), int(last_v.shape[1])
    A, b = (C.c_float * 36)(), (C.c_float * 6)()
    if A0 is not None:
        A[:] = [float(v) for v in np.asarray(A0, np.float32).reshape(36)]
    if b0 is not None:
        b[:] = [float(v) for v in np.asarray(b0, np.float32).reshape(6)]
    m = _i32(0)
    check(lib().svoslam_icp_cost(_ptr(last_v), _ptr(last_n), _ptr(cur_v), _ptr(cur_n), w, h, A, b, C.byref(m), _stream()))
    return np.array(list(A), np.float32).reshape(6, 6), np.array(list(b), np.float32), int(m.value)


def icp_accumulate(last_v, last_n, cur_v, cur_n, first_pixel, num_pixels, acc):
    h, w = int(last_v.shape[0]), int(last_v.shape[1])
    check(lib().svoslam_icp_accumulate(_ptr(last_v), _ptr(last_n), _ptr(cur_v), _ptr(cur_n), w, h, first_pixel, num_pixels,
                                       _ptr(acc), _stream()))


# ----------------------------------------------------------------------------- tracker
TRACK_FORM_NONE, TRACK_FORM_CHAIN, TRACK_FORM_ONE_LAUNCH, TRACK_FORM_STREAM, TRACK_FORM_HYBRID = range(5)   # Camera.last_track_plan()["form"]


class Camera:
    """Mirror of sensor::RGBDCamera (include/octree_slam/sensor/rgbd_camera.h)."""

    def __init__(self, width, height, fx, fy):
        self._h = C.c_void_p()
        self.width, self.height = width, height
        check(lib().svoslam_camera_create(C.byref(self._h), width, height, float(fx), float(fy)))

    def update(self, depth, rgb, timestamp):
        used = C.c_int32(0)
        check(lib().svoslam_camera_update(self._h, _ptr(depth), _ptr(rgb), int(timestamp), C.byref(used), _stream()))
        return int(used.value)

    def set_rgbd(self, enable=True):
        """photometric RGB-D term in every ICP iteration (rgbd_camera.cpp:126-141 switched on); before the first frame"""
        check(lib().svoslam_camera_set_rgbd(self._h, 1 if enable else 0))

    def set_strict_reference(self, strict=True):
        """False: this build's corrected tracker (include/svoslam.h svoslam_camera_set_strict_reference); before the first frame"""
        check(lib().svoslam_camera_set_strict_reference(self._h, 1 if strict else 0))

    def set_model_depth(self, depth):
        """frame-to-model tracking: `depth` (cuda uint16 [h, w], e.g. raycast_model_depth from the pose of the frame just
        tracked) becomes the map set the ICP tracks against (own specification: include/svoslam.h)"""
        check(lib().svoslam_camera_set_model_depth(self._h, _ptr(depth), _stream()))   # (None: no model, frame to frame until the next one)

    def set_frame_to_model(self, enable=True):
        check(lib().svoslam_camera_set_frame_to_model(self._h, 1 if enable else 0))

    def reset(self):
        """identity pose, no frame seen; buffers kept"""
        check(lib().svoslam_camera_reset(self._h))

    def prepare(self, depth, rgb, timestamp):
        """first half of update(): bilateral filter + pyramids of the next frame (may run ahead on another stream)"""
        used = C.c_int32(0)
        check(lib().svoslam_camera_prepare(self._h, _ptr(depth), _ptr(rgb), int(timestamp), C.byref(used), _stream()))
        return int(used.value)

    def pair_delta(self, depth_prev, rgb_prev, depth_cur, rgb_cur, out):
        """update_trans of frame `cur` tracked against frame `prev` -> out (DELTA_FLOATS floats); this camera is scratch"""
        check(lib().svoslam_camera_pair_delta(self._h, _ptr(depth_prev), _ptr(rgb_prev), _ptr(depth_cur), _ptr(rgb_cur), _ptr(out),
                                              _stream()))

    def apply_delta(self, delta, timestamp):
        """the pose step of update() for a frame tracked elsewhere (delta = None: pose unchanged)"""
        used = C.c_int32(0)
        check(lib().svoslam_camera_apply_delta(self._h, _ptr(delta), int(timestamp), C.byref(used), _stream()))
        return int(used.value)

    def track_prepared(self):
        """second half of update(): pose of the oldest prepared frame"""
        check(lib().svoslam_camera_track(self._h, _stream()))

    # multi-GPU stepping (all-reduce between accumulate and solve)
    def set_band(self, first_row, rows):
        check(lib().svoslam_camera_set_band(self._h, first_row, rows))

    def set_acc(self, acc_tensor):
        self._acc_keepalive = acc_tensor
        check(lib().svoslam_camera_set_acc(self._h, _ptr(acc_tensor)))

    def begin(self, depth, rgb, timestamp):
        used = C.c_int32(0)
        check(lib().svoslam_camera_begin(self._h, _ptr(depth), _ptr(rgb), int(timestamp), C.byref(used), _stream()))
        return int(used.value)

    def icp_accumulate(self, level, it):
        check(lib().svoslam_camera_icp_accumulate(self._h, level, it, _stream()))

    def icp_solve(self, level, it):
        check(lib().svoslam_camera_icp_solve(self._h, level, it, _stream()))

    def end(self):
        check(lib().svoslam_camera_end(self._h, _stream()))

    def pose(self):
        p, o = (C.c_float * 3)(), (C.c_float * 9)()
        check(lib().svoslam_camera_pose(self._h, p, o, _stream()))
        return np.array(list(p), np.float32), np.array(list(o), np.float32)

    def last_system(self):
        A, b, x = (C.c_float * 36)(), (C.c_float * 6)(), (C.c_float * 6)()
        check(lib().svoslam_camera_last_system(self._h, A, b, x, _stream()))
        return np.array(list(A), np.float32).reshape(6, 6), np.array(list(b), np.float32), np.array(list(x), np.float32)

    def fusion_transform_ptr(self):
        return int(lib().svoslam_camera_fusion_transform_device(self._h))

    def last_vertex_ptr(self, level):
        return int(lib().svoslam_camera_last_vertex(self._h, level))

    def last_normal_ptr(self, level):
        return int(lib().svoslam_camera_last_normal(self._h, level))

    def track_profile(self):
        """device clock stamps [32, 8] of the last one-launch tracker (SVO_TRK_PROF builds; zeros otherwise)"""
        out = np.zeros((32, 8), np.uint64)
        check(lib().svoslam_camera_track_profile(self._h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), _stream()))
        return out

    def tracking_lost_count(self):
        n = C.c_int32(0)
        check(lib().svoslam_camera_tracking_lost_count(self._h, C.byref(n), _stream()))
        return int(n.value)

    def last_track_plan(self):
        """svoslam_camera_last_track_plan: what the most recent tracked frame enqueued, as {"form", "workers", "participants" [L0, L1, L2],
        "slots" [L0, L1, L2]}; form = TRACK_FORM_NONE / _CHAIN / _ONE_LAUNCH / _STREAM / _HYBRID (0..4).  Host state, no device access."""
        out = (_i32 * 8)()
        check(lib().svoslam_camera_last_track_plan(self._h, out))
        v = [int(x) for x in out]
        return {"form": v[0], "workers": v[1], "participants": v[2:5], "slots": v[5:8]}

    def close(self):
        if self._h:
            lib().svoslam_camera_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def subtree_file_words(file):
    """the stand-alone linear tree stored in a paged-out sub-tree file, as uint32 words (2 per node)"""
    w, n = C.POINTER(C.c_uint32)(), _i32(0)
    check(lib().svoslam_subtree_file_nodes(str(file).encode(), C.byref(w), C.byref(n)))
    try:
        return np.ctypeslib.as_array(w, shape=(2 * n.value,)).copy()
    finally:
        C.CDLL(None).free(w)


def copy_from_device(ptr, shape, dtype):
    """Copy a raw device buffer to a numpy array (tests)."""
    import torch
    torch.cuda.synchronize()
    out = np.empty(shape, dtype=dtype)
    r = _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(ptr)), C.c_size_t(out.nbytes), 2)
    if r != 0:
        raise SvoslamError("hipMemcpy D2H failed: %d" % r)
    return out
