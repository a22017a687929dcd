"""The C ABI as Python sees it: the structs and SIGNATURES of include/svoslam.h, the loader, status checks, the pointer and stream
helpers of every call, and the library's settings.  The loaded library, the raw-stream getter and the HIP runtime handle are
cached here and nowhere else."""
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


def _close_quietly(self):
    # the __del__ of every class that owns a handle of the library: it closes, and raises nothing while the interpreter collects
    try:
        self.close()
    except Exception:
        pass


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


_hiplib = None


def _hip():
    global _hiplib
    if _hiplib is None:
        _hiplib = C.CDLL("libamdhip64.so")
        _hiplib.hipMemcpy.restype = C.c_int
        _hiplib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hiplib


def copy_from_device(ptr, shape, dtype):
    """Copy a raw device buffer to a numpy array (tests)."""
    import torch
    torch.cuda.synchronize()
    out = np.empty(shape, dtype=dtype)
    r = _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(ptr)), C.c_size_t(out.nbytes), 2)
    if r != 0:
        raise SvoslamError("hipMemcpy D2H failed: %d" % r)
    return out
