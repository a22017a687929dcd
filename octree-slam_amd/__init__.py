"""octree_slam_amd -- Python front end of libsvoslam_hip.so (include/svoslam.h).

The product is the C-ABI shared library built from csrc/*.hip for gfx950; this
package only binds it with ctypes and moves pointers of torch CUDA tensors
across the boundary (PyTorch = device memory, streams, torch.distributed).
There is NO CPU fallback: every compute entry point raises SvoslamError when
the library or a gfx950 device is missing.

The directory is called ``octree-slam_amd`` (not importable by name); load it
with ``svoslam_pkg.load()`` from the repo root, which registers it as the module
``octree_slam_amd``.

Where things are: _abi holds the structs, SIGNATURES, the loader and the pointer / stream helpers; _args the argument checks and
result exits the wrappers share.  _fusion: workspace, pool, the fusion phases, sort and scan.  Over a map: _query (points, rays,
boxes), _fields (distance, reach, owner, cost, ground, components, nearest), _paths (trace, shorten, plan), _views (visibility,
cover, observe, frontier), _localize (pose scoring).  _mesh, _runner (with the mailbox), _render, _sensor and _tracker hold what
their names say.  Every name is used through the package, which re-exports them here.
"""
from ._abi import (  # noqa: F401
    LIB_PATH, HEADER_PATH, MAX_DEPTH, FLAG_CHILDREN, CHILD_MASK, RENDER_REFERENCE, RENDER_CARRY, PYRAMID_ITERS, DELTA_FLOATS,
    SvoslamError, build, _PoolStruct, _ReachStats, _OwnerStats, _PlanStats, _GroundStats, _ComponentStats, MeshStruct, TextureStruct,
    FuseStats, CompactStats, AccelView, SurfaceStats, SIGNATURES, lib, check, _stream, _ptr, _fa, ConfigStruct, get_config, configure,
    config_env, device_arch, _hip, copy_from_device)
from ._fusion import (  # noqa: F401
    Workspace, Pool, svo_from_point_cloud, svo_from_point_cloud_async, svo_fuse_sort, svo_fuse_sort_frame, svo_fuse_sort_frame_band,
    svo_fuse_merge_sorted, svo_fuse_export_sorted, sort_words, exclusive_scan_u32, svo_fuse_adopt_sorted, svo_fuse_plan,
    pool_structure_begin, svo_fuse_plan_structure, svo_fuse_split_early, svo_fuse_commit, svo_fuse_commit_deferred, svo_fuse_apply,
    KEYRANGE_OVERFLOW, KEYRANGE_MISMATCH, KEYRANGE_USED_WORD, KEYRANGE_FIXED_WORDS, svo_fuse_keyrange_commit, svo_fuse_keyrange_apply,
    svo_fuse_keyrange_discard, svo_fuse_keyrange_status, svo_from_voxel_grid, extract_voxel_grid, extract_surface_mesh, write_ply,
    subtree_file_words)
from ._query import cast_rays, query_points, count_boxes, nearest_occupied  # noqa: F401
from ._fields import (  # noqa: F401
    distance_field, reach_field, MAX_RING_COST, owner_field, segment_rooms, cost_field, UP_PLUS_Y, UP_MINUS_Y, UP_PLUS_Z, UP_MINUS_Z,
    MAX_STEP_CELLS, MAX_HEIGHT_CELLS, MAX_SNAP_CELLS, ground_field, COMPONENTS_FREE, COMPONENTS_SOLID, label_components,
    NEAREST_OCCUPIED, NEAREST_FREE, nearest_field, box_to_cells)
from ._paths import trace_paths, segment_clearance, shorten_paths, plan_paths, trace_ground_paths, plan_ground_paths  # noqa: F401
from ._views import (  # noqa: F401
    MAX_VIEWS_MASK, visibility_field, COVER_SURFACE, COVER_FREE, COVER_ALL, COVER_TARGETS, MAX_COVER_VIEWS, COVER_OUTPUTS, cover_views,
    OBS_THROUGH, OBS_END, STATE_UNKNOWN, STATE_FREE, STATE_FRONTIER, STATE_OCCUPIED, STATE_VACATED, STATE_UNMAPPED, STATE_NAMES,
    FRONTIER_OUTPUTS, observe_rays, frontier_field, explore_views)
from ._localize import MAX_MISS_COST, SCORE_OUTPUTS, score_poses, pose_grid, relocalize  # noqa: F401
from ._mesh import Mesh, Texture, mesh_to_voxel_grid, mesh_last_fragments, voxel_grid_to_mesh, Scene  # noqa: F401
from ._runner import Runner, Mailbox  # noqa: F401
from ._render import (  # noqa: F401
    cone_trace_svo, raycast_model_depth, cone_trace_svo_band, cone_trace_timing, cone_trace_timing_read, STAGE_MARCH, STAGE_TRACKER,
    STAGE_FUSE_SORT, STAGE_FUSE_PLAN, STAGE_FUSE_COMMIT, STAGE_MAPS, STAGE_MESH_RASTER, STAGE_MESH_SORT, STAGE_MESH_EMIT,
    STAGE_SURFACE_BFS, STAGE_SURFACE_FACES, STAGE_SURFACE_WELD, STAGE_QUERY, STAGE_NAMES, stage_timing, stage_timing_read)
from ._sensor import (  # noqa: F401
    image_load, focal_from_fov, FrameReader, generate_vertex_map, generate_vertex_map_rows, generate_normal_map, bilateral_filter,
    subsample_depth, subsample, color_to_intensity, transform_vertex_map, transform_normal_map, transform_vertex_map_dmat,
    point_cloud_bbox, point_cloud_bbox_device, gradient, difference, rgbd_cost, icp_cost2, icp_cost, icp_accumulate)
from . import corridors  # noqa: F401
from ._tracker import TRACK_FORM_NONE, TRACK_FORM_CHAIN, TRACK_FORM_ONE_LAUNCH, TRACK_FORM_STREAM, TRACK_FORM_HYBRID, Camera  # noqa: F401
