"""Rendering: the cone trace of a pool into an image or a model depth, and the timing of the library's stages."""
import ctypes as C

from ._abi import RENDER_REFERENCE, _fa, _ptr, _stream, check, lib


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
