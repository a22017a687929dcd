"""The tracker: the mirror of sensor::RGBDCamera."""
import ctypes as C

import numpy as np

from ._abi import _close_quietly, _i32, _ptr, _stream, check, lib

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

    __del__ = _close_quietly
