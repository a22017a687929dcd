"""The sensor side: the reader of recorded depth / colour frames, and the image kernels between a frame and the tracker."""
import ctypes as C

import numpy as np

from ._abi import _close_quietly, _fa, _i32, _ptr, _stream, _vp, check, lib


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

    __del__ = _close_quietly


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
