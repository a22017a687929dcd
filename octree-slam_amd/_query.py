"""Queries of the map by point, ray and box: batched lookups whose inputs and outputs are numpy arrays or cuda tensors alike."""
import ctypes as C

import numpy as np

from ._abi import _fa, _ptr, _stream, check, lib
from ._args import Outputs


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
    outs = Outputs(fields, fields if outputs is None else outputs)
    outs.alloc(n)
    call(t_in, n, outs.ptrs())
    return outs.result(as_torch)


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
