"""Safe corridors along planned paths (include/svoslam_corridor.h): boxes of free cells grown over a distance
field, the chain of overlapping boxes that holds a path, and a plan with its corridors from metres.  The two calls have a header
and a SIGNATURES table of their own, bound onto the library on first use; used as pkg.corridors."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._args import device_i32, field_i32, ptr_or_null, region, result

HEADER_PATH = os.path.join(os.path.dirname(_abi.HEADER_PATH), "svoslam_corridor.h")
MAX_EXTENT = 65536  # SVOSLAM_MAX_CORRIDOR_EXTENT

_i32, _vp, _i3 = C.c_int32, C.c_void_p, C.POINTER(C.c_int32)
# name -> (restype, argtypes), as _abi.SIGNATURES holds those of include/svoslam.h
SIGNATURES = {
    "svoslam_field_grow_boxes": (C.c_int, [_vp, _i3, _i3, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "svoslam_field_path_corridors": (C.c_int, [_vp, _i3, _i3, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
}
_bound = None


def lib():
    """_abi.lib() with this module's two symbols bound"""
    global _bound
    L = _abi.lib()
    if _bound is not L:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def grow_boxes(field, origin, dims, clearance_cells, max_extent, seeds, as_tensor=False):
    """svoslam_field_grow_boxes: grow every seed box ([n, 6] absolute cells, lo xyz then hi xyz, inclusive: an array, or an int32
    cuda tensor) over `field` (int32 [nz, ny, nx] over origin[3] .. origin + dims[3], as distance_field returns it WITH A RADIUS >=
    clearance_cells -- the call cannot check that: an array or a cuda tensor).  A cell is free iff it lies in the region and is
    more than clearance_cells from every occupied cell.  Rounds of -x +x -y +y -z +z: a direction that has grown fewer than
    max_extent (0..MAX_EXTENT) layers grows by one iff the whole slab beside that face of the box as it is now is free, until a
    round grows nothing.  -> (boxes int32 [n, 6], layers int32 [n]): the layers added in total; a seed with lo > hi, not wholly in
    the region or with a cell that is not free comes back as it was, with layers -1.  numpy arrays, or with as_tensor cuda tensors
    and nothing is synchronised."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_seeds = device_i32(seeds, "seeds", 6)
    count = int(t_seeds.shape[0])
    boxes = torch.full((count, 6), -1, dtype=torch.int32, device="cuda")
    layers = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    _abi.check(lib().svoslam_field_grow_boxes(ptr_or_null(t_field), o3, n3, int(clearance_cells), int(max_extent), ptr_or_null(t_seeds),
                                              count, ptr_or_null(boxes), ptr_or_null(layers), _abi._stream()))
    return result((boxes, layers), as_tensor)


def path_corridors(field, origin, dims, clearance_cells, max_extent, paths, lengths, max_boxes=None, as_tensor=False):
    """svoslam_field_path_corridors: for every path (paths int32 [n, max_cells, 3], lengths int32 [n], as trace_paths returns them:
    arrays or cuda tensors) a chain of boxes of free cells that holds it, over `field` as grow_boxes reads it.  From the anchor a
    (first 0) the box is grown (grow_boxes' rule, max_extent layers a direction) from p_a, together with p_(a+1) when that is a
    free face neighbour; the next anchor is the last index e up to which the path stays in the box (a + 1 when that is a itself),
    until e is the path's last cell.  A cell p_a that is not free gives the empty box lo = p_a, hi = p_a - 1.  -> (boxes int32 [n,
    max_boxes, 6] lo xyz hi xyz inclusive, anchors int32 [n, max_boxes], counts int32 [n], gaps int32 [n]): counts[i] even beyond
    max_boxes, unwritten rows -1 here; gaps[i] = the anchors with an empty box or a box the path leaves at once -- 0 on a path
    of free face neighbours, where consecutive boxes share the next anchor's cell.  max_boxes=None: two passes, the first for the
    counts alone (it blocks).  numpy arrays, or with as_tensor cuda tensors."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_paths, t_lengths = device_i32(paths, "paths"), device_i32(lengths, "lengths").reshape(-1)
    count = int(t_lengths.shape[0])
    if t_paths.dim() != 3 or t_paths.shape[0] != count or t_paths.shape[2] != 3:
        raise ValueError("paths is [n, max_cells, 3] for lengths [n]")
    cap = int(t_paths.shape[1])

    def run(room):
        boxes = torch.full((count, max(room, 0), 6), -1, dtype=torch.int32, device="cuda")
        anchors = torch.full((count, max(room, 0)), -1, dtype=torch.int32, device="cuda")
        counts = torch.zeros(count, dtype=torch.int32, device="cuda")
        gaps = torch.zeros(count, dtype=torch.int32, device="cuda")
        _abi.check(lib().svoslam_field_path_corridors(ptr_or_null(t_field), o3, n3, int(clearance_cells), int(max_extent),
                                                      ptr_or_null(t_paths), ptr_or_null(t_lengths), count, cap, room, ptr_or_null(boxes),
                                                      ptr_or_null(anchors), ptr_or_null(counts), ptr_or_null(gaps), _abi._stream()))
        return boxes, anchors, counts, gaps
    if max_boxes is None:
        counts = run(0)[2]                                              # the counts alone: the room the longest chain needs
        out = run(int(counts.max()) if count else 0)
    else:
        out = run(int(max_boxes))
    return result(out, as_tensor)


def plan_corridors(ws, pool, max_depth, center, edge_length, box, goal, starts, clearance_cells, comfort_cells, ring_cost, max_extent,
                   **plan_kwargs):
    """plan_paths (its arguments, and max_cells / straighten / max_lookahead as keywords) followed by path_corridors over the kept
    cells of every path, against the plan's own distance field: distance_field at radius comfort_cells over the plan's region, at
    clearance_cells and max_extent.  -> plan_paths' result (None for an empty box), every path dict with four more entries: boxes
    (int32 [k, 6] cells, lo xyz hi xyz inclusive), boxes_m (float64 [k, 6] metres: the lo corner and the hi corner of the box, the
    outer faces of its cubes), anchors (int32 [k] indices into cells) and gaps (int; 0 = the chain is unbroken); all None without a
    path."""
    from ._fields import distance_field
    from ._paths import plan_paths
    plan = plan_paths(ws, pool, max_depth, center, edge_length, box, goal, starts, clearance_cells, comfort_cells, ring_cost, **plan_kwargs)
    if plan is None:
        return None
    kept = [p["cells"] for p in plan["paths"]]
    room = max([0] + [len(c) for c in kept if c is not None])
    paths = np.full((len(kept), room, 3), -1, np.int32)
    lengths = np.zeros(len(kept), np.int32)
    for k, c in enumerate(kept):
        if c is not None:
            paths[k, :len(c)], lengths[k] = c, len(c)
    comfort = distance_field(ws, pool, max_depth, plan["origin"], plan["dims"], comfort_cells, as_tensor=True)
    boxes, anchors, counts, gaps = path_corridors(comfort, plan["origin"], plan["dims"], clearance_cells, max_extent, paths, lengths)
    corner = np.asarray(center, np.float64) - float(edge_length)
    for k, p in enumerate(plan["paths"]):
        if kept[k] is None:
            p.update(boxes=None, boxes_m=None, anchors=None, gaps=None)
            continue
        mine = boxes[k, :int(counts[k])].copy()
        faces = mine.astype(np.float64) + np.array([0, 0, 0, 1, 1, 1], np.float64)
        p.update(boxes=mine, boxes_m=np.tile(corner, 2) + faces * plan["cell_size"], anchors=anchors[k, :int(counts[k])].copy(),
                 gaps=int(gaps[k]))
    return plan
