"""What viewpoints see of a region: the visibility field, a greedy cover by candidate views, the space the sensor's rays have
observed, its frontier to the unknown, and where to look next."""
import ctypes as C

import numpy as np

from ._abi import _fa, _ptr, _stream, check, lib
from ._args import Outputs, device_i32, device_rows, ptr_or_null, region, region_cells, region_shape, result

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
    _, n, o3, n3 = region(origin, dims)
    outs = Outputs({"mask": (torch.int32, np.uint32), "count": (torch.int32, np.int32)}, want)
    t_views = device_i32(views, "views", 3)
    outs.alloc(region_shape(n))
    check(lib().svoslam_pool_visibility_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(range_cells), ptr_or_null(t_views),
                                              int(t_views.shape[0]), *outs.ptrs(), _stream()))
    return outs.result(as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    outs = Outputs({name: (torch.int32, np.int32) for name in COVER_OUTPUTS}, want)
    mode = COVER_TARGETS[targets] if isinstance(targets, str) else int(targets)
    t_cands = device_i32(candidates, "candidates", 3)
    count, k = int(t_cands.shape[0]), int(k_max)
    t_select = None
    if select is not None:
        if isinstance(select, torch.Tensor):
            if not select.is_cuda or select.dtype not in (torch.uint8, torch.bool):
                raise ValueError("a select tensor is uint8 or bool on the device")
            t_select = select.contiguous().view(torch.uint8)
        else:
            t_select = torch.from_numpy(np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)).cuda()
        if t_select.numel() != region_cells(n):
            raise ValueError("select has one byte per region cell")
    # the call's own needs decide what is allocated: the summary always, chosen and gain whenever rounds are played
    bufs = outs.bufs
    bufs["summary"] = torch.empty(4, dtype=torch.int32, device="cuda")
    if "seen" in outs.names:
        bufs["seen"] = torch.zeros(count, dtype=torch.int32, device="cuda")      # a region without cells leaves it unwritten
    if k > 0 or "chosen" in outs.names or "gain" in outs.names:
        bufs["chosen"] = torch.empty(max(k, 0), dtype=torch.int32, device="cuda")
        bufs["gain"] = torch.empty(max(k, 0), dtype=torch.int32, device="cuda")
    if "round" in outs.names:
        bufs["round"] = torch.empty(region_shape(n), dtype=torch.int32, device="cuda")
    ptrs = dict(zip(COVER_OUTPUTS, outs.ptrs()))
    if k <= 0:
        ptrs["chosen"] = ptrs["gain"] = None
    check(lib().svoslam_pool_cover_views(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(range_cells), mode, _ptr(t_select),
                                         ptr_or_null(t_cands), count, k, int(min_gain), *ptrs.values(), _stream()))
    return outs.result(as_tensor)


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
    _, n3, o3c, n3c = region(origin, dims)
    shape = region_shape(n3)
    t_poses = device_rows(poses, torch.float32, np.float32, 16, "poses")
    t_points = device_rows(points, torch.float32, np.float32, 3, "points")
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
    if t_obs.numel() != region_cells(n3):
        raise ValueError("obs has one byte per region cell")
    t_obs = t_obs.view(shape)
    summary = torch.empty(6, dtype=torch.int64, device="cuda")
    check(lib().svoslam_field_observe_rays(ws._h, ptr_or_null(t_obs), int(max_depth), _fa(center, 3), float(edge_length), o3c, n3c,
                                           _ptr(t_points) if n * frames else None, n, _ptr(t_poses) if n * frames else None, frames,
                                           int(range_cells), 1 if accumulate else 0, _ptr(summary), _stream()))
    return result((t_obs, summary), as_tensor)


def frontier_field(ws, pool, max_depth, origin, dims, obs, want=FRONTIER_OUTPUTS, as_tensor=False):
    """svoslam_pool_frontier_field: observe_rays' `obs` (uint8 [nz, ny, nx]: an array, or a uint8 cuda tensor) held against the map
    over the region origin[3] .. origin + dims[3]: "state" (uint8 [nz, ny, nx]: STATE_UNKNOWN, STATE_FREE, STATE_FRONTIER -- free
    with a face neighbour in the region that is unknown --, STATE_OCCUPIED, STATE_VACATED -- occupied, rays passed through it and
    none ended in it --, STATE_UNMAPPED -- a ray ended where the map has nothing), "frontier" (uint8 [nz, ny, nx]: 1 where the state
    is STATE_FRONTIER; cover_views' select) and "summary" (int32 [6]: the cells per state).  `want`: the subset to compute; the
    others are passed as NULL.  -> a dict: numpy, or with as_tensor cuda tensors, in which case nothing is synchronised."""
    import torch
    _, n3, o3c, n3c = region(origin, dims)
    outs = Outputs({"state": (torch.uint8, np.uint8), "frontier": (torch.uint8, np.uint8), "summary": (torch.int32, np.int32)}, want)
    if isinstance(obs, torch.Tensor):
        if not obs.is_cuda or obs.dtype != torch.uint8:
            raise ValueError("an obs tensor is uint8 on the device")
        t_obs = obs.contiguous()
    else:
        t_obs = torch.from_numpy(np.ascontiguousarray(np.asarray(obs, np.uint8))).cuda()
    if t_obs.numel() != region_cells(n3):
        raise ValueError("obs has one byte per region cell")
    outs.alloc(region_shape(n3), summary=6)
    check(lib().svoslam_pool_frontier_field(ws._h, C.byref(pool._p), int(max_depth), o3c, n3c, ptr_or_null(t_obs), *outs.ptrs(), _stream()))
    return outs.result(as_tensor)


def explore_views(ws, pool, max_depth, origin, dims, obs, candidates, range_cells, k_max, min_gain=1):
    """Where to look next: frontier_field of `obs`, then cover_views of the region's free cells selected by the frontier bytes --
    which few of the `candidates` ([n, 3] absolute cells) see the most of the boundary between the observed free space and the
    unknown within range_cells.  The frontier stays on the device between the two calls.  -> (frontier_field's dict, cover_views'
    dict), numpy."""
    field = frontier_field(ws, pool, max_depth, origin, dims, obs, as_tensor=True)
    cover = cover_views(ws, pool, max_depth, origin, dims, range_cells, candidates, k_max, min_gain, "free", field["frontier"])
    return result(field), cover
