"""Fields over a region of the map, one int32 per cell: distance, reach, owner and rooms, cost, ground, components and nearest cell;
and box_to_cells, the region of a box in metres."""
import ctypes as C

import numpy as np

from ._abi import _ComponentStats, _GroundStats, _OwnerStats, _PlanStats, _ReachStats, _fa, _i32, _ptr, _stream, check, lib
from ._args import Outputs, device_i32, ptr_or_null, region, region_shape, result, stats_dict


def distance_field(ws, pool, max_depth, origin, dims, radius_cells, as_tensor=False, launch_ms=None):
    """svoslam_pool_distance_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the squared
    distance in cells to the nearest occupied cell of the map within radius_cells, -1 where there is none: an exact Euclidean
    distance transform truncated at the radius.  -> int32 [nz, ny, nx] (metres = sqrt(dist2) * 2 * edge_length / 2^max_depth), a
    numpy array, or with as_tensor a cuda tensor, in which case nothing is synchronised.  `launch_ms`: a list that receives the
    milliseconds of the four launches (raster, x, y, z pass): svoslam_pool_distance_field_profile, which blocks."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    out = torch.empty(region_shape(n), dtype=torch.int32, device="cuda")
    if launch_ms is None:
        check(lib().svoslam_pool_distance_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(radius_cells), _ptr(out), _stream()))
    else:
        ms = (C.c_float * 4)()
        check(lib().svoslam_pool_distance_field_profile(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(radius_cells), _ptr(out), ms,
                                                        _stream()))
        launch_ms[:] = [float(v) for v in ms]
    return result(out, as_tensor)


def reach_field(ws, pool, max_depth, origin, dims, clearance_cells, seeds, as_tensor=False, stats=None):
    """svoslam_pool_reach_field: for every cell of the region origin[3] .. origin + dims[3] (cells at max_depth, x y z) the number of
    face-neighbour moves of the shortest path from any of `seeds` ([n, 3] absolute cells: an array, or an int32 cuda tensor) that
    stays in the region and in cells with no occupied cell within clearance_cells (those where distance_field with that radius is
    -1); 0 at a seed that counts, -1 where no path leads, -2 where the cell is blocked.  -> int32 [nz, ny, nx] (metres along the
    path = steps * 2 * edge_length / 2^max_depth), a numpy array, or with as_tensor a cuda tensor.  The call blocks either way:
    the host reads a convergence record per round.  `stats`: a dict that receives rounds, tile_runs and seeds_used."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    t_seeds = device_i32(seeds, "seeds", 3)
    out = torch.empty(region_shape(n), dtype=torch.int32, device="cuda")
    st = _ReachStats()
    check(lib().svoslam_pool_reach_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(clearance_cells), ptr_or_null(t_seeds),
                                         int(t_seeds.shape[0]), _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(stats_dict(st))
    return result(out, as_tensor)


MAX_RING_COST = 65534                                                   # include/svoslam.h SVOSLAM_MAX_RING_COST


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
    _, n, o3, n3 = region(origin, dims)
    if (seeds is None) == (seed_field is None):
        raise ValueError("give the seeds as a list (seeds) or as a field of labels (seed_field), one of the two")
    shape = region_shape(n)
    steps = torch.empty(shape, dtype=torch.int32, device="cuda")
    if owner is None:
        owner = torch.empty(shape, dtype=torch.int32, device="cuda")
    elif not (isinstance(owner, torch.Tensor) and owner.is_cuda and owner.dtype == torch.int32 and owner.is_contiguous()
              and list(owner.shape) == shape):
        raise ValueError("owner is a contiguous int32 cuda tensor of the region's shape, [nz, ny, nx]")
    if seed_field is None:
        t_seeds = device_i32(seeds, "seeds", 3)
        seed_args = (ptr_or_null(t_seeds), int(t_seeds.shape[0]), None)
    else:
        t_field = seed_field if seed_field is owner else device_i32(seed_field, "seed_field")   # the very tensor that is grown in place
        if list(t_field.shape) != shape:
            raise ValueError("seed_field has the shape of the region, [nz, ny, nx]")
        if not t_field.numel():                                         # no cell to point at; the pointer only says which form this is
            t_field = torch.zeros(1, dtype=torch.int32, device="cuda")
        seed_args = (None, 0, _ptr(t_field))
    st = _OwnerStats()
    check(lib().svoslam_pool_owner_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(clearance_cells), *seed_args, _ptr(steps),
                                         _ptr(owner), C.byref(st), _stream()))
    if stats is not None:
        stats.update(stats_dict(st))
    return result((steps, owner), as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    ring = [int(v) for v in np.asarray(ring_cost if ring_cost is not None else [], np.int64).reshape(-1)]
    if len(ring) != max(int(comfort_cells) - int(clearance_cells), 0):
        raise ValueError("ring_cost holds comfort_cells - clearance_cells entries")
    if any(v < 0 or v > MAX_RING_COST for v in ring):
        raise ValueError("a ring cost lies in 0 .. %d" % MAX_RING_COST)
    t_seeds = device_i32(seeds, "seeds", 3)
    out = torch.empty(region_shape(n), dtype=torch.int32, device="cuda")
    st = _PlanStats()
    check(lib().svoslam_pool_cost_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(clearance_cells), int(comfort_cells),
                                        (_i32 * len(ring))(*ring) if ring else None, ptr_or_null(t_seeds), int(t_seeds.shape[0]),
                                        _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(stats_dict(st))
    return result(out, as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    t_seeds = device_i32(seeds, "seeds", 3)
    out = torch.empty(region_shape(n), dtype=torch.int32, device="cuda")
    st = _GroundStats()
    check(lib().svoslam_pool_ground_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, _up_code(up), int(radius_cells),
                                          int(height_cells), int(step_cells), int(climb_cost), int(snap_cells), ptr_or_null(t_seeds),
                                          int(t_seeds.shape[0]), _ptr(out), C.byref(st), _stream()))
    if stats is not None:
        stats.update(stats_dict(st))
    return result(out, as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    shape = region_shape(n)
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    count = torch.empty(shape, dtype=torch.int32, device="cuda") if sizes else None
    st = _ComponentStats()
    check(lib().svoslam_pool_label_components(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(clearance_cells),
                                              COMPONENTS_SOLID if solid else COMPONENTS_FREE, _ptr(out), _ptr(count),
                                              C.byref(st) if stats is not None else None, _stream()))
    if stats is not None:
        stats.update(stats_dict(st))
    return result((out, count) if sizes else out, as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    outs = Outputs({"dist2": (torch.int32, np.int32), "cell": (torch.int64, np.uint64), "node": (torch.int32, np.int32),
                    "color": (torch.int32, np.uint32)}, want)
    outs.alloc(region_shape(n))
    check(lib().svoslam_pool_nearest_field(ws._h, C.byref(pool._p), int(max_depth), o3, n3, int(radius_cells), int(which), *outs.ptrs(),
                                           _stream()))
    out = outs.result(as_tensor)
    if "cell" in out:
        c = outs.bufs["cell"]
        xyz = torch.stack([c & 0xFFFF, (c >> 16) & 0xFFFF, (c >> 32) & 0xFFFF], -1).to(torch.int32)
        out["cell_xyz"] = result(torch.where((c < 0).unsqueeze(-1), torch.full_like(xyz, -1), xyz), as_tensor)
    return out


def box_to_cells(max_depth, center, edge_length, box):
    """svoslam_box_to_cells (host only): the inclusive cell range (lo[3], hi[3]) at max_depth of the axis-aligned box[6] (min xyz, max
    xyz; infinities allowed) exactly as count_boxes takes it, or None for an empty box (a NaN, min > max, outside the root).  The
    field of that box: distance_field(ws, pool, max_depth, lo, hi - lo + 1, radius_cells)."""
    lo, hi, empty = (_i32 * 3)(), (_i32 * 3)(), _i32(0)
    check(lib().svoslam_box_to_cells(int(max_depth), _fa(center, 3), float(edge_length), _fa(box, 6), lo, hi, C.byref(empty)))
    if empty.value:
        return None
    return np.array(lo[:], np.int32), np.array(hi[:], np.int32)
