"""Paths through a region: traced down a cost-to-go field, checked and straightened against a distance field, planned from metres;
in free space and over the ground."""
import numpy as np

from ._abi import _stream, check, lib
from ._args import device_i32, field_i32, ptr_or_null, region, result
from ._fields import _up_code, box_to_cells, cost_field, distance_field, ground_field


def trace_paths(field, origin, dims, starts, max_cells, as_tensor=False):
    """svoslam_field_trace_paths: from every start ([n, 3] absolute cells: an array, or an int32 cuda tensor) down `field` (int32 [nz,
    ny, nx] over origin[3] .. origin + dims[3], as cost_field and reach_field return it: an array or a cuda tensor), always to the
    face neighbour in the region with the smallest value below the cell's own, the first of -x +x -y +y -z +z on a tie, until a cell
    of value 0.  -> (paths int32 [n, max_cells, 3], lengths int32 [n]): lengths[i] counts the cells of the whole path, start and
    final cell included, even beyond max_cells; only the first min(length, max_cells) rows of paths[i] are written, the rest are
    -1 here.  Length 0: the start is outside the region or on a negative value; a negative length: the array is not a cost-to-go
    field, the walk stopped after that many cells.  numpy arrays, or with as_tensor cuda tensors and nothing is synchronised."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_starts = device_i32(starts, "starts", 3)
    count, cap = int(t_starts.shape[0]), int(max_cells)
    paths = torch.full((count, max(cap, 0), 3), -1, dtype=torch.int32, device="cuda")
    lengths = torch.zeros(count, dtype=torch.int32, device="cuda")
    check(lib().svoslam_field_trace_paths(ptr_or_null(t_field), o3, n3, ptr_or_null(t_starts), count, cap, ptr_or_null(paths),
                                          ptr_or_null(lengths), _stream()))
    return result((paths, lengths), as_tensor)


def segment_clearance(field, origin, dims, segments, want_cell=False, as_tensor=False):
    """svoslam_field_segment_clearance: for every segment ([n, 6] absolute cells, a xyz then b xyz: an array, or an int32 cuda
    tensor) the smallest value of `field` (int32 [nz, ny, nx] over origin[3] .. origin + dims[3], as distance_field returns it: an
    array or a cuda tensor) over a, the cells whose closed cube the centre-to-centre segment meets, and b; -1 counts as infinite
    and a cell outside the region as 0.  -> int32 [n]: 0 = the segment touches an occupied cell or leaves the region, -1 = nothing
    within the field's radius of it; with want_cell the pair (minimum, cells int32 [n, 3]): the first cell in walk order that
    attains it.  numpy arrays, or with as_tensor cuda tensors and nothing is synchronised."""
    import torch
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_seg = device_i32(segments, "segments", 6)
    count = int(t_seg.shape[0])
    low = torch.zeros(count, dtype=torch.int32, device="cuda")
    at = torch.zeros((count, 3), dtype=torch.int32, device="cuda") if want_cell else None
    check(lib().svoslam_field_segment_clearance(ptr_or_null(t_field), o3, n3, ptr_or_null(t_seg), count, ptr_or_null(low), ptr_or_null(at),
                                                _stream()))
    return result((low, at) if want_cell else low, as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_paths, t_lengths = device_i32(paths, "paths"), device_i32(lengths, "lengths").reshape(-1)
    count = int(t_lengths.shape[0])
    if t_paths.dim() != 3 or t_paths.shape[0] != count or t_paths.shape[2] != 3:
        raise ValueError("paths is [n, max_cells, 3] for lengths [n]")
    cap = int(t_paths.shape[1])

    def run(room):
        vertices = torch.full((count, max(room, 0)), -1, dtype=torch.int32, device="cuda")
        counts = torch.zeros(count, dtype=torch.int32, device="cuda")
        check(lib().svoslam_field_shorten_paths(ptr_or_null(t_field), o3, n3, int(clearance_cells), ptr_or_null(t_paths),
                                                ptr_or_null(t_lengths), count, cap, int(max_lookahead), room, ptr_or_null(vertices),
                                                ptr_or_null(counts), _stream()))
        return vertices, counts
    if max_vertices is None:
        _, counts = run(0)                                              # the counts alone: the room the longest result needs
        vertices, counts = run(int(counts.max()) if count else 0)
    else:
        vertices, counts = run(int(max_vertices))
    return result((vertices, counts), as_tensor)


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
    _, n, o3, n3 = region(origin, dims)
    t_field = field_i32(field, n)
    t_starts = device_i32(starts, "starts", 3)
    count, cap = int(t_starts.shape[0]), int(max_cells)
    paths = torch.full((count, max(cap, 0), 3), -1, dtype=torch.int32, device="cuda")
    lengths = torch.zeros(count, dtype=torch.int32, device="cuda")
    check(lib().svoslam_field_trace_ground_paths(ptr_or_null(t_field), o3, n3, _up_code(up), int(step_cells), int(climb_cost),
                                                 int(snap_cells), ptr_or_null(t_starts), count, cap, ptr_or_null(paths),
                                                 ptr_or_null(lengths), _stream()))
    return result((paths, lengths), as_tensor)


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
