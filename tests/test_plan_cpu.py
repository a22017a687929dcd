"""Path planning in a map region (svoslam_pool_cost_field, svoslam_field_trace_paths; include/svoslam.h): the
cost field's definition restated as Dijkstra's algorithm with a heap on the traversable cells and the weights the distance field's
definition gives; a second restatement that relaxes all cells at once to a fixed point on the separable distance field; the path
rule restated cell by cell.  The two field restatements are proven equal on a pool fused by the CPU oracle and on hand-built pools
with every value written out, and equal to the reach field's restatement where the weights are all 1.  No GPU.

cost_field_words (the definition) and trace_path are what the device calls must produce; tests/test_gpu_plan.py compares against
them value for value."""
import ctypes as C
import heapq
import os

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, distance_field_words, fields, fused_regions  # noqa: F401
from test_reach_cpu import cells_pool, counted_seeds, manhattan_field, reach_field_words, seeds_for
from test_surface_cpu import HandPool, OPAQUE, load_pkg, path_of, rgba
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
NONE = 1 << 30                                                          # "not reached so far" of the relaxation
MAX_RING_COST = 65534
MOVES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))   # the trace's order: -x +x -y +y -z +z


# ---- the specification, restated -------------------------------------------------------------------------------------------
def ceil_sqrt(d):
    """the integer j with (j - 1)^2 < d <= j^2, elementwise, for d >= 1: in integers"""
    d = np.asarray(d, I64)
    j = np.sqrt(d.astype(np.float64)).astype(I64)
    j = np.where(j * j < d, j + 1, j)
    return np.where((j - 1) * (j - 1) >= d, j - 1, j)


def weights_of(field, clearance, comfort, ring_cost):
    """-> (traversable bool [nz, ny, nx], w int64 [nz, ny, nx]) from the distance field with radius = comfort: a cell is traversable
    iff nothing is within clearance^2 of it; w = 1 beyond comfort^2, else 1 + ring_cost[j - clearance - 1] for the ring j of its
    squared distance (w is 0 where the cell is not traversable: it is never entered)"""
    ring = np.asarray(ring_cost, I64).reshape(-1)
    assert 0 <= clearance <= comfort <= MAX_RADIUS and ring.shape[0] == comfort - clearance
    assert ((ring >= 0) & (ring <= MAX_RING_COST)).all()
    d = field.astype(I64)
    free = (d < 0) | (d > clearance * clearance)
    w = np.where(free, 1, 0).astype(I64)
    ringed = free & (d >= 0)
    if ringed.any():
        j = ceil_sqrt(d[ringed])
        assert (j >= clearance + 1).all() and (j <= comfort).all()
        w[ringed] = 1 + ring[j - clearance - 1]
    return free, w


def cost_field_words(words, depth, origin, dims, clearance, comfort, ring_cost, seeds, field=None):
    """-> int32 [nz, ny, nx]: svoslam_pool_cost_field by its definition.  T and w from the distance field with radius = comfort
    (`field`: that field when the caller has it already); then Dijkstra's algorithm from the counted seeds with a heap: entering a
    cell costs its weight, moves go to the face neighbours inside the region."""
    if field is None:
        field = distance_field_words(words, depth, origin, dims, comfort)
    assert field.shape == (dims[2], dims[1], dims[0])
    free, w = weights_of(field, clearance, comfort, ring_cost)
    nx, ny, nz = dims
    out = np.where(free, -1, -2).astype(np.int32)
    if free.size == 0:
        return out
    wt, ok = w.reshape(-1).tolist(), free.reshape(-1).tolist()
    best = [NONE] * len(wt)
    heap = []
    for x, y, z in counted_seeds(free, origin, dims, seeds).tolist():
        at = (z * ny + y) * nx + x
        if best[at]:
            best[at] = 0
            heap.append((0, at))
    heapq.heapify(heap)
    while heap:
        c, at = heapq.heappop(heap)
        if c > best[at]:
            continue
        x, y, z = at % nx, (at // nx) % ny, at // (nx * ny)
        for inside, to in ((x > 0, at - 1), (x + 1 < nx, at + 1), (y > 0, at - nx), (y + 1 < ny, at + nx), (z > 0, at - nx * ny),
                           (z + 1 < nz, at + nx * ny)):
            if inside and ok[to] and c + wt[to] < best[to]:
                best[to] = c + wt[to]
                heapq.heappush(heap, (best[to], to))
    best = np.array(best, I64).reshape(free.shape)
    assert best[best < NONE].max(initial=0) < NONE
    return np.where(free & (best < NONE), best, out).astype(np.int32)


def cost_field_relaxed(words, depth, origin, dims, clearance, comfort, ring_cost, seeds, field=None):
    """the same field by another route: T and w from the separable distance field, then s(q) = min(s(q), s(neighbour) + w(q)) over
    the six neighbours, all cells at once, repeated until nothing changes"""
    if field is None:
        field = distance_field_separable(words, depth, origin, dims, comfort)
    free, w = weights_of(field, clearance, comfort, ring_cost)
    s = np.full(free.shape, NONE, I64)
    c = counted_seeds(free, origin, dims, seeds)
    s[c[:, 2], c[:, 1], c[:, 0]] = 0
    while True:
        t = s.copy()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            t[tuple(hi)] = np.minimum(t[tuple(hi)], s[tuple(lo)] + w[tuple(hi)])
            t[tuple(lo)] = np.minimum(t[tuple(lo)], s[tuple(hi)] + w[tuple(lo)])
        t = np.where(free, np.minimum(t, NONE), NONE)
        if np.array_equal(t, s):
            break
        s = t
    return np.where(~free, -2, np.where(s >= NONE, -1, s)).astype(np.int32)


def trace_path(field, origin, start, max_cells):
    """-> (cells int32 [min(|length|, max_cells), 3] absolute, length): svoslam_field_trace_paths for one start, cell by cell.
    Length 0: the start is outside the region or on a negative value; from a cell of value v > 0 to the face neighbour inside the
    region with the smallest value 0 <= v' < v, the first in MOVES on a tie; at a cell above 0 without one the walk stops and the
    length is minus the cells walked."""
    nz, ny, nx = field.shape
    q = [int(start[a]) - int(origin[a]) for a in range(3)]
    cells, length = [], 0
    if 0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz and field[q[2], q[1], q[0]] >= 0:
        while True:
            v = int(field[q[2], q[1], q[0]])
            if length < max_cells:
                cells.append([q[a] + int(origin[a]) for a in range(3)])
            length += 1
            if v == 0:
                break
            best, to = v, None
            for m in MOVES:
                p = [q[a] + m[a] for a in range(3)]
                if 0 <= p[0] < nx and 0 <= p[1] < ny and 0 <= p[2] < nz and 0 <= field[p[2], p[1], p[0]] < best:
                    best, to = int(field[p[2], p[1], p[0]]), p
            if to is None:
                length = -length
                break
            q = to
    return np.array(cells, np.int32).reshape(-1, 3), length


def check_path(cost, free, w, origin, start):
    """the facts of a traced path on a cost field: face-neighbour moves, cells in T, the weights of all cells but the last -- the
    cells the reverse path from the seed enters -- sum to the value at the start, and it ends on a cell of value 0"""
    cells, length = trace_path(cost, origin, start, cost.size)
    rel = cells.astype(I64) - np.asarray(origin, I64)
    assert length == cells.shape[0] >= 1
    assert (np.abs(np.diff(rel, axis=0)).sum(1) == 1).all()
    assert free[rel[:, 2], rel[:, 1], rel[:, 0]].all()
    assert int(w[rel[:-1, 2], rel[:-1, 1], rel[:-1, 0]].sum()) == int(cost[rel[0, 2], rel[0, 1], rel[0, 0]])
    assert cost[rel[-1, 2], rel[-1, 1], rel[-1, 0]] == 0
    return cells


def check_paths(cost, field, origin, dims, clearance, comfort, ring_cost, seeds, rng=None):
    """check_path from the dearest cell, a cell next to it in output order and a few seeded ones; the ends are counted seeds"""
    free, w = weights_of(field, clearance, comfort, ring_cost)
    reached = np.argwhere(cost >= 0)[:, ::-1]
    if reached.shape[0] == 0:
        return 0
    picks = [np.array(np.unravel_index(np.argmax(cost), cost.shape)[::-1]), reached[0], reached[-1]]
    if rng is not None:
        picks += list(reached[rng.choice(reached.shape[0], min(4, reached.shape[0]), replace=False)])
    counted = {tuple(int(v) for v in s) for s in counted_seeds(free, origin, dims, seeds) + np.asarray(origin, I64)}
    for p in picks:
        cells = check_path(cost, free, w, origin, p + np.asarray(origin, I64))
        assert tuple(int(v) for v in cells[-1]) in counted
    return len(picks)


def ramp(clearance, comfort, penalty):
    """tools/map_plan.py --penalty: ring_cost[k] = penalty * (comfort - clearance - k)"""
    return [penalty * (comfort - clearance - k) for k in range(comfort - clearance)]


def profiles(clearance, comfort):
    """a ramp and a profile that is not monotone"""
    n = comfort - clearance
    return [ramp(clearance, comfort, 3), [(7, 0, 12, 1)[k % 4] for k in range(n)]] if n else [[]]


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_relaxation_is_dijkstra(fused, fields, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    rng = np.random.default_rng(11)
    reached = weighted = walked = 0
    for clearance in (0, 1):
        near = fields(depth, region, clearance)
        for comfort in (clearance, clearance + 1, clearance + 3):
            field = fields(depth, region, comfort)
            separable = distance_field_separable(words, depth, origin, dims, comfort)
            for count in (1, 7):
                seeds = seeds_for(near == -1, origin, dims, depth, count, rng)
                steps = reach_field_words(words, depth, origin, dims, clearance, seeds, field=near)
                for ring in profiles(clearance, comfort):
                    want = cost_field_words(words, depth, origin, dims, clearance, comfort, ring, seeds, field=field)
                    assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
                    got = cost_field_relaxed(words, depth, origin, dims, clearance, comfort, ring, seeds, field=separable)
                    assert np.array_equal(got, want), (clearance, comfort, count, ring)
                    assert np.array_equal(want < 0, steps < 0) and np.array_equal(want[want < 0], steps[steps < 0])
                    assert (want >= steps).all()
                    if comfort == clearance:
                        assert np.array_equal(want, steps)
                    walked += check_paths(want, field, origin, dims, clearance, comfort, ring, seeds, rng)
                    reached, weighted = reached + int((want > 0).sum()), weighted + int((want > steps).sum())
                if comfort > clearance:                                 # every ring cost 0: the reach field
                    zero = [0] * (comfort - clearance)
                    assert np.array_equal(cost_field_words(words, depth, origin, dims, clearance, comfort, zero, seeds, field=field), steps)
                    assert np.array_equal(cost_field_relaxed(words, depth, origin, dims, clearance, comfort, zero, seeds, field=separable), steps)
    if region in ("whole_root", "low_corner"):
        assert reached > 100 and weighted > 20 and walked > 20, (reached, weighted, walked)


def test_the_definition_takes_its_own_fields(fused):
    """without `field` each restatement asks its own distance field"""
    words, _ = fused
    origin, dims = fused_regions(DEPTH - 2)["low_corner"]
    seeds = [(0, 0, 0), (3, 1, 2)]
    for clearance, comfort, ring in ((0, 2, [4, 1]), (1, 2, [9]), (1, 1, [])):
        got = cost_field_words(words, DEPTH - 2, origin, dims, clearance, comfort, ring, seeds)
        assert np.array_equal(got, cost_field_relaxed(words, DEPTH - 2, origin, dims, clearance, comfort, ring, seeds))


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
# one occupied cell, clearance 0, comfort 2, ring cost (5, 2): the weights of the 5 x 5 x 5 block about it, by hand from D = dx^2 +
# dy^2 + dz^2: D = 0 blocked (0 here), D = 1 -> 1 + 5, D = 2, 3, 4 -> 1 + 2, D >= 5 -> 1.  Planes dz = -2 .. 2, rows dy = -2 .. 2.
_FAR = [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 3, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1]]            # dz = +-2: D = 4 at the middle only
_MID = [[1, 1, 1, 1, 1], [1, 3, 3, 3, 1], [1, 3, 6, 3, 1], [1, 3, 3, 3, 1], [1, 1, 1, 1, 1]]            # dz = +-1: D = 1, 2, 3, then 5, 6, 9
_CUT = [[1, 1, 3, 1, 1], [1, 3, 6, 3, 1], [3, 6, 0, 6, 3], [1, 3, 6, 3, 1], [1, 1, 3, 1, 1]]            # dz = 0: D = 0, 1, 2, 4, then 5, 8
BLOCK_WEIGHTS = np.array([_FAR, _MID, _CUT, _MID, _FAR], I64)


def test_the_weights_about_one_cell():
    one = cells_pool([(3, 3, 3)], 3)
    field = distance_field_words(one, 3, (1, 1, 1), (5, 5, 5), 2)
    free, w = weights_of(field, 0, 2, [5, 2])
    assert np.array_equal(w, BLOCK_WEIGHTS) and np.array_equal(free, BLOCK_WEIGHTS > 0)
    assert ceil_sqrt([1, 2, 3, 4, 5, 9, 10, 16, 17, 4096 * 4096, 4096 * 4096 - 1, 4095 * 4095 + 1]).tolist() == [1, 2, 2, 2, 3, 3, 4, 4, 5, 4096, 4096, 4096]


def plan_cases():
    """name -> (words, depth, origin, dims, clearance, comfort, ring cost, seeds, expected int32 [nz, ny, nx], expected seeds_used)"""
    out = {}
    n, u = -2, -1                                                       # n: not traversable, u: unreachable
    empty = HandPool().words()
    # an empty map: every weight is 1 whatever the rings cost, the cost is the Manhattan distance to the seed
    out["empty_map"] = (empty, 2, (1, 0, 1), (3, 4, 2), 0, 2, [5, 2], [(2, 1, 1)], manhattan_field([(2, 1, 1)], (1, 0, 1), (3, 4, 2)), 1)
    out["empty_map_clearance_1"] = (empty, 3, (0, 0, 0), (4, 4, 4), 1, 3, [9, 0], [(0, 0, 0)], manhattan_field([(0, 0, 0)], (0, 0, 0), (4, 4, 4)), 1)
    # one occupied cell (3,3,3), rings (5, 2): the row through it has the weights 1 3 6 . 6 3 1 (D = 9 4 1 0 1 4 9) and is cut by it
    one = cells_pool([(3, 3, 3)], 3)
    out["row_through_the_cell"] = (one, 3, (0, 3, 3), (7, 1, 1), 0, 2, [5, 2], [(0, 3, 3)], np.array([[[0, 3, 9, n, u, u, u]]], np.int32), 1)
    # ... with the row beside it, weights 1 1 3 6 3 1 1 (D = 10 5 2 1 2 5 10), the way round: down at once (1), along the far row
    # (2, 5, 11, 14, 15, 16), and back up where it is cheap: 16 + 1, 15 + 3, 14 + 6; (2,3,3) is cheaper from its own row: 3 + 6
    out["two_rows_round_the_cell"] = (one, 3, (0, 3, 3), (7, 2, 1), 0, 2, [5, 2], [(0, 3, 3)],
                                      np.array([[[0, 3, 9, n, 20, 18, 17], [1, 2, 5, 11, 14, 15, 16]]], np.int32), 1)
    # ... and from the other end of the row, the mirror image
    out["two_rows_from_the_other_end"] = (one, 3, (0, 3, 3), (7, 2, 1), 0, 2, [5, 2], [(6, 3, 3)],
                                          np.array([[[17, 18, 20, n, 9, 3, 0], [16, 15, 14, 11, 5, 2, 1]]], np.int32), 1)
    # a profile that is not monotone, rings (0, 7): D = 1 costs 1, D = 2 .. 4 cost 8
    out["a_cheap_inner_ring"] = (one, 3, (0, 3, 3), (7, 2, 1), 0, 2, [0, 7], [(0, 3, 3)],
                                 np.array([[[0, 8, 9, n, 20, 28, 22], [1, 2, 10, 11, 19, 20, 21]]], np.int32), 1)
    # an occupied cell (3,2,3) one cell outside the row y = 3: it blocks nothing at clearance 0 and raises the weights to 1 1 3 6 3 1 1
    beside = cells_pool([(3, 2, 3)], 3)
    out["a_cell_outside_raises_weights"] = (beside, 3, (0, 3, 3), (7, 1, 1), 0, 2, [5, 2], [(0, 3, 3)],
                                            np.array([[[0, 1, 4, 10, 13, 14, 15]]], np.int32), 1)
    # ... at clearance 1 it blocks the cell beside it, and the ring D = 2 .. 4 costs 1 + 5
    out["a_cell_outside_blocks_at_clearance_1"] = (beside, 3, (0, 3, 3), (7, 1, 1), 1, 2, [5], [(0, 3, 3)],
                                                   np.array([[[0, 1, 7, n, u, u, u]]], np.int32), 1)
    # seeds: the plane z = 3 about (2,3,3), ring (4): the four face neighbours weigh 5
    mid = cells_pool([(2, 3, 3)], 3)
    round_it = np.array([[[2, 1, 6, 7, 8], [1, 0, n, 12, 9], [2, 1, 6, 7, 8]]], np.int32)
    nowhere = np.array([[[u, u, u, u, u], [u, u, n, u, u], [u, u, u, u, u]]], np.int32)
    region = (mid, 3, (0, 2, 3), (5, 3, 1), 0, 1, [4])
    out["one_seed"] = region + ([(1, 3, 3)], round_it, 1)
    out["no_seeds"] = region + ([], nowhere, 0)
    out["seed_on_a_blocked_cell"] = region + ([(2, 3, 3)], nowhere, 0)
    out["seeds_outside_the_region"] = region + ([(5, 3, 3), (1, 1, 3), (1, 5, 3), (1, 3, 2), (1, 3, 4), (7, 7, 7)], nowhere, 0)
    out["seeds_outside_the_root"] = region + ([(-1, 3, 3), (8, 3, 3), (1, -1, 3), (1, 3, 8), ((1 << 31) - 1, 3, 3), (-(1 << 31), 3, 3)], nowhere, 0)
    out["duplicate_seeds"] = region + ([(1, 3, 3), (1, 3, 3), (1, 3, 3)], round_it, 3)
    out["one_seed_of_four_counts"] = region + ([(2, 3, 3), (1, 3, 3), (9, 3, 3), (1, 3, 4)], round_it, 1)
    # two seeds: the cheaper one wins cell by cell; (3,3,3) weighs 5 from either side
    out["two_seeds"] = region + ([(1, 3, 3), (4, 3, 3)], np.array([[[2, 1, 6, 2, 1], [1, 0, n, 5, 0], [2, 1, 6, 2, 1]]], np.int32), 2)
    # d one below the leaf depth: the leaf (5,2,6) of depth 3 is cell (2,1,3) at depth 2; ring (2): its face neighbours weigh 3
    leaf = HandPool()
    leaf.put(path_of(5, 2, 6, 3), [OPAQUE, OPAQUE, rgba(43, 2, 3, 255)])
    out["one_level_above_the_leaf"] = (leaf.words(), 2, (0, 1, 3), (4, 2, 1), 0, 1, [2], [(0, 1, 3)],
                                       np.array([[[0, 3, n, 9], [1, 2, 5, 6]]], np.int32), 1)
    return out


PLAN_CASES = plan_cases()


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, clearance, comfort, ring, seeds, want, used = PLAN_CASES[name]
    assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
    for restatement in (cost_field_words, cost_field_relaxed):
        got = restatement(words, depth, origin, dims, clearance, comfort, ring, seeds)
        assert got.dtype == np.int32 and np.array_equal(got, want), (restatement.__name__, got.tolist())
    field = distance_field_words(words, depth, origin, dims, comfort)
    free, _ = weights_of(field, clearance, comfort, ring)
    assert np.array_equal(free, distance_field_words(words, depth, origin, dims, clearance) == -1)
    assert counted_seeds(free, origin, dims, seeds).shape[0] == used
    steps = reach_field_words(words, depth, origin, dims, clearance, seeds)
    for same in ([0] * len(ring), None):                                # every ring cost 0, and comfort == clearance
        got = [r(words, depth, origin, dims, clearance, comfort if same is not None else clearance, same or [], seeds)
               for r in (cost_field_words, cost_field_relaxed)]
        assert np.array_equal(got[0], steps) and np.array_equal(got[1], steps)
    assert check_paths(want, field, origin, dims, clearance, comfort, ring, seeds) == (3 if (want >= 0).any() else 0)


def test_a_zero_dimension_is_an_empty_field():
    words = PLAN_CASES["one_seed"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        got = cost_field_words(words, 3, (0, 0, 0), dims, 1, 2, [3], [(0, 0, 0)])
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32


# ---- the trace -------------------------------------------------------------------------------------------------------------------
TIE_BREAK_PATH = [(3, 3, 3), (2, 3, 3), (1, 3, 3), (0, 3, 3), (0, 2, 3), (0, 1, 3), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def test_the_trace_goes_down_x_first_then_y_then_z():
    """an empty map: from (3,3,3) every one of -x, -y, -z is one nearer the seed (0,0,0); the first in the order wins"""
    cost = cost_field_words(HandPool().words(), 3, (0, 0, 0), (4, 4, 4), 0, 2, [5, 2], [(0, 0, 0)])
    cells, length = trace_path(cost, (0, 0, 0), (3, 3, 3), 64)
    assert length == 10 and [tuple(c) for c in cells.tolist()] == TIE_BREAK_PATH
    cells, length = trace_path(cost, (0, 0, 0), (3, 3, 3), 4)           # the whole length, the first four cells
    assert length == 10 and [tuple(c) for c in cells.tolist()] == TIE_BREAK_PATH[:4]
    # the same region elsewhere in the root: absolute cells
    moved = cost_field_words(HandPool().words(), 3, (2, 1, 4), (4, 4, 4), 0, 0, [], [(2, 1, 4)])
    cells, length = trace_path(moved, (2, 1, 4), (5, 4, 7), 64)
    assert length == 10 and [tuple(c) for c in cells.tolist()] == [(x + 2, y + 1, z + 4) for x, y, z in TIE_BREAK_PATH]


def test_the_trace_of_the_two_rows():
    """the smallest value wins, not the first neighbour: from (4,3,3), value 20, down to 14 rather than along the row"""
    words, depth, origin, dims, clearance, comfort, ring, seeds, want, used = PLAN_CASES["two_rows_round_the_cell"]
    cells, length = trace_path(want, origin, (6, 3, 3), 64)
    assert length == 9 and cells.tolist() == [[6, 3, 3], [6, 4, 3], [5, 4, 3], [4, 4, 3], [3, 4, 3], [2, 4, 3], [1, 4, 3], [0, 4, 3], [0, 3, 3]]
    assert trace_path(want, origin, (4, 3, 3), 2)[0].tolist() == [[4, 3, 3], [4, 4, 3]]
    assert trace_path(want, origin, (0, 3, 3), 64)[1] == 1 and trace_path(want, origin, (1, 3, 3), 64)[1] == 2
    for start in ((3, 3, 3), (7, 3, 3), (-1, 3, 3), (0, 2, 3), (0, 5, 3), (0, 3, 2), (0, 3, 4)):   # blocked, or outside the region
        cells, length = trace_path(want, origin, start, 64)
        assert length == 0 and cells.shape == (0, 3)
    cut = PLAN_CASES["row_through_the_cell"][8]
    assert trace_path(cut, origin, (5, 3, 3), 64)[1] == 0                # -1: no path


# not a cost-to-go field: two 5s side by side with nothing lower beside the second, and a 6 between a 6 and a 7
PLATEAU = np.array([[[0, 1, 2, 5, 5, 7], [-1, -2, 3, 5, 6, 6]]], np.int32)
PLATEAU_TRACES = {                                                      # start -> (cells walked, length)
    (2, 1, 0): ([(2, 1, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)], 4),       # -x is -2, +x is 5: down to the 2
    (3, 1, 0): ([(3, 1, 0), (2, 1, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)], 5),
    (4, 1, 0): ([(4, 1, 0), (3, 1, 0), (2, 1, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)], 6),   # 5 at -x and at -y: -x comes first
    (5, 0, 0): ([(5, 0, 0), (4, 0, 0)], -2),                            # 7 -> 5 (not the 6 below), whose neighbours are 5, 7 and 6
    (5, 1, 0): ([(5, 1, 0)], -1),                                       # 6 between 6 and 7
    (0, 1, 0): ([], 0), (1, 1, 0): ([], 0), (6, 0, 0): ([], 0),         # -1, -2, outside
}


def test_the_trace_stops_on_a_plateau():
    for start, (cells, length) in PLATEAU_TRACES.items():
        got, n = trace_path(PLATEAU, (0, 0, 0), start, 64)
        assert n == length and [tuple(c) for c in got.tolist()] == cells, start
    assert trace_path(PLATEAU, (0, 0, 0), (5, 0, 0), 1)[0].tolist() == [[5, 0, 0]] and trace_path(PLATEAU, (0, 0, 0), (5, 0, 0), 0)[1] == -2


# ---- the two larger worlds tests/test_gpu_plan.py runs on the device: their facts, on the restatement -----------------------------
WORLD_DEPTH = 7


def two_routes():
    """-> (words, origin, dims, seed, start): a wall 8 cells thick, y 14 .. 21 over all x, z 0 .. 6: one cell beyond the region z
    1 .. 5 on both sides.  Two ways through: a tunnel 3 cells wide at x 9 .. 11, straight between seed and start, and a gate 15
    wide at x 100 .. 114.  Seed and start are absolute cells."""
    cells = [(x, y, z) for z in range(7) for y in range(14, 22) for x in range(128) if not (9 <= x <= 11 or 100 <= x <= 114)]
    return cells_pool(cells, WORLD_DEPTH), (0, 0, 1), (128, 40, 5), (10, 4, 3), (10, 32, 3)


TWO_ROUTES_RINGS = (1, 4, [40, 20, 10])                                 # clearance, comfort, ring cost


def plan_maze(pitch, walls, gap, y0=9, z0=60, nz=5):
    """tests/test_gpu_reach.py's serpentine with the gap as an argument -> (words, origin, dims, seed): corridor k is rows k * pitch
    .. k * pitch + pitch - 2 of the region, wall k the row after it, a full-x plane that reaches one cell beyond the region in z
    on both sides; walls 0 .. walls - 1 have a gap, at the high end of x for even k and at the low end for odd k; wall `walls`
    has none.  The seed is at x = 0 in the middle row of corridor 0."""
    n_side = 1 << WORLD_DEPTH
    cells = []
    for k in range(walls + 1):
        xs = range(n_side) if k == walls else range(0, n_side - gap) if k % 2 == 0 else range(gap, n_side)
        cells += [(x, y0 + k * pitch + pitch - 1, z) for z in range(z0 - 1, z0 + nz + 1) for x in xs]
    return cells_pool(cells, WORLD_DEPTH), (0, y0, z0), (n_side, (walls + 2) * pitch - 1, nz), (0, y0 + (pitch - 2) // 2, z0 + nz // 2)


SERPENTINE = (6, 6, 6)                                                  # pitch, gapped walls, gap
SERPENTINE_RINGS = (0, 2, [8, 3])

_WORLDS = {}


def world(name):
    """'two_routes' | 'serpentine' -> dict of the world, its distance field, the weighted cost field and the reach field, computed
    once and left unchanged"""
    if name not in _WORLDS:
        if name == "two_routes":
            words, origin, dims, seed, start = two_routes()
            r, R, ring = TWO_ROUTES_RINGS
        else:
            words, origin, dims, seed = plan_maze(*SERPENTINE)
            start = None
            r, R, ring = SERPENTINE_RINGS
        field = distance_field_separable(words, WORLD_DEPTH, origin, dims, R)
        near = np.where((field >= 0) & (field <= r * r), field, -1).astype(np.int32)
        _WORLDS[name] = dict(words=words, origin=origin, dims=dims, seed=seed, start=start, clearance=r, comfort=R, ring=ring, field=field,
                             cost=cost_field_words(words, WORLD_DEPTH, origin, dims, r, R, ring, [seed], field=field),
                             steps=reach_field_words(words, WORLD_DEPTH, origin, dims, r, [seed], field=near))
    return _WORLDS[name]


def tile_visits(cells, origin, tile=(64, 8, 8)):
    """the largest number of separate times a path is inside one tile of 64 x 8 x 8 cells of the region"""
    runs, seen = {}, None
    for c in cells.tolist():
        t = tuple((c[a] - origin[a]) // tile[a] for a in range(3))
        if t != seen:
            seen = t
            runs[t] = runs.get(t, 0) + 1
    return max(runs.values())


def test_two_routes_the_weights_choose_the_gate():
    w = world("two_routes")
    o, at = w["origin"], [w["start"][a] - w["origin"][a] for a in range(3)]
    cost, steps = w["cost"], w["steps"]
    assert cost[at[2], at[1], at[0]] == 216 and steps[at[2], at[1], at[0]] == 28
    free, wt = weights_of(w["field"], w["clearance"], w["comfort"], w["ring"])
    heavy = check_path(cost, free, wt, o, w["start"])
    light = check_path(steps, free, np.where(free, 1, 0), o, w["start"])
    assert heavy.shape[0] == 217 and light.shape[0] == 29
    assert ((heavy[:, 0] >= 100) & (heavy[:, 0] <= 114) & (heavy[:, 1] >= 14) & (heavy[:, 1] <= 21)).sum() == 8   # through the gate
    assert (light[:, 0] == 10).all()                                    # through the tunnel
    assert not np.array_equal(cost, steps) and np.array_equal(cost < 0, steps < 0)
    zero = cost_field_words(w["words"], WORLD_DEPTH, o, w["dims"], w["clearance"], w["comfort"], [0, 0, 0], [w["seed"]], field=w["field"])
    same = cost_field_words(w["words"], WORLD_DEPTH, o, w["dims"], w["clearance"], w["clearance"], [], [w["seed"]])
    assert np.array_equal(zero, steps) and np.array_equal(same, steps)


def test_the_weighted_serpentine():
    w = world("serpentine")
    cost, steps = w["cost"], w["steps"]
    assert cost.max() == 904 and steps.max() == 869 and cost.max() > steps.max()
    assert (cost == -1).sum() == 3200 and (cost == -2).sum() == 4300
    assert np.array_equal(cost_field_relaxed(w["words"], WORLD_DEPTH, w["origin"], w["dims"], w["clearance"], w["comfort"], w["ring"], [w["seed"]]), cost)
    free, wt = weights_of(w["field"], w["clearance"], w["comfort"], w["ring"])
    far = np.array(np.unravel_index(np.argmax(cost), cost.shape)[::-1]) + np.asarray(w["origin"])
    assert tile_visits(check_path(cost, free, wt, w["origin"], far), w["origin"]) >= 2


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_plan_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_cost_field", "svoslam_field_trace_paths", "svoslam_workspace_plan_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    for name in ("cost_field", "trace_paths", "plan_paths"):
        assert callable(getattr(pkg, name, None)), name
    assert hasattr(pkg.Workspace, "plan_buffers") and pkg.MAX_RING_COST == MAX_RING_COST
    assert [f[0] for f in pkg._PlanStats._fields_] == ["rounds", "tile_runs", "seeds_used", "max_weight"]
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_cost_field(" in header and "int svoslam_field_trace_paths(" in header
    assert "typedef struct { int32_t rounds, tile_runs, seeds_used, max_weight; } svoslam_plan_stats;" in header
    assert "#define SVOSLAM_MAX_RING_COST %d" % MAX_RING_COST in header
    assert "int svoslam_workspace_plan_buffers(const svoslam_workspace *ws, void *d_ptrs[3], uint64_t bytes[3]);" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
