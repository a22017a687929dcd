"""The reach field of a map region (svoslam_pool_reach_field; include/svoslam.h): the definition restated as a
breadth-first search, level by level, on the traversable cells the distance field's definition gives; a second restatement that
relaxes min-plus sweeps to a fixed point on the traversable cells of the separable distance field; the two proven equal on a pool
fused by the CPU oracle and on hand-built pools with every output value written out.  No GPU.

reach_field_words (the definition) is what the device call must produce; tests/test_gpu_reach.py compares against it value for
value."""
import ctypes as C
import os

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, distance_field_words, fields, fused_regions  # noqa: F401
from test_surface_cpu import HAND, HandPool, OPAQUE, load_pkg, path_of, rgba
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
NONE = 1 << 30                                                          # "not reached so far" of the relaxation


# ---- the specification, restated -------------------------------------------------------------------------------------------
def counted_seeds(traversable, origin, dims, seeds):
    """-> [m, 3] int64 region-relative (x, y, z) of the seed entries that count: inside the region and traversable; every
    duplicate is its own row"""
    s = np.asarray(seeds, I64).reshape(-1, 3) - np.asarray(origin, I64)
    s = s[((s >= 0) & (s < np.asarray(dims, I64))).all(1)]
    return s[traversable[s[:, 2], s[:, 1], s[:, 0]]]


def reach_field_words(words, depth, origin, dims, clearance, seeds, field=None):
    """-> int32 [nz, ny, nx]: svoslam_pool_reach_field by its definition.  The traversable set is where the distance field with
    radius = clearance is -1 (`field`: that field when the caller has it already); then a breadth-first search from the counted
    seeds, one level per step: the cells of level k + 1 are the traversable, unreached face neighbours INSIDE THE REGION of the
    cells of level k (boolean array shifts, which cannot leave the array)."""
    assert 0 <= clearance <= MAX_RADIUS
    if field is None:
        field = distance_field_words(words, depth, origin, dims, clearance)
    assert field.shape == (dims[2], dims[1], dims[0])
    free = field == -1
    steps = np.where(free, -1, -2).astype(np.int32)
    s = counted_seeds(free, origin, dims, seeds)
    front = np.zeros(free.shape, bool)
    front[s[:, 2], s[:, 1], s[:, 0]] = True
    level = 0
    while front.any():
        steps[front] = level
        grown = np.zeros(free.shape, bool)
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            grown[tuple(hi)] |= front[tuple(lo)]
            grown[tuple(lo)] |= front[tuple(hi)]
        front = grown & (steps == -1)
        level += 1
    return steps


def reach_field_relaxed(words, depth, origin, dims, clearance, seeds):
    """the same field by another route: the traversable set from the separable distance field, then s(q) = min(s(q), s(neighbour) +
    1) over the six neighbours, all cells at once, repeated until nothing changes"""
    free = distance_field_separable(words, depth, origin, dims, clearance) == -1
    s = np.full(free.shape, NONE, I64)
    c = counted_seeds(free, origin, dims, seeds)
    s[c[:, 2], c[:, 1], c[:, 0]] = 0
    while True:
        t = s.copy()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            t[tuple(hi)] = np.minimum(t[tuple(hi)], s[tuple(lo)] + 1)
            t[tuple(lo)] = np.minimum(t[tuple(lo)], s[tuple(hi)] + 1)
        t = np.where(free, t, NONE)
        if np.array_equal(t, s):
            break
        s = t
    return np.where(~free, -2, np.where(s >= NONE, -1, s)).astype(np.int32)


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
def seeds_for(free, origin, dims, depth, count, rng):
    """`count` traversable cells of the region (absolute), then one blocked cell of it if there is one, a cell of the root outside
    the region if there is one, and cells outside the root"""
    o = np.asarray(origin, I64)
    at = np.argwhere(free)[:, ::-1]
    pick = at[rng.choice(at.shape[0], min(count, at.shape[0]), replace=False)] + o if at.shape[0] else np.zeros((0, 3), I64)
    extra = [(-1, int(o[1]), int(o[2])), (int(o[0]), 1 << depth, int(o[2])), (int(o[0]), int(o[1]), (1 << 31) - 1),
             (-(1 << 31), int(o[1]), int(o[2]))]
    blocked = np.argwhere(~free)[:, ::-1]
    if blocked.shape[0]:
        extra.append(tuple(int(v) for v in blocked[blocked.shape[0] // 2] + o))
    for a in range(3):
        if o[a] > 0:
            outside = o.copy()
            outside[a] -= 1
            extra.append(tuple(int(v) for v in outside))
    return np.concatenate([pick, np.array(extra, I64)]).astype(I64)


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_relaxation_is_the_breadth_first_search(fused, fields, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    rng = np.random.default_rng(7)
    reached = blocked = zero = 0
    for clearance in (0, 1, 3):
        field = fields(depth, region, clearance)
        for count in (1, 7):
            seeds = seeds_for(field == -1, origin, dims, depth, count, rng)
            want = reach_field_words(words, depth, origin, dims, clearance, seeds, field=field)
            assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
            assert np.array_equal(reach_field_relaxed(words, depth, origin, dims, clearance, seeds), want), (clearance, count)
            assert np.array_equal(want == -2, field != -1)
            assert (want == 0).sum() == min(count, int((field == -1).sum()))
            reached, blocked, zero = reached + int((want > 0).sum()), blocked + int((want == -2).sum()), zero + int((want == 0).sum())
    if region in ("whole_root", "low_corner"):
        assert reached > 100 and blocked > 20 and zero >= 6, (reached, blocked, zero)


def test_the_definition_takes_its_own_traversable_set(fused):
    """without `field` the breadth-first search asks the distance field's definition itself"""
    words, _ = fused
    origin, dims = fused_regions(DEPTH - 2)["low_corner"]
    seeds = [(0, 0, 0), (3, 1, 2)]
    for clearance in (0, 1):
        got = reach_field_words(words, DEPTH - 2, origin, dims, clearance, seeds)
        assert np.array_equal(got, reach_field_relaxed(words, DEPTH - 2, origin, dims, clearance, seeds))


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def manhattan_field(seeds, origin, dims):
    """an empty map: |dx| + |dy| + |dz| to the nearest seed, by the formula itself"""
    out = np.zeros((dims[2], dims[1], dims[0]), np.int32)
    for z in range(dims[2]):
        for y in range(dims[1]):
            for x in range(dims[0]):
                out[z, y, x] = min(abs(origin[0] + x - s[0]) + abs(origin[1] + y - s[1]) + abs(origin[2] + z - s[2]) for s in seeds)
    return out


def cells_pool(cells, depth):
    pool = HandPool()
    for xyz in cells:
        pool.put(path_of(*xyz, depth), [OPAQUE] * depth)
    return pool.words()


def reach_cases():
    """name -> (words, depth, origin, dims, clearance, seeds, expected int32 [nz, ny, nx], expected seeds_used)"""
    out = {}
    n, u = -2, -1                                                       # n: not traversable, u: unreachable
    empty = HandPool().words()
    # an empty pool: everything is reachable, the steps are the Manhattan distance to the seed
    out["empty_pool"] = (empty, 2, (1, 0, 1), (3, 4, 2), 0, [(2, 1, 1)], manhattan_field([(2, 1, 1)], (1, 0, 1), (3, 4, 2)), 1)
    out["empty_pool_clearance_2"] = (empty, 2, (1, 0, 1), (3, 4, 2), 2, [(2, 1, 1)], manhattan_field([(2, 1, 1)], (1, 0, 1), (3, 4, 2)), 1)
    # one occupied cell (2,3,3) between the seed (1,3,3) and (3,3,3): the way round adds 2
    one = cells_pool([(2, 3, 3)], 3)
    round_it = np.array([[[2, 1, 2, 3, 4], [1, 0, n, 4, 5], [2, 1, 2, 3, 4]]], np.int32)
    out["one_cell_in_the_way"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(1, 3, 3)], round_it, 1)
    # ... in a region that is the row alone there is no way round
    out["one_cell_in_the_way_of_a_row"] = (one, 3, (0, 3, 3), (5, 1, 1), 0, [(1, 3, 3)], np.array([[[1, 0, n, u, u]]], np.int32), 1)
    # no seeds; a seed on the blocked cell; seeds outside the region; seeds outside the root: nothing is reached
    nowhere = np.array([[[u, u, u, u, u], [u, u, n, u, u], [u, u, u, u, u]]], np.int32)
    out["no_seeds"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [], nowhere, 0)
    out["seed_on_a_blocked_cell"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(2, 3, 3)], nowhere, 0)
    out["seeds_outside_the_region"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(5, 3, 3), (1, 1, 3), (1, 5, 3), (1, 3, 2), (1, 3, 4), (7, 7, 7)],
                                       nowhere, 0)
    out["seeds_outside_the_root"] = (one, 3, (0, 2, 3), (5, 3, 1), 0,
                                     [(-1, 3, 3), (8, 3, 3), (1, -1, 3), (1, 3, 8), ((1 << 31) - 1, 3, 3), (-(1 << 31), 3, 3)], nowhere, 0)
    # duplicates count each and change nothing; of a good and three ignored seeds one counts
    out["duplicate_seeds"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(1, 3, 3), (1, 3, 3), (1, 3, 3)], round_it, 3)
    out["one_seed_of_four_counts"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(2, 3, 3), (1, 3, 3), (9, 3, 3), (1, 3, 4)], round_it, 1)
    # two seeds: the minimum
    out["two_seeds"] = (empty, 3, (1, 4, 2), (7, 1, 1), 0, [(1, 4, 2), (7, 4, 2)], np.array([[[0, 1, 2, 3, 2, 1, 0]]], np.int32), 2)
    out["two_seeds_round_a_cell"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(1, 3, 3), (4, 4, 3)],
                                     np.array([[[2, 1, 2, 3, 2], [1, 0, n, 2, 1], [2, 1, 2, 1, 0]]], np.int32), 2)
    # a closed box: the shell of the 3 x 3 x 3 block about (3,3,3), seen in the plane z = 3 with a margin of one cell
    shell = cells_pool([(x, y, z) for z in (2, 3, 4) for y in (2, 3, 4) for x in (2, 3, 4) if (x, y, z) != (3, 3, 3)], 3)
    out["closed_box_seed_outside"] = (shell, 3, (1, 1, 3), (5, 5, 1), 0, [(1, 1, 3)],
                                      np.array([[[0, 1, 2, 3, 4], [1, n, n, n, 5], [2, n, u, n, 6], [3, n, n, n, 7], [4, 5, 6, 7, 8]]], np.int32), 1)
    out["closed_box_seed_inside"] = (shell, 3, (1, 1, 3), (5, 5, 1), 0, [(3, 3, 3)],
                                     np.array([[[u, u, u, u, u], [u, n, n, n, u], [u, n, 0, n, u], [u, n, n, n, u], [u, u, u, u, u]]], np.int32), 1)
    # ... and through all three layers of the box: the inside is cut off above and below too
    box3 = np.full((3, 3, 3), n, np.int32)
    box3[1, 1, 1] = u
    out["closed_box_all_layers"] = (shell, 3, (2, 2, 2), (3, 3, 3), 0, [(0, 0, 0), (1, 1, 1)], box3, 0)
    # a wall at y = 1, just outside the region y = 2..3: with clearance 1 it blocks the region's border row
    wall = cells_pool([(x, 1, 3) for x in range(8)], 3)
    out["wall_outside_blocks_the_border_row"] = (wall, 3, (0, 2, 3), (8, 2, 1), 1, [(0, 3, 3), (3, 2, 3)],
                                                 np.array([[[n] * 8, [0, 1, 2, 3, 4, 5, 6, 7]]], np.int32), 1)
    out["wall_outside_clearance_0"] = (wall, 3, (0, 2, 3), (8, 2, 1), 0, [(0, 3, 3)],
                                       np.array([[[1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7]]], np.int32), 1)
    # a wall at x = 3 whose only gap, y = 6, lies outside the region y = 0..3: paths stay in the region, the far side is cut off
    gap = cells_pool([(3, y, 3) for y in range(8) if y != 6], 3)
    out["the_gap_is_outside_the_region"] = (gap, 3, (0, 0, 3), (8, 4, 1), 0, [(0, 0, 3)],
                                            np.array([[[0, 1, 2, n, u, u, u, u], [1, 2, 3, n, u, u, u, u], [2, 3, 4, n, u, u, u, u],
                                                       [3, 4, 5, n, u, u, u, u]]], np.int32), 1)
    # ... a region that holds the gap reaches it: through (3,6,3), 9 steps from (0,0,3), and down the far side
    far = np.array([[[0, 1, 2, n, 16, 17, 18, 19], [1, 2, 3, n, 15, 16, 17, 18], [2, 3, 4, n, 14, 15, 16, 17], [3, 4, 5, n, 13, 14, 15, 16],
                     [4, 5, 6, n, 12, 13, 14, 15], [5, 6, 7, n, 11, 12, 13, 14], [6, 7, 8, 9, 10, 11, 12, 13]]], np.int32)
    out["the_gap_is_inside_the_region"] = (gap, 3, (0, 0, 3), (8, 7, 1), 0, [(0, 0, 3)], far, 1)
    # alpha 127 beside 128 at depth 2: (2,2,2) is occupied, (3,2,2) is not
    out["alpha_127_128"] = (HAND["alpha_127_128"][0], 2, (0, 2, 2), (4, 1, 1), 0, [(3, 2, 2)], np.array([[[u, u, n, 0]]], np.int32), 1)
    out["alpha_127_128_seed_on_128"] = (HAND["alpha_127_128"][0], 2, (0, 2, 2), (4, 1, 1), 0, [(2, 2, 2)], np.array([[[u, u, n, u]]], np.int32), 0)
    # d one below the leaf depth: the leaf (5,2,6) of depth 3 is cell (2,1,3) at depth 2
    leaf = HandPool()
    leaf.put(path_of(5, 2, 6, 3), [OPAQUE, OPAQUE, rgba(43, 2, 3, 255)])
    out["one_level_above_the_leaf"] = (leaf.words(), 2, (0, 1, 3), (4, 2, 1), 0, [(0, 1, 3)],
                                       np.array([[[0, 1, n, 5], [1, 2, 3, 4]]], np.int32), 1)
    # clearance 1 about one cell (2,3,3) in the plane z = 3: the cell and its four face neighbours are blocked
    plus = np.array([[[4, 5, n, 9, 8], [3, n, n, n, 7], [2, 3, n, 5, 6], [1, 2, 3, 4, 5], [0, 1, 2, 3, 4]]], np.int32)
    out["clearance_1_about_a_cell"] = (one, 3, (0, 2, 3), (5, 5, 1), 1, [(0, 6, 3)], plus, 1)
    return out


REACH_CASES = reach_cases()


@pytest.mark.parametrize("name", sorted(REACH_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, clearance, seeds, want, used = REACH_CASES[name]
    assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
    for restatement in (reach_field_words, reach_field_relaxed):
        got = restatement(words, depth, origin, dims, clearance, seeds)
        assert got.dtype == np.int32 and np.array_equal(got, want), (restatement.__name__, got.tolist())
    free = distance_field_words(words, depth, origin, dims, clearance) == -1
    assert counted_seeds(free, origin, dims, seeds).shape[0] == used


def test_a_zero_dimension_is_an_empty_field():
    words = REACH_CASES["one_cell_in_the_way"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        got = reach_field_words(words, 3, (0, 0, 0), dims, 1, [(0, 0, 0)])
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32


def test_library_exports_the_reach_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_reach_field", "svoslam_workspace_reach_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "reach_field") and hasattr(pkg.Workspace, "reach_buffers")
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_reach_field(" in header and "} svoslam_reach_stats;" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header and "#define SVOSLAM_MAX_RADIUS_CELLS %d" % MAX_RADIUS in header
    assert "int svoslam_workspace_field_buffers(const svoslam_workspace *ws, void *d_ptrs[3], uint64_t bytes[3]);" in header
