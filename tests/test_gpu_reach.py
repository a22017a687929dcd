"""svoslam_pool_reach_field on the device: every value equals the host restatement of the specification (tests/test_reach_cpu.py:
reach_field_words, the breadth-first search, on the traversable cells of the distance field's restatements) applied to the pool's
own words -- never a second device result alone.

The serpentine mazes are the cases a relaxation that stops a round early, or forgets to wake a neighbour tile, fails.  The tile
is 64 x 8 x 8 cells, and a clearance of 1 needs corridors three cells wide, walls every four y: at most two corridors cross a
tile, so no tile can be entered three times at clearance 1.  The maze with walls every second y (clearance 0) is the one whose
shortest path enters a tile three separate times; the maze with walls every fourth y runs at clearance 0 and 1 and re-enters tiles
twice; every other fact is asserted of all three runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, distance_field_words
from test_gpu_field import FUSED_CASES as FIELD_FUSED_CASES, case_region, same_field
from test_gpu_query import fused_pool
from test_reach_cpu import REACH_CASES, cells_pool, counted_seeds, reach_field_words, seeds_for
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE, occupied_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILE = (64, 8, 8)              # map_relax.hpp: the cells of a tile, x y z


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """depth -> (pool, its words, the fused points, workspace): fused on the device, twice, shared by the tests below and left
    unchanged"""
    pkg, torch = env
    out = {}
    for depth in (6, 9):
        ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 41)
        out[depth] = (pool, pool.words(), pts, ws)
    return out


def reach(pkg, ws, pool, depth, origin, dims, clearance, seeds, **kw):
    stats = {}
    got = pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds, stats=stats, **kw)
    return got, stats


# ---- hand-built pools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(REACH_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, origin, dims, clearance, seeds, want, used = REACH_CASES[name]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    got, stats = reach(pkg, ws, pool, depth, origin, dims, clearance, seeds)
    same_field(got, want)
    same_field(got, reach_field_words(words, depth, origin, dims, clearance, seeds))
    assert stats["seeds_used"] == used and stats["rounds"] >= 1 and stats["tile_runs"] >= (1 if used else 0)


# ---- serpentine mazes ------------------------------------------------------------------------------------------------------------
MAZE_DEPTH, MAZE_Y0, MAZE_Z0, MAZE_NZ, MAZE_GAP = 7, 9, 60, 5, 4


def maze(pitch, walls):
    """-> (words, origin, dims, seed).  Rows of the region, from its first: corridor k is rows k * pitch .. k * pitch + pitch - 2,
    wall k the row after it, a full-x plane of occupied cells that reaches one cell beyond the region in z on both sides.  Walls
    0 .. walls - 1 have a gap of MAZE_GAP cells, at the high end of x for even k and at the low end for odd k; wall `walls` has
    none, so the corridor behind it is free and cut off.  The seed is at x = 0 in the middle row of corridor 0."""
    n_side = 1 << MAZE_DEPTH
    cells = []
    for k in range(walls + 1):
        xs = range(n_side) if k == walls else range(0, n_side - MAZE_GAP) if k % 2 == 0 else range(MAZE_GAP, n_side)
        cells += [(x, MAZE_Y0 + k * pitch + pitch - 1, z) for z in range(MAZE_Z0 - 1, MAZE_Z0 + MAZE_NZ + 1) for x in xs]
    origin, dims = (0, MAZE_Y0, MAZE_Z0), (n_side, (walls + 2) * pitch - 1, MAZE_NZ)
    return cells_pool(cells, MAZE_DEPTH), origin, dims, (0, MAZE_Y0 + (pitch - 2) // 2, MAZE_Z0 + MAZE_NZ // 2)


def tile_of(q):
    return tuple(int(q[a]) // TILE[a] for a in range(3))


def tile_entries(steps, target):
    """walks a shortest path back from `target` (region-relative x, y, z) to a seed, always to the first neighbour one step nearer;
    -> the largest number of separate times the path is inside one tile"""
    q = np.asarray(target, np.int64)
    seen, runs = tile_of(q), {tile_of(q): 1}
    while steps[q[2], q[1], q[0]] > 0:
        for step in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
            p = q + step
            if (p >= 0).all() and (p < steps.shape[::-1]).all() and steps[p[2], p[1], p[0]] == steps[q[2], q[1], q[0]] - 1:
                break
        else:
            raise AssertionError("no neighbour one step nearer at %s" % q.tolist())
        q = p
        if tile_of(q) != seen:
            seen = tile_of(q)
            runs[seen] = runs.get(seen, 0) + 1
    return max(runs.values())


@pytest.mark.parametrize("pitch,walls,clearance,entries", [(2, 14, 0, 3), (4, 8, 0, 2), (4, 8, 1, 2)],
                         ids=["walls_every_2_clearance_0", "walls_every_4_clearance_0", "walls_every_4_clearance_1"])
def test_serpentine_maze(env, pitch, walls, clearance, entries):
    pkg, torch = env
    words, origin, dims, seed = maze(pitch, walls)
    want = reach_field_words(words, MAZE_DEPTH, origin, dims, clearance, [seed], field=distance_field_separable(words, MAZE_DEPTH, origin, dims, clearance))
    # the facts that make this the case it is meant to be, on the restatement's result
    far = np.unravel_index(np.argmax(want), want.shape)[::-1]
    assert want.max() > 4 * sum(TILE), want.max()
    assert tile_entries(want, far) >= entries
    assert (want == -1).sum() > 0 and (want == -2).sum() > 0 and want[seed[2] - origin[2], seed[1] - origin[1], seed[0] - origin[0]] == 0
    assert far[1] >= walls * pitch                                  # the farthest reached cell is in the last open corridor
    assert dims[0] > TILE[0] and dims[1] > 2 * TILE[1] and dims[2] < TILE[2]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    got, stats = reach(pkg, ws, pool, MAZE_DEPTH, origin, dims, clearance, [seed])
    same_field(got, want)
    assert stats["seeds_used"] == 1 and stats["rounds"] > walls     # every corridor is at least a round


# ---- fused pools -------------------------------------------------------------------------------------------------------------
# (fused depth, d, (nx, ny, nz), origin x: "lo" 0 | "in" 37 | "hi" N - nx | "pt" about the cloud, clearance, seeds from T).  nx 1, 63,
# 64, 65, 130: the edges of a row word, a wavefront and a tile; ny, nz 1, 7, 8, 9, 17: one row, one less than, equal to, one more than
# and more than twice the tile's side.  Sizes that do not fit the lattice of d are cut to it (N = 16 at d = 4, 64 at 6, 128 at 7).
FUSED_CASES = [
    (9, 9, (1, 1, 1), "pt", 0, 1), (9, 9, (63, 7, 17), "in", 1, 7), (9, 9, (64, 17, 8), "lo", 5, 1), (9, 9, (65, 8, 9), "hi", 5, 7),
    (9, 9, (130, 9, 7), "in", 0, 7), (9, 9, (130, 1, 17), "hi", 1, 1), (9, 9, (65, 17, 17), "pt", 5, 7), (9, 9, (130, 8, 8), "pt", 0, 1),
    (9, 9, (130, 17, 9), "pt", 1, 1),
    (9, 7, (64, 9, 17), "in", 5, 7), (9, 7, (130, 1, 8), "lo", 1, 1), (9, 7, (63, 17, 1), "hi", 0, 7), (9, 7, (1, 7, 9), "pt", 1, 1),
    (6, 6, (63, 8, 17), "lo", 5, 7), (6, 6, (64, 17, 1), "lo", 1, 1), (6, 6, (1, 1, 7), "hi", 0, 1), (6, 6, (20, 7, 9), "in", 5, 7),
    (6, 6, (65, 17, 17), "pt", 0, 7), (6, 4, (65, 17, 17), "lo", 1, 7), (6, 4, (1, 9, 1), "hi", 0, 1), (6, 4, (5, 1, 8), "in", 5, 1),
]


@pytest.fixture(scope="module")
def reference(fused):
    """case -> (origin, dims, seeds, the distance field's restatement, the reach field's), computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            depth, d, shape, ox, clearance, count = case
            words = fused[depth][1]
            origin, dims = case_region(words, d, shape, ox, clearance)
            field = distance_field_separable(words, d, origin, dims, clearance)
            seeds = seeds_for(field == -1, origin, dims, d, count, np.random.default_rng(FUSED_CASES.index(case)))
            cache[case] = (origin, dims, seeds, field, reach_field_words(words, d, origin, dims, clearance, seeds, field=field))
        return cache[case]
    return get


def test_the_fused_cases_are_not_empty(fused, reference):
    """on the restatement's results, never the device's"""
    reached = blocked = zero = ignored = 0
    nx, nyz, ox, radii, counts, ds = set(), set(), set(), set(), set(), set()
    for case in FUSED_CASES:
        depth, d, shape, kind, clearance, count = case
        origin, dims, seeds, field, want = reference(case)
        nx.add(shape[0]); nyz.update(shape[1:]); ox.add(kind); radii.add(clearance); counts.add(count); ds.add((depth, d))
        reached, blocked, zero = reached + int((want > 0).sum()), blocked + int((want == -2).sum()), zero + int((want == 0).sum())
        ignored += seeds.shape[0] - counted_seeds(field == -1, origin, dims, seeds).shape[0]
    assert reached > 1000 and blocked > 1000 and zero > 20 and ignored > 4 * len(FUSED_CASES), (reached, blocked, zero, ignored)
    assert nx == {1, 63, 64, 65, 130, 20, 5} and nyz == {1, 7, 8, 9, 17} and ox == {"lo", "in", "hi", "pt"} and radii == {0, 1, 5}
    assert counts == {1, 7} and ds == {(9, 9), (9, 7), (6, 6), (6, 4)}


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-r%d-seeds%d" % (c[0], c[1], *c[2], c[3], c[4], c[5]))
def test_fused_cloud(env, fused, reference, case):
    pkg, torch = env
    pool, words, pts, ws = fused[case[0]]
    origin, dims, seeds, field, want = reference(case)
    got, stats = reach(pkg, ws, pool, case[1], origin, dims, case[4], seeds)
    same_field(got, want)
    assert stats["seeds_used"] == counted_seeds(field == -1, origin, dims, seeds).shape[0] == int((want == 0).sum())


@pytest.mark.parametrize("case", [FUSED_CASES[k] for k in (6, 8, 12, 17)], ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-r%d" % (c[0], c[1], *c[2], c[3], c[4]))
def test_blocked_is_where_the_device_distance_field_is_not_minus_1(env, fused, reference, case):
    pkg, torch = env
    pool, words, pts, ws = fused[case[0]]
    origin, dims, seeds, field, want = reference(case)
    assert (want == -2).sum() > 0 and (want >= 0).sum() > 0        # regions about an occupied cell: both kinds of cell
    dist2 = pkg.distance_field(ws, pool, case[1], origin, dims, case[4])
    got, _ = reach(pkg, ws, pool, case[1], origin, dims, case[4], seeds)
    assert np.array_equal(got == -2, dist2 != -1)
    same_field(dist2, field)


# the smallest shapes with two tiles on x and a partial tile on each other axis
NO_RING_CASES = [(9, 9, shape, "pt", clearance, 7) for shape in ((65, 9, 17), (130, 8, 8)) for clearance in (0, 1)]


@pytest.mark.parametrize("case", NO_RING_CASES, ids=lambda c: "%dx%dx%d-r%d" % (*c[2], c[4]))
def test_the_cost_field_without_rings_is_the_reach_field(env, fused, case):
    """comfort_cells == clearance_cells: every weight is 1, and the two fields share map_relax's seed kernel, staging, write-back and
    finish kernel, so they agree value for value and count the same seeds"""
    pkg, torch = env
    depth, d, shape, ox, clearance, count = case
    pool, words, pts, ws = fused[depth]
    origin, dims = case_region(words, d, shape, ox, clearance)
    field = distance_field_separable(words, d, origin, dims, clearance)
    seeds = seeds_for(field == -1, origin, dims, d, count, np.random.default_rng(100 + NO_RING_CASES.index(case)))
    want = reach_field_words(words, d, origin, dims, clearance, seeds, field=field)
    assert (want >= 1).sum() >= 50, int((want >= 1).sum())                   # on the restatement: the case is not empty
    steps, reach_stats = reach(pkg, ws, pool, d, origin, dims, clearance, seeds)
    cost_stats = {}
    cost = pkg.cost_field(ws, pool, d, origin, dims, clearance, clearance, [], seeds, stats=cost_stats)
    same_field(cost, steps)
    same_field(steps, want)
    assert cost_stats["seeds_used"] == reach_stats["seeds_used"] == int((want == 0).sum())
    assert cost_stats["max_weight"] == 1


def test_the_distance_field_is_unchanged_by_reach_calls_on_its_workspace(env, fused):
    """the reach field runs the distance field's host code in the distance field's slots: a few cases of test_gpu_field.py's table
    give the same values before and after, and the values of the restatement"""
    pkg, torch = env
    for case in [FIELD_FUSED_CASES[k] for k in (2, 4, 8, 12, 20)]:
        depth, d, shape, ox, radius = case
        pool, words, pts, ws = fused[depth]
        origin, dims = case_region(words, d, shape, ox, radius)
        before = pkg.distance_field(ws, pool, d, origin, dims, radius)
        mid = [origin[a] + dims[a] // 2 for a in range(3)]
        reach(pkg, ws, pool, d, origin, dims, 1, [mid, origin])
        reach(pkg, ws, pool, d, [0, 0, 0], [min(1 << d, 70), 9, 9], 3, [[1, 1, 1]])
        after = pkg.distance_field(ws, pool, d, origin, dims, radius)
        same_field(after, before)
        same_field(after, distance_field_separable(words, d, origin, dims, radius))


# ---- the rest ----------------------------------------------------------------------------------------------------------------------
def test_depth_16_cells_beyond_15_bits(env):
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 16, 2000, 43)
    words = pool.words()
    xyz = occupied_cells(words, 16)[0]
    anchor = xyz[np.argmax(xyz.max(1))]
    dims = [65, 9, 3]
    origin = [int(np.clip(anchor[a] - dims[a] // 2, 0, (1 << 16) - dims[a])) for a in range(3)]
    field = distance_field_words(words, 16, origin, dims, 2)
    seeds = seeds_for(field == -1, origin, dims, 16, 2, np.random.default_rng(3))
    want = reach_field_words(words, 16, origin, dims, 2, seeds, field=field)
    assert max(origin) >= 1 << 15 and (want == 0).sum() == 2 and (want > 0).sum() > 100 and (want == -2).sum() > 5
    got, stats = reach(pkg, ws, pool, 16, origin, dims, 2, seeds)
    same_field(got, want)
    assert stats["seeds_used"] == 2


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(hp.words())
    # (1,1,0) and (0,0,1) are occupied; with clearance 1 every cell has one of them as a face neighbour
    for clearance, want, used in ((0, [[[0, 1], [1, -2]], [[-2, 2], [2, 3]]], 1), (1, [[[-2, -2], [-2, -2]], [[-2, -2], [-2, -2]]], 0)):
        got, stats = reach(pkg, ws, pool, 1, (0, 0, 0), (2, 2, 2), clearance, [(0, 0, 0), (1, 1, 0)])
        same_field(got, np.array(want, np.int32))
        same_field(got, reach_field_words(hp.words(), 1, (0, 0, 0), (2, 2, 2), clearance, [(0, 0, 0), (1, 1, 0)]))
        assert stats["seeds_used"] == used


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 17, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    seeds = [origin, [origin[a] + dims[a] - 1 for a in range(3)], [origin[0] + 64, origin[1] + 8, origin[2]]]
    unsynced, _ = reach(pkg, ws, pool, depth, origin, dims, 1, seeds)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want = reach_field_words(words, depth, origin, dims, 1, seeds, field=distance_field_separable(words, depth, origin, dims, 1))
    assert (want == 0).sum() >= 1 and (want > 0).sum() > 100 and (want == -2).sum() > 100
    same_field(reach(pkg, ws, pool, depth, origin, dims, 1, seeds)[0], unsynced)
    same_field(unsynced, want)


def test_workspace_slots_are_reused(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    ws = pkg.Workspace()
    assert ws.reach_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    seeds = [(6, 4, 8), (30, 20, 12), (63, 63, 39), (0, 0, 0)]
    first, _ = reach(pkg, ws, pool, 6, *large, 1, seeds)
    slots, field_slots = ws.reach_buffers(), ws.field_buffers()
    assert all(p != 0 and b > 0 for p, b in slots + field_slots)
    again, _ = reach(pkg, ws, pool, 6, *large, 1, seeds)
    assert ws.reach_buffers() == slots and ws.field_buffers() == field_slots   # a second call of the same size allocates nothing
    want = reach_field_words(words, 6, *large, 1, seeds, field=distance_field_separable(words, 6, *large, 1))
    assert (want > 0).sum() > 1000 and (want == -2).sum() > 1000
    same_field(first, want)
    same_field(again, want)
    got, _ = reach(pkg, ws, pool, 6, *small, 1, seeds)             # a smaller call in the larger call's slots
    assert ws.reach_buffers() == slots and ws.field_buffers() == field_slots
    same_field(got, reach_field_words(words, 6, *small, 1, seeds, field=distance_field_separable(words, 6, *small, 1)))
    ws.close()                                                     # release_all releases the new slots with the rest


def test_as_tensor_and_seeds_as_a_tensor(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (3, 0, 9), (61, 30, 5)
    field = distance_field_separable(words, 6, origin, dims, 1)
    seeds = seeds_for(field == -1, origin, dims, 6, 3, np.random.default_rng(5))
    want = reach_field_words(words, 6, origin, dims, 1, seeds, field=field)
    stats = {}
    got = pkg.reach_field(ws, pool, 6, origin, dims, 1, torch.from_numpy(seeds.astype(np.int32)).cuda(), as_tensor=True, stats=stats)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (5, 30, 61)
    same_field(got.cpu().numpy(), want)
    assert stats["seeds_used"] == 3 and set(stats) == {"rounds", "tile_runs", "seeds_used"}
    same_field(pkg.reach_field(ws, pool, 6, origin, dims, 1, seeds), want)        # an array, no stats
    with pytest.raises(ValueError):
        pkg.reach_field(ws, pool, 6, origin, dims, 1, torch.zeros((1, 3), dtype=torch.int64, device="cuda"))


def test_box_to_cells_then_the_map_reach_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    field = distance_field_separable(words, 6, lo.tolist(), dims.tolist(), 1)
    free = np.argwhere(field == -1)[:, ::-1] + lo
    cell = 2.0 * EDGE / 64
    inside = [(np.asarray(CENTER) - EDGE + (free[k] + 0.5) * cell).tolist() for k in (0, free.shape[0] // 2)]   # the cells' centres
    seeds_m = inside + [[100.0, 0.0, 0.0]]                          # ... and a point outside the root cube
    seed_cells = [pkg.box_to_cells(6, CENTER, EDGE, s + s)[0].tolist() for s in inside]
    assert seed_cells == [free[0].tolist(), free[free.shape[0] // 2].tolist()]
    want = reach_field_words(words, 6, lo.tolist(), dims.tolist(), 1, seed_cells, field=field)
    assert (want == 0).sum() == 2 and (want > 0).sum() > 100 and (want == -2).sum() > 20
    ckpt, out = tmp_path / "map.svopool", tmp_path / "reach.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_reach.py"), str(ckpt), str(out), "--clearance", "1", "--box"] + [repr(float(v)) for v in box]
    for s in seeds_m:
        cmd += ["--seed"] + [repr(float(v)) for v in s]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_field(z["steps"], want)
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    assert z["seed_cells"].tolist() == seed_cells + [[-1, -1, -1]] and int(z["clearance_cells"]) == 1
    assert float(z["cell_size"]) == cell and z["metres"].dtype == np.float32 and z["metres"].shape == want.shape
    assert np.array_equal(z["metres"], np.where(want >= 0, want.astype(np.float64) * cell, np.inf).astype(np.float32))
    assert "2 of 3 seeds counted, %d cells reached" % int((want >= 0).sum()) in r.stdout


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got, stats = reach(pkg, ws, pool, 5, (1, 2, 3), dims, 4, [(1, 2, 3)])
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32
        assert stats == {"rounds": 0, "tile_runs": 0, "seeds_used": 0}
    assert ws.reach_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3   # nothing was launched, nothing allocated
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    seed_buf = torch.tensor([[1, 2, 3], [2, 2, 3]], dtype=torch.int32, device="cuda")
    null, ptr, sp = C.c_void_p(0), pkg._ptr(buf), pkg._ptr(seed_buf)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, seeds=sp, n=2, out=ptr, stats=None):
        return L.svoslam_pool_reach_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, seeds, n, out, stats, pkg._stream())
    st = pkg._ReachStats()
    assert field() == 0 and field(stats=C.byref(st)) == 0 and st.seeds_used == 2 and st.rounds >= 1
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=null) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=null) == 0
    assert field(seeds=null, n=0) == 0 and field(n=0) == 0         # no seeds: allowed, with or without a pointer
    assert field(n=-1) == -1 and field(seeds=null, n=1) == -1 and field(n=-1, dims=(0, 2, 2)) == -1
    assert field(seeds=null, n=2, dims=(0, 2, 2)) == -1
    assert field(ws_ref=None) == -1 and field(origin=None) == -1 and field(dims=None) == -1
    assert field(ws_ref=None, dims=(0, 2, 2)) == -1 and field(depth=0, dims=(0, 2, 2)) == -1
    assert field(depth=0) == -1 and field(depth=17) == -1
    assert field(dims=(-1, 2, 2)) == -1 and field(dims=(4, 2, -1)) == -1 and field(dims=(0, -1, 2)) == -1
    for a in range(3):                                             # one cell outside the root on each side
        origin, dims = [1, 2, 3], [4, 2, 2]
        origin[a] = -1
        assert field(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert field(origin=origin) == -1
        origin[a] = 32 - dims[a]
        assert field(origin=origin) == 0
        origin[a], dims[a] = 0, 33
        assert field(origin=origin, dims=dims) == -1
    assert field(radius=0) == 0 and field(radius=64) == 0
    assert field(radius=-1) == -1 and field(radius=4097) == -1 and field(radius=4097, dims=(0, 2, 2)) == -1
    assert field(pool_ref=None) == -1 and field(out=null) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # the distance field's limits: refused before anything is allocated
    slots, field_slots = ws.reach_buffers(), ws.field_buffers()
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), radius=4096) == -6
    assert field(depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), radius=0) == -6      # 2^25 tiles: more than a launch takes
    assert ws.reach_buffers() == slots and ws.field_buffers() == field_slots
    with pytest.raises(Exception):
        pkg.reach_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097, [(0, 0, 0)])
    with pytest.raises(Exception):
        pkg.reach_field(ws, pool, 5, (30, 0, 0), (4, 4, 4), 3, [(0, 0, 0)])
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        _, stats = reach(pkg, ws, pool, 6, (0, 0, 0), (64, 20, 3), 1, [(63, 19, 2), (0, 0, 0)])
        reach(pkg, ws, pool, 4, (1, 2, 3), (9, 3, 3), 0, [])
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0 and stats["rounds"] >= 1
        reach(pkg, ws, pool, 6, (0, 0, 0), (64, 0, 3), 1, [(0, 0, 0)])   # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            reach(pkg, ws, pool, 6, (0, 0, 0), (65, 2, 3), 1, [(0, 0, 0)])   # refused: not bracketed either
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])
