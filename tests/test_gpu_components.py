"""svoslam_pool_label_components on the device: every value equals the host restatement of the specification
(tests/test_components_cpu.py: component_labels_words, the flood from the smallest unlabelled index, on the set the distance
field's restatements give) applied to the pool's own words -- never a second device result alone.  The sizes equal a count of the
expected labels, the stats the expected numbers.

The cloud the field tests fuse is a closed surface with at most two free and one solid component: it proves nothing about
merging and is kept for the cases about pending fusions and shared workspaces.  The cases that can break a union-find are random
occupancy (thousands of components, hundreds across tile faces, many tile-local parts of one component in one tile), serpentine
mazes (one component that re-enters tiles), staircases (a union chain through twenty tiles), a checkerboard (every cell a root)
and pairs of cells in contact across tile faces, edges and corners.

The mazes: a tile is 64 x 8 x 8 cells and the region is one tile deep.  With walls every second row a tile holds four corridors,
of which the wall gaps at its end join two: three tile-local parts of the one corridor, which is asserted.  With walls every
fourth row no tile holds more than two parts of one component, wherever the region is placed: one of any two consecutive walls
has its gap inside the tile (the argument and the count over placements are in tests/test_components_cpu.py); that maze asserts
two."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_components_cpu import (COMPONENT_CASES, RANDOM_DEPTH, RANDOM_FACTS, RANDOM_P, RANDOM_REGIONS, STAIR_DEPTH, TILE, WIDE_DEPTH, check_contract,
                                 component_labels_words, component_sizes, component_stats, random_expected, random_facts, random_pool,
                                 staircase, tile_facts, wide_random_pool)
from test_field_cpu import distance_field_separable, distance_field_words
from test_gpu_field import FUSED_CASES as FIELD_FUSED_CASES, case_region, same_field
from test_gpu_query import fused_pool
from test_gpu_reach import MAZE_DEPTH, maze
from test_reach_cpu import cells_pool, reach_field_words
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE, occupied_cells
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """(pool, its words, the fused points, workspace) at depth 6: fused on the device, twice, shared and left unchanged"""
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 6, 15000, 41)
    return pool, pool.words(), pts, ws


@pytest.fixture(scope="module")
def random_pools(env):
    """p -> (pool, workspace) of the random occupancy, uploaded once"""
    pkg, torch = env
    cache = {}

    def get(p):
        if p not in cache:
            pool = pkg.Pool()
            pool.set_words(random_pool(p)[0])
            cache[p] = (pool, pkg.Workspace())
        return cache[p]
    return get


def on_device(pkg, words):
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    return ws, pool


def expect(pkg, ws, pool, depth, origin, dims, clearance, solid, want):
    """one call with sizes and stats: every value is the restatement's"""
    stats = {}
    labels, sizes = pkg.label_components(ws, pool, depth, origin, dims, clearance, solid=solid, sizes=True, stats=stats)
    same_field(labels, want)
    same_field(sizes, component_sizes(want))
    components, largest = component_stats(want)
    assert (stats["components"], stats["largest"]) == (components, largest) and set(stats) == {"components", "largest", "tile_passes", "unions"}
    assert stats["tile_passes"] >= (1 if components else 0) and 0 <= stats["unions"]
    return labels, sizes, stats


# ---- hand-built pools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COMPONENT_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, origin, dims, clearance, solid, want, components, largest = COMPONENT_CASES[name]
    ws, pool = on_device(pkg, words)
    _, _, stats = expect(pkg, ws, pool, depth, origin, dims, clearance, solid, want)
    assert (stats["components"], stats["largest"]) == (components, largest)
    same_field(pkg.label_components(ws, pool, depth, origin, dims, clearance, solid=solid),
               component_labels_words(words, depth, origin, dims, clearance, solid))


# ---- random occupancy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solid", [False, True], ids=["free", "solid"])
@pytest.mark.parametrize("clearance", [0, 1])
@pytest.mark.parametrize("region", sorted(RANDOM_REGIONS))
@pytest.mark.parametrize("p", RANDOM_P)
def test_random_occupancy(env, random_pools, p, region, clearance, solid):
    pkg, torch = env
    origin, dims, want = random_expected(p, region, clearance, solid)
    if (p, clearance, solid) == (0.31, 0, True) and region in RANDOM_FACTS:      # a condition on the restatement, not a measurement
        facts = random_facts(region)
        assert all(got >= need for got, need in zip(facts, RANDOM_FACTS[region])), facts
    pool, ws = random_pools(p)
    labels, sizes, stats = expect(pkg, ws, pool, RANDOM_DEPTH, origin, dims, clearance, solid, want)
    check_contract(labels)
    roots = labels.reshape(-1) == np.arange(labels.size)
    assert sizes.reshape(-1)[roots].sum() == (labels >= 0).sum()
    if region != "B" and stats["components"] > 1:
        assert stats["unions"] > 0


# ---- serpentine mazes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch,walls,clearance,parts", [(2, 14, 0, 3), (4, 8, 0, 2), (4, 8, 1, 2)],
                         ids=["walls_every_2_clearance_0", "walls_every_4_clearance_0", "walls_every_4_clearance_1"])
def test_serpentine_maze(env, pitch, walls, clearance, parts):
    pkg, torch = env
    words, origin, dims, seed = maze(pitch, walls)
    field = distance_field_separable(words, MAZE_DEPTH, origin, dims, clearance)
    free = component_labels_words(words, MAZE_DEPTH, origin, dims, clearance, False, field=field)
    solid = component_labels_words(words, MAZE_DEPTH, origin, dims, clearance, True, field=field)
    # the facts that make this the case it is meant to be, on the restatement's result
    components, spanning, most = tile_facts(free)
    assert components == 2 and spanning == 2 and most >= parts        # the corridor and the corridor cut off behind the last wall
    corridor = free[seed[2] - origin[2], seed[1] - origin[1], seed[0] - origin[0]]
    assert corridor == free[free >= 0].min() and (free == corridor).sum() > (free > corridor).sum() > 0
    assert np.array_equal(reach_field_words(words, MAZE_DEPTH, origin, dims, clearance, [seed], field=field) >= 0, free == corridor)
    assert component_stats(solid)[0] == walls + 1                       # each wall is its own component
    assert dims[0] > TILE[0] and dims[1] > 2 * TILE[1] and dims[2] < TILE[2]
    ws, pool = on_device(pkg, words)
    expect(pkg, ws, pool, MAZE_DEPTH, origin, dims, clearance, False, free)
    expect(pkg, ws, pool, MAZE_DEPTH, origin, dims, clearance, True, solid)


# ---- staircases: a long union chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirrored", [False, True], ids=["minimum_at_one_end", "minimum_in_the_middle"])
def test_staircase(env, mirrored):
    pkg, torch = env
    cells, origin, dims, first = staircase(mirrored)
    words = cells_pool(cells, STAIR_DEPTH)
    want = component_labels_words(words, STAIR_DEPTH, origin, dims, 0, True, field=distance_field_separable(words, STAIR_DEPTH, origin, dims, 0))
    rel = np.asarray(cells, np.int64) - np.asarray(origin, np.int64)
    tiles = len(set(map(tuple, (rel // np.asarray(TILE)).tolist())))
    start = rel[first]
    assert tiles >= 20 and component_stats(want) == (1, len(cells))
    assert want.max() == (start[2] * dims[1] + start[1]) * dims[0] + start[0]
    ws, pool = on_device(pkg, words)
    _, _, stats = expect(pkg, ws, pool, STAIR_DEPTH, origin, dims, 0, True, want)
    assert stats["unions"] == tiles - 1                               # a path: one link per tile face it crosses, none twice


# ---- a checkerboard: every cell is a root ---------------------------------------------------------------------------------------
def test_checkerboard(env):
    pkg, torch = env
    origin, dims = (64, 8, 16), (64, 16, 16)
    cells = [(origin[0] + x, origin[1] + y, origin[2] + z) for z in range(16) for y in range(16) for x in range(64) if (x + y + z) % 2 == 0]
    words = cells_pool(cells, 7)
    ws, pool = on_device(pkg, words)
    index = np.arange(64 * 16 * 16, dtype=np.int32).reshape(16, 16, 64)
    field = distance_field_separable(words, 7, origin, dims, 0)
    for solid in (False, True):
        want = component_labels_words(words, 7, origin, dims, 0, solid, field=field)
        assert np.array_equal(want, np.where((field == -1) != solid, index, -1)) and component_stats(want) == (8192, 1)
        _, _, stats = expect(pkg, ws, pool, 7, origin, dims, 0, solid, want)
        assert stats["unions"] == 0


# ---- contacts across tile faces, edges and corners ---------------------------------------------------------------------------------
@pytest.mark.parametrize("other,joined", [((64, 7, 7), True), ((63, 8, 7), True), ((63, 7, 8), True), ((64, 8, 7), False), ((64, 8, 8), False)],
                         ids=["x_face", "y_face", "z_face", "tile_edge", "tile_corner"])
def test_contacts_across_tile_borders(env, other, joined):
    pkg, torch = env
    origin, dims = (0, 0, 0), (130, 17, 17)
    words = cells_pool([(63, 7, 7), other], 8)
    want = component_labels_words(words, 8, origin, dims, 0, True, field=distance_field_separable(words, 8, origin, dims, 0))
    a, b = (7 * 17 + 7) * 130 + 63, (other[2] * 17 + other[1]) * 130 + other[0]
    assert want[7, 7, 63] == a and want[other[2], other[1], other[0]] == (a if joined else b) and (want >= 0).sum() == 2
    ws, pool = on_device(pkg, words)
    _, _, stats = expect(pkg, ws, pool, 8, origin, dims, 0, True, want)
    assert stats["unions"] == (1 if joined else 0)
    free = component_labels_words(words, 8, origin, dims, 0, False, field=distance_field_separable(words, 8, origin, dims, 0))
    expect(pkg, ws, pool, 8, origin, dims, 0, False, free)            # everything else: one component through every tile
    assert component_stats(free)[0] == 1


# ---- sizes and offsets -------------------------------------------------------------------------------------------------------------
# ((nx, ny, nz), origin x: "lo" 0 | "in" 37 | "hi" N - nx, clearance, solid), y and z from (5, 52).  nx 1, 63, 64, 65, 130: the edges of
# a row word, a wavefront and a tile; ny, nz 1, 7, 8, 9, 17: one row, one less than, equal to, one more than and more than twice a
# tile's side.  nx up to 65 on the random pool at p = 0.31 (depth 7, N = 128); nx = 130 does not fit that lattice and runs on the
# draw of the same density at depth 8 (N = 256): three row words, two cells in the last, at every offset.
SHAPE_CASES = [
    ((1, 1, 1), "in", 0, True), ((1, 9, 17), "hi", 0, False), ((63, 7, 17), "in", 0, True), ((63, 17, 1), "lo", 1, False),
    ((64, 8, 8), "lo", 0, True), ((64, 17, 9), "hi", 0, False), ((64, 1, 7), "in", 1, True), ((65, 9, 8), "in", 0, True),
    ((65, 7, 17), "hi", 1, False), ((65, 17, 17), "lo", 0, False), ((130, 1, 1), "in", 0, True), ((130, 9, 7), "hi", 1, True),
    ((130, 8, 17), "lo", 0, False), ((130, 17, 9), "in", 0, True), ((1, 17, 8), "lo", 1, False), ((63, 8, 9), "hi", 0, False),
    ((130, 17, 17), "hi", 0, True), ((130, 7, 8), "in", 1, False),
]


def shape_region(shape, kind):
    """-> (depth, origin, dims)"""
    depth = WIDE_DEPTH if shape[0] > 1 << RANDOM_DEPTH else RANDOM_DEPTH
    return depth, ({"lo": 0, "in": 37, "hi": (1 << depth) - shape[0]}[kind], 5, 52), tuple(shape)


def test_the_shape_cases_cover_the_edges():
    assert {c[0][0] for c in SHAPE_CASES} == {1, 63, 64, 65, 130} and {v for c in SHAPE_CASES for v in c[0][1:]} == {1, 7, 8, 9, 17}
    assert {c[2:] for c in SHAPE_CASES} == {(0, False), (0, True), (1, False), (1, True)}
    for nx in (1, 63, 64, 65, 130):                                # every width at every offset but 1 x "lo"
        assert {c[1] for c in SHAPE_CASES if c[0][0] == nx} >= ({"lo", "in", "hi"} if nx > 1 else {"in", "hi"}), nx
    assert shape_region((130, 1, 1), "hi")[:2] == (8, (126, 5, 52)) and shape_region((65, 1, 1), "hi")[:2] == (7, (63, 5, 52))


@pytest.fixture(scope="module")
def wide_pool(env):
    pkg, torch = env
    return on_device(pkg, wide_random_pool()[0])


@pytest.mark.parametrize("case", SHAPE_CASES, ids=lambda c: "%dx%dx%d-%s-r%d-%s" % (*c[0], c[1], c[2], "solid" if c[3] else "free"))
def test_sizes_and_offsets(env, random_pools, wide_pool, case):
    pkg, torch = env
    shape, kind, clearance, solid = case
    depth, origin, dims = shape_region(shape, kind)
    words = (wide_random_pool() if depth == WIDE_DEPTH else random_pool(0.31))[0]
    want = component_labels_words(words, depth, origin, dims, clearance, solid, field=distance_field_separable(words, depth, origin, dims, clearance))
    if shape == (130, 17, 17):                                      # dense occupancy across the x face at 127 | 128 and in the 2-bit tail
        assert tile_facts(want)[1] >= 50 and (want[:, :, 127] >= 0).any() and (want[:, :, 128:] >= 0).any()
    pool, ws = random_pools(0.31) if depth == RANDOM_DEPTH else wide_pool[::-1]
    expect(pkg, ws, pool, depth, origin, dims, clearance, solid, want)


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
    assert max(origin) >= 1 << 15 and (field == -1).sum() > 100 and (field != -1).sum() > 5
    for solid in (False, True):
        expect(pkg, ws, pool, 16, origin, dims, 2, solid, component_labels_words(words, 16, origin, dims, 2, solid, field=field))


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    ws, pool = on_device(pkg, hp.words())
    # (1,1,0) and (0,0,1) are occupied and do not touch by a face; the six free cells are one ring; at clearance 1 all is solid
    for clearance, solid, want in ((0, False, [[[0, 0], [0, -1]], [[-1, 0], [0, 0]]]), (0, True, [[[-1, -1], [-1, 3]], [[4, -1], [-1, -1]]]),
                                   (1, False, [[[-1, -1], [-1, -1]], [[-1, -1], [-1, -1]]]), (1, True, [[[0, 0], [0, 0]], [[0, 0], [0, 0]]])):
        want = np.array(want, np.int32)
        expect(pkg, ws, pool, 1, (0, 0, 0), (2, 2, 2), clearance, solid, want)
        same_field(want, component_labels_words(hp.words(), 1, (0, 0, 0), (2, 2, 2), clearance, solid))


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 17, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    unsynced = pkg.label_components(ws, pool, depth, origin, dims, 1, solid=True, as_tensor=True)        # no stats: nothing blocks
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    unsynced = unsynced.cpu().numpy()
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want = component_labels_words(words, depth, origin, dims, 1, True, field=distance_field_separable(words, depth, origin, dims, 1))
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 100
    same_field(unsynced, want)
    expect(pkg, ws, pool, depth, origin, dims, 1, True, want)


def test_a_deferred_commit_is_read_in_its_old_state(env):
    """between svoslam_svo_fuse_commit_deferred and svoslam_svo_fuse_apply the labels are those of the words the pool held before
    the commit -- the field's launches and the pack, tile, merge and size launches behind it -- and after the apply those of the
    new words; on the workspace that holds the deferred commit"""
    pkg, torch = env
    depth, n = 6, 15000
    rng = np.random.default_rng(53)
    ws, pool = pkg.Workspace(), pkg.Pool()
    pts, col = surface_cloud(rng, n)
    pkg.svo_from_point_cloud_async(ws, torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda(), depth, pool, CENTER, EDGE)
    old = pool.words().copy()
    more, more_col = surface_cloud(rng, n)
    more = (more * np.float32(0.8) + np.float32(0.07)).astype(np.float32)   # the same shapes, smaller and moved: new cells
    tp, tc = torch.from_numpy(more).cuda(), torch.from_numpy(more_col).cuda()
    pkg.svo_fuse_sort(ws, tp, depth, CENTER, EDGE)
    pkg.svo_fuse_plan(ws, n, depth, pool)
    pkg.svo_fuse_commit_deferred(ws, tc, depth, pool)
    origin, dims = (0, 0, 8), (64, 64, 48)
    before = {}
    for solid in (False, True):
        before[solid] = component_labels_words(old, depth, origin, dims, 1, solid, field=distance_field_separable(old, depth, origin, dims, 1))
        expect(pkg, ws, pool, depth, origin, dims, 1, solid, before[solid])
    pkg.svo_fuse_apply(ws, pool)
    new = pool.words()
    for solid in (False, True):
        want = component_labels_words(new, depth, origin, dims, 1, solid, field=distance_field_separable(new, depth, origin, dims, 1))
        assert ((want >= 0) != (before[solid] >= 0)).sum() > 1000   # the commit changed the set in this region
        expect(pkg, ws, pool, depth, origin, dims, 1, solid, want)


def test_workspace_slots_are_reused_and_two_calls_agree(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused
    ws = pkg.Workspace()
    assert ws.component_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    want = component_labels_words(words, 6, *large, 1, False, field=distance_field_separable(words, 6, *large, 1))
    assert (want >= 0).sum() > 1000 and (want < 0).sum() > 1000
    first = expect(pkg, ws, pool, 6, *large, 1, False, want)
    slots, field_slots = ws.component_buffers(), ws.field_buffers()
    assert all(p != 0 and b > 0 for p, b in slots + field_slots) and slots[1][1] >= 32
    again = expect(pkg, ws, pool, 6, *large, 1, False, want)
    assert ws.component_buffers() == slots and ws.field_buffers() == field_slots   # a second call of the same size allocates nothing
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert (first[2]["components"], first[2]["largest"]) == (again[2]["components"], again[2]["largest"])
    for solid in (False, True):                                    # a smaller call in the larger call's slots
        expect(pkg, ws, pool, 6, *small, 1, solid, component_labels_words(words, 6, *small, 1, solid, field=distance_field_separable(words, 6, *small, 1)))
    assert ws.component_buffers() == slots and ws.field_buffers() == field_slots and ws.reach_buffers() == [(0, 0)] * 2
    ws.close()                                                     # release_all releases the new slots with the rest


def test_without_stats_the_call_is_asynchronous_and_equal(env, random_pools):
    pkg, torch = env
    origin, dims, want = random_expected(0.31, "A", 0, True)
    pool, ws = random_pools(0.31)
    labels, sizes = pkg.label_components(ws, pool, RANDOM_DEPTH, origin, dims, 0, solid=True, sizes=True, as_tensor=True)   # stats=None
    only = pkg.label_components(ws, pool, RANDOM_DEPTH, origin, dims, 0, solid=True, as_tensor=True)
    for t in (labels, sizes, only):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (dims[2], dims[1], dims[0])
    torch.cuda.synchronize()
    same_field(labels.cpu().numpy(), want)
    same_field(only.cpu().numpy(), want)
    same_field(sizes.cpu().numpy(), component_sizes(want))
    stats = {}
    blocking = pkg.label_components(ws, pool, RANDOM_DEPTH, origin, dims, 0, solid=True, stats=stats)            # no sizes: largest is 0
    same_field(blocking, want)
    assert stats["components"] == component_stats(want)[0] and stats["largest"] == 0


def test_the_field_and_the_reach_field_are_unchanged_by_component_calls_on_their_workspace(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    for case in [c for c in FIELD_FUSED_CASES if c[0] == 6][:3]:
        depth, d, shape, ox, radius = case
        origin, dims = case_region(words, d, shape, ox, radius)
        seeds = [origin, [origin[a] + dims[a] // 2 for a in range(3)]]
        before = pkg.distance_field(ws, pool, d, origin, dims, radius)
        steps = pkg.reach_field(ws, pool, d, origin, dims, 1, seeds)
        for solid in (False, True):
            expect(pkg, ws, pool, d, origin, dims, 1, solid,
                   component_labels_words(words, d, origin, dims, 1, solid, field=distance_field_separable(words, d, origin, dims, 1)))
        pkg.label_components(ws, pool, d, [0, 0, 0], [min(1 << d, 70), 9, 9], 3, sizes=True)
        same_field(pkg.distance_field(ws, pool, d, origin, dims, radius), before)
        same_field(before, distance_field_separable(words, d, origin, dims, radius))
        same_field(pkg.reach_field(ws, pool, d, origin, dims, 1, seeds), steps)
        same_field(steps, reach_field_words(words, d, origin, dims, 1, seeds, field=distance_field_separable(words, d, origin, dims, 1)))


def test_box_to_cells_then_the_map_components_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    want = component_labels_words(words, 6, lo.tolist(), dims.tolist(), 0, True, field=distance_field_separable(words, 6, lo.tolist(), dims.tolist(), 0))
    sizes = component_sizes(want)
    components, largest = component_stats(want)
    assert components >= 1 and (want < 0).sum() > 100
    ckpt, out = tmp_path / "map.svopool", tmp_path / "components.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_components.py"), str(ckpt), str(out), "--clearance", "0", "--solid", "--min-size",
           str(largest), "--box"] + [repr(float(v)) for v in box]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_field(z["labels"], want)
    same_field(z["sizes"], sizes)
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    assert int(z["components"]) == components and int(z["largest"]) == largest and int(z["clearance_cells"]) == 0 and bool(z["solid"])
    assert float(z["cell_size"]) == 2.0 * EDGE / 64 and z["keep"].dtype == np.bool_ and np.array_equal(z["keep"], sizes >= largest)
    assert "%d components in %d cells, the largest %d cells" % (components, int((want >= 0).sum()), largest) in r.stdout


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        stats = {}
        labels, sizes = pkg.label_components(ws, pool, 5, (1, 2, 3), dims, 4, sizes=True, stats=stats)
        assert labels.shape == sizes.shape == (dims[2], dims[1], dims[0]) and labels.dtype == sizes.dtype == np.int32
        assert stats == {"components": 0, "largest": 0, "tile_passes": 0, "unions": 0}
    assert ws.component_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3   # nothing was launched, nothing allocated
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    size_buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    null, ptr, sp = C.c_void_p(0), pkg._ptr(buf), pkg._ptr(size_buf)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def call(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, which=0, out=ptr, sizes=sp, stats=None):
        return L.svoslam_pool_label_components(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, which, out, sizes, stats, pkg._stream())
    st = pkg._ComponentStats()
    assert call() == 0 and call(stats=C.byref(st)) == 0 and (st.components, st.largest) == (1, 16)   # an empty pool: all free
    assert call(which=1, stats=C.byref(st)) == 0 and (st.components, st.largest, st.unions) == (0, 0, 0)
    assert call(sizes=null) == 0 and call(sizes=null, stats=C.byref(st)) == 0 and (st.components, st.largest) == (1, 0)
    assert call(dims=(0, 2, 2)) == 0 and call(pool_ref=None, dims=(4, 0, 2)) == 0
    assert call(dims=(4, 2, 0), out=null) == 0 and call(pool_ref=None, dims=(0, 0, 0), out=null, sizes=null) == 0
    assert call(which=2) == -1 and call(which=-1) == -1 and call(which=2, dims=(0, 2, 2)) == -1
    assert call(ws_ref=None) == -1 and call(origin=None) == -1 and call(dims=None) == -1
    assert call(ws_ref=None, dims=(0, 2, 2)) == -1 and call(depth=0, dims=(0, 2, 2)) == -1
    assert call(depth=0) == -1 and call(depth=17) == -1
    assert call(dims=(-1, 2, 2)) == -1 and call(dims=(4, 2, -1)) == -1 and call(dims=(0, -1, 2)) == -1
    for a in range(3):                                             # one cell outside the root on each side
        origin, dims = [1, 2, 3], [4, 2, 2]
        origin[a] = -1
        assert call(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert call(origin=origin) == -1
        origin[a] = 32 - dims[a]
        assert call(origin=origin) == 0
        origin[a], dims[a] = 0, 33
        assert call(origin=origin, dims=dims) == -1
    assert call(radius=0) == 0 and call(radius=64) == 0
    assert call(radius=-1) == -1 and call(radius=4097) == -1 and call(radius=4097, dims=(0, 2, 2)) == -1
    assert call(pool_ref=None) == -1 and call(out=null) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert call(pool_ref=C.byref(blank)) == -1 and call(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # the limits: refused before anything is allocated or written
    slots, field_slots = ws.component_buffers(), ws.field_buffers()
    assert call(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert call(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), radius=4096) == -6
    assert call(depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), radius=0) == -6       # 2^25 tiles, by the dims alone
    assert b"tiles" in L.svoslam_last_error()
    huge = dict(depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), radius=0)                     # argument errors come before the limits
    assert call(pool_ref=None, **huge) == -1 and call(out=null, **huge) == -1 and call(pool_ref=C.byref(pkg._PoolStruct(None, 0, 0, None, 0, 0)), **huge) == -1
    assert ws.component_buffers() == slots and ws.field_buffers() == field_slots
    fresh = pkg.Workspace()
    assert call(ws_ref=fresh._h, depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), radius=0) == -6
    assert fresh.component_buffers() == [(0, 0)] * 2 and fresh.field_buffers() == [(0, 0)] * 3
    with pytest.raises(Exception):
        pkg.label_components(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097)
    with pytest.raises(Exception):
        pkg.label_components(ws, pool, 5, (30, 0, 0), (4, 4, 4), 3)
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.label_components(ws, pool, 6, (0, 0, 0), (64, 20, 3), 1, sizes=True, stats={})
        pkg.label_components(ws, pool, 4, (1, 2, 3), (9, 3, 3), 0, solid=True)
        torch.cuda.synchronize()
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0                              # the field's launches are inside the call's one bracket
        pkg.label_components(ws, pool, 6, (0, 0, 0), (64, 0, 3), 1)   # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            pkg.label_components(ws, pool, 6, (0, 0, 0), (65, 2, 3), 1)   # refused: not bracketed either
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])
