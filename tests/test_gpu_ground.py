"""svoslam_pool_ground_field and svoslam_field_trace_ground_paths on the device: every value equals the host restatements of the
specification (tests/test_ground_cpu.py: ground_field_words, the foothold set by its definition and Dijkstra's algorithm, and
trace_ground_path, the rule cell by cell) applied to the pool's own words -- never a second device result alone.

The worlds: the hand-built pools with every cell as a trace start; ground_routes, where the step, the climb cost, the radius and
the headroom each choose another route; corner_stairs, staircases whose risers meet the corners of the 64 x 8 x 8 tile
(map_ground.hip) at one of eight offsets; a seeded terrain at every edge of a row word and of the tile; a serpentine of kerbs whose
cheapest path comes back into a tile it has left."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_field import same_field
from test_gpu_query import fused_pool
from test_ground_cpu import (CORNER_STAIRS, GROUND_CASES, GROUND_ROUTES_ROWS, PLATEAU, PLATEAU_TRACES, REFUSED_ROW, WORLD_DEPTH, cells_pool,
                             check_ground_path, corner_stairs, corner_stairs_costs, footholds_words, ground_field_words, ground_routes,
                             ground_seeds, snapped, trace_ground_path)
from test_plan_cpu import tile_visits
from test_surface_cpu import CENTER, EDGE, HandPool, occupied_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = np.int64


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


def ground(pkg, ws, pool, depth, origin, dims, up, r, H, S, c, seeds, snap=0, **kw):
    stats = {}
    got = pkg.ground_field(ws, pool, depth, origin, dims, up, r, H, S, c, seeds, snap_cells=snap, stats=stats, **kw)
    return got, stats


def pool_of(pkg, words):
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    return ws, pool


def same_paths(pkg, field, origin, dims, up, S, c, starts, max_cells, snap=0, fill=-1):
    """the device's paths and lengths of `starts` equal trace_ground_path's, and nothing behind a path's cells was written"""
    paths, lengths = pkg.trace_ground_paths(field, origin, dims, up, S, c, starts, max_cells, snap_cells=snap)
    assert paths.dtype == np.int32 and lengths.dtype == np.int32 and paths.shape == (len(starts), max_cells, 3) and lengths.shape == (len(starts),)
    for k, start in enumerate(starts):
        cells, length = trace_ground_path(field, origin, up, S, c, start, max_cells, snap)
        assert int(lengths[k]) == length, (k, start, int(lengths[k]), length)
        assert np.array_equal(paths[k, :cells.shape[0]], cells), (k, start)
        assert (paths[k, cells.shape[0]:] == fill).all(), (k, start)
    return paths, lengths


def every_cell(origin, dims):
    return [(origin[0] + x, origin[1] + y, origin[2] + z) for z in range(dims[2]) for y in range(dims[1]) for x in range(dims[0])]


# ---- hand-built pools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GROUND_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    k = GROUND_CASES[name]
    ws, pool = pool_of(pkg, k["words"])
    args = (k["depth"], k["origin"], k["dims"], k["up"], k["r"], k["H"], k["S"], k["c"], k["seeds"], k["snap"])
    got, stats = ground(pkg, ws, pool, *args)
    same_field(got, k["want"])
    same_field(got, ground_field_words(k["words"], *args)[0])
    assert stats["footholds"] == k["footholds"] and stats["seeds_used"] == k["seeds_used"]
    assert stats["rounds"] >= 1 and stats["tile_runs"] >= (1 if k["seeds_used"] else 0)
    cap = k["dims"][0] * k["dims"][1] * k["dims"][2]
    for snap in (0, 2):
        same_paths(pkg, got, k["origin"], k["dims"], k["up"], k["S"], k["c"], every_cell(k["origin"], k["dims"]), cap, snap=snap)


def test_depth_one_and_depth_sixteen(env):
    pkg, torch = env
    words = cells_pool([(0, 0, 0), (1, 0, 1)], 1)
    ws, pool = pool_of(pkg, words)
    for up in (2, 3, 4, 5):
        got, stats = ground(pkg, ws, pool, 1, (0, 0, 0), (2, 2, 2), up, 0, 1, 0, 0, every_cell((0, 0, 0), (2, 2, 2)))
        want, facts = ground_field_words(words, 1, (0, 0, 0), (2, 2, 2), up, 0, 1, 0, 0, every_cell((0, 0, 0), (2, 2, 2)))
        same_field(got, want)
        assert stats["footholds"] == facts["footholds"] and stats["seeds_used"] == facts["seeds_used"]
    assert (ground(pkg, ws, pool, 1, (0, 0, 0), (2, 2, 2), 2, 0, 1, 0, 0, [(0, 1, 0)])[0] == 0).sum() == 1
    # beyond 2^15: a floor strip with a riser of 1, a post and a beam about cell 40000
    b = 40000
    cells = [(b + x, b, b + z) for z in range(3) for x in range(70)] + [(b + x, b + 1, b + 1) for x in range(30, 70)] + [(b + 10, b + 3, b + 1)]
    cells += [(b + 50, b + 2, b + 2), (b + 50, b + 3, b + 2)]
    words = cells_pool(cells, 16)
    ws, pool = pool_of(pkg, words)
    origin, dims = (b - 3, b - 1, b + 1), (80, 6, 1)
    for r, H, S, c in ((0, 2, 1, 4), (1, 3, 1, 0)):
        seeds = [(b, b + 1, b + 1), (b + 69, b + 4, b + 1), (65535, 65535, 65535)]
        got, stats = ground(pkg, ws, pool, 16, origin, dims, 2, r, H, S, c, seeds, snap=3)
        want, facts = ground_field_words(words, 16, origin, dims, 2, r, H, S, c, seeds, snap=3, G=footholds_words(words, 16, origin, dims, 2, r, H, S, cells=cells))
        same_field(got, want)
        assert stats["footholds"] == facts["footholds"] > 50 and stats["seeds_used"] == 2 and (want == -1).sum() + (want > 30).sum() > 0
        same_paths(pkg, got, origin, dims, 2, S, c, [(b + 35, b + 5, b + 1), (b + 5, b + 1, b + 1), (b + 10, b + 2, b + 1)], 90, snap=4)


# ---- ground routes -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def routes(env):
    pkg, torch = env
    w = ground_routes()
    return (w,) + pool_of(pkg, w["words"])


@pytest.mark.parametrize("row", sorted(GROUND_ROUTES_ROWS))
def test_ground_routes(env, routes, row):
    pkg, torch = env
    w, ws, pool = routes
    r, H, S, c = row
    footholds, reached, cut, value, length = GROUND_ROUTES_ROWS[row]
    want = w["fields"][row]
    at = w["start"]
    # on the restatement first
    assert ((want != -2).sum(), (want >= 0).sum(), (want == -1).sum(), want[at[2], at[1], at[0]]) == (footholds, reached, cut, value)
    if row == REFUSED_ROW:                                              # S > H - 1: the call's limits
        with pytest.raises(pkg.SvoslamError):
            ground(pkg, ws, pool, WORLD_DEPTH, w["origin"], w["dims"], w["up"], r, H, S, c, [w["seed"]])
        same_paths(pkg, want, w["origin"], w["dims"], w["up"], S, c, [at], 120)   # the trace takes any field
        return
    got, stats = ground(pkg, ws, pool, WORLD_DEPTH, w["origin"], w["dims"], w["up"], r, H, S, c, [w["seed"]])
    same_field(got, want)
    assert stats["footholds"] == footholds and stats["seeds_used"] == 1
    paths, lengths = same_paths(pkg, got, w["origin"], w["dims"], w["up"], S, c, [at, (at[0], at[1] + 2, at[2])], 160, snap=2)
    assert lengths.tolist() == [length, length]
    if length:
        assert np.array_equal(paths[0, :length], check_ground_path(want, w["origin"], w["up"], S, c, at)[0])


def test_flat_layer_is_the_reach_field(env, routes):
    """S = 0, c = 0, H = 1, r = 0 on the floor's foothold layer: the device's own reach field of that layer at clearance 0"""
    pkg, torch = env
    w, ws, pool = routes
    origin, dims = (0, 4, 0), (128, 1, 40)
    got, stats = ground(pkg, ws, pool, WORLD_DEPTH, origin, dims, 2, 0, 1, 0, 0, [w["seed"]])
    same_field(got, ground_field_words(w["words"], WORLD_DEPTH, origin, dims, 2, 0, 1, 0, 0, [w["seed"]])[0])
    assert (got > 0).sum() == 2283 and (got == -2).sum() == 5120 - 2284      # test_ground_cpu's hand count; the rest stands on cells
    same_field(got, pkg.reach_field(ws, pool, WORLD_DEPTH, origin, dims, 0, [w["seed"]]))


# ---- corner stairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", range(8))
def test_corner_stairs(env, offset):
    pkg, torch = env
    words, seed, top_x, top_z = corner_stairs(offset)
    ws, pool = pool_of(pkg, words)
    k = CORNER_STAIRS
    G = footholds_words(words, WORLD_DEPTH, k["origin"], k["dims"], 2, 0, k["H"], k["S"])
    for c in (0, 3):
        want, facts = ground_field_words(words, WORLD_DEPTH, k["origin"], k["dims"], 2, 0, k["H"], k["S"], c, [seed], G=G)
        assert (want[top_x[2], top_x[1], top_x[0]], want[top_z[2], top_z[1], top_z[0]]) == corner_stairs_costs(c)
        got, stats = ground(pkg, ws, pool, WORLD_DEPTH, k["origin"], k["dims"], 2, 0, k["H"], k["S"], c, [seed])
        same_field(got, want)
        assert stats["footholds"] == facts["footholds"] and stats["rounds"] > 10
        same_paths(pkg, got, k["origin"], k["dims"], 2, k["S"], c, [top_x, top_z], 260)


def test_corner_stairs_minus_z(env):
    pkg, torch = env
    words, seed, top_x, top_z = corner_stairs(3, up=5)
    ws, pool = pool_of(pkg, words)
    k = CORNER_STAIRS
    want, facts = ground_field_words(words, WORLD_DEPTH, k["origin"], k["dims"], 5, 0, k["H"], k["S"], 3, [seed])
    assert (want[top_x[2], top_x[1], top_x[0]], want[top_z[2], top_z[1], top_z[0]]) == corner_stairs_costs(3)
    got, stats = ground(pkg, ws, pool, WORLD_DEPTH, k["origin"], k["dims"], 5, 0, k["H"], k["S"], 3, [seed])
    same_field(got, want)
    same_paths(pkg, got, k["origin"], k["dims"], 5, k["S"], 3, [top_x, top_z], 260)


# ---- terrain ---------------------------------------------------------------------------------------------------------------------
def terrain_cells(up):
    """a seeded integer height walk over x 0 .. 127 and 24 cells of width: steps of -2 .. 2 per cell along x, level more often than
    not, and now and then a step of 1 across; solid from the bottom; a few slabs 3 and 4 above the ground and posts 6 tall on it.
    Generic cells (x, w, t) are mapped by `up`."""
    rng = np.random.default_rng(77)
    h = np.zeros((128, 24), I64)
    h[0, 0] = 9
    for x in range(1, 128):
        h[x, 0] = np.clip(h[x - 1, 0] + rng.choice([-2, -1, 0, 0, 0, 0, 0, 0, 1, 2]), 3, 20)
    for w in range(1, 24):
        h[:, w] = np.clip(h[:, w - 1] + rng.integers(-1, 2, 128) * (rng.random(128) < 0.12), 3, 20)
    cells = [(x, w, t) for x in range(128) for w in range(24) for t in range(int(h[x, w]) + 1)]
    for x0, w0, lift in ((20, 2, 3), (60, 8, 4), (100, 5, 3), (40, 14, 4)):
        cells += [(x, w, int(h[x, w]) + lift + 1) for x in range(x0, x0 + 9) for w in range(w0, w0 + 4)]
    for x, w in ((10, 6), (33, 9), (64, 7), (65, 12), (90, 4), (120, 10), (50, 16)):
        cells += [(x, w, int(h[x, w]) + k) for k in range(1, 7)]
    return [generic(p, up) for p in cells]


def generic(p, up):
    """(x, w, t) -> (x, y, z) for `up`"""
    x, w, t = p
    t = 127 - t if up & 1 else t
    return (x, t, w) if up >> 1 == 1 else (x, w, t)


def generic_box(x0, nx, w0, nw, t0, nt, up):
    """the region x0 .. x0 + nx, w0 .. w0 + nw, t0 .. t0 + nt in generic cells -> (origin, dims)"""
    t_lo = 127 - (t0 + nt - 1) if up & 1 else t0
    return ((x0, t_lo, w0), (nx, nt, nw)) if up >> 1 == 1 else ((x0, w0, t_lo), (nx, nw, nt))


# (nx, origin x, width, up extent, first layer, up, (r, H, S, c), seeds).  nx 63, 64, 65 and 128 (130 does not fit the 128 cells of a
# depth-7 root and is cut to them): the edges of a row word
# and a tile; width 7, 8, 9, 17 and up extent 8, 9, 24: one less than, equal to, one more than and more than twice the tile's side.
# nx 1, width 1 and up extent 5 hold fewer than 50 footholds above cost 0 on this terrain, whatever the rest: they are not listed,
# and test_thin_regions runs them without that demand.  The last three pair S = 4 with widths and up extents of 8 and 9 for y-up: the
# halo of four layers then crosses the tile's top and its side at once.
TERRAIN_CASES = [
    (63, 0, 17, 24, 0, 2, (1, 4, 2, 5), 1), (64, 37, 9, 24, 2, 3, (3, 6, 4, 1), 7), (65, 63, 8, 9, 6, 4, (0, 1, 0, 0), 7),
    (128, 0, 7, 24, 1, 5, (1, 4, 2, 5), 1), (128, 0, 17, 8, 7, 2, (0, 1, 0, 0), 7), (65, 37, 17, 24, 0, 4, (3, 6, 4, 1), 1),
    (64, 64, 9, 9, 5, 2, (1, 4, 2, 5), 7), (63, 65, 8, 24, 3, 5, (0, 1, 0, 0), 7), (128, 0, 9, 8, 6, 3, (1, 4, 2, 5), 7),
    (64, 37, 8, 9, 5, 2, (3, 6, 4, 1), 7), (65, 0, 9, 8, 6, 3, (3, 6, 4, 1), 7), (128, 0, 9, 9, 6, 2, (3, 6, 4, 1), 1),
]
_TERRAIN = {}


def terrain_world(up):
    """-> (words, cells) of the terrain for `up`, built once"""
    if up not in _TERRAIN:
        cells = terrain_cells(up)
        _TERRAIN[up] = (cells_pool(cells, WORLD_DEPTH), cells)
    return _TERRAIN[up]


def terrain(case):
    """-> (words, origin, dims, seeds, the definition's field and facts), computed once"""
    if case not in _TERRAIN:
        nx, x0, nw, nt, t0, up, (r, H, S, c), count = case
        words, cells = terrain_world(up)
        origin, dims = generic_box(x0, nx, 3, nw, t0, nt, up)
        G = footholds_words(words, WORLD_DEPTH, origin, dims, up, r, H, S, cells=cells)
        seeds = ground_seeds(G, origin, dims, WORLD_DEPTH, count, np.random.default_rng(TERRAIN_CASES.index(case)))
        _TERRAIN[case] = (words, origin, dims, seeds) + ground_field_words(words, WORLD_DEPTH, origin, dims, up, r, H, S, c, seeds, snap=2, G=G)
    return _TERRAIN[case]


@pytest.fixture(scope="module")
def terrain_pools(env):
    pkg, torch = env
    pools = {}

    def get(up):
        if up not in pools:
            pools[up] = pool_of(pkg, terrain_world(up)[0])
        return pools[up]
    return get


@pytest.mark.parametrize("case", TERRAIN_CASES, ids=lambda k: "nx%d-x%d-w%d-t%d+%d-up%d-r%dH%dS%dc%d-seeds%d" % (k[:6] + k[6] + k[7:]))
def test_terrain(env, terrain_pools, case):
    pkg, torch = env
    up, (r, H, S, c) = case[5], case[6]
    words, origin, dims, seeds, want, facts = terrain(case)
    # on the restatement first
    assert (want >= 1).sum() >= 50 and (want == -1).sum() > 0 and (want == -2).sum() > 0, ((want >= 1).sum(), (want == -1).sum())
    ws, pool = terrain_pools(up)
    got, stats = ground(pkg, ws, pool, WORLD_DEPTH, origin, dims, up, r, H, S, c, seeds, snap=2)
    same_field(got, want)
    assert stats["footholds"] == facts["footholds"] and stats["seeds_used"] == facts["seeds_used"] >= 1
    reached = np.argwhere(want >= 0)[:, ::-1] + np.asarray(origin)
    starts = reached[np.random.default_rng(3).choice(reached.shape[0], min(9, reached.shape[0]), replace=False)].tolist()
    starts.append((np.array(np.unravel_index(np.argmax(want), want.shape)[::-1]) + np.asarray(origin)).tolist())
    same_paths(pkg, got, origin, dims, up, S, c, starts, int(want.max()) + 1)


def test_the_terrain_cases_cover_the_edges():
    cases = TERRAIN_CASES
    assert {k[0] for k in cases} == {63, 64, 65, 128} and {k[1] for k in cases} >= {0, 37, 64, 65, 63}
    assert {k[2] for k in cases} == {7, 8, 9, 17} and {k[3] for k in cases} == {8, 9, 24} and {k[5] for k in cases} == {2, 3, 4, 5}
    assert {k[6] for k in cases} == {(0, 1, 0, 0), (1, 4, 2, 5), (3, 6, 4, 1)} and {k[7] for k in cases} == {1, 7}
    assert any(k[0] + k[1] == 128 for k in cases)                       # origin x = N - nx


@pytest.mark.parametrize("shape", [(1, 17, 24), (130, 1, 24), (65, 9, 5), (1, 1, 24)])
def test_thin_regions(env, terrain_pools, shape):
    """one cell along x, one cell across, five layers: the sizes that hold too few footholds for test_terrain's demand"""
    pkg, torch = env
    for up, params in ((2, (1, 4, 2, 5)), (5, (0, 1, 0, 0))):
        words, cells = terrain_world(up)
        ws, pool = terrain_pools(up)
        r, H, S, c = params
        origin, dims = generic_box(60 if shape[0] == 1 else 0, min(shape[0], 128), 9, shape[1], 4, shape[2], up)
        G = footholds_words(words, WORLD_DEPTH, origin, dims, up, r, H, S, cells=cells)
        seeds = ground_seeds(G, origin, dims, WORLD_DEPTH, 1, np.random.default_rng(5))
        want, facts = ground_field_words(words, WORLD_DEPTH, origin, dims, up, r, H, S, c, seeds, G=G)
        got, stats = ground(pkg, ws, pool, WORLD_DEPTH, origin, dims, up, r, H, S, c, seeds)
        same_field(got, want)
        assert stats["footholds"] == facts["footholds"] and stats["seeds_used"] == facts["seeds_used"]
        same_paths(pkg, got, origin, dims, up, S, c, every_cell(origin, dims)[::7][:60], 40)


# ---- a serpentine of kerbs -------------------------------------------------------------------------------------------------------
def kerb_maze(pitch=6, walls=6, gap=6, nw=47):
    """a floor at y = 3 over x 0 .. 127, z 0 .. nw; kerbs 2 high (S = 1 does not climb them) along x at z = k * pitch + pitch - 1, with
    a gap at the high end of x for even k and at the low end for odd k; the last kerb has none.  The seed stands in corridor 0."""
    cells = [(x, 3, z) for z in range(nw) for x in range(128)]
    for k in range(walls + 1):
        xs = range(128) if k == walls else range(0, 128 - gap) if k % 2 == 0 else range(gap, 128)
        cells += [(x, y, k * pitch + pitch - 1) for x in xs for y in (4, 5)]
    return cells_pool(cells, WORLD_DEPTH), (0, 0, 0), (128, 10, nw), (0, 4, (pitch - 2) // 2), walls


def test_kerb_serpentine(env):
    pkg, torch = env
    words, origin, dims, seed, walls = kerb_maze()
    want, facts = ground_field_words(words, WORLD_DEPTH, origin, dims, 2, 0, 3, 1, 2, [seed])
    # on the restatement first: the far corridor is reached round every kerb, the last corridor is cut off
    assert want.max() > 7 * 110 and (want == -1).sum() > 500 and (want == -2).sum() > 1000
    far = np.array(np.unravel_index(np.argmax(want), want.shape)[::-1]) + np.asarray(origin)
    path, climbed = check_ground_path(want, origin, 2, 1, 2, far)
    assert climbed == 0 and tile_visits(path, origin) >= 2
    ws, pool = pool_of(pkg, words)
    got, stats = ground(pkg, ws, pool, WORLD_DEPTH, origin, dims, 2, 0, 3, 1, 2, [seed])
    same_field(got, want)
    assert stats["seeds_used"] == 1 and stats["rounds"] > walls
    paths, lengths = same_paths(pkg, got, origin, dims, 2, 1, 2, [far.tolist()], path.shape[0] + 3)
    assert int(lengths[0]) == path.shape[0] and np.array_equal(paths[0, :path.shape[0]], path)


# ---- fused pools: the foothold set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth, d, origin_of, dims, up, params", [
    (6, 6, "cloud", (64, 30, 30), 2, (1, 4, 2, 5)), (6, 6, "cloud", (33, 17, 9), 5, (3, 6, 4, 1)), (6, 4, "low", (16, 16, 16), 3, (0, 1, 0, 0)),
    (9, 9, "cloud", (130, 40, 17), 4, (1, 4, 2, 5)), (9, 9, "cloud", (65, 24, 65), 2, (3, 6, 4, 1)), (9, 7, "cloud", (128, 9, 30), 3, (0, 3, 1, 0)),
])
def test_fused_footholds(env, fused, depth, d, origin_of, dims, up, params):
    pkg, torch = env
    pool, words, pts, ws = fused[depth]
    n_side = 1 << d
    cells = occupied_cells(words, d)[0]
    anchor = cells[cells.shape[0] // 2]
    origin = [0, 0, 0] if origin_of == "low" else [int(np.clip(anchor[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
    r, H, S, c = params
    G = footholds_words(words, d, origin, dims, up, r, H, S, cells=cells)
    seeds = ground_seeds(G, origin, dims, d, 7, np.random.default_rng(depth + d))
    want, facts = ground_field_words(words, d, origin, dims, up, r, H, S, c, seeds, snap=1, G=G)
    got, stats = ground(pkg, ws, pool, d, origin, dims, up, r, H, S, c, seeds, snap=1)
    assert np.array_equal(got != -2, G) and stats["footholds"] == int(G.sum()) == facts["footholds"]
    same_field(got, want)
    assert stats["seeds_used"] == facts["seeds_used"]


def test_the_fused_cases_hold_footholds(fused):
    """on the restatement: the cloud's surfaces give footholds for every up"""
    words = fused[6][1]
    for up in (2, 3, 4, 5):
        assert footholds_words(words, 6, (0, 0, 0), (64, 64, 64), up, 0, 3, 1).sum() > 30


# ---- the trace -------------------------------------------------------------------------------------------------------------------
def test_trace_plateau_sentinel_and_many_starts(env, routes):
    pkg, torch = env
    # an array that is not a ground field: minus the cells walked
    for (start, snap), (cells, length) in PLATEAU_TRACES.items():
        paths, lengths = same_paths(pkg, PLATEAU, (0, 0, 0), (4, 3, 1), 2, 1, 2, [start], 8, snap=snap)
        assert int(lengths[0]) == length and [tuple(q) for q in paths[0, :len(cells)].tolist()] == cells
    same_paths(pkg, PLATEAU, (-5, 100000, 7), (4, 3, 1), 2, 1, 2, [(s[0] - 5, s[1] + 100000, s[2] + 7) for s, _ in PLATEAU_TRACES], 8)
    w, ws, pool = routes
    row = (0, 4, 2, 20)
    field, origin, dims, S, c = w["fields"][row], w["origin"], w["dims"], row[2], row[3]
    reached = np.argwhere(field >= 0)[:, ::-1]
    starts = reached[np.random.default_rng(1).choice(reached.shape[0], 257, replace=False)].tolist()   # more than one workgroup
    paths, lengths = same_paths(pkg, field, origin, dims, 2, S, c, starts, int(field.max()) + 1)
    assert lengths.min() >= 1 and lengths.max() > 100
    same_paths(pkg, field, origin, dims, 2, S, c, starts[:1], 200)      # 1 start
    # max_cells shorter than the paths: the whole length, the first cells, and the rest of a sentinel-filled buffer untouched
    t_field, t_starts = torch.from_numpy(field).cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda")
    buf = torch.full((257, 7, 3), -77, dtype=torch.int32, device="cuda")
    out_len = torch.full((257,), -77, dtype=torch.int32, device="cuda")
    o3, n3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
    L = pkg.lib()
    assert L.svoslam_field_trace_ground_paths(pkg._ptr(t_field), o3, n3, 2, S, c, 0, pkg._ptr(t_starts), 257, 7, pkg._ptr(buf), pkg._ptr(out_len),
                                              pkg._stream()) == 0
    buf, out_len = buf.cpu().numpy(), out_len.cpu().numpy()
    assert np.array_equal(out_len, lengths) and (lengths > 7).sum() > 100
    for k in range(257):
        kept = min(int(lengths[k]), 7)
        assert np.array_equal(buf[k, :kept], paths[k, :kept]) and (buf[k, kept:] == -77).all()
    # max_cells 0 with a NULL path buffer: the lengths alone
    out_len = torch.full((257,), -77, dtype=torch.int32, device="cuda")
    assert L.svoslam_field_trace_ground_paths(pkg._ptr(t_field), o3, n3, 2, S, c, 0, pkg._ptr(t_starts), 257, 0, None, pkg._ptr(out_len),
                                              pkg._stream()) == 0
    assert np.array_equal(out_len.cpu().numpy(), lengths)
    # tensors in, tensors out
    paths, lengths = pkg.trace_ground_paths(t_field, origin, dims, "+y", S, c, t_starts[:2], 3, as_tensor=True)
    assert isinstance(paths, torch.Tensor) and paths.is_cuda and paths.dtype == torch.int32 and tuple(paths.shape) == (2, 3, 3)
    assert isinstance(lengths, torch.Tensor) and lengths.tolist() == out_len[:2].tolist()
    with pytest.raises(ValueError):
        pkg.trace_ground_paths(field, origin, (128, 16, 39), 2, S, c, starts, 3)


def test_trace_argument_errors(env):
    pkg, torch = env
    L = pkg.lib()
    field = torch.zeros(64, dtype=torch.int32, device="cuda")
    starts = torch.tensor([[0, 0, 0], [3, 3, 3]], dtype=torch.int32, device="cuda")
    paths = torch.full((2, 4, 3), -77, dtype=torch.int32, device="cuda")
    lengths = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    null = C.c_void_p(0)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def trace(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), up=2, S=1, c=0, snap=0, s=pkg._ptr(starts), n=2, cap=4, p=pkg._ptr(paths),
              out=pkg._ptr(lengths)):
        return L.svoslam_field_trace_ground_paths(f, i3(origin), i3(dims), up, S, c, snap, s, n, cap, p, out, pkg._stream())
    assert trace() == 0 and lengths.tolist() == [1, 1]                   # all zeros: every cell is a goal
    assert trace(n=0, s=null, out=null, p=null, f=null) == 0 and trace(cap=0, p=null) == 0
    for up in (3, 4, 5):
        assert trace(up=up) == 0
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):                       # a zero entry of dims: lengths 0
        lengths.fill_(-77)
        assert trace(dims=dims, f=null) == 0 and lengths.tolist() == [0, 0]
    assert trace(origin=None) == -1 and trace(dims=None) == -1
    assert trace(dims=(-1, 4, 4)) == -1 and trace(dims=(4, 4, -1)) == -1 and trace(n=-1) == -1 and trace(cap=-1) == -1
    assert trace(f=null) == -1 and trace(s=null) == -1 and trace(out=null) == -1 and trace(p=null) == -1
    assert trace(up=0) == -1 and trace(up=1) == -1 and trace(up=6) == -1 and trace(up=-1) == -1
    assert trace(S=-1) == -1 and trace(S=5) == -1 and trace(S=4) == 0 and trace(c=-1) == -1 and trace(c=65535) == -1 and trace(c=65534) == 0
    assert trace(snap=-1) == -1 and trace(snap=257) == -1 and trace(snap=256) == 0
    assert trace(dims=(65536, 65536, 1)) == -6 and trace(dims=(2048, 1024, 1024)) == -6
    assert trace(n=1 << 20, cap=1 << 10) == -6
    assert (paths[:, 1:] == -77).all()


# ---- conventions -----------------------------------------------------------------------------------------------------------------
def test_the_other_fields_are_unchanged_by_ground_calls_on_their_workspace(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (2, 0, 5), (62, 33, 11)
    seeds = [(3, 1, 6), (60, 30, 14)]

    def others():
        return (pkg.distance_field(ws, pool, 6, origin, dims, 3), pkg.reach_field(ws, pool, 6, origin, dims, 1, seeds),
                pkg.cost_field(ws, pool, 6, origin, dims, 1, 3, [4, 2], seeds), pkg.label_components(ws, pool, 6, origin, dims, 1))
    before = others()
    ground(pkg, ws, pool, 6, origin, dims, 2, 2, 4, 2, 3, seeds, snap=4)
    ground(pkg, ws, pool, 6, (0, 0, 0), (64, 9, 9), 5, 0, 1, 0, 0, [(1, 1, 1)])
    for a, b in zip(others(), before):
        same_field(a, b)


def test_workspace_slots_are_reused(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    ws = pkg.Workspace()
    assert ws.ground_buffers() == [(0, 0)] * 6
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    seeds = ground_seeds(footholds_words(words, 6, *large, 2, 2, 5, 2), *large, 6, 3, np.random.default_rng(2)) + np.array([0, 2, 0])
    first, _ = ground(pkg, ws, pool, 6, *large, 2, 2, 5, 2, 3, seeds, snap=60)
    slots = ws.ground_buffers()
    assert all(p != 0 and b > 0 for p, b in slots) and ws.field_buffers() == [(0, 0)] * 3 and ws.plan_buffers() == [(0, 0)] * 3
    assert slots[0][1] >= 64 * 40 * 8 and slots[4][1] >= 64 * 40 * 8 and slots[5][1] >= 32 + 8 * 5 * 8
    again, _ = ground(pkg, ws, pool, 6, *large, 2, 2, 5, 2, 3, seeds, snap=60)
    assert ws.ground_buffers() == slots                                  # a second call of the same size allocates nothing
    want = ground_field_words(words, 6, *large, 2, 2, 5, 2, 3, seeds, snap=60)[0]
    assert (want >= 0).sum() >= 1 and (want == -2).sum() > 1000
    same_field(first, want)
    same_field(again, want)
    got, _ = ground(pkg, ws, pool, 6, *small, 4, 1, 3, 1, 0, seeds, snap=9)      # a smaller call in the larger call's slots
    assert ws.ground_buffers() == slots
    same_field(got, ground_field_words(words, 6, *small, 4, 1, 3, 1, 0, seeds, snap=9)[0])
    lean = pkg.Workspace()                                              # r = 0 needs no transform: its three slots stay empty
    ground(pkg, lean, pool, 6, *small, 2, 0, 3, 1, 0, seeds)
    assert [b > 0 for _, b in lean.ground_buffers()] == [True, False, False, False, True, True]
    lean.close()
    ws.close()                                                          # release_all releases the new slots with the rest


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 17, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    seeds = [[origin[0] + x, origin[1] + dims[1] - 1, origin[2] + 4] for x in range(0, 130, 5)]
    unsynced, _ = ground(pkg, ws, pool, depth, origin, dims, 2, 1, 3, 2, 1, seeds, snap=16)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want, facts = ground_field_words(words, depth, origin, dims, 2, 1, 3, 2, 1, seeds, snap=16)
    same_field(ground(pkg, ws, pool, depth, origin, dims, 2, 1, 3, 2, 1, seeds, snap=16)[0], unsynced)
    same_field(unsynced, want)


def test_as_tensor_stats_and_up_names(env, routes):
    pkg, torch = env
    w, ws, pool = routes
    row = (2, 4, 2, 0)
    stats = {}
    seeds = torch.tensor([w["seed"], w["seed"], (0, 0, 0)], dtype=torch.int32, device="cuda")
    got = pkg.ground_field(ws, pool, WORLD_DEPTH, w["origin"], w["dims"], "+y", *row, seeds, as_tensor=True, stats=stats)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (40, 16, 128)
    same_field(got.cpu().numpy(), w["fields"][row])
    assert set(stats) == {"footholds", "seeds_used", "rounds", "tile_runs"} and stats["seeds_used"] == 2 and stats["footholds"] == 5165
    same_field(pkg.ground_field(ws, pool, WORLD_DEPTH, w["origin"], w["dims"], pkg.UP_PLUS_Y, *row, [w["seed"]]), w["fields"][row])
    with pytest.raises(ValueError):
        pkg.ground_field(ws, pool, WORLD_DEPTH, w["origin"], w["dims"], 2, *row, torch.zeros((1, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        pkg.ground_field(ws, pool, WORLD_DEPTH, w["origin"], w["dims"], "+x", *row, [w["seed"]])
    with pytest.raises(pkg.SvoslamError):
        pkg.ground_field(ws, pool, WORLD_DEPTH, w["origin"], w["dims"], 1, *row, [w["seed"]])


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got, stats = ground(pkg, ws, pool, 5, (1, 2, 3), dims, 2, 2, 4, 2, 7, [(1, 2, 3)])
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32
        assert stats == {"footholds": 0, "seeds_used": 0, "rounds": 0, "tile_runs": 0}
    assert ws.ground_buffers() == [(0, 0)] * 6                           # nothing was launched, nothing allocated
    buf = torch.zeros(64 * 16 * 17, dtype=torch.int32, device="cuda")
    seed_buf = torch.tensor([[1, 2, 3], [2, 2, 3]], dtype=torch.int32, device="cuda")
    null, ptr, sp = C.c_void_p(0), pkg._ptr(buf), pkg._ptr(seed_buf)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=7, origin=(1, 2, 3), dims=(4, 2, 2), up=2, r=1, H=3, S=1, c=2, snap=0, seeds=sp, n=2,
              out=ptr, stats=None):
        return L.svoslam_pool_ground_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), up, r, H, S, c, snap, seeds, n, out, stats, pkg._stream())
    st = pkg._GroundStats()
    assert field() == 0 and field(stats=C.byref(st)) == 0 and st.seeds_used == 0 and st.footholds == 0 and st.rounds >= 1   # an empty pool
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=null) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=null) == 0
    assert field(seeds=null, n=0) == 0 and field(n=0) == 0
    for up in (3, 4, 5):
        assert field(up=up) == 0
    assert field(r=0) == 0 and field(H=1, S=0) == 0 and field(H=256, S=4, depth=9) == 0 and field(c=65534, snap=256) == 0 and field(H=5, S=4) == 0
    assert field(n=-1) == -1 and field(seeds=null, n=1) == -1 and field(n=-1, dims=(0, 2, 2)) == -1
    assert field(ws_ref=None) == -1 and field(origin=None) == -1 and field(dims=None) == -1
    assert field(depth=0) == -1 and field(depth=17) == -1 and field(depth=0, dims=(0, 2, 2)) == -1
    assert field(dims=(-1, 2, 2)) == -1 and field(dims=(4, 2, -1)) == -1
    assert field(origin=(-1, 2, 3)) == -1 and field(origin=(125, 2, 3)) == -1 and field(origin=(124, 2, 3)) == 0
    assert field(up=0) == -1 and field(up=1) == -1 and field(up=6) == -1 and field(up=-2) == -1 and field(up=1, dims=(0, 2, 2)) == -1
    assert field(r=-1) == -1 and field(r=4097) == -1 and field(H=0, S=0) == -1 and field(H=257) == -1
    assert field(S=-1) == -1 and field(H=3, S=3) == -1 and field(H=4, S=4) == -1 and field(H=9, S=5) == -1 and field(H=1, S=1) == -1
    assert field(c=-1) == -1 and field(c=65535) == -1 and field(snap=-1) == -1 and field(snap=257) == -1
    assert field(pool_ref=None) == -1 and field(out=null) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # the limits: refused before anything is allocated
    slots = ws.ground_buffers()
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), r=4096, H=256) == -6      # the inflated intermediates
    assert field(depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), r=0) == -6                   # 2^25 tiles
    # n_out * (1 + c * S) >= 2^30: 2^20 cells at 1024 a move; 65 * 16 * 16 cells at 1 + 4 * 16384, while 64 * 16 * 16 still fit
    assert field(depth=16, origin=(0, 0, 0), dims=(1024, 1024, 1), r=0, c=1023) == -6
    assert field(origin=(0, 0, 0), dims=(65, 16, 16), r=0, H=5, S=4, c=16384) == -6
    assert ws.ground_buffers() == slots
    assert field(origin=(0, 0, 0), dims=(64, 16, 16), r=0, H=5, S=4, c=16383) == 0
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, routes):
    pkg, torch = env
    w, ws, pool = routes
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        got, stats = ground(pkg, ws, pool, WORLD_DEPTH, w["origin"], w["dims"], 2, 2, 4, 2, 0, [w["seed"]], as_tensor=True)
        ground(pkg, ws, pool, 4, (1, 2, 3), (9, 3, 3), 4, 0, 1, 0, 0, [])
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0 and stats["rounds"] >= 1
        pkg.trace_ground_paths(got, w["origin"], w["dims"], 2, 2, 0, [w["start"]], 4)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1
        ground(pkg, ws, pool, WORLD_DEPTH, (0, 0, 0), (64, 0, 3), 2, 2, 4, 2, 0, [(0, 0, 0)])     # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            ground(pkg, ws, pool, WORLD_DEPTH, (0, 0, 0), (129, 2, 3), 2, 2, 4, 2, 0, [(0, 0, 0)])   # refused: not bracketed either
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])


# ---- plan_ground_paths and the tool ------------------------------------------------------------------------------------------------
def test_plan_ground_paths_then_the_map_ground_tool(env, routes, tmp_path):
    pkg, torch = env
    w, ws, pool = routes
    row = (0, 4, 2, 20)
    r, H, S, c = row
    want = w["fields"][row]
    cell = 2.0 * EDGE / (1 << WORLD_DEPTH)
    corner = np.asarray(CENTER, np.float64) - EDGE

    def centre(q):
        return (corner + (np.asarray(q, np.float64) + 0.5) * cell).tolist()
    lo, hi = np.zeros(3), np.asarray(w["dims"], np.float64)
    box = np.concatenate([corner + (lo + 0.25) * cell, corner + (hi - 0.25) * cell]).astype(np.float32)
    got_lo, got_hi = pkg.box_to_cells(WORLD_DEPTH, CENTER, EDGE, box)
    assert got_lo.tolist() == [0, 0, 0] and (got_hi + 1).tolist() == list(w["dims"])
    snap = 3
    goal_cell = (w["seed"][0], w["seed"][1] + 2, w["seed"][2])          # two cells above its foothold
    start_cells = [w["start"], (w["start"][0], w["start"][1] + 3, w["start"][2]), w["seed"], (70, 5, 20), None]   # ... inside the platform
    starts_m = [centre(q) for q in start_cells[:4]] + [[100.0, 0.0, 0.0]]
    plan = pkg.plan_ground_paths(ws, pool, WORLD_DEPTH, CENTER, EDGE, box, centre(goal_cell), starts_m, "+y", r, H, S, c, snap)
    same_field(plan["cost"], want)
    assert plan["origin"].tolist() == [0, 0, 0] and plan["dims"].tolist() == list(w["dims"]) and plan["cell_size"] == cell
    assert plan["goal_cell"].tolist() == list(goal_cell) and len(plan["paths"]) == 5 and plan["footholds"] == 5480
    for k, q in enumerate(start_cells):
        p = plan["paths"][k]
        assert (p["cell"] is None) == (q is None) and (q is None or p["cell"].tolist() == list(q))
        if k >= 3:
            assert p["cost"] is None and p["length"] is None and p["cells"] is None and p["polyline"] is None and p["climb"] is None
            continue
        cells, length = trace_ground_path(want, w["origin"], 2, S, c, q, want.size, snap)
        path, climbed = check_ground_path(want, w["origin"], 2, S, c, q, snap)
        assert p["length"] == length and np.array_equal(p["cells"], cells) and np.array_equal(cells, path) and p["climb"] == climbed
        assert p["cost"] == int(want[cells[0][2], cells[0][1], cells[0][0]])
        assert p["polyline"].dtype == np.float64 and np.array_equal(p["polyline"], corner + (cells.astype(np.float64) + 0.5) * cell)
        assert p["polyline"][-1].tolist() == centre(w["seed"])
    assert plan["paths"][0]["cost"] == 228 and plan["paths"][0]["length"] == 149 and plan["paths"][0]["climb"] == 4
    assert np.array_equal(plan["paths"][1]["cells"], plan["paths"][0]["cells"]) and plan["paths"][2]["length"] == 1
    kept = pkg.plan_ground_paths(ws, pool, WORLD_DEPTH, CENTER, EDGE, box, centre(goal_cell), starts_m[:2], 2, r, H, S, c, snap, max_cells=3)
    assert [p["length"] for p in kept["paths"]] == [149, 149] and all(np.array_equal(k["cells"], plan["paths"][0]["cells"][:3]) for k in kept["paths"])
    assert pkg.plan_ground_paths(ws, pool, WORLD_DEPTH, CENTER, EDGE, [5.0, 0, 0, 4.0, 1, 1], centre(goal_cell), starts_m, 2, r, H, S, c, snap) is None
    # the tool
    ckpt, out = tmp_path / "map.svopool", tmp_path / "ground.npz"
    pool.save(ckpt, CENTER, EDGE, WORLD_DEPTH)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_ground.py"), str(ckpt), str(out), "--up", "+y", "--radius", str(r), "--height", str(H),
           "--step", str(S), "--climb-cost", str(c), "--snap", str(snap), "--box"] + [repr(float(v)) for v in box]
    cmd += ["--goal"] + [repr(float(v)) for v in centre(goal_cell)]
    for s in starts_m:
        cmd += ["--start"] + [repr(float(v)) for v in s]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(out)
    same_field(z["cost"], want)
    assert z["origin"].tolist() == [0, 0, 0] and z["dims"].tolist() == list(w["dims"]) and int(z["depth"]) == WORLD_DEPTH
    assert z["goal_cell"].tolist() == list(goal_cell) and z["start_cells"].tolist() == [list(q) for q in start_cells[:4]] + [[-1, -1, -1]]
    assert (int(z["radius_cells"]), int(z["height_cells"]), int(z["step_cells"]), int(z["climb_cost"]), int(z["snap_cells"])) == (r, H, S, c, snap)
    assert str(z["up"]) == "+y" and int(z["footholds"]) == 5480
    assert z["lengths"].tolist() == [149, 149, 1, 0, 0] and z["costs"].tolist() == [228, 228, 0, -1, -1] and z["climbs"].tolist() == [4, 4, 0, 0, 0]
    stored = np.asarray(CENTER, np.float32).astype(np.float64) - EDGE   # the checkpoint keeps the centre in binary32
    for k, p in enumerate(plan["paths"]):
        if p["cells"] is None:
            assert z["cells_%d" % k].shape == (0, 3) and z["polyline_%d" % k].shape == (0, 3)
        else:
            assert np.array_equal(z["cells_%d" % k], p["cells"])
            assert np.array_equal(z["polyline_%d" % k], stored + (p["cells"].astype(np.float64) + 0.5) * cell)
