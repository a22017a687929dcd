"""svoslam_pool_cost_field and svoslam_field_trace_paths on the device: every value equals the host restatements of the specification
(tests/test_plan_cpu.py: cost_field_words, Dijkstra's algorithm on the weights of the distance field's restatements, and trace_path,
the rule cell by cell) applied to the pool's own words -- never a second device result alone.

Two worlds make the weights matter: a wall with a tunnel and a gate, where the weighted field sends the path through the gate and
the unweighted one through the tunnel, and a serpentine whose cheapest path crosses tile faces dozens of times and comes back into
a tile it has left.  The tile is 64 x 8 x 8 cells (map_plan.hip)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable
from test_gpu_field import case_region, same_field
from test_gpu_query import fused_pool
from test_plan_cpu import (PLAN_CASES, PLATEAU, PLATEAU_TRACES, SERPENTINE, TIE_BREAK_PATH, WORLD_DEPTH, check_path, cost_field_words, ramp,
                           tile_visits, trace_path, weights_of, world)
from test_reach_cpu import counted_seeds, reach_field_words, seeds_for
from test_surface_cpu import CENTER, EDGE, HandPool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def cost(pkg, ws, pool, depth, origin, dims, clearance, comfort, ring, seeds, **kw):
    stats = {}
    got = pkg.cost_field(ws, pool, depth, origin, dims, clearance, comfort, ring, seeds, stats=stats, **kw)
    return got, stats


def same_paths(pkg, field, origin, dims, starts, max_cells, fill=-1):
    """the device's paths and lengths of `starts` equal trace_path's, and nothing behind a path's cells was written"""
    paths, lengths = pkg.trace_paths(field, origin, dims, starts, max_cells)
    assert paths.dtype == np.int32 and lengths.dtype == np.int32 and paths.shape == (len(starts), max_cells, 3) and lengths.shape == (len(starts),)
    for k, start in enumerate(starts):
        cells, length = trace_path(field, origin, start, max_cells)
        assert int(lengths[k]) == length, (k, start, int(lengths[k]), length)
        assert np.array_equal(paths[k, :cells.shape[0]], cells), (k, start)
        assert (paths[k, cells.shape[0]:] == fill).all(), (k, start)
    return paths, lengths


# ---- hand-built pools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, origin, dims, clearance, comfort, ring, seeds, want, used = PLAN_CASES[name]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    got, stats = cost(pkg, ws, pool, depth, origin, dims, clearance, comfort, ring, seeds)
    same_field(got, want)
    same_field(got, cost_field_words(words, depth, origin, dims, clearance, comfort, ring, seeds))
    assert stats["seeds_used"] == used and stats["rounds"] >= 1 and stats["tile_runs"] >= (1 if used else 0)
    assert stats["max_weight"] == 1 + max(ring, default=0)
    steps = pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds)
    same_field(cost(pkg, ws, pool, depth, origin, dims, clearance, comfort, [0] * len(ring), seeds)[0], steps)
    same_field(cost(pkg, ws, pool, depth, origin, dims, clearance, clearance, [], seeds)[0], steps)
    every = [(origin[0] + x, origin[1] + y, origin[2] + z) for z in range(dims[2]) for y in range(dims[1]) for x in range(dims[0])]
    same_paths(pkg, got, origin, dims, every, dims[0] * dims[1] * dims[2])


# ---- two routes ------------------------------------------------------------------------------------------------------------------
def test_two_routes(env):
    pkg, torch = env
    w = world("two_routes")
    o, dims, seed, start, r, R, ring = w["origin"], w["dims"], w["seed"], w["start"], w["clearance"], w["comfort"], w["ring"]
    at = [start[a] - o[a] for a in range(3)]
    # on the restatement first
    assert tuple(dims) == (128, 40, 5) and tuple(o) == (0, 0, 1) and (r, R, ring) == (1, 4, [40, 20, 10])
    assert [seed[a] - o[a] for a in range(3)] == [10, 4, 2] and at == [10, 32, 2]
    assert w["cost"][at[2], at[1], at[0]] == 216 and w["steps"][at[2], at[1], at[0]] == 28
    free, wt = weights_of(w["field"], r, R, ring)
    heavy, light = check_path(w["cost"], free, wt, o, start), check_path(w["steps"], free, np.where(free, 1, 0), o, start)
    assert heavy.shape[0] == 217 and ((heavy[:, 0] >= 100) & (heavy[:, 0] <= 114)).sum() >= 8 and not (heavy[:, 0] == 10).all()
    assert light.shape[0] == 29 and (light[:, 0] == 10).all()
    assert not np.array_equal(w["cost"], w["steps"])
    # the device
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(w["words"])
    got, stats = cost(pkg, ws, pool, WORLD_DEPTH, o, dims, r, R, ring, [seed])
    same_field(got, w["cost"])
    assert stats == dict(stats, seeds_used=1, max_weight=41)
    paths, lengths = same_paths(pkg, got, o, dims, [start], 300)
    assert int(lengths[0]) == 217 and np.array_equal(paths[0, :217], heavy)
    plain = pkg.reach_field(ws, pool, WORLD_DEPTH, o, dims, r, [seed])
    same_field(plain, w["steps"])
    same_field(cost(pkg, ws, pool, WORLD_DEPTH, o, dims, r, r, [], [seed])[0], plain)
    same_field(cost(pkg, ws, pool, WORLD_DEPTH, o, dims, r, R, [0, 0, 0], [seed])[0], plain)
    paths, lengths = same_paths(pkg, plain, o, dims, [start], 29)
    assert int(lengths[0]) == 29 and np.array_equal(paths[0], light)


# ---- the weighted serpentine -----------------------------------------------------------------------------------------------------
def test_weighted_serpentine(env):
    pkg, torch = env
    w = world("serpentine")
    o, dims, seed, r, R, ring = w["origin"], w["dims"], w["seed"], w["clearance"], w["comfort"], w["ring"]
    want, steps = w["cost"], w["steps"]
    pitch, walls, gap = SERPENTINE
    # on the restatement first
    assert (pitch, walls, gap) == (6, 6, 6) and tuple(dims) == (128, 47, 5) and (r, R, ring) == (0, 2, [8, 3])
    assert seed[0] == 0 and 0 <= seed[1] - o[1] < pitch - 1
    assert want.max() == 904 and steps.max() == 869 and want.max() > steps.max()
    assert (want == -1).sum() == 3200 and (want == -2).sum() == 4300
    free, wt = weights_of(w["field"], r, R, ring)
    far = np.array(np.unravel_index(np.argmax(want), want.shape)[::-1]) + np.asarray(o)
    path = check_path(want, free, wt, o, far)
    assert tile_visits(path, o) >= 2
    # the device
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(w["words"])
    got, stats = cost(pkg, ws, pool, WORLD_DEPTH, o, dims, r, R, ring, [seed])
    same_field(got, want)
    assert stats["seeds_used"] == 1 and stats["max_weight"] == 9 and stats["rounds"] > walls
    paths, lengths = same_paths(pkg, got, o, dims, [far.tolist()], path.shape[0] + 3)
    assert int(lengths[0]) == path.shape[0] and np.array_equal(paths[0, :path.shape[0]], path)


# ---- fused pools -------------------------------------------------------------------------------------------------------------
# (fused depth, d, (nx, ny, nz), origin x: "lo" 0 | "in" 37 | "hi" N - nx | "pt" about the cloud, clearance, comfort, profile, seeds
# from T).  nx 1, 63, 64, 65, 130: the edges of a row word, a wavefront and a tile; ny, nz 1, 7, 8, 9, 17: one row, one less than,
# equal to, one more than and more than twice the tile's side.  Sizes that do not fit the lattice of d are cut to it.
FUSED_CASES = [
    (9, 9, (1, 1, 1), "pt", 0, 0, "ramp", 1), (9, 9, (63, 7, 17), "in", 1, 4, "ramp", 7), (9, 9, (64, 17, 8), "lo", 5, 6, "bumpy", 1),
    (9, 9, (65, 8, 9), "hi", 0, 2, "bumpy", 7), (9, 9, (130, 9, 7), "in", 0, 2, "ramp", 7), (9, 9, (130, 1, 17), "hi", 1, 4, "bumpy", 1),
    (9, 9, (65, 17, 17), "pt", 5, 6, "ramp", 7), (9, 9, (130, 8, 8), "pt", 0, 2, "bumpy", 1), (9, 9, (130, 17, 9), "pt", 1, 4, "ramp", 1),
    (9, 7, (64, 9, 17), "in", 1, 4, "bumpy", 7), (9, 7, (130, 1, 8), "lo", 0, 2, "ramp", 1), (9, 7, (63, 17, 1), "hi", 0, 0, "ramp", 7),
    (9, 7, (1, 7, 9), "pt", 1, 4, "ramp", 1),
    (6, 6, (63, 8, 17), "lo", 5, 6, "bumpy", 7), (6, 6, (64, 17, 1), "lo", 1, 4, "bumpy", 1), (6, 6, (1, 1, 7), "hi", 0, 2, "ramp", 1),
    (6, 6, (20, 7, 9), "in", 5, 6, "ramp", 7), (6, 6, (65, 17, 17), "pt", 0, 2, "ramp", 7), (6, 4, (65, 17, 17), "lo", 1, 4, "bumpy", 7),
    (6, 4, (1, 9, 1), "hi", 0, 0, "ramp", 1), (6, 4, (5, 1, 8), "in", 0, 2, "bumpy", 1),
]


def profile(kind, clearance, comfort):
    n = comfort - clearance
    return ramp(clearance, comfort, 4) if kind == "ramp" else [(9, 0, 30)[k % 3] for k in range(n)]


@pytest.fixture(scope="module")
def reference(fused):
    """case -> (origin, dims, ring, seeds, the distance field's restatement with the comfort radius, the reach field's restatement, the
    cost field's), computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            depth, d, shape, ox, clearance, comfort, kind, count = case
            words = fused[depth][1]
            origin, dims = case_region(words, d, shape, ox, comfort)
            field = distance_field_separable(words, d, origin, dims, comfort)
            near = np.where((field >= 0) & (field <= clearance * clearance), field, -1).astype(np.int32)
            ring = profile(kind, clearance, comfort)
            seeds = seeds_for(near == -1, origin, dims, d, count, np.random.default_rng(FUSED_CASES.index(case)))
            cache[case] = (origin, dims, ring, seeds, field, reach_field_words(words, d, origin, dims, clearance, seeds, field=near),
                           cost_field_words(words, d, origin, dims, clearance, comfort, ring, seeds, field=field))
        return cache[case]
    return get


def test_the_fused_cases_are_not_empty(fused, reference):
    """on the restatements' results, never the device's"""
    reached = blocked = dearer = ignored = 0
    nx, nyz, ox, radii, kinds, counts, ds = set(), set(), set(), set(), set(), set(), set()
    for case in FUSED_CASES:
        depth, d, shape, where, clearance, comfort, kind, count = case
        origin, dims, ring, seeds, field, steps, want = reference(case)
        nx.add(shape[0]); nyz.update(shape[1:]); ox.add(where); radii.add((clearance, comfort)); kinds.add(kind); counts.add(count); ds.add((depth, d))
        reached, blocked = reached + int((want > 0).sum()), blocked + int((want == -2).sum())
        dearer += int((want != steps).sum())
        free, _ = weights_of(field, clearance, comfort, ring)
        ignored += seeds.shape[0] - counted_seeds(free, origin, dims, seeds).shape[0]
    assert reached > 1000 and blocked > 1000 and dearer > 1000 and ignored > 4 * len(FUSED_CASES), (reached, blocked, dearer, ignored)
    assert nx == {1, 63, 64, 65, 130, 20, 5} and nyz == {1, 7, 8, 9, 17} and ox == {"lo", "in", "hi", "pt"}
    assert radii == {(0, 0), (0, 2), (1, 4), (5, 6)} and kinds == {"ramp", "bumpy"}
    assert counts == {1, 7} and ds == {(9, 9), (9, 7), (6, 6), (6, 4)}


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-r%d-R%d-%s-seeds%d" % (c[0], c[1], *c[2], *c[3:]))
def test_fused_cloud(env, fused, reference, case):
    pkg, torch = env
    pool, words, pts, ws = fused[case[0]]
    origin, dims, ring, seeds, field, steps, want = reference(case)
    got, stats = cost(pkg, ws, pool, case[1], origin, dims, case[4], case[5], ring, seeds)
    same_field(got, want)
    assert stats["seeds_used"] == int((want == 0).sum()) and stats["max_weight"] == 1 + max(ring, default=0)
    reached = np.argwhere(want >= 0)[:, ::-1] + np.asarray(origin)
    if reached.shape[0]:
        rng = np.random.default_rng(3)
        starts = reached[rng.choice(reached.shape[0], min(9, reached.shape[0]), replace=False)].tolist()
        starts.append((np.array(np.unravel_index(np.argmax(want), want.shape)[::-1]) + np.asarray(origin)).tolist())
        same_paths(pkg, got, origin, dims, starts, int(want.max()) + 1)


@pytest.mark.parametrize("case", [FUSED_CASES[k] for k in (6, 8, 9, 17)], ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-r%d-R%d" % (c[0], c[1], *c[2], *c[3:6]))
def test_blocked_is_where_the_device_distance_field_is_not_minus_1(env, fused, reference, case):
    pkg, torch = env
    pool, words, pts, ws = fused[case[0]]
    origin, dims, ring, seeds, field, steps, want = reference(case)
    assert (want == -2).sum() > 0 and (want >= 0).sum() > 0
    dist2 = pkg.distance_field(ws, pool, case[1], origin, dims, case[4])
    got, _ = cost(pkg, ws, pool, case[1], origin, dims, case[4], case[5], ring, seeds)
    assert np.array_equal(got == -2, dist2 != -1)
    same_field(pkg.distance_field(ws, pool, case[1], origin, dims, case[5]), field)


# ---- the trace -------------------------------------------------------------------------------------------------------------------
def test_trace_on_cost_and_reach_fields(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (0, 0, 0), (64, 40, 12)
    near = distance_field_separable(words, 6, origin, dims, 1)
    seeds = seeds_for(near == -1, origin, dims, 6, 2, np.random.default_rng(9))
    seed = [int(v) for v in seeds[0]]
    fields = (pkg.cost_field(ws, pool, 6, origin, dims, 1, 3, [6, 2], seeds), pkg.reach_field(ws, pool, 6, origin, dims, 1, seeds))
    for field in fields:
        assert (field > 0).sum() > 1000 and (field == -2).sum() > 100
        beside = [seed[0], seed[1], seed[2]]
        for m in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):   # a traversable cell next to the seed
            p = [seed[a] + m[a] for a in range(3)]
            if all(0 <= p[a] < dims[a] for a in range(3)) and field[p[2], p[1], p[0]] > 0:
                beside = p
        blocked = np.argwhere(field == -2)[0][::-1].tolist()
        paths, lengths = same_paths(pkg, field, origin, dims, [seed], 5)                   # 1 start: on the seed
        assert int(lengths[0]) == 1 and paths[0, 0].tolist() == seed
        paths, lengths = same_paths(pkg, field, origin, dims, [beside, blocked, [64, 0, 0], [-1, 0, 0], [0, 40, 0], [0, 0, 12]], 5)
        assert lengths.tolist() == [2, 0, 0, 0, 0, 0] and paths[0, 1].tolist() == seed
        reached = np.argwhere(field >= 0)[:, ::-1]
        starts = reached[np.random.default_rng(1).choice(reached.shape[0], 257, replace=False)].tolist()   # more than one workgroup
        far = int(field.max()) + 1
        paths, lengths = same_paths(pkg, field, origin, dims, starts, far)
        assert lengths.min() >= 1 and lengths.max() > 20
        # max_cells shorter than the paths: the whole length, the first cells, and the rest of a sentinel-filled buffer untouched
        short, short_lengths = same_paths(pkg, field, origin, dims, starts, 7)
        assert np.array_equal(short_lengths, lengths) and (lengths > 7).sum() > 100
        t_field, t_starts = torch.from_numpy(field).cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda")
        buf = torch.full((257, 7, 3), -77, dtype=torch.int32, device="cuda")
        out_len = torch.full((257,), -77, dtype=torch.int32, device="cuda")
        o3, n3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
        assert pkg.lib().svoslam_field_trace_paths(pkg._ptr(t_field), o3, n3, pkg._ptr(t_starts), 257, 7, pkg._ptr(buf), pkg._ptr(out_len), pkg._stream()) == 0
        buf, out_len = buf.cpu().numpy(), out_len.cpu().numpy()
        assert np.array_equal(out_len, lengths)
        for k in range(257):
            kept = min(int(lengths[k]), 7)
            assert np.array_equal(buf[k, :kept], paths[k, :kept]) and (buf[k, kept:] == -77).all()
        # max_cells 0 with a NULL path buffer: the lengths alone
        out_len = torch.full((257,), -77, dtype=torch.int32, device="cuda")
        assert pkg.lib().svoslam_field_trace_paths(pkg._ptr(t_field), o3, n3, pkg._ptr(t_starts), 257, 0, None, pkg._ptr(out_len), pkg._stream()) == 0
        assert np.array_equal(out_len.cpu().numpy(), lengths)
        none, none_lengths = pkg.trace_paths(field, origin, dims, starts, 0)
        assert none.shape == (257, 0, 3) and np.array_equal(none_lengths, lengths)
    # tensors in, tensors out
    paths, lengths = pkg.trace_paths(torch.from_numpy(fields[0]).cuda(), origin, dims, torch.tensor([seed], dtype=torch.int32, device="cuda"), 3, as_tensor=True)
    assert isinstance(paths, torch.Tensor) and paths.is_cuda and paths.dtype == torch.int32 and tuple(paths.shape) == (1, 3, 3)
    assert isinstance(lengths, torch.Tensor) and lengths.tolist() == [1] and paths[0, 0].tolist() == seed
    with pytest.raises(ValueError):
        pkg.trace_paths(torch.zeros((12, 40, 64), dtype=torch.int64, device="cuda"), origin, dims, [seed], 3)
    with pytest.raises(ValueError):
        pkg.trace_paths(fields[0], origin, (64, 40, 11), [seed], 3)


def test_trace_tie_break_and_plateau(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(HandPool().words())
    field = pkg.cost_field(ws, pool, 3, (0, 0, 0), (4, 4, 4), 0, 2, [5, 2], [(0, 0, 0)])
    paths, lengths = same_paths(pkg, field, (0, 0, 0), (4, 4, 4), [(3, 3, 3)], 12)
    assert int(lengths[0]) == 10 and [tuple(c) for c in paths[0, :10].tolist()] == TIE_BREAK_PATH
    moved = pkg.reach_field(ws, pool, 3, (2, 1, 4), (4, 4, 4), 0, [(2, 1, 4)])
    paths, lengths = same_paths(pkg, moved, (2, 1, 4), (4, 4, 4), [(5, 4, 7)], 10)
    assert [tuple(c) for c in paths[0].tolist()] == [(x + 2, y + 1, z + 4) for x, y, z in TIE_BREAK_PATH]
    # an array that is not a cost-to-go field: minus the cells walked
    starts = sorted(PLATEAU_TRACES)
    paths, lengths = same_paths(pkg, PLATEAU, (0, 0, 0), (6, 2, 1), starts, 8)
    for k, start in enumerate(starts):
        cells, length = PLATEAU_TRACES[start]
        assert int(lengths[k]) == length and [tuple(c) for c in paths[k, :len(cells)].tolist()] == cells
    assert -2 in lengths.tolist() and -1 in lengths.tolist()
    # ... at an origin that is not in any root: the region is whatever the caller says
    same_paths(pkg, PLATEAU, (-5, 100000, 7), (6, 2, 1), [(s[0] - 5, s[1] + 100000, s[2] + 7) for s in starts], 8)


def test_trace_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    L = pkg.lib()
    field = torch.zeros(64, dtype=torch.int32, device="cuda")
    starts = torch.tensor([[0, 0, 0], [3, 3, 3]], dtype=torch.int32, device="cuda")
    paths = torch.full((2, 4, 3), -77, dtype=torch.int32, device="cuda")
    lengths = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    null = C.c_void_p(0)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def trace(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), s=pkg._ptr(starts), n=2, cap=4, p=pkg._ptr(paths), out=pkg._ptr(lengths)):
        return L.svoslam_field_trace_paths(f, i3(origin), i3(dims), s, n, cap, p, out, pkg._stream())
    assert trace() == 0 and lengths.tolist() == [1, 1]                   # all zeros: every cell is a goal
    assert trace(n=0, s=null, out=null, p=null, f=null) == 0 and trace(cap=0, p=null) == 0
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):                       # a zero entry of dims: lengths 0
        lengths.fill_(-77)
        assert trace(dims=dims, f=null) == 0 and lengths.tolist() == [0, 0]
    assert trace(origin=None) == -1 and trace(dims=None) == -1
    assert trace(dims=(-1, 4, 4)) == -1 and trace(dims=(4, 4, -1)) == -1 and trace(n=-1) == -1 and trace(cap=-1) == -1
    assert trace(f=null) == -1 and trace(s=null) == -1 and trace(out=null) == -1 and trace(p=null) == -1
    assert trace(dims=(65536, 65536, 1)) == -6 and trace(dims=(2048, 1024, 1024)) == -6 and trace(dims=(65536, 65536, 65536)) == -6
    assert trace(n=1 << 20, cap=1 << 10) == -6 and trace(n=(1 << 31) - 1, cap=(1 << 31) - 1) == -6
    assert (paths[:, 1:] == -77).all()


# ---- conventions -----------------------------------------------------------------------------------------------------------------
def test_the_other_fields_are_unchanged_by_plan_calls_on_their_workspace(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (2, 0, 5), (62, 33, 11)
    seeds = [(3, 1, 6), (60, 30, 14)]
    before = (pkg.distance_field(ws, pool, 6, origin, dims, 3), pkg.reach_field(ws, pool, 6, origin, dims, 1, seeds),
              pkg.label_components(ws, pool, 6, origin, dims, 1))
    cost(pkg, ws, pool, 6, origin, dims, 1, 4, [9, 5, 1], seeds)
    cost(pkg, ws, pool, 6, (0, 0, 0), (64, 9, 9), 0, 0, [], [(1, 1, 1)])
    after = (pkg.distance_field(ws, pool, 6, origin, dims, 3), pkg.reach_field(ws, pool, 6, origin, dims, 1, seeds),
             pkg.label_components(ws, pool, 6, origin, dims, 1))
    for a, b in zip(after, before):
        same_field(a, b)
    same_field(after[0], distance_field_separable(words, 6, origin, dims, 3))
    same_field(after[1], reach_field_words(words, 6, origin, dims, 1, seeds))


def test_workspace_slots_are_reused(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    ws = pkg.Workspace()
    assert ws.plan_buffers() == [(0, 0)] * 3 and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    seeds = [(6, 4, 8), (30, 20, 12), (63, 63, 39), (0, 0, 0)]
    first, _ = cost(pkg, ws, pool, 6, *large, 1, 3, [7, 2], seeds)
    slots, field_slots = ws.plan_buffers(), ws.field_buffers()
    assert all(p != 0 and b > 0 for p, b in slots + field_slots) and ws.reach_buffers() == [(0, 0)] * 2
    assert slots[0][1] >= 64 * 40 * 8 and slots[1][1] >= 64 * 64 * 40 * 2 and slots[2][1] >= 32 + 40 * 8 + 2 * 4
    again, _ = cost(pkg, ws, pool, 6, *large, 1, 3, [7, 2], seeds)
    assert ws.plan_buffers() == slots and ws.field_buffers() == field_slots      # a second call of the same size allocates nothing
    want = cost_field_words(words, 6, *large, 1, 3, [7, 2], seeds, field=distance_field_separable(words, 6, *large, 3))
    assert (want > 0).sum() > 1000 and (want == -2).sum() > 1000
    same_field(first, want)
    same_field(again, want)
    got, _ = cost(pkg, ws, pool, 6, *small, 1, 3, [0, 9], seeds)                # a smaller call in the larger call's slots
    assert ws.plan_buffers() == slots and ws.field_buffers() == field_slots
    same_field(got, cost_field_words(words, 6, *small, 1, 3, [0, 9], seeds))
    ws.close()                                                                  # release_all releases the new slots with the rest


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 17, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    seeds = [origin, [origin[a] + dims[a] - 1 for a in range(3)], [origin[0] + 64, origin[1] + 8, origin[2]]]
    unsynced, _ = cost(pkg, ws, pool, depth, origin, dims, 1, 3, [5, 2], seeds)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want = cost_field_words(words, depth, origin, dims, 1, 3, [5, 2], seeds, field=distance_field_separable(words, depth, origin, dims, 3))
    assert (want == 0).sum() >= 1 and (want > 0).sum() > 100 and (want == -2).sum() > 100
    same_field(cost(pkg, ws, pool, depth, origin, dims, 1, 3, [5, 2], seeds)[0], unsynced)
    same_field(unsynced, want)


def test_as_tensor_and_seeds_as_a_tensor(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (3, 0, 9), (61, 30, 5)
    field = distance_field_separable(words, 6, origin, dims, 2)
    near = np.where((field >= 0) & (field <= 1), field, -1)
    seeds = seeds_for(near == -1, origin, dims, 6, 3, np.random.default_rng(5))
    want = cost_field_words(words, 6, origin, dims, 1, 2, [11], seeds, field=field)
    stats = {}
    got = pkg.cost_field(ws, pool, 6, origin, dims, 1, 2, [11], torch.from_numpy(seeds.astype(np.int32)).cuda(), as_tensor=True, stats=stats)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (5, 30, 61)
    same_field(got.cpu().numpy(), want)
    assert stats["seeds_used"] == 3 and stats["max_weight"] == 12 and set(stats) == {"rounds", "tile_runs", "seeds_used", "max_weight"}
    same_field(pkg.cost_field(ws, pool, 6, origin, dims, 1, 2, np.array([11]), seeds), want)     # arrays, no stats
    with pytest.raises(ValueError):
        pkg.cost_field(ws, pool, 6, origin, dims, 1, 2, [11], torch.zeros((1, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        pkg.cost_field(ws, pool, 6, origin, dims, 1, 2, [11, 3], seeds)
    with pytest.raises(ValueError):
        pkg.cost_field(ws, pool, 6, origin, dims, 1, 2, [65535], seeds)


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got, stats = cost(pkg, ws, pool, 5, (1, 2, 3), dims, 2, 4, [7, 3], [(1, 2, 3)])
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32
        assert stats == {"rounds": 0, "tile_runs": 0, "seeds_used": 0, "max_weight": 8}
    assert ws.plan_buffers() == [(0, 0)] * 3 and ws.field_buffers() == [(0, 0)] * 3     # nothing was launched, nothing allocated
    buf = torch.zeros(64 * 16 * 17, dtype=torch.int32, device="cuda")
    seed_buf = torch.tensor([[1, 2, 3], [2, 2, 3]], dtype=torch.int32, device="cuda")
    null, ptr, sp = C.c_void_p(0), pkg._ptr(buf), pkg._ptr(seed_buf)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=7, origin=(1, 2, 3), dims=(4, 2, 2), r=1, R=3, ring=(6, 2), seeds=sp, n=2, out=ptr,
              stats=None):
        return L.svoslam_pool_cost_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), r, R, None if ring is None else (C.c_int32 * len(ring))(*ring),
                                         seeds, n, out, stats, pkg._stream())
    st = pkg._PlanStats()
    assert field() == 0 and field(stats=C.byref(st)) == 0 and st.seeds_used == 2 and st.rounds >= 1 and st.max_weight == 7
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=null) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=null) == 0
    assert field(seeds=null, n=0) == 0 and field(n=0) == 0
    assert field(r=2, R=2, ring=None) == 0 and field(r=0, R=0, ring=None) == 0 and field(r=2, R=2, ring=(9,)) == 0
    assert field(ring=(0, 65534)) == 0 and field(ring=(65534, 0), stats=C.byref(st)) == 0 and st.max_weight == 65535
    assert field(n=-1) == -1 and field(seeds=null, n=1) == -1 and field(n=-1, dims=(0, 2, 2)) == -1
    assert field(ws_ref=None) == -1 and field(origin=None) == -1 and field(dims=None) == -1
    assert field(depth=0) == -1 and field(depth=17) == -1 and field(depth=0, dims=(0, 2, 2)) == -1
    assert field(dims=(-1, 2, 2)) == -1 and field(dims=(4, 2, -1)) == -1
    assert field(origin=(-1, 2, 3)) == -1 and field(origin=(125, 2, 3)) == -1 and field(origin=(124, 2, 3)) == 0
    assert field(r=-1) == -1 and field(r=4, R=3) == -1 and field(r=4097, R=4097, ring=None) == -1 and field(r=1, R=4097) == -1
    assert field(r=4, R=3, dims=(0, 2, 2)) == -1
    assert field(ring=None) == -1 and field(ring=None, dims=(0, 2, 2)) == -1      # R > r needs its costs
    assert field(ring=(6, -1)) == -1 and field(ring=(65535, 2)) == -1 and field(ring=(6, 1 << 30)) == -1
    assert field(pool_ref=None) == -1 and field(out=null) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # the limits: refused before anything is allocated
    slots, field_slots = ws.plan_buffers(), ws.field_buffers()
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), r=0, R=4096, ring=(0,) * 4096) == -6
    assert field(depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), r=0, R=0, ring=None) == -6     # 2^25 tiles
    # n_out * max_weight >= 2^30: 2^20 cells of weight 1024; 16640 cells of weight 65535, while 16384 of them still fit
    assert field(depth=16, origin=(0, 0, 0), dims=(1024, 1024, 1), r=0, R=1, ring=(1023,)) == -6
    assert field(origin=(0, 0, 0), dims=(65, 16, 16), r=0, R=1, ring=(65534,)) == -6
    assert ws.plan_buffers() == slots and ws.field_buffers() == field_slots
    assert field(origin=(0, 0, 0), dims=(64, 16, 16), r=0, R=1, ring=(65534,)) == 0
    with pytest.raises(Exception):
        pkg.cost_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 1, 4097, [0] * 4096, [(0, 0, 0)])
    with pytest.raises(Exception):
        pkg.cost_field(ws, pool, 5, (30, 0, 0), (4, 4, 4), 1, 2, [3], [(0, 0, 0)])
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        got, stats = cost(pkg, ws, pool, 6, (0, 0, 0), (64, 20, 3), 1, 3, [4, 2], [(63, 19, 2), (0, 0, 0)], as_tensor=True)
        cost(pkg, ws, pool, 4, (1, 2, 3), (9, 3, 3), 0, 0, [], [])
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0 and stats["rounds"] >= 1
        pkg.trace_paths(got, (0, 0, 0), (64, 20, 3), [(5, 5, 1)], 4)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1
        cost(pkg, ws, pool, 6, (0, 0, 0), (64, 0, 3), 1, 3, [4, 2], [(0, 0, 0)])       # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            cost(pkg, ws, pool, 6, (0, 0, 0), (65, 2, 3), 1, 3, [4, 2], [(0, 0, 0)])   # refused: not bracketed either
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])


# ---- plan_paths and the tool -----------------------------------------------------------------------------------------------------
def test_plan_paths_then_the_map_plan_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    clearance, comfort, penalty = 1, 3, 5
    ring = ramp(clearance, comfort, penalty)
    assert ring == [10, 5]
    field = distance_field_separable(words, 6, lo.tolist(), dims.tolist(), comfort)
    free, wt = weights_of(field, clearance, comfort, ring)
    at = np.argwhere(free)[:, ::-1] + lo
    cell = 2.0 * EDGE / 64
    corner = np.asarray(CENTER, np.float64) - EDGE

    def centre(c):
        return (corner + (np.asarray(c, np.float64) + 0.5) * cell).tolist()
    goal_cell = at[0].tolist()
    want = cost_field_words(words, 6, lo.tolist(), dims.tolist(), clearance, comfort, ring, [goal_cell], field=field)
    reached = np.argwhere(want > 0)[:, ::-1] + lo
    blocked = (np.argwhere(want == -2)[0][::-1] + lo).tolist()
    assert reached.shape[0] > 100 and (want != reach_field_words(words, 6, lo.tolist(), dims.tolist(), clearance, [goal_cell])).sum() > 20
    start_cells = [reached[reached.shape[0] // 2].tolist(), reached[-1].tolist(), goal_cell, blocked, None]
    starts_m = [centre(c) for c in start_cells[:4]] + [[100.0, 0.0, 0.0]]       # ... and a point outside the root cube
    plan = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m, clearance, comfort, ring)
    same_field(plan["cost"], want)
    assert plan["origin"].tolist() == lo.tolist() and plan["dims"].tolist() == dims.tolist() and plan["cell_size"] == cell
    assert plan["goal_cell"].tolist() == goal_cell and len(plan["paths"]) == 5
    for k, c in enumerate(start_cells):
        p = plan["paths"][k]
        assert (p["cell"] is None) == (c is None) and (c is None or p["cell"].tolist() == c)
        if k >= 3:
            assert p["cost"] is None and p["length"] is None and p["cells"] is None and p["polyline"] is None
            continue
        cells, length = trace_path(want, lo.tolist(), c, want.size)
        assert p["length"] == length and np.array_equal(p["cells"], cells)
        assert p["cost"] == int(want[c[2] - lo[2], c[1] - lo[1], c[0] - lo[0]])
        assert np.array_equal(cells, check_path(want, free, wt, lo.tolist(), c))
        assert p["polyline"].dtype == np.float64 and np.array_equal(p["polyline"], corner + (cells.astype(np.float64) + 0.5) * cell)
        assert p["polyline"][0].tolist() == centre(c) and p["polyline"][-1].tolist() == centre(goal_cell)
    assert plan["paths"][2]["length"] == 1 and plan["paths"][2]["cost"] == 0
    kept = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m[:2], clearance, comfort, ring, max_cells=3)
    assert [p["length"] for p in kept["paths"]] == [p["length"] for p in plan["paths"][:2]]
    assert all(np.array_equal(k["cells"], p["cells"][:3]) for k, p in zip(kept["paths"], plan["paths"]))
    assert pkg.plan_paths(ws, pool, 6, CENTER, EDGE, [5.0, 0, 0, 4.0, 1, 1], centre(goal_cell), starts_m, clearance, comfort, ring) is None
    # the tool
    ckpt, out = tmp_path / "map.svopool", tmp_path / "plan.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_plan.py"), str(ckpt), str(out), "--clearance", str(clearance), "--comfort", str(comfort),
           "--penalty", str(penalty), "--box"] + [repr(float(v)) for v in box] + ["--goal"] + [repr(float(v)) for v in centre(goal_cell)]
    for s in starts_m:
        cmd += ["--start"] + [repr(float(v)) for v in s]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_field(z["cost"], want)
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6 and float(z["cell_size"]) == cell
    assert z["goal_cell"].tolist() == goal_cell and z["start_cells"].tolist() == start_cells[:4] + [[-1, -1, -1]]
    assert z["ring_cost"].tolist() == ring and int(z["clearance_cells"]) == clearance and int(z["comfort_cells"]) == comfort
    assert z["lengths"].tolist() == [p["length"] or 0 for p in plan["paths"]] and z["costs"].tolist() == [-1 if p["cost"] is None else p["cost"] for p in plan["paths"]]
    stored = np.asarray(CENTER, np.float32).astype(np.float64) - EDGE   # the checkpoint keeps the centre in binary32
    for k, p in enumerate(plan["paths"]):
        if p["cells"] is None:
            assert z["cells_%d" % k].shape == (0, 3) and z["polyline_%d" % k].shape == (0, 3)
        else:
            assert np.array_equal(z["cells_%d" % k], p["cells"])
            assert np.array_equal(z["polyline_%d" % k], stored + (p["cells"].astype(np.float64) + 0.5) * cell)
            assert np.array_equal(z["polyline_%d" % k][-1], stored + (np.asarray(goal_cell) + 0.5) * cell)
    assert "start 0: %d cells" % plan["paths"][0]["length"] in r.stdout and "start 3: no path" in r.stdout
