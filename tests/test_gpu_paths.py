"""svoslam_field_segment_clearance and svoslam_field_shorten_paths on the device: every value equals the host restatements of the
specification (tests/test_paths_cpu.py: segment_clearance_ref, the walk cell by cell, and shorten_path_ref, every j of the window
tried) -- on fields the device's own distance_field produced and on paths its own trace_paths produced, each first proven equal
to its own restatement.  Exact integers, no tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable
from test_gpu_field import case_region, same_field
from test_gpu_query import fused_pool
from test_paths_cpu import (LOOKAHEADS, SEGMENT_CASES, SHORTEN_CASES, PINNED, TWO_ROUTES_WAYPOINTS, segment_clearance_ref, shorten_first_failure,
                            shorten_path_ref, world_path, world_vertices)
from test_plan_cpu import WORLD_DEPTH, ramp, trace_path, world
from test_surface_cpu import CENTER, EDGE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -6


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


def same_clearance(pkg, field, origin, dims, segments):
    """the device's minimum and first attaining cell of every segment equal segment_clearance_ref's"""
    segments = np.asarray(segments, np.int64).reshape(-1, 6)
    low, at = pkg.segment_clearance(field, origin, dims, segments.astype(np.int32), want_cell=True)
    assert low.dtype == np.int32 and at.dtype == np.int32 and low.shape == (segments.shape[0],) and at.shape == (segments.shape[0], 3)
    for k, s in enumerate(segments.tolist()):
        want = segment_clearance_ref(field, origin, s[:3], s[3:])
        assert (int(low[k]), tuple(at[k].tolist())) == want, (k, s, int(low[k]), at[k].tolist(), want)
    assert np.array_equal(pkg.segment_clearance(field, origin, dims, segments.astype(np.int32)), low)    # d_at NULL
    return low, at


def stored_cells(paths, lengths, k):
    """the cells of path k the call uses: the first min(|length|, max_cells)"""
    return [tuple(c) for c in paths[k, :min(abs(int(lengths[k])), paths.shape[1])].tolist()]


def same_vertices(pkg, field, origin, dims, r, paths, lengths, lookahead):
    """the device's vertices and counts of every path equal shorten_path_ref's, and nothing behind a path's vertices was written"""
    vertices, counts = pkg.shorten_paths(field, origin, dims, r, paths, lengths, max_lookahead=lookahead)
    n = paths.shape[0]
    assert vertices.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (n,)
    assert vertices.shape == (n, int(counts.max()) if n else 0)
    for k in range(n):
        want = shorten_path_ref(field, origin, r, stored_cells(paths, lengths, k), lookahead)
        assert int(counts[k]) == len(want) and vertices[k, :len(want)].tolist() == want, (k, lookahead, vertices[k].tolist(), want)
        assert (vertices[k, len(want):] == -1).all()
    return vertices, counts


def random_segments(rng, origin, dims, count, margin=2):
    o, n = np.asarray(origin), np.asarray(dims)
    return np.concatenate([rng.integers(-margin, n + margin, (count, 3)) + o, rng.integers(-margin, n + margin, (count, 3)) + o], 1)


# ---- segment_clearance ---------------------------------------------------------------------------------------------------------
def test_segment_hand_cases(env):
    pkg, torch = env
    for k, (field, origin, a, b, low, at) in enumerate(SEGMENT_CASES):
        dims = field.shape[::-1]
        got, cell = pkg.segment_clearance(field, origin, dims, [list(a) + list(b)], want_cell=True)
        assert (int(got[0]), tuple(cell[0].tolist())) == (low, at), (k, a, b)
    # all of one field's cases in one call
    same = [c for c in SEGMENT_CASES if np.array_equal(c[0], SEGMENT_CASES[-2][0])]
    assert len(same) >= 5
    got, cell = pkg.segment_clearance(same[0][0], same[0][1], same[0][0].shape[::-1], [list(c[2]) + list(c[3]) for c in same], want_cell=True)
    assert got.tolist() == [c[4] for c in same] and [tuple(c) for c in cell.tolist()] == [c[5] for c in same]


def test_every_ordered_pair_of_a_small_region(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = case_region(words, 6, (6, 5, 4), "pt", 3)
    field = pkg.distance_field(ws, pool, 6, origin, dims, 3)
    same_field(field, distance_field_separable(words, 6, origin, dims, 3))
    assert (field == 0).sum() > 0 and (field > 0).sum() > 10            # decided on the restatement's equal
    cells = [(origin[0] + x, origin[1] + y, origin[2] + z) for z in range(dims[2]) for y in range(dims[1]) for x in range(dims[0])]
    low, at = same_clearance(pkg, field, origin, dims, [a + b for a in cells for b in cells])
    assert len(set(low.tolist())) > 3 and (low > 0).sum() > 200


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_segment_counts(env, fused, count):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = case_region(words, 6, (20, 9, 7), "pt", 4)
    field = pkg.distance_field(ws, pool, 6, origin, dims, 4)
    same_field(field, distance_field_separable(words, 6, origin, dims, 4))
    low, at = same_clearance(pkg, field, origin, dims, random_segments(np.random.default_rng(count), origin, dims, count))
    if count >= 63:
        assert (low == 0).any() and (low != 0).any()


def test_long_segments(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[9]
    origin, dims = case_region(words, 9, (200, 3, 2), "pt", 6)
    field = pkg.distance_field(ws, pool, 9, origin, dims, 6)
    same_field(field, distance_field_separable(words, 9, origin, dims, 6))
    rng = np.random.default_rng(2)
    segments = random_segments(rng, origin, dims, 120, margin=0)
    ends = [[origin[0], origin[1] + y0, origin[2] + z0, origin[0] + 199, origin[1] + y1, origin[2] + z1]
            for y0 in range(3) for y1 in range(3) for z0 in range(2) for z1 in range(2)]
    low, at = same_clearance(pkg, field, origin, dims, np.concatenate([segments, np.array(ends), np.array(ends)[:, [3, 4, 5, 0, 1, 2]]]))
    assert (np.abs(segments[:, 3] - segments[:, 0]) > 128).sum() > 10 and len(set(low.tolist())) > 3
    # tensors in, tensors out
    t_low, t_at = pkg.segment_clearance(torch.from_numpy(field).cuda(), origin, dims, torch.tensor(ends, dtype=torch.int32, device="cuda"),
                                        want_cell=True, as_tensor=True)
    assert isinstance(t_low, torch.Tensor) and t_low.is_cuda and t_low.dtype == torch.int32 and tuple(t_at.shape) == (len(ends), 3)
    assert np.array_equal(t_low.cpu().numpy(), low[120:120 + len(ends)]) and np.array_equal(t_at.cpu().numpy(), at[120:120 + len(ends)])
    only = pkg.segment_clearance(torch.from_numpy(field).cuda(), origin, dims, ends, as_tensor=True)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), t_low.cpu().numpy())
    with pytest.raises(ValueError):
        pkg.segment_clearance(torch.zeros((2, 3, 200), dtype=torch.int64, device="cuda"), origin, dims, ends)
    with pytest.raises(ValueError):
        pkg.segment_clearance(field, origin, (200, 3, 1), ends)


# ---- shorten_paths -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHORTEN_CASES))
def test_shorten_hand_cases(env, name):
    pkg, torch = env
    field, origin, r, cells, lookahead, want = SHORTEN_CASES[name]
    want = PINNED[name] if want is None else want
    dims = field.shape[::-1]
    paths = np.asarray(cells, np.int32).reshape(1, -1, 3)
    vertices, counts = same_vertices(pkg, field, origin, dims, r, paths, np.array([len(cells)], np.int32), lookahead)
    assert vertices[0].tolist() == want and counts.tolist() == [len(want)]


def world_on_the_device(pkg, name):
    """-> (the device's distance field with the comfort radius, paths, lengths) of a world of tests/test_plan_cpu.py: the weighted
    and the reach path from the world's start (the serpentine: from its dearest cell), each equal to its restatement"""
    w = world(name)
    o, dims, r, R = w["origin"], w["dims"], w["clearance"], w["comfort"]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(w["words"])
    field = pkg.distance_field(ws, pool, WORLD_DEPTH, o, dims, R)
    same_field(field, w["field"])
    heavy, light = world_path(name, "weighted"), world_path(name, "reach")
    cost = pkg.cost_field(ws, pool, WORLD_DEPTH, o, dims, r, R, w["ring"], [w["seed"]])
    steps = pkg.reach_field(ws, pool, WORLD_DEPTH, o, dims, r, [w["seed"]])
    room = len(heavy) + 2
    paths, lengths = pkg.trace_paths(cost, o, dims, [heavy[0]], room)
    paths2, lengths2 = pkg.trace_paths(steps, o, dims, [heavy[0]], room)
    assert lengths.tolist() == [len(heavy)] and [tuple(c) for c in paths[0, :len(heavy)].tolist()] == heavy
    assert lengths2.tolist() == [len(light)] and [tuple(c) for c in paths2[0, :len(light)].tolist()] == light
    return field, np.concatenate([paths, paths2]), np.concatenate([lengths, lengths2])


@pytest.mark.parametrize("name", ["two_routes", "serpentine"])
def test_the_worlds(env, name):
    pkg, torch = env
    w = world(name)
    field, paths, lengths = world_on_the_device(pkg, name)
    heavy = world_path(name, "weighted")
    for lookahead in LOOKAHEADS:
        vertices, counts = pkg.shorten_paths(field, w["origin"], w["dims"], w["clearance"], paths, lengths, max_lookahead=lookahead)
        # (the serpentine's reach path is much like its weighted one: the restatement's seconds go to the weighted path alone)
        for k, which in enumerate(("weighted", "reach") if name == "two_routes" else ("weighted",)):
            want = world_vertices(name, which, lookahead)[0]
            assert int(counts[k]) == len(want) and vertices[k, :len(want)].tolist() == want, (which, lookahead)
    vertices, counts = pkg.shorten_paths(field, w["origin"], w["dims"], w["clearance"], paths, lengths)
    if name == "two_routes":
        assert [heavy[v] for v in vertices[0, :counts[0]]] == TWO_ROUTES_WAYPOINTS and counts.tolist() == [6, 2]
        # not "scan until the first failure": that gives another result here
        wrong = shorten_first_failure(field, w["origin"], w["clearance"], heavy, 0)
        assert wrong != vertices[0, :counts[0]].tolist()
        # against the field truncated to the clearance radius: plain line of sight, one segment through the tunnel
        near = np.where((field >= 0) & (field <= w["clearance"] ** 2), field, -1).astype(np.int32)
        plain, n = pkg.shorten_paths(near, w["origin"], w["dims"], w["clearance"], paths, lengths)
        assert n.tolist() == [2, 2] and plain[0].tolist() == [0, 216]
    else:
        assert counts[0] == 20


@pytest.mark.parametrize("cells", [1, 2, 3, 65, 66, 67, 129, 130])
def test_path_lengths_about_the_batch_edges(env, cells):
    """the serpentine's path cut by max_cells: the length says 894, the stored prefix is what is shortened"""
    pkg, torch = env
    w = world("serpentine")
    heavy = world_path("serpentine", "weighted")
    paths = np.asarray(heavy[:cells], np.int32).reshape(1, cells, 3)
    lengths = np.array([len(heavy)], np.int32)
    for lookahead in (0, 64):
        vertices, counts = same_vertices(pkg, w["field"], w["origin"], w["dims"], w["clearance"], paths, lengths, lookahead)
        assert vertices[0, 0] == 0 and vertices[0, counts[0] - 1] == cells - 1


@pytest.fixture(scope="module")
def many_paths(env, fused):
    """257 traced paths on a region of the depth-6 pool, some of length 0, some lengths negated as a stopped walk's are: (field,
    origin, dims, clearance, paths, lengths, the restatement's vertices per path)"""
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    r, R = 1, 3
    origin, dims = case_region(words, 6, (40, 24, 8), "pt", R)
    field = pkg.distance_field(ws, pool, 6, origin, dims, R)
    same_field(field, distance_field_separable(words, 6, origin, dims, R))
    free = np.argwhere((field < 0) | (field > r * r))[:, ::-1] + np.asarray(origin)
    rng = np.random.default_rng(9)
    cost = pkg.cost_field(ws, pool, 6, origin, dims, r, R, [6, 2], [free[rng.integers(free.shape[0])].tolist()])
    reached, blocked = np.argwhere(cost >= 0)[:, ::-1] + np.asarray(origin), np.argwhere(cost == -2)[:, ::-1] + np.asarray(origin)
    assert reached.shape[0] >= 237 and blocked.shape[0] >= 10
    starts = np.concatenate([reached[rng.choice(reached.shape[0], 237, replace=False)], blocked[:10], np.array([[origin[0] + 40, origin[1], origin[2]]] * 10)])
    starts = starts[rng.permutation(257)]
    paths, lengths = pkg.trace_paths(cost, origin, dims, starts, int(cost.max()) + 1)
    for k in range(0, 257, 16):                                         # a sample: the trace has its own tests
        cells, length = trace_path(cost, origin, starts[k], paths.shape[1])
        assert int(lengths[k]) == length and np.array_equal(paths[k, :cells.shape[0]], cells)
    lengths = lengths.copy()
    lengths[::5] = -lengths[::5]
    assert (lengths == 0).sum() == 20 and (lengths < 0).sum() > 30 and lengths.max() > 20
    want = [shorten_path_ref(field, origin, r, stored_cells(paths, lengths, k), 0) for k in range(257)]
    return field, origin, dims, r, paths, lengths, want


def test_many_paths_in_one_call(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, paths, lengths, want = many_paths
    vertices, counts = pkg.shorten_paths(field, origin, dims, r, paths, lengths)
    assert counts.tolist() == [len(v) for v in want]
    for k in range(257):
        assert vertices[k, :len(want[k])].tolist() == want[k] and (vertices[k, len(want[k]):] == -1).all(), k
    assert sum(len(v) > 2 for v in want) > 50 and sum(len(v) == 0 for v in want) == 20
    assert sum(len(v) < abs(int(n)) for v, n in zip(want, lengths)) > 150          # most paths were shortened
    for k in (3, 255):                                                  # one path in a call
        one, n = pkg.shorten_paths(field, origin, dims, r, paths[k:k + 1], lengths[k:k + 1])
        assert n.tolist() == [len(want[k])] and one[0].tolist() == want[k]
    same_vertices(pkg, field, origin, dims, r, paths[:70], lengths[:70], 7)
    # tensors in, tensors out
    t = [torch.from_numpy(a).cuda() for a in (field, paths, lengths)]
    tv, tn = pkg.shorten_paths(t[0], origin, dims, r, t[1], t[2], as_tensor=True)
    assert isinstance(tv, torch.Tensor) and tv.is_cuda and tv.dtype == torch.int32 and isinstance(tn, torch.Tensor)
    assert np.array_equal(tv.cpu().numpy(), vertices) and np.array_equal(tn.cpu().numpy(), counts)
    with pytest.raises(ValueError):
        pkg.shorten_paths(field, origin, dims, r, paths[:, :, :2], lengths)
    with pytest.raises(ValueError):
        pkg.shorten_paths(field, origin, dims, r, t[1].to(torch.int64), t[2])


def test_max_vertices(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, paths, lengths, want = many_paths
    L = pkg.lib()
    t_field, t_paths, t_lengths = (torch.from_numpy(a).cuda() for a in (field, paths, lengths))
    o3, n3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
    counts = torch.full((257,), -77, dtype=torch.int32, device="cuda")
    # 0 with a NULL buffer: the counts alone
    assert L.svoslam_field_shorten_paths(pkg._ptr(t_field), o3, n3, r, pkg._ptr(t_paths), pkg._ptr(t_lengths), 257, paths.shape[1], 0, 0, None,
                                         pkg._ptr(counts), pkg._stream()) == 0
    assert counts.tolist() == [len(v) for v in want]
    # shorter than the counts: the first three, the whole count, the rest of a sentinel-filled buffer untouched
    buf = torch.full((257, 5), -77, dtype=torch.int32, device="cuda")
    counts.fill_(-77)
    assert L.svoslam_field_shorten_paths(pkg._ptr(t_field), o3, n3, r, pkg._ptr(t_paths), pkg._ptr(t_lengths), 257, paths.shape[1], 0, 3,
                                         pkg._ptr(buf), pkg._ptr(counts), pkg._stream()) == 0
    assert counts.tolist() == [len(v) for v in want] and sum(len(v) > 3 for v in want) > 20
    flat = buf.cpu().numpy().reshape(-1)                                # rows of 3 in a buffer of 257 * 5
    for k in range(257):
        kept = min(len(want[k]), 3)
        assert flat[3 * k:3 * k + kept].tolist() == want[k][:kept] and (flat[3 * k + kept:3 * k + 3] == -77).all(), k
    assert (flat[257 * 3:] == -77).all()
    short, n = pkg.shorten_paths(field, origin, dims, r, paths, lengths, max_vertices=2)
    assert short.shape == (257, 2) and n.tolist() == [len(v) for v in want]
    assert all(short[k, :min(len(want[k]), 2)].tolist() == want[k][:2] for k in range(257))


# (fused depth, d, (nx, ny, nz), origin x: "lo" 0 | "in" 37 | "hi" N - nx, clearance, comfort): nx 1, 63, 64, 65, 130
FUSED_CASES = [
    (9, 9, (130, 9, 7), "in", 0, 2), (9, 9, (65, 17, 9), "hi", 1, 4), (9, 9, (64, 17, 8), "lo", 1, 3), (9, 9, (63, 7, 17), "in", 0, 2),
    (9, 7, (130, 8, 8), "lo", 0, 2), (9, 7, (64, 9, 17), "in", 1, 4), (9, 7, (1, 7, 9), "hi", 0, 2), (9, 7, (65, 17, 3), "hi", 1, 3),
    (6, 6, (63, 8, 17), "lo", 1, 3), (6, 6, (64, 17, 1), "hi", 1, 4), (6, 6, (1, 9, 7), "in", 0, 2), (6, 4, (16, 16, 16), "lo", 0, 2),
    (6, 4, (5, 1, 8), "in", 0, 2),
]


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-r%d-R%d" % (c[0], c[1], *c[2], *c[3:]))
def test_fused_cloud(env, fused, case):
    pkg, torch = env
    depth, d, shape, where, r, R = case
    pool, words, pts, ws = fused[depth]
    origin, dims = case_region(words, d, shape, where, R)
    field = pkg.distance_field(ws, pool, d, origin, dims, R)
    same_field(field, distance_field_separable(words, d, origin, dims, R))
    free = np.argwhere((field < 0) | (field > r * r))[:, ::-1] + np.asarray(origin)
    assert free.shape[0] > 0
    rng = np.random.default_rng(FUSED_CASES.index(case))
    cost = pkg.cost_field(ws, pool, d, origin, dims, r, R, ramp(r, R, 4), [free[rng.integers(free.shape[0])].tolist()])
    reached = np.argwhere(cost >= 0)[:, ::-1] + np.asarray(origin)
    starts = reached[rng.choice(reached.shape[0], min(9, reached.shape[0]), replace=False)].tolist()
    starts.append((np.array(np.unravel_index(np.argmax(cost), cost.shape)[::-1]) + np.asarray(origin)).tolist())
    paths, lengths = pkg.trace_paths(cost, origin, dims, starts, int(cost.max()) + 1)
    for k, start in enumerate(starts):
        cells, length = trace_path(cost, origin, start, paths.shape[1])
        assert int(lengths[k]) == length and np.array_equal(paths[k, :cells.shape[0]], cells)
    for lookahead in (0, 7):
        same_vertices(pkg, field, origin, dims, r, paths, lengths, lookahead)
    same_clearance(pkg, field, origin, dims, random_segments(rng, origin, dims, 40))


# ---- around the calls ------------------------------------------------------------------------------------------------------------
def test_the_other_results_are_unchanged_around_the_calls(env, fused, many_paths):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    field, origin, dims, r, paths, lengths, want = many_paths
    seeds = [[origin[a] + v for a, v in enumerate(c)] for c in ((3, 1, 6), (30, 20, 5))]
    starts = [[origin[a] + v for a, v in enumerate(c)] for c in ((10, 10, 3), (30, 20, 6))]

    def others():
        cost = pkg.cost_field(ws, pool, 6, origin, dims, 1, 3, [6, 2], seeds)
        return pkg.distance_field(ws, pool, 6, origin, dims, 3), cost, pkg.trace_paths(cost, origin, dims, starts, 200)
    before = others()
    pkg.shorten_paths(field, origin, dims, r, paths, lengths)
    pkg.segment_clearance(field, origin, dims, random_segments(np.random.default_rng(1), origin, dims, 100), want_cell=True)
    after = others()
    same_field(after[0], before[0])
    same_field(after[1], before[1])
    same_field(after[0], field)
    assert np.array_equal(after[2][0], before[2][0]) and np.array_equal(after[2][1], before[2][1])


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    L = pkg.lib()
    field = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    segments = torch.tensor([[0, 0, 0, 3, 3, 3], [1, 1, 1, 1, 1, 1]], dtype=torch.int32, device="cuda")
    low = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    at = torch.full((2, 3), -77, dtype=torch.int32, device="cuda")
    paths = torch.tensor([[[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0]], [[3, 3, 3], [3, 3, 2], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([4, 2], dtype=torch.int32, device="cuda")
    vertices = torch.full((2, 4), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    null = C.c_void_p(0)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def clear(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), s=pkg._ptr(segments), n=2, out=pkg._ptr(low), cell=pkg._ptr(at)):
        return L.svoslam_field_segment_clearance(f, i3(origin), i3(dims), s, n, out, cell, pkg._stream())

    def shorten(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), r=1, p=pkg._ptr(paths), ln=pkg._ptr(lengths), n=2, cap=4, look=0, room=4,
                v=pkg._ptr(vertices), out=pkg._ptr(counts)):
        return L.svoslam_field_shorten_paths(f, i3(origin), i3(dims), r, p, ln, n, cap, look, room, v, out, pkg._stream())
    # every error first: nothing is written
    assert clear(origin=None) == INVALID and clear(dims=None) == INVALID and clear(dims=(-1, 4, 4)) == INVALID and clear(dims=(4, 4, -1)) == INVALID
    assert clear(n=-1) == INVALID and clear(f=null) == INVALID and clear(s=null) == INVALID and clear(out=null) == INVALID
    assert clear(dims=(65536, 65536, 1)) == LIMIT and clear(dims=(2048, 1024, 1024)) == LIMIT and clear(dims=(65537, 1, 1)) == LIMIT
    assert clear(dims=(1, 65537, 1)) == LIMIT and clear(dims=(1, 1, 65537)) == LIMIT and clear(dims=(65536, 65536, 65536)) == LIMIT
    assert shorten(origin=None) == INVALID and shorten(dims=None) == INVALID and shorten(dims=(4, -1, 4)) == INVALID
    assert shorten(n=-1) == INVALID and shorten(cap=-1) == INVALID and shorten(look=-1) == INVALID and shorten(room=-1) == INVALID
    assert shorten(r=-1) == INVALID and shorten(r=4097) == INVALID and shorten(r=-1, n=0) == INVALID
    assert shorten(f=null) == INVALID and shorten(p=null) == INVALID and shorten(ln=null) == INVALID and shorten(v=null) == INVALID
    assert shorten(out=null) == INVALID
    assert shorten(dims=(65536, 65536, 1)) == LIMIT and shorten(dims=(65537, 1, 1)) == LIMIT and shorten(dims=(1, 1, 65537)) == LIMIT
    assert shorten(n=1 << 20, cap=1 << 10) == LIMIT and shorten(n=(1 << 31) - 1, cap=(1 << 31) - 1) == LIMIT
    assert shorten(n=1 << 20, cap=4, room=1 << 12) == LIMIT and shorten(n=(1 << 31) - 1, cap=0, room=2) == LIMIT
    for t in (low, at, vertices, counts):
        assert (t == -77).all()
    # nothing to do
    assert clear(n=0, s=null, out=null, cell=null, f=null) == 0 and shorten(n=0, f=null, p=null, ln=null, v=null, out=null) == 0
    assert (low == -77).all() and (counts == -77).all()
    # the calls themselves: an all -1 field
    assert clear() == 0 and low.tolist() == [-1, -1] and at.tolist() == [[0, 0, 0], [1, 1, 1]]
    assert clear(cell=null) == 0 and clear(dims=(65536, 1, 1), f=pkg._ptr(torch.zeros(65536, dtype=torch.int32, device="cuda"))) == 0
    assert shorten() == 0 and counts.tolist() == [2, 2] and vertices.tolist() == [[0, 3, -77, -77], [0, 1, -77, -77]]
    assert shorten(r=4096) == 0 and shorten(r=0) == 0 and shorten(look=1 << 30) == 0 and counts.tolist() == [2, 2]
    vertices.fill_(-77)
    assert shorten(cap=0, p=null) == 0 and counts.tolist() == [0, 0] and shorten(room=0, v=null) == 0 and counts.tolist() == [2, 2]
    assert (vertices == -77).all()
    # a zero entry of dims: every cell has g = 0, only the j == a + 1 steps remain; a segment is 0 at a
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        counts.fill_(-77)
        assert shorten(dims=dims, f=null) == 0 and counts.tolist() == [4, 2] and vertices.tolist() == [[0, 1, 2, 3], [0, 1, -77, -77]]
        assert clear(dims=dims, f=null) == 0 and low.tolist() == [0, 0] and at.tolist() == [[0, 0, 0], [1, 1, 1]]
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, paths, lengths, want = many_paths
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.segment_clearance(field, origin, dims, [[0, 0, 0, 5, 5, 5]])
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
        pkg.shorten_paths(field, origin, dims, r, paths, lengths, max_vertices=4)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
        pkg.shorten_paths(field, origin, dims, r, paths, lengths)      # two passes: two calls
        assert pkg.stage_timing_read(pkg.STAGE_QUERY)[1] == 2
        pkg.segment_clearance(field, origin, dims, np.zeros((0, 6), np.int32))          # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            pkg.shorten_paths(field, origin, dims, 4097, paths, lengths, max_vertices=4)   # refused: not bracketed either
        assert pkg.stage_timing_read(pkg.STAGE_QUERY)[1] == 0
    finally:
        pkg.stage_timing([])


# ---- plan_paths and the tool -----------------------------------------------------------------------------------------------------
def test_plan_paths_straighten_then_the_map_plan_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    clearance, comfort, penalty = 1, 3, 5
    ring = ramp(clearance, comfort, penalty)
    field = distance_field_separable(words, 6, lo.tolist(), dims.tolist(), comfort)
    cell = 2.0 * EDGE / 64
    corner = np.asarray(CENTER, np.float64) - EDGE

    def centre(c):
        return (corner + (np.asarray(c, np.float64) + 0.5) * cell).tolist()
    free = np.argwhere((field < 0) | (field > clearance * clearance))[:, ::-1] + lo
    goal_cell = free[0].tolist()
    old = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), [centre(goal_cell)], clearance, comfort, ring)
    reached = np.argwhere(old["cost"] > 0)[:, ::-1] + lo
    blocked = (np.argwhere(old["cost"] == -2)[0][::-1] + lo).tolist()
    assert reached.shape[0] > 100
    far = (np.array(np.unravel_index(np.argmax(old["cost"]), old["cost"].shape)[::-1]) + lo).tolist()
    starts_m = [centre(c) for c in (far, reached[reached.shape[0] // 2].tolist(), goal_cell, blocked)] + [[100.0, 0.0, 0.0]]
    old = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m, clearance, comfort, ring)
    assert set(old["paths"][0]) == {"cell", "cost", "length", "cells", "polyline"}                  # the default: nothing new
    shortened = 0
    for lookahead in (0, 5):
        new = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m, clearance, comfort, ring, straighten=True,
                             max_lookahead=lookahead)
        assert set(new) == set(old) and np.array_equal(new["cost"], old["cost"])
        for p, q in zip(new["paths"], old["paths"]):
            assert set(p) == set(q) | {"vertices", "waypoints", "waypoint_polyline", "straight_length"}
            if q["cells"] is None:
                assert all(p[k] is None for k in p if k != "cell")
                continue
            assert all(np.array_equal(p[k], q[k]) for k in q)
            want = shorten_path_ref(field, lo.tolist(), clearance, [tuple(c) for c in p["cells"].tolist()], lookahead)
            assert p["vertices"].dtype == np.int32 and p["vertices"].tolist() == want
            assert np.array_equal(p["waypoints"], p["cells"][want]) and np.array_equal(p["waypoint_polyline"], p["polyline"][want])
            assert p["waypoint_polyline"].dtype == np.float64 and isinstance(p["straight_length"], float)
            assert p["straight_length"] == float(np.sqrt((np.diff(p["polyline"][want], axis=0) ** 2).sum(1)).sum())
            assert p["straight_length"] <= (p["length"] - 1) * cell * (1 + 1e-12)
            shortened += len(want) < p["length"]
        assert new["paths"][2]["vertices"].tolist() == [0] and new["paths"][2]["straight_length"] == 0.0
    assert shortened >= 3
    # the tool, in a child process
    ckpt = tmp_path / "map.svopool"
    pool.save(ckpt, CENTER, EDGE, 6)
    base = [sys.executable, os.path.join(ROOT, "tools", "map_plan.py"), str(ckpt), "OUT", "--clearance", str(clearance), "--comfort", str(comfort),
            "--penalty", str(penalty), "--box"] + [repr(float(v)) for v in box] + ["--goal"] + [repr(float(v)) for v in centre(goal_cell)]
    for s in starts_m:
        base += ["--start"] + [repr(float(v)) for v in s]
    cmd = list(base) + ["--straighten", "--lookahead", "5"]
    cmd[3] = str(tmp_path / "straight.npz")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(cmd[3])
    # every old key is what plan_paths gives without straightening (tests/test_gpu_plan.py holds the tool to that without the flag)
    same_field(z["cost"], old["cost"])
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and float(z["cell_size"]) == cell
    assert z["lengths"].tolist() == [q["length"] or 0 for q in old["paths"]] and z["costs"].tolist() == [-1 if q["cost"] is None else q["cost"] for q in old["paths"]]
    assert int(z["lookahead"]) == 5 and z["straight_lengths"].dtype == np.float64 and z["straight_lengths"].shape == (5,)
    stored = np.asarray(CENTER, np.float32).astype(np.float64) - EDGE   # the checkpoint keeps the centre in binary32
    device_field = pkg.distance_field(ws, pool, 6, lo, dims, comfort)
    for k, q in enumerate(old["paths"]):
        if q["cells"] is None:
            assert z["cells_%d" % k].shape == (0, 3) and z["vertices_%d" % k].shape == (0,) and z["waypoints_%d" % k].shape == (0, 3)
            assert z["waypoint_polyline_%d" % k].shape == (0, 3) and z["straight_lengths"][k] == 0.0
            continue
        assert np.array_equal(z["cells_%d" % k], q["cells"])
        assert np.array_equal(z["polyline_%d" % k], stored + (q["cells"].astype(np.float64) + 0.5) * cell)
        vertices, counts = pkg.shorten_paths(device_field, lo, dims, clearance, q["cells"][None], [q["length"]], max_lookahead=5)
        at = vertices[0, :counts[0]]
        assert z["vertices_%d" % k].dtype == np.int32 and z["vertices_%d" % k].tolist() == at.tolist()
        assert np.array_equal(z["waypoints_%d" % k], q["cells"][at])
        assert np.array_equal(z["waypoint_polyline_%d" % k], z["polyline_%d" % k][at])
        assert z["straight_lengths"][k] == float(np.sqrt((np.diff(z["polyline_%d" % k][at], axis=0) ** 2).sum(1)).sum())
    r = subprocess.run(base[:3] + [str(tmp_path / "no.npz")] + base[4:] + ["--lookahead", "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--straighten" in r.stderr
