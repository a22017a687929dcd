"""svoslam_pool_count_boxes and svoslam_pool_nearest_occupied on the device: every output field, `steps` included, equals the host
restatement of the specification (tests/test_volume_cpu.py: count_boxes_words, nearest_occupied_words) applied to the pool's own
words -- never a second device result alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_query import fused_pool, same
from test_query_cpu import F, plane
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE
from test_volume_cpu import (BOX_FIELDS, CASES, NEAR_FIELDS, check_expected, count_boxes_words, morton, nearest_occupied_words,
                             run_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """depth -> (pool, its words, the fused points): fused on the device, twice, shared by the tests below and left unchanged"""
    pkg, torch = env
    out = {}
    for depth in (6, 9):
        ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 41)
        out[depth] = (pool, pool.words(), pts, ws)
    return out


def mixed_boxes(n, depth, pts, max_cells=8):
    """seeded boxes of 1 .. max_cells cells a side, half of them about fused points, with thin columns of the whole height, faces
    on lattice planes, boxes that poke out of the root, and empty ones (NaN, inverted, outside) mixed in: lanes that do nothing
    beside lanes with long walks in one wavefront.  (The sizes keep the longest walk at some hundreds of steps: the host
    restatement pays milliseconds for each.)"""
    rng = np.random.default_rng(100 + n)
    n_side = 1 << depth
    cell = 2.0 * EDGE / n_side
    h = F(EDGE) / F(n_side)
    c = np.asarray(CENTER)
    mid_ = c + (rng.random((n, 3)) * 2 - 1) * EDGE * 1.05
    near = np.arange(0, n, 2)
    mid_[near] = pts[(near * 7) % pts.shape[0]] + rng.normal(scale=cell, size=(near.size, 3))
    side = cell * max_cells ** rng.random((n, 3))
    for k in range(0, n, 7):
        side[k] = cell * (1.0 + rng.random(3))                                # a column is one to three cells wide
    b = np.concatenate([mid_ - side / 2, mid_ + side / 2], 1).astype(F)
    for k in range(0, n, 7):
        a = (k // 7) % 3
        b[k, a], b[k, 3 + a] = -np.inf, np.inf                                # a column through the whole root
    for k in range(3, n, 11):
        a = (k // 11) % 3
        j = int(np.clip(np.rint((float(b[k, a + 3 * (k % 2)]) - (CENTER[a] - EDGE)) / cell), 0, n_side)) if k % 4 else (k * 5) % (n_side + 1)
        b[k, a + 3 * (k % 2)] = plane(CENTER[a], j, n_side, h)               # a face ON a lattice plane: mostly the nearest, some anywhere
    for k in range(5, n, 13):
        b[k, (k // 13) % 6] = np.nan
    for k in range(6, n, 17):
        a = (k // 17) % 3
        b[k, a], b[k, 3 + a] = b[k, 3 + a], b[k, a]                           # inverted (or a point-box, where the two are equal)
    for k in range(9, n, 19):
        a = (k // 19) % 3
        b[k, a], b[k, 3 + a] = (5.0, np.inf) if k % 2 else (-np.inf, -5.0)    # outside the root
    return b


def mixed_points(n, depth, pts, anywhere=32):
    """fused points moved by up to 3 cells per axis, every fourth by up to 12 cells; every 32nd point (`anywhere`) anywhere in a cube a little
    larger than the root (some outside it: those are the long walks, and the host restatement pays milliseconds per step); points
    on lattice planes and root faces, NaN and infinite ones mixed in"""
    rng = np.random.default_rng(200 + n)
    n_side = 1 << depth
    cell = 2.0 * EDGE / n_side
    h = F(EDGE) / F(n_side)
    reach = np.where(np.arange(n) % 4 == 1, 12.0, 3.0)[:, None]
    p = pts[(np.arange(n) * 5) % pts.shape[0]] + (rng.random((n, 3)) * 2 - 1) * reach * cell
    far = np.arange(2 % anywhere, n, anywhere)
    p[far] = np.asarray(CENTER) + (rng.random((far.size, 3)) * 2 - 1) * EDGE * 1.05
    p = p.astype(F)
    for k in range(3, n, 11):
        a = (k // 11) % 3
        p[k, a] = plane(CENTER[a], (k * 5) % (n_side + 1), n_side, h)
    for k in range(5, n, 13):
        p[k, (k // 13) % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    return p


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    case = CASES[name]
    kind, words, depth = case[:3]
    pool = pkg.Pool()
    pool.set_words(words)

    def boxes(_, d, center, edge, inputs, stop_after):
        return pkg.count_boxes(pool, d, center, edge, inputs, stop_after)

    def points(_, d, center, edge, inputs, radius):
        return pkg.nearest_occupied(pool, d, center, edge, inputs, radius)
    fields = BOX_FIELDS if kind == "boxes" else NEAR_FIELDS
    got = run_case(case, boxes, points)
    check_expected(got, case[5])
    same(got, run_case(case, count_boxes_words, nearest_occupied_words), fields)
    if depth > 1:                                                  # the level above, from the same words
        same(run_case(case, boxes, points, depth - 1), run_case(case, count_boxes_words, nearest_occupied_words, depth - 1), fields)


N_MOST = 4099


def fused_inputs(depth, pts, radius=None):
    """the N_MOST boxes or (radius given) points every size of test_fused_cloud takes its first n of.  A walk starts at the corner
    of its range, so with radius 64 every point inside the root walks hundreds of blocks before it comes near itself: there eleven
    points of twelve are moved out of the root -- idle lanes beside the long walks, and a host restatement that stays affordable"""
    if radius is None:
        return mixed_boxes(N_MOST, depth, pts)
    p = mixed_points(N_MOST, depth, pts)
    if radius == 64:
        p[np.arange(N_MOST) % 12 != 2, 1] = F(CENTER[1] + 1.5 * EDGE)
    return p


@pytest.fixture(scope="module")
def reference(fused):
    """(depth, d, "boxes" | "points", stop_after | radius) -> the restatement's result for all N_MOST entries, computed once: entries
    do not depend on each other, so the first n of it are the result for the first n inputs"""
    cache = {}

    def get(depth, d, kind, param):
        key = (depth, d, kind, param)
        if key not in cache:
            _, words, pts, _ = fused[depth]
            if kind == "boxes":
                cache[key] = count_boxes_words(words, d, CENTER, EDGE, fused_inputs(depth, pts), param)
            else:
                cache[key] = nearest_occupied_words(words, d, CENTER, EDGE, fused_inputs(depth, pts, param), param)
        return cache[key]
    return get


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, N_MOST])
@pytest.mark.parametrize("depth", [6, 9])
def test_fused_cloud(env, fused, reference, depth, n):
    pkg, torch = env
    pool, words, pts, _ = fused[depth]
    boxes = fused_inputs(depth, pts)[:n]
    for d in (depth, depth - 2):
        for stop in (0, 1, 5):
            want = reference(depth, d, "boxes", stop)
            if n == N_MOST and stop == 0:
                # the batch itself (the restatement's result, not the device's): long walks beside idle lanes, more non-trivial
                # entries than one workgroup has lanes, and boxes that count something beside boxes that count nothing
                assert int(want["steps"].max()) > 64 and (want["steps"] > 0).sum() > 256 and (want["steps"] == 0).sum() > 256
                assert (want["count"] > 0).sum() > 256 and ((want["count"] == 0) & (want["steps"] > 0)).sum() > 256
            same(pkg.count_boxes(pool, d, CENTER, EDGE, boxes, stop), {k: v[:n] for k, v in want.items()}, BOX_FIELDS)
        for radius in (0, 5, 64):
            want = reference(depth, d, "points", radius)
            if n == N_MOST and radius >= 5:
                assert int(want["steps"].max()) > 64 and (want["steps"] > 1).sum() > 256 and (want["dist2"] == -2).sum() > 256
                assert (want["dist2"] >= 0).sum() > 256 and (want["dist2"] > 0).sum() > 64
            points = fused_inputs(depth, pts, radius)[:n]
            same(pkg.nearest_occupied(pool, d, CENTER, EDGE, points, radius), {k: v[:n] for k, v in want.items()}, NEAR_FIELDS)


def test_every_subset_of_outputs_and_tensors(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    boxes, points = mixed_boxes(257, 6, pts), mixed_points(257, 6, pts)
    want = count_boxes_words(words, 6, CENTER, EDGE, boxes, 3)
    for r in range(0, len(BOX_FIELDS) + 1):
        for names in itertools.combinations(BOX_FIELDS, r):
            same(pkg.count_boxes(pool, 6, CENTER, EDGE, boxes, 3, outputs=names), {k: want[k] for k in names}, names)
    wantp = nearest_occupied_words(words, 6, CENTER, EDGE, points, 7)
    for r in range(0, len(NEAR_FIELDS) + 1):
        for names in itertools.combinations(NEAR_FIELDS, r):
            same(pkg.nearest_occupied(pool, 6, CENTER, EDGE, points, 7, outputs=names), {k: wantp[k] for k in names}, names)
    # cuda tensors in, cuda tensors out: the same bits
    got = pkg.count_boxes(pool, 6, CENTER, EDGE, torch.from_numpy(boxes).cuda(), 3)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    same({k: v.cpu().numpy().view(want[k].dtype) for k, v in got.items()}, want, BOX_FIELDS)
    got = pkg.nearest_occupied(pool, 6, CENTER, EDGE, torch.from_numpy(points).cuda(), 7)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    same({k: v.cpu().numpy().view(wantp[k].dtype) for k, v in got.items()}, wantp, NEAR_FIELDS)


def test_depth_16_cells_beyond_15_bits_and_codes_beyond_32(env):
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 16, 2000, 43)
    words = pool.words()
    boxes, points = mixed_boxes(513, 16, pts, max_cells=6), mixed_points(513, 16, pts)
    want = count_boxes_words(words, 16, CENTER, EDGE, boxes)
    found = want["count"] > 0
    xyz = np.stack([(want["first_cell"][found] >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32)], 1).astype(np.int64)
    assert found.sum() > 50 and int(xyz.max()) >= 1 << 15 and int(morton(xyz[:, 0], xyz[:, 1], xyz[:, 2], 16).max()) >= 1 << 32
    same(pkg.count_boxes(pool, 16, CENTER, EDGE, boxes), want, BOX_FIELDS)
    wantp = nearest_occupied_words(words, 16, CENTER, EDGE, points, 5)
    near = wantp["dist2"] >= 0
    assert near.sum() > 50 and (wantp["dist2"] > 0).sum() > 20 and int((wantp["cell"][near] & np.uint64(0xFFFF)).max()) >= 1 << 15
    same(pkg.nearest_occupied(pool, 16, CENTER, EDGE, points, 5), wantp, NEAR_FIELDS)


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    pool = pkg.Pool()
    pool.set_words(hp.words())
    pts = np.asarray(CENTER, F)[None, :] + np.array([[0.5, 0.5, -0.5], [-0.5, -0.5, 0.5]], F)
    boxes, points = mixed_boxes(257, 1, pts, max_cells=2), mixed_points(257, 1, pts, anywhere=1)   # 3 cells from a point is outside
    want = count_boxes_words(hp.words(), 1, CENTER, EDGE, boxes)
    assert (want["count"] > 0).sum() > 20 and (want["count"] == 2).sum() > 0
    same(pkg.count_boxes(pool, 1, CENTER, EDGE, boxes), want, BOX_FIELDS)
    for radius in (0, 1):
        wantp = nearest_occupied_words(hp.words(), 1, CENTER, EDGE, points, radius)
        assert (wantp["dist2"] == 0).sum() > 20
        same(pkg.nearest_occupied(pool, 1, CENTER, EDGE, points, radius), wantp, NEAR_FIELDS)


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    boxes, points = mixed_boxes(1001, depth, pts), mixed_points(1001, depth, pts)
    unsynced = pkg.count_boxes(pool, depth, CENTER, EDGE, boxes)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    unsynced_p = pkg.nearest_occupied(pool, depth, CENTER, EDGE, points, 9)
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    same(pkg.count_boxes(pool, depth, CENTER, EDGE, boxes), unsynced, BOX_FIELDS)
    same(unsynced, count_boxes_words(words, depth, CENTER, EDGE, boxes), BOX_FIELDS)
    same(pkg.nearest_occupied(pool, depth, CENTER, EDGE, points, 9), unsynced_p, NEAR_FIELDS)
    same(unsynced_p, nearest_occupied_words(words, depth, CENTER, EDGE, points, 9), NEAR_FIELDS)


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    pool = pkg.Pool()
    L = pkg.lib()
    got = pkg.count_boxes(pool, 5, CENTER, EDGE, np.zeros((0, 6), F))
    assert set(got) == set(BOX_FIELDS) and all(v.shape == (0,) for v in got.values())
    got = pkg.nearest_occupied(pool, 5, CENTER, EDGE, np.zeros((0, 3), F), 4)
    assert set(got) == set(NEAR_FIELDS) and all(v.shape == (0,) for v in got.values())
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    null, ptr, ctr = C.c_void_p(0), pkg._ptr(buf), pkg._fa(CENTER, 3)

    def count(pool_ref=C.byref(pool._p), depth=5, edge=1.0, inputs=ptr, n=4, stop_after=0):
        return L.svoslam_pool_count_boxes(pool_ref, depth, ctr, edge, inputs, stop_after, n, null, null, null, null, pkg._stream())

    def near(pool_ref=C.byref(pool._p), depth=5, edge=1.0, inputs=ptr, n=4, radius=3):
        return L.svoslam_pool_nearest_occupied(pool_ref, depth, ctr, edge, inputs, radius, n, null, null, null, null, null, pkg._stream())
    for call in (count, near):
        assert call() == 0 and call(n=0) == 0 and call(None, n=0) == 0
        assert call(None) == -1 and call(n=-1) == -1 and call(depth=0) == -1 and call(depth=17) == -1
        assert call(edge=0.0) == -1 and call(edge=-1.0) == -1 and call(edge=float("nan")) == -1
        assert call(inputs=null) == -1 and call(inputs=null, n=0) == 0
    assert count(stop_after=-7) == 0 and count(stop_after=1 << 40) == 0
    assert near(radius=0) == 0 and near(radius=4096) == 0
    assert near(radius=-1) == -1 and near(radius=4097) == -1 and near(radius=4097, n=0) == -1 and near(radius=-1, n=0) == -1
    with pytest.raises(Exception):
        pkg.nearest_occupied(pool, 5, CENTER, EDGE, np.zeros((2, 3), F), 4097)
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_launch(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    boxes, points = mixed_boxes(257, 6, pts), mixed_points(257, 6, pts)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.count_boxes(pool, 6, CENTER, EDGE, boxes)
        pkg.count_boxes(pool, 4, CENTER, EDGE, boxes, 1)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.nearest_occupied(pool, 6, CENTER, EDGE, points, 5)
        pkg.count_boxes(pool, 6, CENTER, EDGE, np.zeros((0, 6), F))        # nothing is launched, nothing is bracketed
        pkg.nearest_occupied(pool, 6, CENTER, EDGE, np.zeros((0, 3), F), 5)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
    finally:
        pkg.stage_timing([])
