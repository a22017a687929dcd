"""svoslam_pool_cast_rays and svoslam_pool_query_points on the device: t (as bits), node, cell, colour, steps, key and level equal
the host restatement of the specification (tests/test_query_cpu.py: cast_rays_words, query_points_words) applied to the pool's own
words -- never a second device result alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_query_cpu import (CASES, F, cast_rays_words, check_against_the_occupied_set, check_expected, plane, query_points_words,
                            seeded_rays)
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE
from util import surface_cloud

pytestmark = pytest.mark.gpu

RAY_FIELDS = ("t", "node", "cell", "color", "steps")
POINT_FIELDS = ("node", "level", "key", "color")


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def same(got, want, fields):
    assert set(got) == set(fields)
    for name in fields:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (name, bad[:5], g[bad[:5]], w[bad[:5]])


def fused_pool(pkg, torch, depth, n_points, seed, times=2):
    pts, col = surface_cloud(np.random.default_rng(seed), n_points)
    ws, pool = pkg.Workspace(), pkg.Pool()
    tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
    for _ in range(times):
        pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, CENTER, EDGE)
    return ws, pool, pts


@pytest.fixture(scope="module")
def fused(env):
    """depth -> (pool, its words, the fused points): fused on the device, twice, shared by the tests below and left unchanged"""
    pkg, torch = env
    out = {}
    for depth in (6, 9):
        ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 41)
        out[depth] = (pool, pool.words(), pts, ws)
    return out


def mixed_rays(n, depth, rays=None):
    """seeded rays (or `rays`) with zero components, origins on lattice planes, tiny components and invalid rays mixed in: lanes
    that do nothing beside lanes with long rays in one wavefront"""
    rays = seeded_rays(n, seed=11 + n) if rays is None else rays
    n_side = 1 << depth
    h = F(EDGE) / F(n_side)
    for k in range(0, n, 7):
        rays[k, 3 + (k // 7) % 3] = 0.0                                       # one zero component
    for k in range(3, n, 11):
        a = (k // 11) % 3
        rays[k, a] = plane(CENTER[a], (k * 5) % (n_side + 1), n_side, h)      # the origin on a lattice plane (a root face included)
    for k in range(5, n, 13):
        a = (k // 13) % 3
        rays[k, 3:] = 0.0
        rays[k, 3 + a] = -2.5 if k % 2 else 0.5                               # two zero components, not a unit vector
    for k in range(6, n, 17):
        rays[k, 3 + (k // 17) % 3] = 1e-30 if k % 2 else -1e-30               # a component that never gets anywhere
    for k in range(9, n, 19):
        rays[k, (k // 19) % 6] = (np.nan, np.inf, -np.inf)[k % 3]              # invalid
    for k in range(10, n, 23):
        rays[k, 3:] = 0.0                                                     # invalid: v == 0
    return rays


def fused_cloud_rays(n, depth, pts):
    """mixed_rays, every fourth of the seeded rays aimed at a fused point first (at depth 9 the cloud's cells are too small for
    unaimed rays to meet many of them)"""
    rays = seeded_rays(n, seed=11 + n)
    aim = np.arange(0, n, 4)
    v = pts[(aim * 3) % pts.shape[0]] - rays[aim, :3]
    rays[aim, 3:] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return mixed_rays(n, depth, rays)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, center, edge, rays, t_max, want = CASES[name]
    pool = pkg.Pool()
    pool.set_words(words)
    got = pkg.cast_rays(pool, depth, center, edge, rays, t_max)
    check_expected(got, want)
    same(got, cast_rays_words(words, depth, center, edge, rays, t_max), RAY_FIELDS)
    if depth > 1:                                                  # the level above, from the same words
        same(pkg.cast_rays(pool, depth - 1, center, edge, rays, t_max), cast_rays_words(words, depth - 1, center, edge, rays, t_max), RAY_FIELDS)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize("depth", [6, 9])
def test_fused_cloud(env, fused, depth, n):
    pkg, torch = env
    pool, words, pts, _ = fused[depth]
    rays = fused_cloud_rays(n, depth, pts)
    t_max = (np.random.default_rng(n).random(n) * 4.0).astype(F)
    for d in (depth, depth - 2):
        for tm in (None, t_max):
            want = cast_rays_words(words, d, CENTER, EDGE, rays, tm)
            if n == 4099:
                # the batch itself (the restatement's result, not the device's) holds what the comparison is meant to cover: more
                # hits than one workgroup has lanes -- a quarter of the rays are aimed at fused points, whose cells are occupied; of
                # those about a quarter are then bent or made invalid by mixed_rays, and a t_max drawn from 0..4 cuts up to half of
                # the rest, which leaves about n / 11 = 370 -- as well as invalid rays and rays of more than 8 blocks
                assert (want["node"] >= 0).sum() > 256 and np.isnan(want["t"]).sum() > 100 and int(want["steps"].max()) > 8
            got = pkg.cast_rays(pool, d, CENTER, EDGE, rays, tm)
            same(got, want, RAY_FIELDS)
    if n == 4099:                                                  # (a) and (b) on the device's own output (valid rays only)
        ok = ~np.isnan(got["t"])
        sub = {k: a[ok] for k, a in got.items()}
        assert check_against_the_occupied_set(words, depth - 2, rays[ok], t_max[ok], sub, geometry=False)[0] > 500


def test_every_subset_of_outputs(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    rays = mixed_rays(257, 6)
    want = cast_rays_words(words, 6, CENTER, EDGE, rays)
    for r in range(0, len(RAY_FIELDS) + 1):
        for names in itertools.combinations(RAY_FIELDS, r):
            same(pkg.cast_rays(pool, 6, CENTER, EDGE, rays, outputs=names), {k: want[k] for k in names}, names)
    p = pts[:300]
    wantp = query_points_words(words, 6, CENTER, EDGE, p)
    for r in range(0, len(POINT_FIELDS) + 1):
        for names in itertools.combinations(POINT_FIELDS, r):
            same(pkg.query_points(pool, 6, CENTER, EDGE, p, outputs=names), {k: wantp[k] for k in names}, names)
    # cuda tensors in, cuda tensors out: the same bits
    got = pkg.cast_rays(pool, 6, CENTER, EDGE, torch.from_numpy(rays).cuda())
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got.values())
    same({k: v.cpu().numpy().view(want[k].dtype) for k, v in got.items()}, want, RAY_FIELDS)


def test_depth_16_cell_coordinates_beyond_15_bits(env):
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 16, 2000, 43)
    words = pool.words()
    rays = mixed_rays(257, 16)
    aimed = seeded_rays(256, seed=3)                               # rays that end on fused points: hits deep in the tree
    aimed[:, 3:] = pts[:256] - aimed[:, :3]
    rays = np.concatenate([rays, aimed])
    want = cast_rays_words(words, 16, CENTER, EDGE, rays)
    hit = want["node"] >= 0
    xyz = np.stack([(want["cell"][hit] >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32)], 1)
    assert hit.sum() > 20 and int(xyz.max()) >= 1 << 15
    same(pkg.cast_rays(pool, 16, CENTER, EDGE, rays), want, RAY_FIELDS)
    same(pkg.query_points(pool, 16, CENTER, EDGE, pts), query_points_words(words, 16, CENTER, EDGE, pts), POINT_FIELDS)


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    pool = pkg.Pool()
    pool.set_words(hp.words())
    rays = mixed_rays(257, 1)
    want = cast_rays_words(hp.words(), 1, CENTER, EDGE, rays)
    assert (want["node"] >= 0).sum() > 20
    same(pkg.cast_rays(pool, 1, CENTER, EDGE, rays), want, RAY_FIELDS)
    pts = rays[:, :3]
    same(pkg.query_points(pool, 1, CENTER, EDGE, pts), query_points_words(hp.words(), 1, CENTER, EDGE, pts), POINT_FIELDS)


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    rays = mixed_rays(4099, depth)
    unsynced = pkg.cast_rays(pool, depth, CENTER, EDGE, rays)
    unsynced_p = pkg.query_points(pool, depth, CENTER, EDGE, pts[:1001])
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    same(pkg.cast_rays(pool, depth, CENTER, EDGE, rays), unsynced, RAY_FIELDS)
    same(unsynced, cast_rays_words(words, depth, CENTER, EDGE, rays), RAY_FIELDS)
    same(unsynced_p, query_points_words(words, depth, CENTER, EDGE, pts[:1001]), POINT_FIELDS)


def test_no_rays_and_argument_errors(env):
    pkg, torch = env
    pool = pkg.Pool()
    L = pkg.lib()
    got = pkg.cast_rays(pool, 5, CENTER, EDGE, np.zeros((0, 6), F))
    assert all(got[k].shape == (0,) for k in RAY_FIELDS)
    assert all(v.shape == (0,) for v in pkg.query_points(pool, 5, CENTER, EDGE, np.zeros((0, 3), F)).values())
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    null, ptr, ctr = C.c_void_p(0), pkg._ptr(buf), pkg._fa(CENTER, 3)

    def cast(pool_ref=C.byref(pool._p), depth=5, edge=1.0, rays=ptr, n=4):
        return L.svoslam_pool_cast_rays(pool_ref, depth, ctr, edge, rays, null, n, null, null, null, null, null, pkg._stream())

    def look(pool_ref=C.byref(pool._p), depth=5, edge=1.0, points=ptr, n=4):
        return L.svoslam_pool_query_points(pool_ref, depth, ctr, edge, points, n, null, null, null, null, pkg._stream())
    for call in (cast, look):
        assert call() == 0 and call(n=0) == 0 and call(None, n=0) == 0
        assert call(None) == -1 and call(n=-1) == -1 and call(depth=0) == -1 and call(depth=17) == -1
        assert call(edge=0.0) == -1 and call(edge=-1.0) == -1 and call(edge=float("nan")) == -1
    assert cast(rays=null) == -1 and look(points=null) == -1 and cast(rays=null, n=0) == 0
    assert L.svoslam_abi_version() == 1


@pytest.mark.parametrize("depth", [6, 9])
def test_query_points_of_the_fused_cloud(env, fused, oracle, depth):
    pkg, torch = env
    pool, words, pts, _ = fused[depth]
    n = pts.shape[0]
    assert n % 256 != 0
    extra = np.array([[np.nan, 0, 0], [0, 5.0, 0], [0, 0, -np.inf]], F)
    p = np.concatenate([pts, extra])
    for d in (depth, depth - 2, depth + 3):
        want = query_points_words(words, d, CENTER, EDGE, p)
        got = pkg.query_points(pool, d, CENTER, EDGE, p)
        same(got, want, POINT_FIELDS)
        assert (got["node"][n:] == -1).all() and (got["key"][n:] == 0).all()
    got = pkg.query_points(pool, depth, CENTER, EDGE, pts)
    assert (got["level"] == depth).all()                           # every fused point is found in its own leaf
    assert np.array_equal(got["key"].astype(np.int64), oracle.compute_keys(pts, depth, CENTER, EDGE))


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    rays = mixed_rays(257, 6)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.cast_rays(pool, 6, CENTER, EDGE, rays)
        pkg.cast_rays(pool, 4, CENTER, EDGE, rays)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.query_points(pool, 6, CENTER, EDGE, pts)
        pkg.cast_rays(pool, 6, CENTER, EDGE, np.zeros((0, 6), F))  # nothing is launched, nothing is bracketed
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
    finally:
        pkg.stage_timing([])
