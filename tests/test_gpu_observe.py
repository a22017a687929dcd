"""svoslam_field_observe_rays and svoslam_pool_frontier_field on the device: obs, state, frontier and both summaries equal the host
restatement of the specification (tests/test_observe_cpu.py: observe_rays_host and frontier_field_host, checked there against the
supercover's definition, the visibility field and figures written out by hand), byte for byte -- never a second device result alone.

The long rays (depth 12 and 16, int64 keys near 2^49) are held against the supercover's definition in Fractions on the cells of a
small region (slab_cells); the walk of the restatement asserts small keys and is not used for them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_coverage_cpu import cover_views_host, same_cover
from test_field_cpu import fused_regions, region_cells
from test_gpu_query import fused_pool
from test_observe_cpu import (END, FLOATER, FREE, FRONTIER, FUSED_RANGE, HAND_CENTER, HAND_DEPTH, HAND_EDGE, HAND_ENDS, HAND_REGION, NOT_ALL_STATES,
                              OCCUPIED, ROOT_REGION, SENSOR, THROUGH, UNKNOWN, VACATED, WALL, centres, frame_to, frontier_field_host, fused_frame,
                              observe_rays_host, same_bytes, slab_cells)
from test_reach_cpu import cells_pool
from test_surface_cpu import CENTER, EDGE
from test_visibility_cpu import occupancy, visibility_field_walk
from test_volume_cpu import ROOT_CENTER, ROOT_EDGE
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NO_SLOT = [(0, 0)]


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def on_device(pkg, words):
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    return ws, pool


@pytest.fixture(scope="module")
def oracle_words(oracle):
    """test_volume_cpu's fused pool: the cloud the CPU oracle fused twice at depth 6"""
    pts, col = surface_cloud(np.random.default_rng(41), 15000)
    pool = oracle.Pool()
    for _ in range(2):
        pool.insert_cloud(pts, col, 6, ROOT_CENTER, ROOT_EDGE)
    return pool.words()


@pytest.fixture(scope="module")
def fused(env, oracle_words):
    """(pool, workspace, occupancy) of the oracle's fused words at depth 6, set on the device: shared and left unchanged"""
    pkg, torch = env
    ws, pool = on_device(pkg, oracle_words)
    return pool, ws, occupancy(oracle_words, 6)


def lattice(depth):
    """(center, edge) of a root whose plane k is the number k on every axis: cell centres are k + 1/2, exact in binary32"""
    half = float(1 << (depth - 1))
    return (half, half, half), half


def expect_obs(pkg, ws, depth, center, edge, origin, dims, points, poses, range_cells=0, want=None):
    """one observe_rays call: every byte and count is the restatement's -> (obs, summary) of the device"""
    obs, summary = pkg.observe_rays(ws, None, depth, center, edge, origin, dims, points, poses, range_cells)
    if want is None:
        want = observe_rays_host(depth, center, edge, origin, dims, points, poses, range_cells)
    same_bytes(obs, want[0])
    assert summary.dtype == np.int64 and summary.tolist() == want[1].tolist(), (summary.tolist(), want[1].tolist())
    return obs, summary


def expect_field(pkg, ws, pool, occ, depth, origin, dims, obs):
    got = pkg.frontier_field(ws, pool, depth, origin, dims, obs)
    want = frontier_field_host(occ, depth, origin, dims, obs)
    for name in ("state", "frontier", "summary"):
        same_bytes(got[name], want[name], name)
    return got


# ---- 1. the hand scene and the fused pool ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floater", [True, False])
def test_the_hand_scene(env, floater):
    pkg, torch = env
    words = cells_pool(WALL + ([FLOATER] if floater else []), HAND_DEPTH)
    occ = occupancy(words, HAND_DEPTH)
    ws, pool = on_device(pkg, words)
    points, pose = frame_to(SENSOR, HAND_ENDS)
    obs, summary = expect_obs(pkg, ws, HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, points, pose)
    assert summary.tolist() == [0, 0, 0, 81, 197, 81]
    got = expect_field(pkg, ws, pool, occ, HAND_DEPTH, *ROOT_REGION, obs)
    assert got["summary"].tolist() == ([3643, 93, 103, 255, 1, 1] if floater else [3643, 94, 103, 255, 0, 1])
    assert np.argwhere(got["state"] == VACATED)[:, ::-1].tolist() == ([list(FLOATER)] if floater else [])
    obs, summary = expect_obs(pkg, ws, HAND_DEPTH, HAND_CENTER, HAND_EDGE, *HAND_REGION, points, pose)
    got = expect_field(pkg, ws, pool, occ, HAND_DEPTH, *HAND_REGION, obs)
    assert got["summary"].tolist() == ([457, 93, 98, 80, 1, 0] if floater else [457, 94, 98, 80, 0, 0])
    row = expect_field(pkg, ws, pool, occ, HAND_DEPTH, (2, 8, 8), (6, 1, 1), obs[4:5, 4:5, 1:7])   # the border makes no frontier
    assert row["summary"][FRONTIER] == 0 and row["summary"][FREE] == (5 if floater else 6)


@pytest.mark.parametrize("region", sorted(fused_regions(6)))
def test_fused_cloud(env, fused, region):
    """test_observe_cpu's fused cases: the synthetic frame of the oracle-fused pool, with and without the range limit"""
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)[region]
    points, poses, ends = fused_frame(occ)
    for range_cells in (FUSED_RANGE, 12, 0):
        obs, summary = expect_obs(pkg, ws, 6, ROOT_CENTER, ROOT_EDGE, origin, dims, points, poses, range_cells)
        got = expect_field(pkg, ws, pool, occ, 6, origin, dims, obs)
        if range_cells == 12:
            assert summary[2] > 0 and summary[3] > 0                   # some rays are far, some are marked
    if region not in NOT_ALL_STATES:
        assert all(got["summary"][k] > 0 for k in (UNKNOWN, FREE, FRONTIER, OCCUPIED))


# ---- 2. rows, wavefronts, workgroups and frames at their edges ------------------------------------------------------------------------
WIDE_DEPTH = 8                                                          # 256 cells a side
WIDE_ORIGIN = (37, 19, 29)                                              # rows that start inside a 64-cell word of the root
WIDE_OCCUPIED = [(36, 20, 30), (50, 19, 29), (69, 20, 29), (70, 20, 30), (88, 19, 30), (101, 20, 30), (102, 21, 30), (60, 18, 30), (75, 20, 31),
                 (45, 20, 28), (95, 19, 28), (64, 20, 29), (63, 19, 30), (37, 19, 29), (100, 21, 30), (165, 21, 30), (130, 20, 29)]


def aimed_frames(rng, depth, origin, dims, n_frames, n, reach):
    """frames whose sensors and ray ends lie within `reach` cells of the region (clipped to the root), a different sensor cell per
    frame: (points [n_frames, n, 3], poses [n_frames, 16]) on the lattice of lattice(depth)"""
    center, edge = lattice(depth)
    lo = np.maximum(np.asarray(origin) - reach, 0)
    hi = np.minimum(np.asarray(origin) + np.asarray(dims) + reach, 1 << depth)
    points, poses = np.zeros((n_frames, n, 3), F), np.zeros((n_frames, 16), F)
    for f in range(n_frames):
        points[f], poses[f] = frame_to(rng.integers(lo, hi), rng.integers(lo, hi, (n, 3)), depth, center, edge)
    return points, poses


@pytest.mark.parametrize("nx", [1, 63, 64, 65, 129])
def test_bit_row_edges(env, nx):
    """rows of less than a word, exactly one, one and a bit, and two and a bit, not at the root's origin"""
    pkg, torch = env
    words = cells_pool(WIDE_OCCUPIED, WIDE_DEPTH)
    occ = occupancy(words, WIDE_DEPTH)
    ws, pool = on_device(pkg, words)
    center, edge = lattice(WIDE_DEPTH)
    dims = (nx, 3, 2)
    rng = np.random.default_rng(100 + nx)
    lo, hi = np.asarray(WIDE_ORIGIN), np.asarray(WIDE_ORIGIN) + np.asarray(dims)
    points, poses = np.zeros((2, 90, 3), F), np.zeros((2, 16), F)
    for f in range(2):                                                  # the sensors up to 6 cells outside the region, the ends in it
        ends = rng.integers(lo, hi, (90, 3))
        ends[0], ends[1] = (hi[0] - 1, lo[1] + 1, lo[2]), (lo[0], lo[1], lo[2] + 1)   # the last and the first cell of a row
        points[f], poses[f] = frame_to(rng.integers(lo - 6, hi + 6), ends, WIDE_DEPTH, center, edge)
    obs, summary = expect_obs(pkg, ws, WIDE_DEPTH, center, edge, WIDE_ORIGIN, dims, points, poses)
    assert summary[3] == 180 and summary[4] > 0 and summary[5] > 0
    assert (obs[0, 1, -1] & END) and (obs[1, 0, 0] & END)
    got = expect_field(pkg, ws, pool, occ, WIDE_DEPTH, WIDE_ORIGIN, dims, obs)
    assert got["summary"][OCCUPIED] + got["summary"][VACATED] >= 1 and got["summary"].sum() == nx * 6


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_wavefront_workgroup_and_frame_edges(env, n, n_frames):
    """n at the edges of a wavefront and a workgroup; with 3 frames of 65 rays a wavefront holds the end of one frame and the start
    of the next, whose poses differ"""
    pkg, torch = env
    ws = pkg.Workspace()
    center, edge = lattice(5)
    origin, dims = (3, 2, 1), (20, 25, 28)
    points, poses = aimed_frames(np.random.default_rng(7 * n + n_frames), 5, origin, dims, n_frames, n, 4)
    if n >= 63:
        points[0, 5] = np.nan                                           # a void and an outside ray among them
        points[-1, 60] = (1000, 0, 0)
    assert len({tuple(p[12:15]) for p in poses}) == n_frames
    obs, summary = expect_obs(pkg, ws, 5, center, edge, origin, dims, points, poses)
    assert summary[:4].sum() == n * n_frames and (n == 0) == (not obs.any())
    if n >= 63:
        assert summary[0] == 1 and summary[1] == 1
        for f in range(n_frames):                                       # every frame marked under its own pose
            alone, _ = observe_rays_host(5, center, edge, origin, dims, points[f:f + 1], poses[f:f + 1])
            assert alone.any() and ((obs & alone) == alone).all()


# ---- 3. long rays: int64 keys near 2^49 ---------------------------------------------------------------------------------------------
def long_ray_case(depth, a, b, origin, dims):
    """(points, pose, the bytes of the region by the supercover's definition) for the one ray from cell a to cell b"""
    center, edge = lattice(depth)
    points, pose = frame_to(a, [b], depth, center, edge)
    cells = region_cells(origin, dims)
    want = np.zeros(cells.shape[0], np.uint8)
    want[slab_cells(a, b, cells)] |= THROUGH
    want[(cells == np.asarray(a)).all(1)] |= THROUGH
    want[(cells == np.asarray(b)).all(1)] |= END
    return points, pose, want.reshape(dims[2], dims[1], dims[0])


LONG_RAYS = {
    "depth12_4095_4094_4093": (12, (0, 0, 0), (4095, 4094, 4093), (2044, 2043, 2042), (8, 8, 8)),
    "depth12_reversed": (12, (4095, 4094, 4093), (0, 0, 0), (2044, 2043, 2042), (8, 8, 8)),
    "depth16_diagonal": (16, (0, 0, 0), (65535, 65535, 65535), (32764, 32764, 32764), (8, 8, 8)),
    "depth16_65535_65534_65533": (16, (0, 0, 0), (65535, 65534, 65533), (32764, 32763, 32762), (8, 8, 8)),
    "depth16_anti_diagonal": (16, (65535, 0, 65535), (0, 65535, 0), (32764, 32764, 32764), (8, 8, 8)),
    "depth12_along_x_through_a_corner": (12, (0, 2044, 2044), (4095, 2044, 2044), (2044, 2044, 2044), (8, 8, 8)),
    "depth16_along_z_through_the_far_corner": (16, (32771, 32771, 65535), (32771, 32771, 0), (32764, 32764, 32764), (8, 8, 8)),
    "depth12_starts_in_the_region": (12, (2045, 2046, 2047), (4095, 0, 4000), (2044, 2044, 2044), (8, 8, 8)),
    "depth12_ends_in_the_region": (12, (5, 4090, 17), (2050, 2045, 2049), (2044, 2044, 2044), (8, 8, 8)),
}


@pytest.mark.parametrize("name", sorted(LONG_RAYS))
def test_long_rays_against_the_definition(env, name):
    pkg, torch = env
    depth, a, b, origin, dims = LONG_RAYS[name]
    center, edge = lattice(depth)
    points, pose, want = long_ray_case(depth, a, b, origin, dims)
    ws = pkg.Workspace()
    obs, summary = pkg.observe_rays(ws, None, depth, center, edge, origin, dims, points, pose)
    same_bytes(obs, want)
    assert summary.tolist() == [0, 0, 0, 1, int(((want & THROUGH) != 0).sum()), int(((want & END) != 0).sum())]
    assert summary[4] >= 8                                              # the ray does cross the region
    far, counts = pkg.observe_rays(ws, None, depth, center, edge, origin, dims, points, pose, range_cells=(1 << depth) // 2)
    assert not far.any() and counts.tolist() == [0, 0, 1, 0, 0, 0]       # |D|^2 against R^2 in 64 bits
    limit = 1 << 16                                                     # the largest range: it still cuts the diagonals of a root of depth 16
    whole, counts = pkg.observe_rays(ws, None, depth, center, edge, origin, dims, points, pose, range_cells=limit)
    if sum((int(y) - int(x)) ** 2 for x, y in zip(a, b)) > limit * limit:
        assert depth == 16 and not whole.any() and counts.tolist() == [0, 0, 1, 0, 0, 0]
    else:
        same_bytes(whole, want)
        assert counts.tolist() == summary.tolist()


def test_4096_rays_between_the_same_two_cells_are_one_ray(env):
    pkg, torch = env
    ws = pkg.Workspace()
    center, edge = lattice(6)
    a, b = (3, 5, 7), (60, 41, 22)
    points, pose = frame_to(a, [b], 6, center, edge)
    one, _ = expect_obs(pkg, ws, 6, center, edge, (0, 0, 0), (64, 64, 64), points, pose)
    many, summary = pkg.observe_rays(ws, None, 6, center, edge, (0, 0, 0), (64, 64, 64), np.tile(points, (4096, 1)), pose)
    same_bytes(many, one)
    assert summary.tolist() == [0, 0, 0, 4096, int(((one & THROUGH) != 0).sum()), 1]
    split, summary = pkg.observe_rays(ws, None, 6, center, edge, (0, 0, 0), (64, 64, 64), np.tile(points, (4096, 1)), np.tile(pose, (64, 1)))
    same_bytes(split, one)                                              # the same rays as 64 frames of 64
    assert summary[3] == 4096


# ---- 4. tensors and options -----------------------------------------------------------------------------------------------------------
def test_accumulate_and_tensors_in_and_out(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    points, poses, _ = fused_frame(occ)
    rng = np.random.default_rng(5)
    more = aimed_frames(rng, 6, origin, dims, 2, 70, 3)
    center, edge = lattice(6)
    before = rng.integers(0, 256, (dims[2], dims[1], dims[0])).astype(np.uint8)
    t_obs = torch.from_numpy(before).cuda()
    got, summary = pkg.observe_rays(ws, t_obs, 6, ROOT_CENTER, ROOT_EDGE, origin, dims, torch.from_numpy(points).cuda(),
                                    torch.from_numpy(poses).cuda(), FUSED_RANGE, accumulate=True, as_tensor=True)
    assert got.data_ptr() == t_obs.data_ptr() and summary.is_cuda and summary.dtype == torch.int64   # written in place
    want, counts = observe_rays_host(6, ROOT_CENTER, ROOT_EDGE, origin, dims, points, poses, FUSED_RANGE, accumulate=True, obs=before)
    same_bytes(t_obs.cpu().numpy(), want)
    assert summary.cpu().tolist() == counts.tolist() and np.array_equal(want & 0xFC, before & 0xFC) and (want != before).any()
    # a second lattice over the same cells, added to the first: marking in parts is marking at once
    both, _ = pkg.observe_rays(ws, t_obs, 6, center, edge, origin, dims, *more, accumulate=True)
    want2, _ = observe_rays_host(6, center, edge, origin, dims, *more, accumulate=True, obs=want)
    same_bytes(both, want2)
    fresh, _ = pkg.observe_rays(ws, t_obs, 6, center, edge, origin, dims, *more)     # without accumulate the bytes are the marks alone
    same_bytes(fresh, observe_rays_host(6, center, edge, origin, dims, *more)[0])
    assert not (t_obs.cpu().numpy() & 0xFC).any()
    kept, counts = pkg.observe_rays(ws, before, 6, center, edge, origin, dims, more[0][:, :0], more[1], accumulate=True)   # no rays
    same_bytes(kept, before)
    assert counts.tolist() == [0, 0, 0, 0, int(((before & THROUGH) != 0).sum()), int(((before & END) != 0).sum())]
    cleared, counts = pkg.observe_rays(ws, before, 6, center, edge, origin, dims, more[0][:0], more[1][:0])               # no frames
    assert not cleared.any() and counts.tolist() == [0] * 6
    field = pkg.frontier_field(ws, pool, 6, origin, dims, torch.from_numpy(want).cuda(), as_tensor=True)
    host = frontier_field_host(occ, 6, origin, dims, want)                # bits 2..7 are ignored
    for name in ("state", "frontier", "summary"):
        assert field[name].is_cuda and field[name].dtype == (torch.int32 if name == "summary" else torch.uint8)
        same_bytes(field[name].cpu().numpy(), host[name], name)
    with pytest.raises(ValueError):
        pkg.observe_rays(ws, None, 6, center, edge, origin, dims, *more, accumulate=True)
    with pytest.raises(ValueError):
        pkg.observe_rays(ws, before[:1], 6, center, edge, origin, dims, *more)
    with pytest.raises(ValueError):
        pkg.observe_rays(ws, None, 6, center, edge, origin, dims, more[0][:, :69].reshape(-1, 3)[:-1], more[1])


def test_each_optional_output_alone_and_zero_dims(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    points, poses, ends = fused_frame(occ)
    obs, _ = pkg.observe_rays(ws, None, 6, ROOT_CENTER, ROOT_EDGE, origin, dims, points, poses, FUSED_RANGE)
    want = frontier_field_host(occ, 6, origin, dims, obs)
    for names in (("state",), ("frontier",), ("summary",), ("state", "summary"), ("frontier", "state")):
        got = pkg.frontier_field(ws, pool, 6, origin, dims, obs, want=names)
        assert set(got) == set(names)
        for name in names:
            same_bytes(got[name], want[name], name)
    assert set(pkg.frontier_field(ws, pool, 6, origin, dims, obs)) == {"state", "frontier", "summary"}
    with pytest.raises(KeyError):
        pkg.frontier_field(ws, pool, 6, origin, dims, obs, want=("mask",))
    for zero in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got, summary = pkg.observe_rays(ws, None, 6, ROOT_CENTER, ROOT_EDGE, (1, 2, 3), zero, points, poses, FUSED_RANGE)
        assert got.shape == (zero[2], zero[1], zero[0]) and summary.tolist() == [3, 0, 0, ends.shape[0], 0, 0]
        field = pkg.frontier_field(ws, pool, 6, (1, 2, 3), zero, got)
        assert field["state"].shape == got.shape and field["summary"].tolist() == [0] * 6


def test_explore_views_is_the_cover_of_the_frontier(env):
    pkg, torch = env
    words = cells_pool(WALL + [FLOATER], HAND_DEPTH)
    occ = occupancy(words, HAND_DEPTH)
    ws, pool = on_device(pkg, words)
    obs, _ = pkg.observe_rays(ws, None, HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, *frame_to(SENSOR, HAND_ENDS))
    cands = np.array([(3, 8, 8), (4, 3, 8), (4, 13, 8), (12, 8, 8), (4, 8, 13), (-1, 0, 0), (3, 8, 8)], np.int32)
    field, cover = pkg.explore_views(ws, pool, HAND_DEPTH, *ROOT_REGION, obs, cands, 6, 4)
    host = frontier_field_host(occ, HAND_DEPTH, *ROOT_REGION, obs)
    for name in ("state", "frontier", "summary"):
        same_bytes(field[name], host[name], name)
    same_cover(cover, cover_views_host(occ, HAND_DEPTH, *ROOT_REGION, 6, 1, host["frontier"], cands, 4))
    assert cover["summary"][0] == 103 and cover["summary"][1] >= 2


# ---- 5. conventions ---------------------------------------------------------------------------------------------------------------------
def test_a_deferred_commit_is_read_in_its_old_state(env):
    """between svoslam_svo_fuse_commit_deferred and svoslam_svo_fuse_apply the frontier field is that of the words the pool held
    before the commit, and after the apply that of the new words; on the workspace that holds the deferred commit"""
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
    origin, dims = (0, 0, 8), (64, 64, 12)
    occ_old = occupancy(old, depth)
    points, poses = aimed_frames(np.random.default_rng(8), depth, origin, dims, 2, 200, 0)
    center, edge = lattice(depth)
    obs, _ = expect_obs(pkg, ws, depth, center, edge, origin, dims, points, poses)      # sees no pool: the commit does not matter to it
    before = expect_field(pkg, ws, pool, occ_old, depth, origin, dims, obs)
    pkg.svo_fuse_apply(ws, pool)
    occ_new = occupancy(pool.words(), depth)
    after = expect_field(pkg, ws, pool, occ_new, depth, origin, dims, obs)
    assert (after["state"] != before["state"]).any() and (occ_new != occ_old).any() and before["summary"][FRONTIER] > 0


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 6
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    origin, dims = (0, 3, 10), (64, 40, 9)
    center, edge = lattice(depth)
    points, poses = aimed_frames(np.random.default_rng(9), depth, origin, dims, 1, 150, 0)
    obs = observe_rays_host(depth, center, edge, origin, dims, points, poses)[0]
    unsynced = pkg.frontier_field(ws, pool, depth, origin, dims, obs)
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    want = frontier_field_host(occupancy(pool.words(), depth), depth, origin, dims, obs)
    for name in ("state", "frontier", "summary"):
        same_bytes(unsynced[name], want[name], name)
    assert want["summary"][OCCUPIED] > 20 and want["summary"][FRONTIER] > 20


def test_the_slots_are_reused_and_the_other_fields_slots_are_left_alone(env, fused):
    """(a failed allocation is not provoked: no test of this suite shows a way to make hipMalloc fail without asking for memory the
    machine may well have, so the rollback after SVOSLAM_ERR_OOM is left to SlotRollback's own use in the cover's limit test)"""
    pkg, torch = env
    pool, _, occ = fused
    ws = pkg.Workspace()
    assert ws.observe_buffers() == NO_SLOT and ws.frontier_buffers() == NO_SLOT and ws.visibility_buffers() == NO_SLOT
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    views = np.array([[10, 10, 10], [5, 12, 9]], np.int32)
    mask = pkg.visibility_field(ws, pool, 6, *small, 5, views)["mask"]
    cover = pkg.cover_views(ws, pool, 6, *small, 5, views, 2)
    vis_slots, cover_slots = ws.visibility_buffers(), ws.cover_buffers()
    points, poses, _ = fused_frame(occ)
    obs, _ = expect_obs(pkg, ws, 6, ROOT_CENTER, ROOT_EDGE, *large, points, poses)
    assert ws.frontier_buffers() == NO_SLOT                        # observe_rays sees no pool and none of the frontier's slot
    expect_field(pkg, ws, pool, occ, 6, *large, obs)
    slots = ws.observe_buffers() + ws.frontier_buffers()
    rows = 64 * 40                                                 # one word a row
    assert all(ptr != 0 for ptr, _ in slots)
    assert 2 * rows * 8 <= slots[0][1] < 4 * rows * 8 and rows * 8 <= slots[1][1] < 2 * rows * 8      # two planes; one; and the slots' headroom
    expect_obs(pkg, ws, 6, ROOT_CENTER, ROOT_EDGE, *large, points, poses)
    expect_field(pkg, ws, pool, occ, 6, *large, obs)
    assert ws.observe_buffers() + ws.frontier_buffers() == slots   # a second call of the same size allocates nothing
    part, _ = expect_obs(pkg, ws, 6, ROOT_CENTER, ROOT_EDGE, *small, points, poses)     # a smaller call in the larger call's slots
    expect_field(pkg, ws, pool, occ, 6, *small, part)
    assert ws.observe_buffers() + ws.frontier_buffers() == slots
    assert ws.visibility_buffers() == vis_slots and ws.cover_buffers() == cover_slots
    assert np.array_equal(pkg.visibility_field(ws, pool, 6, *small, 5, views)["mask"], mask)
    same_cover(pkg.cover_views(ws, pool, 6, *small, 5, views, 2), cover)
    assert ws.observe_buffers() + ws.frontier_buffers() == slots and ws.visibility_buffers() == vis_slots
    assert np.array_equal(mask, visibility_field_walk(occ, 6, *small, 5, views)["mask"])
    ws.close()                                                     # release_all releases the new slots with the rest


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    words = cells_pool([(4, 4, 4), (10, 4, 4)], 5)
    ws, pool = on_device(pkg, words)
    L = pkg.lib()
    center, edge = lattice(5)
    points, poses = aimed_frames(np.random.default_rng(2), 5, (3, 3, 3), (8, 2, 2), 2, 20, 3)
    t_points, t_poses = torch.from_numpy(points).cuda(), torch.from_numpy(poses).cuda()
    bufs = {name: torch.full((64,), 0x55, dtype=dtype, device="cuda") for name, dtype in
            (("obs", torch.uint8), ("counts", torch.int64), ("state", torch.uint8), ("frontier", torch.uint8), ("summary", torch.int32))}
    null = C.c_void_p(0)
    p = {name: pkg._ptr(b) for name, b in bufs.items()}

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def f3(v):
        return None if v is None else (C.c_float * 3)(*v)

    def observe(ws_ref=ws._h, obs=p["obs"], depth=5, at=center, size=edge, origin=(3, 3, 3), dims=(8, 2, 2), pts=pkg._ptr(t_points), n=20,
                mats=pkg._ptr(t_poses), frames=2, radius=0, accumulate=0, counts=p["counts"]):
        return L.svoslam_field_observe_rays(ws_ref, obs, depth, f3(at), size, i3(origin), i3(dims), pts, n, mats, frames, radius, accumulate,
                                            counts, pkg._stream())

    def frontier(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(3, 3, 3), dims=(8, 2, 2), obs=p["obs"], out=(p["state"], p["frontier"], p["summary"])):
        return L.svoslam_pool_frontier_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), obs, *out, pkg._stream())
    assert observe() == 0 and observe(counts=null) == 0 and observe(radius=1 << 16) == 0 and observe(pts=null, mats=null, n=0) == 0
    assert observe(pts=null, mats=null, frames=0) == 0 and observe(accumulate=7) == 0
    assert frontier() == 0 and frontier(out=(null, null, p["summary"])) == 0 and frontier(out=(p["state"], null, null)) == 0
    torch.cuda.synchronize()
    assert bufs["summary"][:6].sum().item() == 32 and bufs["counts"][:4].sum().item() == 40
    for b in bufs.values():
        b.fill_(0x55)
    torch.cuda.synchronize()
    slots = ws.observe_buffers() + ws.frontier_buffers()
    assert all(size > 0 for _, size in slots)
    # svoslam_field_observe_rays
    assert observe(ws_ref=None) == -1 and observe(at=None) == -1 and observe(origin=None) == -1 and observe(dims=None) == -1
    assert observe(ws_ref=None, dims=(0, 2, 2)) == -1 and observe(depth=0, dims=(0, 2, 2)) == -1
    assert observe(depth=0) == -1 and observe(depth=17) == -1
    assert observe(size=0.0) == -1 and observe(size=-1.0) == -1 and observe(size=float("nan")) == -1
    assert observe(dims=(-1, 2, 2)) == -1 and observe(dims=(8, 2, -1)) == -1 and observe(dims=(0, -1, 2)) == -1
    for a in range(3):                                             # one cell outside the root on each side
        origin, dims = [3, 3, 3], [8, 2, 2]
        origin[a] = -1
        assert observe(origin=origin) == -1 and frontier(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert observe(origin=origin) == -1 and frontier(origin=origin) == -1
        origin[a], dims[a] = 0, 33
        assert observe(origin=origin, dims=dims) == -1 and frontier(origin=origin, dims=dims) == -1
    assert observe(n=-1) == -1 and observe(frames=-1) == -1 and observe(n=-1, dims=(0, 2, 2)) == -1
    assert observe(radius=-1) == -1 and observe(radius=(1 << 16) + 1) == -1 and observe(radius=-1, dims=(0, 2, 2)) == -1
    assert observe(obs=null) == -1 and observe(pts=null) == -1 and observe(mats=null) == -1 and observe(pts=null, dims=(0, 2, 2)) == -1
    # svoslam_pool_frontier_field
    assert frontier(ws_ref=None) == -1 and frontier(origin=None) == -1 and frontier(dims=None) == -1 and frontier(ws_ref=None, dims=(0, 2, 2)) == -1
    assert frontier(depth=0) == -1 and frontier(depth=17) == -1 and frontier(depth=0, dims=(0, 2, 2)) == -1
    assert frontier(dims=(-1, 2, 2)) == -1 and frontier(dims=(8, 2, -1)) == -1 and frontier(dims=(0, -1, 2)) == -1
    assert frontier(obs=null) == -1 and frontier(out=(null, null, null)) == -1 and frontier(out=(null, null, null), dims=(0, 2, 2)) == -1
    assert frontier(pool_ref=None) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert frontier(pool_ref=C.byref(blank)) == -1
    # more than 2^31 - 1 region cells, more than 2^31 - 1 rays: refused with nothing allocated or grown
    fresh = pkg.Workspace()
    for ref in (ws._h, fresh._h):
        assert observe(ws_ref=ref, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
        assert observe(ws_ref=ref, n=1 << 16, frames=1 << 15) == -6
        assert frontier(ws_ref=ref, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert observe(ws_ref=fresh._h, radius=-1) == -1 and frontier(ws_ref=fresh._h, obs=null) == -1
    torch.cuda.synchronize()
    assert fresh.observe_buffers() == NO_SLOT and fresh.frontier_buffers() == NO_SLOT
    assert ws.observe_buffers() + ws.frontier_buffers() == slots    # none of the refused calls allocated or grew anything
    assert all((b == 0x55).all().item() for b in bufs.values())    # none of the refused calls wrote anything
    # valid calls without cells: the ray counts and a zero summary, nothing else, no pool needed
    assert observe(dims=(0, 2, 2), obs=null) == 0 and frontier(pool_ref=None, dims=(8, 0, 2), obs=null) == 0
    assert frontier(pool_ref=C.byref(blank), dims=(8, 2, 0), obs=null, out=(p["state"], null, null)) == 0
    torch.cuda.synchronize()
    want = observe_rays_host(5, center, edge, (3, 3, 3), (0, 2, 2), points, poses)[1]
    assert bufs["counts"][:7].tolist() == want.tolist() + [0x55] and want[3] == 40
    assert bufs["summary"][:7].tolist() == [0] * 6 + [0x55]
    assert (bufs["obs"] == 0x55).all().item() and (bufs["state"] == 0x55).all().item() and (bufs["frontier"] == 0x55).all().item()
    assert fresh.observe_buffers() == NO_SLOT and L.svoslam_abi_version() == 1
    with pytest.raises(Exception):
        pkg.observe_rays(ws, None, 5, center, edge, (0, 0, 0), (4, 4, 4), points, poses, range_cells=-1)
    with pytest.raises(Exception):
        pkg.frontier_field(ws, pool, 5, (0, 0, 0), (4, 4, 33), np.zeros((33, 4, 4), np.uint8))


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    points, poses, _ = fused_frame(occ)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        obs, _ = pkg.observe_rays(ws, None, 6, ROOT_CENTER, ROOT_EDGE, (0, 0, 0), (64, 20, 12), points, poses, as_tensor=True)
        pkg.observe_rays(ws, None, 6, ROOT_CENTER, ROOT_EDGE, (1, 2, 3), (9, 0, 3), points, poses)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.frontier_field(ws, pool, 6, (0, 0, 0), (64, 20, 12), obs)
        pkg.frontier_field(ws, pool, 6, (1, 2, 3), (9, 0, 3), np.zeros((3, 0, 9), np.uint8), want=("summary",))
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
    finally:
        pkg.stage_timing([])


# ---- 6. the tool ------------------------------------------------------------------------------------------------------------------------
def test_the_map_frontier_tool(env, tmp_path):
    """tools/map_frontier.py on the saved hand-built map: two frames given as points and poses, a second run that adds a frame to
    the first run's obs, and views chosen for the frontier"""
    pkg, torch = env
    words = cells_pool(WALL + [FLOATER], HAND_DEPTH)
    occ = occupancy(words, HAND_DEPTH)
    ws, pool = on_device(pkg, words)
    low = np.asarray(HAND_CENTER) - HAND_EDGE                           # the root cube is [0, 16]^3 metres, a cell is one metre
    box = np.array([1.5, 4.5, 4.5, 9.5, 12.5, 12.5], np.float32)
    lo, hi = pkg.box_to_cells(HAND_DEPTH, HAND_CENTER, HAND_EDGE, box)
    dims = hi - lo + 1
    assert lo.tolist() == list(HAND_REGION[0]) and dims.tolist() == list(HAND_REGION[1]) and (low == 0).all()
    first, pose = frame_to(SENSOR, HAND_ENDS[:40])
    second, _ = frame_to(SENSOR, HAND_ENDS[41:])
    third, pose3 = frame_to((3, 5, 6), HAND_ENDS[40:41] * 40)
    ckpt, out, out2 = tmp_path / "map.svopool", tmp_path / "frontier.npz", tmp_path / "frontier2.npz"
    pool.save(ckpt, HAND_CENTER, HAND_EDGE, HAND_DEPTH)
    np.save(tmp_path / "pts.npy", np.stack([first, second]))
    np.save(tmp_path / "poses.npy", np.stack([pose, pose]))
    np.save(tmp_path / "pts3.npy", third[None])
    np.save(tmp_path / "poses3.npy", pose3[None])
    tool = [sys.executable, os.path.join(ROOT, "tools", "map_frontier.py"), str(ckpt)]
    args = ["--box"] + [repr(float(v)) for v in box]
    r = subprocess.run(tool + [str(out)] + args + ["--points", str(tmp_path / "pts.npy"), "--poses", str(tmp_path / "poses.npy")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    want_obs, want_rays = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *HAND_REGION, np.stack([first, second]), np.stack([pose, pose]))
    want = frontier_field_host(occ, HAND_DEPTH, *HAND_REGION, want_obs)
    same_bytes(z["obs"], want_obs)
    for name in ("state", "frontier"):
        same_bytes(z[name], want[name], name)
    assert z["ray_summary"].tolist() == want_rays.tolist() and z["state_summary"].tolist() == want["summary"].tolist() and want_rays[3] == 80
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == HAND_DEPTH and float(z["cell_size"]) == 1.0
    r = subprocess.run(tool + [str(out2)] + args + ["--points", str(tmp_path / "pts3.npy"), "--poses", str(tmp_path / "poses3.npy"), "--obs", str(out),
                                                    "--range", "9", "--views", "3", "--grid", "2", "--clearance", "1", "--view-range", "6"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out2)
    more_obs, more_rays = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *HAND_REGION, third[None], pose3[None], 9, accumulate=True, obs=want_obs)
    more = frontier_field_host(occ, HAND_DEPTH, *HAND_REGION, more_obs)
    same_bytes(z["obs"], more_obs)
    same_bytes(z["state"], more["state"], "state")
    assert z["ray_summary"].tolist() == more_rays.tolist() and (more_obs != want_obs).any() and more_rays[3] == 40
    grid = region_cells(lo.tolist(), dims.tolist())
    grid = grid[((grid - lo) % 2 == 0).all(1)]
    near = np.argwhere(occ)[:, ::-1]
    clear = np.array([((near - g) ** 2).sum(1).min() > 1 for g in grid])
    assert np.array_equal(z["candidate_cells"], grid[clear].astype(np.int32)) and 0 < clear.sum() < grid.shape[0]
    cover = cover_views_host(occ, HAND_DEPTH, lo.tolist(), dims.tolist(), 6, 1, more["frontier"], grid[clear], 3)
    same_cover({"seen": z["seen"], "chosen": z["chosen"], "gain": z["gain"], "round": z["round"], "summary": z["cover_summary"]}, cover)
    n = int(cover["summary"][1])
    assert n >= 2 and np.array_equal(z["chosen_cells"][:n], grid[clear][cover["chosen"][:n]]) and (z["chosen_cells"][n:] == -1).all()
    assert np.allclose(z["chosen_centres"][:n], grid[clear][cover["chosen"][:n]] + 0.5, atol=1e-6)
