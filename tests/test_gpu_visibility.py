"""svoslam_pool_visibility_field on the device: mask and count equal the host restatement of the specification
(tests/test_visibility_cpu.py: visibility_field_walk, the integer walk proven equal there to the definition by exact fractions)
applied to the pool's own words, bit for bit -- never a second device result alone.

The fused pool works at depth 6.  The whole root at R = 64 is 262144 cells times up to 32 viewpoints with lines of up to 190 steps,
more than the numpy walk does in seconds: there the device's whole field is compared at a sample of a few thousand cells (the
region's corners, a border face and a seeded sample: test_field_cpu.sample_cells), every viewpoint of every sampled cell.  The
cases about row words and long walks need a root of 256 cells a side: hand-built pools at depth 8 on regions of a few hundred
cells."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, fused_regions, region_cells, sample_cells
from test_gpu_field import same_field
from test_gpu_query import fused_pool
from test_nearest_cpu import nearest_field_separable
from test_reach_cpu import cells_pool
from test_surface_cpu import CENTER, EDGE, HandPool
from test_visibility_cpu import (HAND_CASES, HAND_DEPTH, ROOT_REGION, check_hand_case, choose_views, counting, occupancy, popcount,
                                 same_outputs, visibility_at, visibility_field_walk)
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("mask", "count")
GPU_RANGES = (0, 1, 3, 8, 64)
HOST_WALK_LIMIT = 1 << 18                                               # (viewpoint, cell) pairs the numpy walk takes in a test


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """(pool, its words, the fused points, workspace, occupancy) at depth 6: fused on the device, twice, shared and left unchanged"""
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 6, 15000, 41)
    words = pool.words()
    return pool, words, pts, ws, occupancy(words, 6)


def on_device(pkg, words):
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    return ws, pool


def expect(pkg, ws, pool, occ, depth, origin, dims, radius, views):
    """one call with both outputs: every value is the walk's.  -> (the device's field, the walk's)"""
    got = pkg.visibility_field(ws, pool, depth, origin, dims, radius, views, want=BOTH)
    want = visibility_field_walk(occ, depth, origin, dims, radius, views)
    same_outputs(got, want, BOTH)
    return got, want


# ---- 1. the fused pool ---------------------------------------------------------------------------------------------------------
# the (region, range) cases that reach into the fused cloud at a range at which a pair can be blocked: with 5 or 32 viewpoints each
# of them must decide something.  (At R = 0 and 1 nothing lies between the cells in range; in this root the other regions lie
# beside the cloud, low_corner more than 8 cells from it.)
DECIDED = {("whole_root", 3), ("whole_root", 8), ("whole_root", 64), ("low_corner", 64)}


@pytest.mark.parametrize("n_views", [1, 5, 32])
@pytest.mark.parametrize("region", sorted(fused_regions(6)))
def test_fused_cloud(env, fused, region, n_views):
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    origin, dims = fused_regions(6)[region]
    cells = dims[0] * dims[1] * dims[2]
    for radius in GPU_RANGES:
        views = choose_views(occ, 6, origin, dims, radius, n_views, 10 * radius + n_views)
        pairs = int(counting(views, 6).sum()) * min(cells, (2 * radius + 1) ** 3)
        live = views[counting(views, 6)].astype(np.int64)
        if pairs <= HOST_WALK_LIMIT:
            got, want = expect(pkg, ws, pool, occ, 6, origin, dims, radius, views)
            if (region, radius) in DECIDED and n_views >= 5:            # some in-range cells seen, some not
                in_range = sum(int((((region_cells(origin, dims) - v) ** 2).sum(1) <= radius * radius).sum()) for v in live)
                assert 0 < int(want["count"].sum()) < in_range, (int(want["count"].sum()), in_range)
        else:                                                           # the whole root at R = 64: the whole field at a sample of its cells
            got = pkg.visibility_field(ws, pool, 6, origin, dims, radius, views, want=BOTH)
            at = sample_cells(origin, dims, {1: 1 << 15, 5: 1 << 13, 32: 1 << 12}[n_views], 90 + n_views)
            mask, count = visibility_at(occ, 6, region_cells(origin, dims)[at], radius, views)
            assert got["mask"].dtype == np.uint32 and got["count"].dtype == np.int32 and got["mask"].shape == (dims[2], dims[1], dims[0])
            assert np.array_equal(got["mask"].reshape(-1)[at], mask) and np.array_equal(got["count"].reshape(-1)[at], count)
            in_range = sum((((region_cells(origin, dims)[at] - v) ** 2).sum(1) <= radius * radius).astype(np.int32) for v in live)
            assert (count > 0).sum() > 100 and (count < in_range).sum() > 10   # sampled cells seen, and in-range ones that are blocked
        assert np.array_equal(got["count"], popcount(got["mask"]))      # at most 32 viewpoints: a duplicate has a bit of its own


def test_the_fused_cases_are_not_empty(fused):
    """on the restatement's results: pairs seen and pairs not seen at the ranges at which a pair can be blocked at all (at R = 1 only
    face neighbours are in range, with nothing between), viewpoints outside the region, outside the root and duplicated among the 32"""
    occ = fused[4]
    for radius in (3, 8):
        seen = unseen = 0
        for region, (origin, dims) in fused_regions(6).items():
            views = choose_views(occ, 6, origin, dims, radius, 5, 10 * radius + 5)
            live = counting(views, 6)
            want = visibility_field_walk(occ, 6, origin, dims, radius, views)
            in_range = sum((((region_cells(origin, dims) - v) ** 2).sum(1) <= radius * radius).sum() for v in views[live].astype(np.int64))
            seen, unseen = seen + int(want["count"].sum()), unseen + int(in_range - want["count"].sum())
        assert seen > 50 and unseen >= 5, (radius, seen, unseen)
    origin, dims = fused_regions(6)["low_corner"]
    views = choose_views(occ, 6, origin, dims, 8, 32, 85)
    live = counting(views, 6)
    inside = ((views >= np.asarray(origin)) & (views < np.asarray(origin) + np.asarray(dims))).all(1)
    assert (~live).sum() >= 4 and (live & ~inside).sum() >= 1 and len({tuple(v) for v in views.tolist()}) <= 32 - 4


# ---- 2. hand-built pools -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in HAND_CASES if not n.startswith("531_")) + ["531"])
def test_hand_built_pools(env, name):
    pkg, torch = env
    for case in [n for n in sorted(HAND_CASES) if n.startswith("531_")] if name == "531" else [name]:
        occupied, radius, views, want = HAND_CASES[case]
        words = cells_pool(occupied, HAND_DEPTH) if occupied else HandPool().words()
        ws, pool = on_device(pkg, words)
        got, _ = expect(pkg, ws, pool, occupancy(words, HAND_DEPTH), HAND_DEPTH, *ROOT_REGION, radius, views)
        check_hand_case(got, want)


# ---- 3. rows, words and long walks ---------------------------------------------------------------------------------------------------
WIDE_DEPTH = 8                                                          # 256 cells a side


def wide_cases():
    """name -> (occupied cells, origin, dims, range, viewpoints) at depth 8"""
    out = {}
    for nx in (1, 63, 64, 65):                                          # rows that start at x = 37: bit 37 of the first word when R = 0
        occupied = [(36, 20, 30), (37 + nx // 2, 21, 30), (37 + nx, 19, 31), (37 + nx - 1, 20, 29), (37 + nx // 3, 20, 30)]
        views = [(35, 20, 30), (37 + nx // 2, 19, 30), (37 + nx + 3, 20, 30), (37 + nx // 2, 25, 33), (37, 20, 30)]
        out["nx_%d" % nx] = (occupied, (37, 19, 29), (nx, 3, 3), 9, views)
        out["nx_%d_range_0" % nx] = (occupied, (37, 19, 29), (nx, 3, 3), 0, views)
    # rows of 200 cells from x = 37, four words with the halo; viewpoints one, two and three words away from the cells they see
    occupied = [(100, 50, 50), (101, 51, 51), (150, 50, 51), (64, 51, 50), (127, 50, 50), (128, 51, 51), (191, 50, 51), (192, 51, 50)]
    views = [(40, 50, 50), (236, 51, 51), (130, 50, 50), (5, 50, 51), (255, 51, 50), (63, 49, 50), (64, 52, 51)]
    out["several_words"] = (occupied, (37, 50, 50), (200, 2, 2), 130, views)
    # a thin region in the middle of the root with R = 130: the inflated region is clipped by both root faces on every axis;
    # viewpoints on the root's faces, far along x, along y and along z, each with cells on some of its lines and beside others
    rng = np.random.default_rng(19)
    occupied = [(60, 121, 127), (180, 122, 126), (120, 60, 127), (125, 190, 126), (130, 121, 60), (112, 122, 200)]
    occupied += [(129, 60, 127), (129, 190, 126), (120, 122, 188), (127, 186, 123), (120, 121, 191), (127, 186, 126), (124, 60, 127)]   # halfway along other lines
    occupied += [tuple(int(t) for t in c) for c in rng.integers(90, 170, (60, 3))]
    views = [(0, 121, 127), (255, 122, 126), (120, 0, 127), (125, 250, 126), (130, 121, 0), (112, 122, 255), (129, 121, 126)]
    for tag, dims in (("x", (40, 7, 2)), ("y", (3, 40, 2)), ("z", (2, 7, 40))):   # 7 rows: y reaches both faces too
        origin = {"x": (110, 120, 126), "y": (128, 100, 126), "z": (128, 120, 100)}[tag]
        out["long_walks_thin_in_" + tag] = (occupied, origin, dims, 130, views)
    return out


WIDE_CASES = wide_cases()


@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_rows_words_and_long_walks(env, name):
    pkg, torch = env
    occupied, origin, dims, radius, views = WIDE_CASES[name]
    words = cells_pool(occupied, WIDE_DEPTH)
    occ = occupancy(words, WIDE_DEPTH)
    ws, pool = on_device(pkg, words)
    got, want = expect(pkg, ws, pool, occ, WIDE_DEPTH, origin, dims, radius, views)
    if radius:
        bits = [((want["mask"] >> np.uint32(k)) & 1).sum() for k in range(len(views))]
        assert sum(b > 0 for b in bits) >= 3 and want["count"].max() >= 2, bits
    else:                                                               # a viewpoint sees its own cell, and only if that is in the region
        assert want["count"].sum() == sum(all(origin[a] <= v[a] < origin[a] + dims[a] for a in range(3)) for v in views)
    if name.startswith("long_walks"):
        o, n = np.asarray(origin), np.asarray(dims)
        assert (o - radius < 0).all() and (o + n + radius > 256).all()   # clipped by both faces of every axis
        assert 4 * 256 * 256 * 8 <= ws.visibility_buffers()[0][1] < 6 * 256 * 256 * 8   # the whole root, four words a row, and the slot's headroom
        q = region_cells(origin, dims)
        for k, v in enumerate(views[:6]):                               # within range each far viewpoint sees some cells and not others
            in_range = (((q - np.asarray(v)) ** 2).sum(1) <= radius * radius)
            seen = ((want["mask"].reshape(-1) >> np.uint32(k)) & 1).astype(bool)
            assert (seen & in_range).sum() > 0 and (~seen & in_range).sum() > 0, (k, v)
            assert np.abs(q[in_range] - np.asarray(v)).max() > 64          # a walk over more than one word's worth of cells


# ---- 4. the viewpoints and the outputs ----------------------------------------------------------------------------------------------
def test_no_viewpoints_and_more_than_32(env, fused):
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    got = pkg.visibility_field(ws, pool, 6, origin, dims, 8, np.zeros((0, 3), np.int32), want=BOTH)
    assert got["mask"].shape == (dims[2], dims[1], dims[0]) and not got["mask"].any() and not got["count"].any()
    views = np.concatenate([choose_views(occ, 6, origin, dims, 8, 32, 85), [[2, 3, 1]]]).astype(np.int32)
    got = pkg.visibility_field(ws, pool, 6, origin, dims, 8, views, want=("count",))
    want = visibility_field_walk(occ, 6, origin, dims, 8, views)
    assert set(got) == {"count"} and "mask" not in want
    same_outputs(got, want, ("count",))
    assert (want["count"] > visibility_field_walk(occ, 6, origin, dims, 8, views[:32])["count"]).any()   # the 33rd sees something
    for names in (("mask",), BOTH):
        with pytest.raises(Exception):
            pkg.visibility_field(ws, pool, 6, origin, dims, 8, views, want=names)
    only_outside = np.array([[-1, 2, 2], [64, 0, 0], [3, 3, -2]], np.int32)  # none counts
    got = pkg.visibility_field(ws, pool, 6, origin, dims, 8, only_outside, want=BOTH)
    assert not got["mask"].any() and not got["count"].any()


def test_each_output_alone_and_both(env, fused):
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    views = choose_views(occ, 6, origin, dims, 8, 32, 85)
    want = visibility_field_walk(occ, 6, origin, dims, 8, views)
    assert len(set(want["mask"].reshape(-1).tolist())) > 4
    for names in (("mask",), ("count",), BOTH, ("count", "mask")):
        got = pkg.visibility_field(ws, pool, 6, origin, dims, 8, views, want=names)
        assert set(got) == set(names)
        same_outputs(got, want, names)
    assert set(pkg.visibility_field(ws, pool, 6, origin, dims, 8, views)) == {"mask"}    # the default


def test_as_tensor_and_views_on_the_device(env, fused):
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    origin, dims = (3, 0, 9), (61, 30, 5)
    views = choose_views(occ, 6, origin, dims, 5, 5, 31)
    got = pkg.visibility_field(ws, pool, 6, origin, dims, 5, torch.from_numpy(views).cuda(), want=BOTH, as_tensor=True)
    for name in BOTH:
        assert isinstance(got[name], torch.Tensor) and got[name].is_cuda and got[name].dtype == torch.int32 and tuple(got[name].shape) == (5, 30, 61)
    want = visibility_field_walk(occ, 6, origin, dims, 5, views)
    same_outputs({"mask": got["mask"].cpu().numpy().view(np.uint32), "count": got["count"].cpu().numpy()}, want, BOTH)


def symmetry_views(occ):
    """two lists of up to 32 viewpoints near the fused cloud, all of which count"""
    a = choose_views(occ, 6, (0, 0, 0), (64, 64, 64), 8, 32, 61, "inside")
    b = choose_views(occ, 6, (0, 0, 0), (64, 64, 64), 8, 32, 62, "inside")
    return a[counting(a, 6)], b[counting(b, 6)]


def test_sight_is_symmetric_on_the_device(env, fused):
    """the field from viewpoint a read at b equals the field from b read at a: two calls, each over the other's viewpoints"""
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    a, b = symmetry_views(occ)
    lo, hi = np.minimum(a.min(0), b.min(0)), np.maximum(a.max(0), b.max(0))
    field_a = pkg.visibility_field(ws, pool, 6, lo, hi - lo + 1, 30, a)["mask"]
    field_b = pkg.visibility_field(ws, pool, 6, lo, hi - lo + 1, 30, b)["mask"]
    ab = np.array([[(field_a[tuple((q - lo)[::-1])] >> np.uint32(i)) & 1 for q in b] for i in range(a.shape[0])])
    ba = np.array([[(field_b[tuple((q - lo)[::-1])] >> np.uint32(j)) & 1 for j in range(b.shape[0])] for q in a])
    assert np.array_equal(ab, ba) and ab.sum() > 20 and (ab == 0).sum() > 20


# ---- 5. conventions --------------------------------------------------------------------------------------------------------------
def test_a_deferred_commit_is_read_in_its_old_state(env):
    """between svoslam_svo_fuse_commit_deferred and svoslam_svo_fuse_apply the field is that of the words the pool held before the
    commit, and after the apply that of the new words; on the workspace that holds the deferred commit"""
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
    views = choose_views(occ_old, depth, origin, dims, 10, 32, 12)
    _, before = expect(pkg, ws, pool, occ_old, depth, origin, dims, 10, views)
    pkg.svo_fuse_apply(ws, pool)
    occ_new = occupancy(pool.words(), depth)
    _, after = expect(pkg, ws, pool, occ_new, depth, origin, dims, 10, views)
    # the commit changed what is seen in this region: the comparison is bit for bit, so one changed cell already tells a call that
    # read the wrong state from one that read the right one
    assert (after["mask"] != before["mask"]).any() and (occ_new != occ_old).any()


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 6
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    origin, dims = (0, 3, 10), (64, 40, 9)
    views = np.array([[20, 20, 14], [40, 10, 12], [3, 30, 30]], np.int32)
    unsynced = pkg.visibility_field(ws, pool, depth, origin, dims, 9, views, want=BOTH, as_tensor=True)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    unsynced = {"mask": unsynced["mask"].cpu().numpy().view(np.uint32), "count": unsynced["count"].cpu().numpy()}
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    occ = occupancy(pool.words(), depth)
    want = visibility_field_walk(occ, depth, origin, dims, 9, views)
    assert (want["count"] > 0).sum() > 100
    same_outputs(unsynced, want, BOTH)
    expect(pkg, ws, pool, occ, depth, origin, dims, 9, views)


def test_the_slot_is_reused_and_the_other_fields_slots_are_left_alone(env, fused):
    pkg, torch = env
    pool, words, pts, _, occ = fused
    ws = pkg.Workspace()
    assert ws.visibility_buffers() == [(0, 0)] and ws.field_buffers() == [(0, 0)] * 3 and ws.nearest_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    field = pkg.distance_field(ws, pool, 6, *small, 5)
    near = pkg.nearest_field(ws, pool, 6, *small, 5)
    field_slots, near_slots = ws.field_buffers(), ws.nearest_buffers()
    views = choose_views(occ, 6, *large, 5, 5, 77)
    first, want = expect(pkg, ws, pool, occ, 6, *large, 5, views)
    slots = ws.visibility_buffers()
    assert slots[0][0] != 0 and 64 * 45 * 8 <= slots[0][1] < 2 * 64 * 45 * 8   # one word a row, 64 rows, 40 + 5 planes, and the slot's headroom
    assert ws.field_buffers() == field_slots and ws.nearest_buffers() == near_slots
    again, _ = expect(pkg, ws, pool, occ, 6, *large, 5, views)
    assert ws.visibility_buffers() == slots                        # a second call of the same size allocates nothing
    for name in BOTH:
        assert np.array_equal(first[name], again[name])
    expect(pkg, ws, pool, occ, 6, *small, 5, views)                # a smaller call in the larger call's slot
    assert ws.visibility_buffers() == slots and ws.field_buffers() == field_slots and ws.nearest_buffers() == near_slots
    same_field(pkg.distance_field(ws, pool, 6, *small, 5), field)
    again_near = pkg.nearest_field(ws, pool, 6, *small, 5)
    assert np.array_equal(again_near["dist2"], near["dist2"]) and np.array_equal(again_near["cell"], near["cell"])
    assert ws.field_buffers() == field_slots and ws.nearest_buffers() == near_slots and ws.visibility_buffers() == slots
    same_field(field, distance_field_separable(words, 6, *small, 5))
    want_near = nearest_field_separable(words, 6, *small, 5)
    assert np.array_equal(near["dist2"], want_near["dist2"]) and np.array_equal(near["cell"], want_near["cell"])
    ws.close()                                                     # release_all releases the new slot with the rest


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    some = np.array([[1, 2, 3], [4, 4, 4]], np.int32)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got = pkg.visibility_field(ws, pool, 5, (1, 2, 3), dims, 4, some, want=BOTH)
        assert all(got[name].shape == (dims[2], dims[1], dims[0]) for name in BOTH)
    assert ws.visibility_buffers() == [(0, 0)]                     # nothing was launched, nothing allocated
    bufs = [torch.full((64,), 0x55, dtype=torch.int32, device="cuda") for _ in range(2)]
    t_views = torch.from_numpy(np.tile(some, (20, 1))).cuda()      # 40 viewpoints
    null, ptrs, d_views = C.c_void_p(0), [pkg._ptr(b) for b in bufs], pkg._ptr(t_views)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, views=d_views, n=2, out=ptrs):
        return L.svoslam_pool_visibility_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, views, n, *out, pkg._stream())
    nulls, count_only, mask_only = [null, null], [null, ptrs[1]], [ptrs[0], null]
    assert field() == 0 and field(out=count_only, n=40) == 0 and field(out=mask_only, n=32) == 0 and field(views=null, n=0) == 0
    for b in bufs:
        b.fill_(0x55)
    torch.cuda.synchronize()
    slots = ws.visibility_buffers()
    assert slots[0][1] > 0
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=nulls) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=nulls, views=null, n=0) == 0
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
        origin[a], dims[a] = 0, 33
        assert field(origin=origin, dims=dims) == -1
    assert field(radius=-1) == -1 and field(radius=4097) == -1 and field(radius=4097, dims=(0, 2, 2)) == -1
    assert field(n=-1) == -1 and field(n=-1, dims=(0, 2, 2)) == -1
    assert field(views=null, n=1) == -1 and field(views=null, n=1, dims=(0, 2, 2)) == -1
    assert field(n=33) == -1 and field(n=33, out=mask_only) == -1 and field(n=33, dims=(0, 2, 2)) == -1   # a mask has 32 bits
    assert field(out=nulls) == -1 and field(out=nulls, views=null, n=0) == -1                              # nothing asked for
    assert field(pool_ref=None) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # more than 2^31 - 1 output cells, and more than 2^31 - 1 row words: refused before anything is allocated
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 4, 4), radius=4096) == -6
    fresh = pkg.Workspace()                                        # ... also on a workspace whose slot does not exist yet
    assert field(ws_ref=fresh._h, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(ws_ref=fresh._h, depth=16, origin=(0, 4096, 4096), dims=(65536, 4, 4), radius=4096) == -6
    assert field(ws_ref=fresh._h, radius=4097) == -1 and field(ws_ref=fresh._h, n=33) == -1 and field(ws_ref=fresh._h, out=nulls) == -1
    torch.cuda.synchronize()
    assert fresh.visibility_buffers() == [(0, 0)]
    assert ws.visibility_buffers() == slots                        # none of the refused calls allocated or grew anything
    assert ws.field_buffers() == [(0, 0)] * 3 and ws.nearest_buffers() == [(0, 0)] * 3
    assert all((b == 0x55).all().item() for b in bufs)             # none of the refused calls wrote anything
    with pytest.raises(Exception):
        pkg.visibility_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097, some)
    with pytest.raises(KeyError):
        pkg.visibility_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, some, want=("steps",))
    with pytest.raises(ValueError):
        pkg.visibility_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, torch.zeros((2, 3), dtype=torch.int64, device="cuda"))
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    views = np.array([[5, 5, 5], [70, 1, 1]], np.int32)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.visibility_field(ws, pool, 6, (0, 0, 0), (64, 20, 3), 5, views, want=BOTH)
        pkg.visibility_field(ws, pool, 4, (1, 2, 3), (9, 3, 3), 70, views[:0], want=("count",))
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.visibility_field(ws, pool, 6, (0, 0, 0), (64, 0, 3), 5, views)   # nothing is launched, nothing is bracketed
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])


def test_box_to_cells_then_the_map_visibility_tool(env, fused, tmp_path):
    """tools/map_visibility.py writes mask and count of a saved map's box, with the viewpoints given in metres"""
    pkg, torch = env
    pool, words, pts, ws, occ = fused
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    metres = [pts[0] + np.float32(0.1), pts[7], pts[0] - np.float32(0.5), np.asarray(CENTER, np.float32) + np.float32(3.0 * EDGE)]
    cells = np.full((4, 3), -1, np.int32)
    for k, p in enumerate(metres):
        at = pkg.box_to_cells(6, CENTER, EDGE, np.concatenate([p, p]))
        if at is not None:
            cells[k] = at[0]
    assert (cells[3] == -1).all() and (cells[:3] >= 0).all()        # the last viewpoint lies outside the root cube
    want = visibility_field_walk(occ, 6, lo.tolist(), dims.tolist(), 12, cells)
    ckpt, out = tmp_path / "map.svopool", tmp_path / "visibility.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_visibility.py"), str(ckpt), str(out), "--range", "12", "--box"] + [repr(float(v)) for v in box]
    for p in metres:
        cmd += ["--view"] + [repr(float(v)) for v in p]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_outputs({"mask": z["mask"], "count": z["count"]}, want, BOTH)
    assert (want["count"] > 0).sum() > 50 and (want["count"] == 0).sum() > 50 and not (want["mask"] & np.uint32(8)).any()
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    assert np.array_equal(z["view_cells"], cells) and int(z["range_cells"]) == 12
    assert float(z["cell_size"]) == 2.0 * EDGE / 64
