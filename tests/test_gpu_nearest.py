"""svoslam_pool_nearest_field on the device: every output equals the host restatement of the specification
(tests/test_nearest_cpu.py: nearest_field_words, the definition, where brute force is affordable; nearest_field_separable, proven
equal to it there, for the whole root and for the free cells of sparse pools) applied to the pool's own words -- never a second
device result alone.

The fused pools and the FREE cases work at depth 5 or 6.  The cases about column segments (ny, nz of 65 and 129), about rows of
several 64-bit words and about nx = 65 need a root of at least 256 cells a side: they use hand-built pools of a few cells at depth
8, on regions of a few hundred to a few thousand cells."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, fused_regions, midpoints
from test_gpu_field import same_field
from test_gpu_query import fused_pool
from test_nearest_cpu import (FREE, NEAREST_CASES, NO_CELL, OCCUPIED, colored_pool, nearest_field_separable, nearest_field_words,
                              nearest_untruncated, same_outputs, truncate, unpack)
from test_reach_cpu import cells_pool
from test_surface_cpu import CENTER, EDGE, MASK, occupied_cells, path_of
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_MAX_RADIUS = 64            # map_nearest.hip: a larger radius reads the intermediates from global memory
SEGMENT = 64                   # ... and a column is cut into segments of this many outputs
ALL = ("dist2", "cell", "node", "color")
FREE_OUTPUTS = ("dist2", "cell")


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


def on_device(pkg, words):
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    return ws, pool


def outputs_of(which):
    return ALL if which == OCCUPIED else FREE_OUTPUTS


def expect(pkg, ws, pool, depth, origin, dims, radius, which, want):
    """one call with every output the target set allows: every value is the restatement's; cell_xyz is the cell unpacked"""
    got = pkg.nearest_field(ws, pool, depth, origin, dims, radius, which=which, want=outputs_of(which))
    same_outputs(got, want, outputs_of(which))
    assert got["cell_xyz"].dtype == np.int32 and np.array_equal(got["cell_xyz"], unpack(want["cell"]))
    return got


# ---- 1. the fused pool ---------------------------------------------------------------------------------------------------------
FUSED_RADII = (0, 1, 3, LDS_MAX_RADIUS, LDS_MAX_RADIUS + 1)


@pytest.fixture(scope="module")
def reference(fused):
    """(region, which, radius) -> the outputs by the definition: brute force once per (region, which), truncated per radius; for
    the whole root the separable restatement"""
    words = fused[1]
    cache = {}

    def get(region, which, radius):
        origin, dims = fused_regions(6)[region]
        if region == "whole_root":
            if (region, which, radius) not in cache:
                cache[(region, which, radius)] = nearest_field_separable(words, 6, origin, dims, radius, which)
            return cache[(region, which, radius)]
        if (region, which) not in cache:
            cache[(region, which)] = nearest_untruncated(words, 6, origin, dims, which)
        return truncate(words, dims, radius, *cache[(region, which)])
    return get


@pytest.mark.parametrize("which", [OCCUPIED, FREE])
@pytest.mark.parametrize("region", sorted(fused_regions(6)))
def test_fused_cloud(env, fused, reference, region, which):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)[region]
    for radius in FUSED_RADII:
        expect(pkg, ws, pool, 6, origin, dims, radius, which, reference(region, which, radius))


def test_the_fused_cases_are_not_empty(fused, reference):
    """on the restatement's results: found and none, witnesses outside their region, ties the rule has to decide, occupied cells
    with a positive depth"""
    words = fused[1]
    occ = occupied_cells(words, 6)[0]
    found = none = outside = tied = deep = 0
    for region, (origin, dims) in fused_regions(6).items():
        want = reference(region, OCCUPIED, 3)
        ok = want["dist2"].reshape(-1) >= 0
        found, none = found + int(ok.sum()), none + int((~ok).sum())
        wit = unpack(want["cell"]).reshape(-1, 3)
        outside += int((ok & ((wit < np.asarray(origin)) | (wit >= np.asarray(origin) + np.asarray(dims))).any(1)).sum())
        z, y, x = np.nonzero(want["dist2"] > 0)
        q = (np.stack([x, y, z], 1) + np.asarray(origin))[:300]
        d2 = ((q[:, None, :] - occ[None, :, :]) ** 2).sum(2)
        tied += int(((d2 == d2.min(1)[:, None]).sum(1) > 1).sum())
        deep += int((reference(region, FREE, 3)["dist2"] > 0).sum())
    assert found > 1000 and none > 100 and outside >= 1 and tied > 50 and deep > 20, (found, none, outside, tied, deep)


# ---- 2. ties, hand-built: the region a few cells wide -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NEAREST_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, origin, dims, radius, which, want = NEAREST_CASES[name]
    ws, pool = on_device(pkg, words)
    expect(pkg, ws, pool, depth, origin, dims, radius, which, want)
    expect(pkg, ws, pool, depth, origin, dims, radius, which, nearest_field_words(words, depth, origin, dims, radius, which))


@pytest.mark.parametrize("radius", [2, 3, LDS_MAX_RADIUS, LDS_MAX_RADIUS + 1])
def test_ties_on_both_paths(env, radius):
    """the six cells at distance 2 about (9,9,9) at depth 5, each alone and in every combination of axes, on a region a few cells
    wide in which the winning witnesses lie outside: with R = 65 through the global-memory form"""
    pkg, torch = env
    c = 9
    six = {"x": [(c - 2, c, c), (c + 2, c, c)], "y": [(c, c - 2, c), (c, c + 2, c)], "z": [(c, c, c - 2), (c, c, c + 2)]}
    for axes in ("x", "y", "z", "xy", "xz", "yz", "xyz"):
        cells = [cell for a in axes for cell in six[a]]
        words, where = colored_pool(cells[::-1], 5)                 # put in descending order: the node numbers do not follow the rule
        ws, pool = on_device(pkg, words)
        origin, dims = (c - 1, c - 1, c - 1), (3, 3, 3)             # x, y, z 8..10: none of the six is inside
        want = nearest_field_words(words, 5, origin, dims, radius, OCCUPIED)
        winner = six[axes[-1]][0]                                   # the lowest cell of the last axis: z before y before x
        assert want["dist2"][1, 1, 1] == 4 and unpack(want["cell"])[1, 1, 1].tolist() == list(winner)
        assert (want["node"][1, 1, 1], want["color"][1, 1, 1]) == where[winner]
        expect(pkg, ws, pool, 5, origin, dims, radius, OCCUPIED, want)


# ---- 3. the edges of the machinery ---------------------------------------------------------------------------------------------------
WIDE_DEPTH = 8                                                          # 256 cells a side


def wide_cases():
    """name -> (occupied cells, origin, dims, radius) at depth 8"""
    out = {}
    for n in (65, 129):
        # a column along y (and along z) of n outputs, 3 cells wide in x: occupied cells just before a segment boundary, whose
        # nearest outputs lie behind it; one inside the halo below the region; the region starts 5 cells from the root's face, so
        # the halo is clipped by it; two cells at equal distance from output 64 + 20, of which the lower is in the segment before
        cells_y = [(101, 5 + 60, 77), (100, 5 + 100, 77), (102, 2, 77), (100, 5 + 63, 78), (100, 5 + 105, 78)]
        out["ny_%d" % n] = (cells_y, (100, 5, 77), (3, n, 1), 40)
        out["ny_%d_two_planes" % n] = (cells_y, (100, 5, 77), (3, n, 2), LDS_MAX_RADIUS)
        cells_z = [(x, z, y) for x, y, z in cells_y]
        out["nz_%d" % n] = (cells_z, (100, 77, 5), (3, 1, n), 40)
        out["nz_%d_global" % n] = (cells_z, (100, 77, 5), (3, 1, n), LDS_MAX_RADIUS + 6)
        # ... and against the high face
        high = [(101, 255 - 3, 77), (100, 255 - n + 10, 77), (101, 255 - 70, 76)]
        out["ny_%d_high_face" % n] = (high, (100, 256 - n, 77), (3, n, 1), 50)
    # the region's rows start at x = 37 and span three 64-bit words with the halo; one occupied cell about 100 cells away in x, at
    # R = 130: whole words are skipped in the x pass, below and above
    out["word_skip_above"] = ([(37 + 139, 50, 50)], (37, 49, 50), (40, 3, 1), 130)
    out["word_skip_below"] = ([(3, 50, 50)], (100, 50, 49), (70, 1, 3), 130)
    out["word_skip_tie"] = ([(20, 50, 50), (220, 50, 50)], (110, 50, 50), (21, 1, 1), 130)  # x = 120 is 100 from both: the lower
    for nx in (1, 63, 64, 65):
        out["nx_%d" % nx] = ([(36, 20, 30), (37 + nx // 2, 21, 30), (37 + nx, 19, 31), (37 + nx - 1, 20, 29)], (37, 19, 29), (nx, 3, 3), 9)
    return out


WIDE_CASES = wide_cases()


@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_sizes_offsets_and_segments(env, name):
    pkg, torch = env
    cells, origin, dims, radius = WIDE_CASES[name]
    words, where = colored_pool(cells, WIDE_DEPTH)
    want = nearest_field_words(words, WIDE_DEPTH, origin, dims, radius, OCCUPIED)
    assert (want["dist2"] >= 0).sum() > 0 and len(set(want["cell"].reshape(-1).tolist())) >= min(len(cells), 2)
    if name == "word_skip_tie":
        assert want["dist2"][0, 0, 10] == 10000 and unpack(want["cell"])[0, 0, 10].tolist() == [20, 50, 50]
    if name.startswith("ny_129") and "high" not in name:            # a witness in the segment before the output's own
        wit = unpack(want["cell"])[0, :, 0, 1] - origin[1]
        assert ((wit >= 0) & (wit < SEGMENT) & (np.arange(dims[1]) >= SEGMENT)).any()
    ws, pool = on_device(pkg, words)
    expect(pkg, ws, pool, WIDE_DEPTH, origin, dims, radius, OCCUPIED, want)
    free = pkg.nearest_field(ws, pool, WIDE_DEPTH, origin, dims, min(radius, 3), which=FREE)   # the complement on the same rows
    same_outputs(free, nearest_field_separable(words, WIDE_DEPTH, origin, dims, min(radius, 3), FREE), FREE_OUTPUTS)


# ---- 4. FREE -----------------------------------------------------------------------------------------------------------------------
def full_root(depth):
    n = 1 << depth
    return [(x, y, z) for z in range(n) for y in range(n) for x in range(n)]


def node_of(words, xyz, depth):
    """the level-`depth` node on the path of cell xyz, all of whose levels exist"""
    base = 0
    for o in path_of(*xyz, depth):
        node = base + o
        base = int(words[2 * node]) & MASK
    return node


def grid(origin, dims):
    """[nz, ny, nx, 3]: x, y, z of every cell of the region"""
    z, y, x = np.meshgrid(*[np.arange(origin[a], origin[a] + dims[a]) for a in (2, 1, 0)], indexing="ij")
    return np.stack([x, y, z], -1)


@pytest.fixture(scope="module")
def solid_5(env):
    """a fully occupied depth-5 root on the device (a row is 32 cells, half a row word), and one with the free pocket (20,9,13)"""
    pkg, torch = env
    pocket = (20, 9, 13)
    full = cells_pool(full_root(5), 5)
    holed = full.copy()
    holed[2 * node_of(full, pocket, 5) + 1] = 0                      # alpha 0: the leaf is free, its node stays
    assert occupied_cells(holed, 5)[0].shape[0] == 32 ** 3 - 1
    return on_device(pkg, full), full, on_device(pkg, holed), holed, pocket


def test_free_of_a_fully_occupied_root_is_none_everywhere(env, solid_5):
    """R = 40 reaches past every face of the 32-cell root: bits past the row's end or outside the root would read as free"""
    pkg, torch = env
    (ws, pool), words = solid_5[0], solid_5[1]
    for radius in (40, LDS_MAX_RADIUS + 1):
        got = pkg.nearest_field(ws, pool, 5, (0, 0, 0), (32, 32, 32), radius, which=FREE)
        assert (got["dist2"] == -1).all() and (got["cell"] == NO_CELL).all() and (got["cell_xyz"] == -1).all()
    got = pkg.nearest_field(ws, pool, 5, (3, 30, 0), (29, 2, 7), 40, which=FREE)
    assert (got["dist2"] == -1).all() and (got["cell"] == NO_CELL).all()
    occ = pkg.nearest_field(ws, pool, 5, (3, 30, 0), (29, 2, 7), 40, which=OCCUPIED)
    assert (occ["dist2"] == 0).all() and np.array_equal(occ["cell_xyz"], grid((3, 30, 0), (29, 2, 7)))


def test_free_of_a_solid_block_with_one_pocket(env, solid_5):
    pkg, torch = env
    (ws, pool), words, pocket = solid_5[2], solid_5[3], solid_5[4]
    origin, dims = (0, 0, 0), (32, 32, 32)
    z, y, x = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    depth2 = ((x - pocket[0]) ** 2 + (y - pocket[1]) ** 2 + (z - pocket[2]) ** 2).astype(np.int32)
    for radius in (5, 40):
        got = pkg.nearest_field(ws, pool, 5, origin, dims, radius, which=FREE)
        ok = depth2 <= radius * radius
        same_field(got["dist2"], np.where(ok, depth2, -1).astype(np.int32))            # the depths, exactly
        assert (got["cell_xyz"][ok] == np.asarray(pocket)).all() and (got["cell"][~ok] == NO_CELL).all()
        same_outputs(got, nearest_field_separable(words, 5, origin, dims, radius, FREE), FREE_OUTPUTS)
    occ = pkg.nearest_field(ws, pool, 5, origin, dims, 2, which=OCCUPIED)               # the pocket is one cell from six occupied ones
    assert occ["dist2"][pocket[2], pocket[1], pocket[0]] == 1 and (occ["dist2"] == 0).sum() == 32 ** 3 - 1
    assert occ["cell_xyz"][pocket[2], pocket[1], pocket[0]].tolist() == [pocket[0], pocket[1], pocket[2] - 1]


def test_free_in_a_free_region_is_the_cell_itself(env):
    pkg, torch = env
    words, _ = colored_pool([(1, 1, 1), (30, 30, 30)], 5)
    ws, pool = on_device(pkg, words)
    origin, dims = (5, 6, 7), (20, 9, 4)
    for radius in (0, 7):
        got = pkg.nearest_field(ws, pool, 5, origin, dims, radius, which=FREE)
        assert (got["dist2"] == 0).all()
        assert np.array_equal(got["cell_xyz"], grid(origin, dims))
        same_outputs(got, nearest_field_words(words, 5, origin, dims, radius, FREE), FREE_OUTPUTS)


# ---- 5. cross-checks on the device ---------------------------------------------------------------------------------------------------
def test_dist2_is_the_distance_field_and_the_node_is_the_query_calls(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    mids = [midpoints(6, CENTER, EDGE, [0, 0, 0], [64 if a == b else 1 for b in range(3)])[:, a] for a in range(3)]
    for region, (origin, dims) in sorted(fused_regions(6).items()):
        for radius in (3, LDS_MAX_RADIUS + 1):
            got = pkg.nearest_field(ws, pool, 6, origin, dims, radius, want=ALL)
            same_field(got["dist2"], pkg.distance_field(ws, pool, 6, origin, dims, radius))
            ok = got["dist2"].reshape(-1) >= 0
            wit = got["cell_xyz"].reshape(-1, 3)[ok]
            at = np.stack([mids[a][wit[:, a]] for a in range(3)], 1).astype(np.float32)
            there = pkg.query_points(pool, 6, CENTER, EDGE, at, outputs=("node", "level", "color"))
            assert (there["level"] == 6).all()
            assert np.array_equal(there["node"], got["node"].reshape(-1)[ok]) and np.array_equal(there["color"], got["color"].reshape(-1)[ok])
            assert (got["node"].reshape(-1)[~ok] == -1).all() and (got["color"].reshape(-1)[~ok] == 0).all()


def test_each_output_alone_and_each_left_out(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)["low_corner"]
    full = pkg.nearest_field(ws, pool, 6, origin, dims, 3, want=ALL)
    for name in ALL:
        alone = pkg.nearest_field(ws, pool, 6, origin, dims, 3, want=(name,))
        assert set(alone) == {name} | ({"cell_xyz"} if name == "cell" else set())
        same_outputs(alone, full, (name,))
        rest = tuple(n for n in ALL if n != name)
        same_outputs(pkg.nearest_field(ws, pool, 6, origin, dims, 3, want=rest), full, rest)


def test_as_tensor(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = (3, 0, 9), (61, 30, 5)
    got = pkg.nearest_field(ws, pool, 6, origin, dims, 5, want=ALL, as_tensor=True)
    kinds = {"dist2": torch.int32, "cell": torch.int64, "node": torch.int32, "color": torch.int32}
    for name in ALL:
        assert isinstance(got[name], torch.Tensor) and got[name].is_cuda and got[name].dtype == kinds[name] and tuple(got[name].shape) == (5, 30, 61)
    assert tuple(got["cell_xyz"].shape) == (5, 30, 61, 3) and got["cell_xyz"].dtype == torch.int32
    want = nearest_field_separable(words, 6, origin, dims, 5)
    same_outputs({"dist2": got["dist2"].cpu().numpy(), "cell": got["cell"].cpu().numpy().view(np.uint64), "node": got["node"].cpu().numpy(),
                  "color": got["color"].cpu().numpy().view(np.uint32)}, want)
    assert np.array_equal(got["cell_xyz"].cpu().numpy(), unpack(want["cell"]))


# ---- 6. conventions --------------------------------------------------------------------------------------------------------------
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
    before = {}
    for which in (OCCUPIED, FREE):
        before[which] = nearest_field_separable(old, depth, origin, dims, 4, which)
        expect(pkg, ws, pool, depth, origin, dims, 4, which, before[which])
    pkg.svo_fuse_apply(ws, pool)
    new = pool.words()
    for which in (OCCUPIED, FREE):
        want = nearest_field_separable(new, depth, origin, dims, 4, which)
        # the commit changed witnesses in this region: the comparison is bit for bit, so one changed cell already tells a call that
        # read the wrong state from one that read the right one
        assert (want["cell"] != before[which]["cell"]).any() and (want["dist2"] != before[which]["dist2"]).any()
        expect(pkg, ws, pool, depth, origin, dims, 4, which, want)


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 6
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    origin, dims = (0, 3, 10), (64, 40, 9)
    unsynced = pkg.nearest_field(ws, pool, depth, origin, dims, 9, want=ALL, as_tensor=True)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    unsynced = {"dist2": unsynced["dist2"].cpu().numpy(), "cell": unsynced["cell"].cpu().numpy().view(np.uint64),
                "node": unsynced["node"].cpu().numpy(), "color": unsynced["color"].cpu().numpy().view(np.uint32)}
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    want = nearest_field_separable(pool.words(), depth, origin, dims, 9)
    assert (want["dist2"] == 0).sum() > 100 and (want["dist2"] > 0).sum() > 100
    same_outputs(unsynced, want)
    expect(pkg, ws, pool, depth, origin, dims, 9, OCCUPIED, want)


def test_workspace_slots_are_reused_and_the_distance_fields_are_left_alone(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused
    ws = pkg.Workspace()
    assert ws.nearest_buffers() == [(0, 0)] * 3 and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    field = pkg.distance_field(ws, pool, 6, *small, 5)
    field_slots = ws.field_buffers()
    want = nearest_field_separable(words, 6, *large, 5)
    first = expect(pkg, ws, pool, 6, *large, 5, OCCUPIED, want)
    slots = ws.nearest_buffers()
    assert all(p != 0 and b > 0 for p, b in slots) and ws.field_buffers() == field_slots   # what the distance-field call left
    again = expect(pkg, ws, pool, 6, *large, 5, OCCUPIED, want)
    assert ws.nearest_buffers() == slots                           # a second call of the same size allocates nothing
    for name in ALL:
        assert np.array_equal(first[name], again[name])
    for which in (OCCUPIED, FREE):                                 # a smaller call in the larger call's slots
        got = expect(pkg, ws, pool, 6, *small, 5, which, nearest_field_separable(words, 6, *small, 5, which))
    assert ws.nearest_buffers() == slots and ws.field_buffers() == field_slots
    same_field(pkg.distance_field(ws, pool, 6, *small, 5), field)
    assert ws.field_buffers() == field_slots
    same_field(field, distance_field_separable(words, 6, *small, 5))
    ws.close()                                                     # release_all releases the new slots with the rest


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got = pkg.nearest_field(ws, pool, 5, (1, 2, 3), dims, 4, want=ALL)
        assert all(got[name].shape == (dims[2], dims[1], dims[0]) for name in ALL) and got["cell_xyz"].shape == (dims[2], dims[1], dims[0], 3)
    assert ws.nearest_buffers() == [(0, 0)] * 3                    # nothing was launched, nothing allocated
    bufs = [torch.full((64,), 0x55, dtype=torch.int64, device="cuda") for _ in range(4)]
    null, ptrs = C.c_void_p(0), [pkg._ptr(b) for b in bufs]

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, which=OCCUPIED, out=ptrs):
        return L.svoslam_pool_nearest_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, which, *out, pkg._stream())
    free_out, nulls = ptrs[:2] + [null, null], [null] * 4
    assert field() == 0 and field(which=FREE, out=free_out) == 0
    for b in bufs:
        b.fill_(0x55)
    torch.cuda.synchronize()
    slots = ws.nearest_buffers()
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=nulls) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=nulls) == 0
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
    assert field(which=-1) == -1 and field(which=2) == -1 and field(which=2, dims=(0, 2, 2)) == -1
    assert field(which=FREE) == -1                                 # FREE takes no node and no colour
    assert field(which=FREE, out=ptrs[:2] + [ptrs[2], null]) == -1 and field(which=FREE, out=ptrs[:2] + [null, ptrs[3]]) == -1
    assert field(out=nulls) == -1 and field(which=FREE, out=nulls) == -1   # nothing asked for
    assert field(pool_ref=None) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # more than 2^31 - 1 output cells, and an intermediate of more than 2^31 - 1 elements: refused before anything is allocated
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), radius=4096) == -6
    torch.cuda.synchronize()
    assert ws.nearest_buffers() == slots and ws.field_buffers() == [(0, 0)] * 3
    assert all((b == 0x55).all().item() for b in bufs)             # none of the refused calls wrote anything
    with pytest.raises(Exception):
        pkg.nearest_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097)
    with pytest.raises(Exception):
        pkg.nearest_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, which=FREE, want=("node",))
    with pytest.raises(KeyError):
        pkg.nearest_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, want=("steps",))
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.nearest_field(ws, pool, 6, (0, 0, 0), (64, 20, 3), 5, want=ALL)
        pkg.nearest_field(ws, pool, 4, (1, 2, 3), (9, 3, 3), LDS_MAX_RADIUS + 1, which=FREE)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.nearest_field(ws, pool, 6, (0, 0, 0), (64, 0, 3), 5)   # nothing is launched, nothing is bracketed
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])


def test_box_to_cells_then_the_map_gradient_tool(env, fused, tmp_path):
    """tools/map_gradient.py writes both fields of a saved map's box, the signed distance and the unit vectors"""
    pkg, torch = env
    pool, words, pts, ws = fused
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    occ = nearest_field_separable(words, 6, lo.tolist(), dims.tolist(), 7, OCCUPIED)
    free = nearest_field_separable(words, 6, lo.tolist(), dims.tolist(), 7, FREE)
    ckpt, out = tmp_path / "map.svopool", tmp_path / "gradient.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_gradient.py"), str(ckpt), str(out), "--radius", "7", "--box"] +
                       [repr(float(v)) for v in box], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_field(z["dist2_occupied"], occ["dist2"])
    same_field(z["dist2_free"], free["dist2"])
    assert np.array_equal(z["witness_occupied"], unpack(occ["cell"])) and np.array_equal(z["witness_free"], unpack(free["cell"]))
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    cell = 2.0 * EDGE / 64
    assert float(z["cell_size"]) == cell
    inside = occ["dist2"] == 0
    assert inside.sum() > 20 and (~inside).sum() > 100
    mag = np.where(inside, -np.sqrt(np.maximum(free["dist2"], 0).astype(np.float64)), np.sqrt(np.maximum(occ["dist2"], 0).astype(np.float64))) * cell
    none = np.where(inside, free["dist2"], occ["dist2"]) < 0
    want = np.where(none, np.where(inside, -np.inf, np.inf), mag).astype(np.float32)
    assert z["signed_metres"].dtype == np.float32 and np.array_equal(z["signed_metres"], want)
    q = grid(lo, dims)
    wit = np.where(inside[..., None], unpack(free["cell"]), unpack(occ["cell"]))
    vec = np.where(none[..., None], 0, q - wit).astype(np.float64)
    norm = np.sqrt((vec ** 2).sum(-1, keepdims=True))
    unit = np.where(norm > 0, vec / np.maximum(norm, 1e-30), 0.0).astype(np.float32)
    assert z["direction"].dtype == np.float32 and np.array_equal(z["direction"], unit)
