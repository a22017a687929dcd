"""svoslam_pool_cover_views on the device: seen, chosen, gain, round and summary equal the host restatement of the specification
(tests/test_coverage_cpu.py: cover_views_host, proven there against the visibility field's mask and a brute-force cover) applied to
the pool's own words, bit for bit -- never a second device result alone.

The fused cases are test_coverage_cpu's: the words the CPU oracle fused, set on the device, so that the cases written out there as
deciding something are the ones run here.  The cases about matrix words need targets counted one by one: hand-built pools at depth
8 with COVER_ALL and a select mask on rows that start at x = 37."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_coverage_cpu import (ALL, FREE, HAND_CASES, HAND_DEPTH, MODES, OUTPUTS, SURFACE, check_hand_case, cover_views_host, draw_candidates,
                               fused_case, hand_call, hand_words, same_cover, targets_host)
from test_field_cpu import distance_field_separable, fused_regions, region_cells
from test_gpu_field import same_field
from test_gpu_query import fused_pool
from test_reach_cpu import cells_pool
from test_surface_cpu import CENTER, EDGE
from test_visibility_cpu import occupancy, visibility_field_walk
from test_volume_cpu import ROOT_CENTER, ROOT_EDGE
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_RANGES = (0, 1, 3, 8)
NO_SLOTS = [(0, 0)] * 4


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


def expect(pkg, ws, pool, occ, depth, origin, dims, radius, mode, select, cands, k_max, min_gain=1, want=None):
    """one call with every output: every value is the restatement's.  -> (the device's outputs, the restatement's)"""
    got = pkg.cover_views(ws, pool, depth, origin, dims, radius, cands, k_max, min_gain, mode, select)
    want = want or cover_views_host(occ, depth, origin, dims, radius, mode, select, cands, k_max, min_gain)
    same_cover(got, want)
    return got, want


# ---- 1. the fused pool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", sorted(fused_regions(6)))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fused_cloud(env, fused, mode, region):
    """every case of test_coverage_cpu's fused pool, and the same in the third mode: 64 candidates, up to 64 rounds"""
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)[region]
    for radius in GPU_RANGES:
        cands, want = fused_case(occ, mode, region, radius)
        got, _ = expect(pkg, ws, pool, occ, 6, origin, dims, radius, mode, None, cands, 64, want=want)
        assert got["summary"][0] == targets_host(occ, 6, origin, dims, MODES[mode]).sum()


def test_the_fused_cases_are_not_empty(fused):
    """on the restatement's results: rounds, blocked pairs, ties, rows of more than 64 words and matrices of more than 256"""
    occ = fused[2]
    _, want = fused_case(occ, "surface", "whole_root", 8)
    assert want["summary"][0] == 554 and want["summary"][1] >= 9 and want["_ties"] >= 1
    assert want["_in_range"] - want["_matrix"].sum() > 1000
    _, want = fused_case(occ, "all", "whole_root", 8)
    assert want["summary"][0] == 64 ** 3 and want["summary"][1] >= 9      # 4096 words a row
    _, want = fused_case(occ, "free", "low_corner", 8)
    assert want["summary"][0] == 2393 and want["summary"][1] >= 2 and want["_in_range"] > want["_matrix"].sum()


# ---- 2. hand-built pools -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    case = HAND_CASES[name]
    words = hand_words(case)
    ws, pool = on_device(pkg, words)
    got, _ = expect(pkg, ws, pool, occupancy(words, HAND_DEPTH), HAND_DEPTH, *hand_call(case))
    check_hand_case(got, case)


# ---- 3. words, rows and rounds at their edges ----------------------------------------------------------------------------------
WIDE_DEPTH = 8                                                          # 256 cells a side
WIDE_ORIGIN, WIDE_DIMS = (37, 19, 29), (65, 2, 2)                       # rows that start at x = 37, 260 cells
WIDE_OCCUPIED = [(36, 20, 30), (50, 19, 29), (69, 20, 29), (70, 20, 30), (88, 19, 30), (101, 20, 30), (102, 21, 30), (60, 18, 30), (75, 20, 31),
                 (45, 20, 28), (95, 19, 28), (64, 20, 29), (63, 19, 30)]


def wide_candidates(occ, count):
    """free cells around the region, seeded; from 3 on the third lies outside the root and the second repeats the first"""
    cands = draw_candidates(occ, WIDE_DEPTH, WIDE_ORIGIN, WIDE_DIMS, 6, ALL, count, 23 + count)
    if count >= 3:
        cands[2], cands[1] = (40, 20, 256), cands[0]
    return cands


@pytest.mark.parametrize("n_targets", [0, 1, 63, 64, 65, 256, 257])
def test_word_and_workgroup_edges(env, n_targets):
    """T at the edges of a matrix word and of the 256 lanes that rank the flags, n_cands at the edges of a wavefront's and a
    workgroup's candidates, k_max of 0, 1 and more than the rounds needed"""
    pkg, torch = env
    words = cells_pool(WIDE_OCCUPIED, WIDE_DEPTH)
    occ = occupancy(words, WIDE_DEPTH)
    ws, pool = on_device(pkg, words)
    select = np.zeros((WIDE_DIMS[2], WIDE_DIMS[1], WIDE_DIMS[0]), np.uint8)
    select.reshape(-1)[:n_targets] = 1
    for n_cands in (0, 1, 2, 65, 300):
        cands = wide_candidates(occ, n_cands)
        full = cover_views_host(occ, WIDE_DEPTH, WIDE_ORIGIN, WIDE_DIMS, 40, ALL, select, cands, 64)
        assert full["summary"][0] == n_targets and full["summary"][1] < 64   # 64 rounds are more than the cover needs
        for k_max in (0, 1, 64):
            got, want = expect(pkg, ws, pool, occ, WIDE_DEPTH, WIDE_ORIGIN, WIDE_DIMS, 40, ALL, select, cands, k_max, want=full if k_max == 64 else None)
            assert want["summary"][3] == full["summary"][3] and np.array_equal(want["seen"], full["seen"])
        if n_targets >= 63 and n_cands >= 65:                           # blocked pairs, several rounds, and bits in the last word
            assert full["_in_range"] > full["_matrix"].sum() > 0 and full["summary"][1] >= 2 and full["_matrix"][:, -1].any()


def test_more_candidates_than_one_grid_of_wavefronts(env):
    """262150 candidates, more than the 4 x 65535 wavefronts of a launch: the candidates that decide the cover stand at the end of
    the list, where a wavefront comes to them in its second pass, and their indices go through the round's record"""
    pkg, torch = env
    words = cells_pool([(4, 4, 4), (10, 4, 4)], 5)
    occ = occupancy(words, 5)
    ws, pool = on_device(pkg, words)
    cands = np.tile(np.array([[20, 20, 20]], np.int32), (4 * 65535 + 10, 1))   # far from both targets
    cands[262145], cands[262148], cands[262149] = (4, 6, 4), (4, 6, 4), (10, 6, 4)
    got, want = expect(pkg, ws, pool, occ, 5, (3, 3, 3), (8, 2, 2), 3, SURFACE, None, cands, 3)
    assert want["chosen"].tolist() == [262145, 262149, -1] and want["gain"].tolist() == [1, 1, 0] and want["seen"].sum() == 3
    all_cells = np.ones((2, 2, 8), np.uint8)                        # 32 targets: the far candidates see none of them
    got, want = expect(pkg, ws, pool, occ, 5, (3, 3, 3), (8, 2, 2), 3, ALL, all_cells, cands, 3)
    assert want["chosen"][0] >= 262145 and want["summary"][1] >= 2 and want["seen"][:262145].sum() == 0


# ---- 4. the same sight as the visibility field --------------------------------------------------------------------------------------
def test_seen_is_the_visibility_fields_mask_on_the_device(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    cands = draw_candidates(occ, 6, origin, dims, 8, SURFACE, 32, 77)
    cands[4], cands[6] = (3, 64, 3), cands[5]
    got = pkg.cover_views(ws, pool, 6, origin, dims, 8, cands, 0, want=("seen", "round", "summary"))
    mask = pkg.visibility_field(ws, pool, 6, origin, dims, 8, cands)["mask"]
    targets = got["round"] != -1
    assert targets.sum() == got["summary"][0] == 77 and (got["round"][targets] == -2).all()
    seen = [int(((mask[targets] >> np.uint32(c)) & 1).sum()) for c in range(32)]
    assert got["seen"].tolist() == seen and got["seen"][4] == 0 and got["seen"][6] == got["seen"][5] and max(seen) > 10
    assert got["summary"][3] == (mask[targets] != 0).sum()


# ---- 5. inputs and outputs -------------------------------------------------------------------------------------------------------
def test_tensors_in_and_out(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    cands, _ = fused_case(occ, "free", "low_corner", 8)
    select = np.ones((dims[2], dims[1], dims[0]), np.uint8)
    select[:, ::3] = 0
    want = cover_views_host(occ, 6, origin, dims, 8, FREE, select, cands, 12, 2)
    got = pkg.cover_views(ws, pool, 6, origin, dims, 8, torch.from_numpy(cands).cuda(), 12, 2, "free", torch.from_numpy(select).cuda(),
                          as_tensor=True)
    for name in OUTPUTS:
        assert isinstance(got[name], torch.Tensor) and got[name].is_cuda and got[name].dtype == torch.int32
    same_cover({name: got[name].cpu().numpy() for name in OUTPUTS}, want)
    assert want["summary"][1] >= 2 and (select.reshape(-1)[want["round"].reshape(-1) != -1] == 1).all()
    as_bool = pkg.cover_views(ws, pool, 6, origin, dims, 8, cands, 12, 2, pkg.COVER_FREE, torch.from_numpy(select != 0).cuda())
    same_cover(as_bool, want)


def test_each_optional_output_alone(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    origin, dims = fused_regions(6)["low_corner"]
    cands, want = fused_case(occ, "surface", "low_corner", 8)
    for names in (("seen",), ("round",), ("summary",), ("chosen",), ("gain",), ("chosen", "gain"), ("round", "seen"), OUTPUTS):
        got = pkg.cover_views(ws, pool, 6, origin, dims, 8, cands, 64, want=names)
        assert set(got) == set(names)
        same_cover(got, want, names)
    assert set(pkg.cover_views(ws, pool, 6, origin, dims, 8, cands, 64)) == set(OUTPUTS)    # the default
    with pytest.raises(KeyError):
        pkg.cover_views(ws, pool, 6, origin, dims, 8, cands, 64, want=("matrix",))


# ---- 6. conventions --------------------------------------------------------------------------------------------------------------
def test_a_deferred_commit_is_read_in_its_old_state(env):
    """between svoslam_svo_fuse_commit_deferred and svoslam_svo_fuse_apply the cover is that of the words the pool held before the
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
    cands = draw_candidates(occ_old, depth, origin, dims, 6, SURFACE, 40, 12)
    _, before = expect(pkg, ws, pool, occ_old, depth, origin, dims, 6, SURFACE, None, cands, 8)
    pkg.svo_fuse_apply(ws, pool)
    occ_new = occupancy(pool.words(), depth)
    _, after = expect(pkg, ws, pool, occ_new, depth, origin, dims, 6, SURFACE, None, cands, 8)
    assert (after["round"] != before["round"]).any() and before["summary"][1] >= 2 and (occ_new != occ_old).any()


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 6
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    origin, dims = (0, 3, 10), (64, 40, 9)
    cands = np.array([[20, 20, 14], [40, 10, 12], [3, 30, 30], [12, 12, 16], [25, 8, 13]], np.int32)
    unsynced = pkg.cover_views(ws, pool, depth, origin, dims, 9, cands, 4)
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    occ = occupancy(pool.words(), depth)
    want = cover_views_host(occ, depth, origin, dims, 9, SURFACE, None, cands, 4)
    assert want["summary"][2] > 20
    same_cover(unsynced, want)


def test_the_slots_are_reused_and_the_other_fields_slots_are_left_alone(env, fused, oracle_words):
    pkg, torch = env
    pool, _, occ = fused
    ws = pkg.Workspace()
    assert ws.cover_buffers() == NO_SLOTS and ws.visibility_buffers() == [(0, 0)] and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    field = pkg.distance_field(ws, pool, 6, *small, 5)
    views = np.array([[10, 10, 10], [5, 12, 9]], np.int32)
    mask = pkg.visibility_field(ws, pool, 6, *small, 5, views)["mask"]
    field_slots, vis_slots = ws.field_buffers(), ws.visibility_buffers()
    cands = draw_candidates(occ, 6, *large, 5, SURFACE, 40, 3)
    first, want = expect(pkg, ws, pool, occ, 6, *large, 5, SURFACE, None, cands, 8)
    slots = ws.cover_buffers()
    T, cells = int(want["summary"][0]), 64 * 64 * 40
    assert all(ptr != 0 for ptr, _ in slots) and want["summary"][1] >= 2
    assert 64 * 45 * 8 <= slots[0][1] < 2 * 64 * 45 * 8             # one word a row, 64 rows, 40 + 5 planes, and the slot's headroom
    assert 8 * cells <= slots[1][1] < 16 * cells                    # a rank and a list entry per region cell
    assert 40 * ((T + 63) // 64) * 8 <= slots[2][1] < 2 * 40 * ((T + 63) // 64) * 8 + 512
    assert ((T + 63) // 64 + 8) * 8 <= slots[3][1] < 2 * ((T + 63) // 64 + 8) * 8 + 512
    assert ws.field_buffers() == field_slots and ws.visibility_buffers() == vis_slots
    again, _ = expect(pkg, ws, pool, occ, 6, *large, 5, SURFACE, None, cands, 8, want=want)
    assert ws.cover_buffers() == slots                             # a second call of the same size allocates nothing
    expect(pkg, ws, pool, occ, 6, *small, 5, SURFACE, None, cands[:7], 3)   # a smaller call in the larger call's slots
    assert ws.cover_buffers() == slots and ws.field_buffers() == field_slots and ws.visibility_buffers() == vis_slots
    same_field(pkg.distance_field(ws, pool, 6, *small, 5), field)
    assert np.array_equal(pkg.visibility_field(ws, pool, 6, *small, 5, views)["mask"], mask)
    assert ws.field_buffers() == field_slots and ws.visibility_buffers() == vis_slots and ws.cover_buffers() == slots
    same_field(field, distance_field_separable(oracle_words, 6, *small, 5))
    assert np.array_equal(mask, visibility_field_walk(occ, 6, *small, 5, views)["mask"])
    ws.close()                                                     # release_all releases the new slots with the rest


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    words = cells_pool([(4, 4, 4), (10, 4, 4)], 5)
    ws, pool = on_device(pkg, words)
    L = pkg.lib()
    some = np.array([[4, 6, 4], [10, 6, 4]], np.int32)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):                 # no region: the entries past the end and a zero summary
        got = pkg.cover_views(ws, pool, 5, (1, 2, 3), dims, 4, some, 3)
        assert got["round"].shape == (dims[2], dims[1], dims[0]) and got["summary"].tolist() == [0, 0, 0, 0]
        assert got["chosen"].tolist() == [-1] * 3 and got["gain"].tolist() == [0] * 3 and got["seen"].tolist() == [0, 0]
    assert ws.cover_buffers() == NO_SLOTS                          # nothing was allocated
    bufs = [torch.full((64,), 0x55, dtype=torch.int32, device="cuda") for _ in range(5)]
    t_cands = torch.from_numpy(np.tile(some, (20, 1))).cuda()      # 40 candidates
    t_select = torch.ones(64, dtype=torch.uint8, device="cuda")
    null, ptrs, d_cands = C.c_void_p(0), [pkg._ptr(b) for b in bufs], pkg._ptr(t_cands)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def cover(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(3, 3, 3), dims=(8, 2, 2), radius=3, mode=0, select=null,
              cands=d_cands, n=2, k_max=3, min_gain=1, out=ptrs):
        return L.svoslam_pool_cover_views(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, mode, select, cands, n, k_max, min_gain,
                                          *out, pkg._stream())
    seen, chosen, gain, rounds, summary = ptrs
    assert cover() == 0 and cover(n=40, select=pkg._ptr(t_select)) == 0 and cover(cands=null, n=0) == 0
    assert cover(out=[null, chosen, gain, null, summary]) == 0 and cover(k_max=0, out=[seen, null, null, rounds, summary]) == 0
    torch.cuda.synchronize()
    assert bufs[4][:4].tolist() == [2, 0, 0, 2]                    # the last call: two targets, both coverable, no rounds
    for b in bufs:
        b.fill_(0x55)
    torch.cuda.synchronize()
    slots = ws.cover_buffers()
    assert all(size > 0 for _, size in slots)
    assert cover(ws_ref=None) == -1 and cover(origin=None) == -1 and cover(dims=None) == -1
    assert cover(ws_ref=None, dims=(0, 2, 2)) == -1 and cover(depth=0, dims=(0, 2, 2)) == -1
    assert cover(depth=0) == -1 and cover(depth=17) == -1
    assert cover(dims=(-1, 2, 2)) == -1 and cover(dims=(8, 2, -1)) == -1 and cover(dims=(0, -1, 2)) == -1
    for a in range(3):                                             # one cell outside the root on each side
        origin, dims = [3, 3, 3], [8, 2, 2]
        origin[a] = -1
        assert cover(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert cover(origin=origin) == -1
        origin[a], dims[a] = 0, 33
        assert cover(origin=origin, dims=dims) == -1
    assert cover(radius=-1) == -1 and cover(radius=4097) == -1 and cover(radius=4097, dims=(0, 2, 2)) == -1
    assert cover(n=-1) == -1 and cover(n=-1, dims=(0, 2, 2)) == -1
    assert cover(cands=null, n=1) == -1 and cover(cands=null, n=1, dims=(0, 2, 2)) == -1
    assert cover(mode=-1) == -1 and cover(mode=3) == -1 and cover(mode=3, dims=(0, 2, 2)) == -1
    assert cover(k_max=-1) == -1 and cover(k_max=1025) == -1 and cover(k_max=1025, dims=(0, 2, 2)) == -1
    assert cover(min_gain=0) == -1 and cover(min_gain=-5) == -1 and cover(min_gain=0, dims=(0, 2, 2)) == -1
    assert cover(out=[seen, chosen, gain, rounds, null]) == -1 and cover(out=[seen, chosen, gain, rounds, null], dims=(0, 2, 2)) == -1
    assert cover(out=[seen, null, gain, rounds, summary]) == -1 and cover(out=[seen, chosen, null, rounds, summary]) == -1
    assert cover(out=[seen, null, gain, rounds, summary], dims=(0, 2, 2)) == -1
    assert cover(pool_ref=None) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert cover(pool_ref=C.byref(blank)) == -1
    # more than 2^31 - 1 region cells, more than 2^31 - 1 row words, and a matrix of more than 2^29 words (one word a row here: the
    # candidates are never read): refused with nothing allocated or grown
    fresh = pkg.Workspace()
    for ref in (ws._h, fresh._h):
        assert cover(ws_ref=ref, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
        assert cover(ws_ref=ref, depth=16, origin=(0, 4096, 4096), dims=(65536, 4, 4), radius=4096) == -6
        assert cover(ws_ref=ref, mode=2, dims=(1, 1, 1), n=(1 << 29) + 1) == -6
    assert cover(ws_ref=fresh._h, radius=4097) == -1 and cover(ws_ref=fresh._h, mode=3) == -1 and cover(ws_ref=fresh._h, k_max=1025) == -1
    torch.cuda.synchronize()
    assert fresh.cover_buffers() == NO_SLOTS
    assert ws.cover_buffers() == slots                             # none of the refused calls allocated or grew anything
    assert ws.visibility_buffers() == [(0, 0)] and ws.field_buffers() == [(0, 0)] * 3
    assert all((b == 0x55).all().item() for b in bufs)             # none of the refused calls wrote anything
    assert cover(mode=2, dims=(1, 1, 1), n=40) == 0                # under the limit the same call runs
    torch.cuda.synchronize()
    small = cover_views_host(occupancy(words, 5), 5, (3, 3, 3), (1, 1, 1), 3, ALL, None, np.tile(some, (20, 1)), 3)
    assert bufs[4][:4].tolist() == small["summary"].tolist() and bufs[0][:40].tolist() == small["seen"].tolist()
    for b in bufs:
        b.fill_(0x55)
    assert cover(pool_ref=None, dims=(0, 2, 2)) == 0 and cover(pool_ref=C.byref(blank), dims=(8, 0, 2), k_max=0, out=[null] * 4 + [summary]) == 0
    torch.cuda.synchronize()
    assert bufs[1][:4].tolist() == [-1, -1, -1, 0x55] and bufs[2][:4].tolist() == [0, 0, 0, 0x55] and bufs[4][:5].tolist() == [0, 0, 0, 0, 0x55]
    assert (bufs[0] == 0x55).all().item()                          # a region without cells: nothing else is written
    with pytest.raises(Exception):
        pkg.cover_views(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097, some, 2)
    with pytest.raises(KeyError):
        pkg.cover_views(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, some, 2, targets="edges")
    with pytest.raises(ValueError):
        pkg.cover_views(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, torch.zeros((2, 3), dtype=torch.int64, device="cuda"), 2)
    with pytest.raises(ValueError):
        pkg.cover_views(ws, pool, 5, (0, 0, 0), (4, 4, 4), 3, some, 2, select=np.ones(63, np.uint8))
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, ws, occ = fused
    cands = np.array([[5, 5, 5], [70, 1, 1], [12, 14, 9]], np.int32)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.cover_views(ws, pool, 6, (0, 0, 0), (64, 20, 12), 5, cands, 6)
        pkg.cover_views(ws, pool, 6, (1, 2, 3), (9, 3, 3), 70, cands[:0], 0, targets="all")
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
    finally:
        pkg.stage_timing([])


# ---- 7. the tool -------------------------------------------------------------------------------------------------------------------
def test_the_map_cover_tool(env, tmp_path):
    """tools/map_cover.py on a saved map: candidates given in metres, and candidates taken from the box's clear cells"""
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 6, 15000, 41)
    occ = occupancy(pool.words(), 6)
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    rng = np.random.default_rng(4)
    metres = np.concatenate([pts[0] + rng.uniform(-0.4, 0.4, (30, 3)), [np.asarray(CENTER) + 3.0 * EDGE]]).astype(np.float32)
    cells = np.full((31, 3), -1, np.int32)
    for k, p in enumerate(metres):
        at = pkg.box_to_cells(6, CENTER, EDGE, np.concatenate([p, p]))
        if at is not None:
            cells[k] = at[0]
    assert (cells[30] == -1).all() and (cells[:30] >= 0).all()      # the last candidate lies outside the root cube
    want = cover_views_host(occ, 6, lo.tolist(), dims.tolist(), 12, SURFACE, None, cells, 5, 2)
    ckpt, out, npy = tmp_path / "map.svopool", tmp_path / "cover.npz", tmp_path / "cands.npy"
    pool.save(ckpt, CENTER, EDGE, 6)
    np.save(npy, metres)
    tool = [sys.executable, os.path.join(ROOT, "tools", "map_cover.py"), str(ckpt), str(out), "--range", "12", "--box"] + [repr(float(v)) for v in box]
    r = subprocess.run(tool + ["--candidates", str(npy), "--views", "5", "--min-gain", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_cover({name: z[name] for name in OUTPUTS}, want)
    assert want["summary"][1] >= 2 and want["summary"][0] > 20
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    assert np.array_equal(z["candidate_cells"], cells) and int(z["range_cells"]) == 12 and float(z["cell_size"]) == 2.0 * EDGE / 64
    n = int(want["summary"][1])
    assert np.array_equal(z["chosen_cells"][:n], cells[want["chosen"][:n]]) and (z["chosen_cells"][n:] == -1).all()
    size = 2.0 * EDGE / 64
    centres = (np.asarray(CENTER) - EDGE) + (cells[want["chosen"][:n]] + 0.5) * size
    assert np.allclose(z["chosen_centres"][:n], centres, atol=1e-5)
    # --grid: every 4th cell of the box that is 2 cells clear, by the distance field
    r = subprocess.run(tool + ["--grid", "4", "--clearance", "2", "--views", "3", "--targets", "free"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    grid = region_cells(lo.tolist(), dims.tolist())                # in region order, x fastest
    grid = grid[((grid - lo) % 4 == 0).all(1)]
    near = np.argwhere(occ)[:, ::-1]
    clear = np.array([((near - g) ** 2).sum(1).min() > 4 for g in grid])
    assert np.array_equal(z["candidate_cells"], grid[clear].astype(np.int32)) and 0 < clear.sum() < grid.shape[0]
    same_cover({name: z[name] for name in OUTPUTS}, cover_views_host(occ, 6, lo.tolist(), dims.tolist(), 12, FREE, None, grid[clear], 3))
