"""svoslam_pool_owner_field on the device: steps and owner equal, value for value, the host restatement of the specification
(tests/test_owner_cpu.py: owner_field_words, one reach field per label and the smallest label at the minimum) applied to the pool's
own words -- never a second device result alone.  The cases are the smallest shapes at which the kernels can go wrong: the hand
pools in both seed forms, random occupancy at every edge of a row word and a tile, ties that lie on tile faces, an owner that
reaches a converged tile rounds late, the serpentine maze, label fields grown in place, and segment_rooms against its restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_components_cpu import component_labels_words
from test_field_cpu import distance_field_separable
from test_gpu_field import FUSED_CASES as FIELD_FUSED_CASES, case_region, same_field
from test_gpu_query import fused_pool
from test_gpu_reach import MAZE_DEPTH, maze
from test_owner_cpu import (FACE_DEPTH, FACE_DIMS, FACE_ORIGIN, FACE_PAIRS, LATE_DEPTH, LATE_DIMS, LATE_ORIGIN, OWNER_CASES, RANDOM_CASES,
                            ROOMS_DEPTH, ROOMS_DIMS, ROOMS_ORIGIN, face_seeds, field_of_list, late_pool, owner_field_words, random_case,
                            rooms_pool, rooms_scene_expected, segment_rooms_words)
from test_reach_cpu import cells_pool, reach_field_words, seeds_for
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE, occupied_cells
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {"rounds", "tile_runs", "seeds_used", "owner_rounds", "owner_tile_runs"}


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """(pool, its words, the fused points, workspace) at depth 6: fused on the device, shared by the tests below, left unchanged"""
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 6, 15000, 41)
    return pool, pool.words(), pts, ws


@pytest.fixture(scope="module")
def pools(env):
    """words -> (pool, workspace) on the device, one per distinct set of words"""
    pkg, torch = env
    cache = {}

    def get(words):
        key = words.tobytes() if hasattr(words, "tobytes") else bytes(words)
        if key not in cache:
            ws, pool = pkg.Workspace(), pkg.Pool()
            pool.set_words(words)
            cache[key] = (pool, ws)
        return cache[key]
    return get


def own(pkg, ws, pool, depth, origin, dims, clearance, seeds=None, seed_field=None, **kw):
    stats = {}
    steps, owner = pkg.owner_field(ws, pool, depth, origin, dims, clearance, seeds=seeds, seed_field=seed_field, stats=stats, **kw)
    return steps, owner, stats


def expect(pkg, ws, pool, words, depth, origin, dims, clearance, seeds=None, seed_field=None, want=None):
    """one call in the given form, compared with the brute force on `words` (`want`: its result, when the caller has it)"""
    if want is None:
        want = owner_field_words(words, depth, origin, dims, clearance, seeds, seed_field)
    steps, owner, stats = own(pkg, ws, pool, depth, origin, dims, clearance, seeds, seed_field)
    same_field(steps, want[0])
    same_field(owner, want[1])
    assert stats["seeds_used"] == want[2] and set(stats) == STATS
    return steps, owner, stats


# ---- hand-built pools, in both seed forms ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["list", "field"])
@pytest.mark.parametrize("name", sorted(OWNER_CASES))
def test_hand_built_pools(env, pools, name, form):
    pkg, torch = env
    words, depth, origin, dims, clearance, seeds, seed_field, want_steps, want_owner, used = OWNER_CASES[name]
    pool, ws = pools(words)
    if form == "list" and seeds is None:                                # a field form's seeds as a list: labels become indices
        at = np.argwhere((seed_field >= 0) & (seed_field < (1 << 31) - 1))
        seeds = at[:, ::-1] + np.asarray(origin)
        want = owner_field_words(words, depth, origin, dims, clearance, seeds)
        expect(pkg, ws, pool, words, depth, origin, dims, clearance, seeds, want=want)
        return
    if form == "field" and seed_field is None:                          # a list's seeds as a field: a cell carries its smallest index
        seed_field = field_of_list(origin, dims, seeds)
        cells = int(((seed_field >= 0) & (want_steps == 0)).sum())
        steps, owner, stats = own(pkg, ws, pool, depth, origin, dims, clearance, seed_field=seed_field)
        same_field(steps, want_steps)
        same_field(owner, want_owner)
        assert stats["seeds_used"] == cells                             # seed cells, not entries
        return
    steps, owner, stats = expect(pkg, ws, pool, words, depth, origin, dims, clearance, seeds, seed_field, want=(want_steps, want_owner, used))
    assert stats["rounds"] >= 1 and stats["owner_rounds"] >= 1 and stats["owner_tile_runs"] >= (1 if used else 0)


# ---- random occupancy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "p%s-%dx%dx%d-r%d-seeds%d" % (c[0], *c[2], c[3], c[4]))
def test_random_occupancy(env, pools, case):
    pkg, torch = env
    words, depth, origin, dims, clearance, seeds, want_steps, want_owner, used, ties = random_case(case)
    pool, ws = pools(words)
    steps, owner, stats = expect(pkg, ws, pool, words, depth, origin, dims, clearance, seeds, want=(want_steps, want_owner, used))
    same_field(pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds), steps)      # the device's own reach field
    same_field(own(pkg, ws, pool, depth, origin, dims, clearance, seed_field=field_of_list(origin, dims, seeds))[1], want_owner)


# ---- ties on tile faces ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("name", sorted(FACE_PAIRS))
def test_ties_across_tile_faces(env, pools, name, swapped):
    pkg, torch = env
    words = HandPool().words()
    pool, ws = pools(words)
    seeds, axis, plane = face_seeds(name, swapped)
    expect(pkg, ws, pool, words, FACE_DEPTH, FACE_ORIGIN, FACE_DIMS, 0, seeds)


def test_a_seed_alone_on_a_tile_face(env, pools):
    """a seed whose only free neighbour lies across a tile face: nothing in the seed's own tile is lowered, and the tile across
    the face must run all the same -- for the steps and for the owners, in both seed forms, and for the reach field itself"""
    pkg, torch = env
    depth, origin, dims = 8, (0, 9, 9), (130, 1, 1)
    words = cells_pool([(x, 9, 9) for x in (62, 120)], depth)
    pool, ws = pools(words)
    seeds = [(63, 9, 9), (64, 9, 9), (128, 9, 9)]
    for chosen in (seeds[:1], seeds[1:2], seeds[::-1]):
        want = owner_field_words(words, depth, origin, dims, 0, chosen)
        assert (want[0][0, 0, 64:120] >= 0).all() and (want[0][0, 0, :62] == -1).all()
        expect(pkg, ws, pool, words, depth, origin, dims, 0, chosen, want=want)
        same_field(own(pkg, ws, pool, depth, origin, dims, 0, seed_field=field_of_list(origin, dims, chosen))[1], want[1])
        same_field(pkg.reach_field(ws, pool, depth, origin, dims, 0, chosen), want[0])


# ---- the owner that arrives late ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_label_far", [True, False])
def test_the_late_owner_lowers_a_converged_tile(env, pools, low_label_far):
    """tests/test_owner_cpu.py asserts the geometry: the last tile's row 0 is as near to the seed coiled up inside that tile, which
    reaches it in the first round, as to the seed three tile faces away, whose label is the smaller one when low_label_far"""
    pkg, torch = env
    words, seeds = late_pool(low_label_far)
    pool, ws = pools(words)
    steps, owner, stats = expect(pkg, ws, pool, words, LATE_DEPTH, LATE_ORIGIN, LATE_DIMS, 0, seeds)
    assert (owner[0, 0, 192:] == 0).all() and stats["owner_rounds"] >= 4 and stats["owner_tile_runs"] > 4
    expect(pkg, ws, pool, words, LATE_DEPTH, LATE_ORIGIN, LATE_DIMS, 0, seed_field=field_of_list(LATE_ORIGIN, LATE_DIMS, seeds))


def test_serpentine_maze(env, pools):
    """section 16's maze with walls every second row: the shortest path, and with it the owner, enters a tile three separate times;
    a second seed with the smaller label in the last open corridor owns the maze's far half"""
    pkg, torch = env
    words, origin, dims, seed = maze(2, 14)
    last = (origin[0] + dims[0] - 1, origin[1] + 14 * 2, origin[2] + 1)
    field = distance_field_separable(words, MAZE_DEPTH, origin, dims, 0)
    for seeds in ([last, seed], [seed, last], [seed]):
        want = owner_field_words(words, MAZE_DEPTH, origin, dims, 0, seeds, field=field)
        assert want[2] == len(seeds) and all((want[1] == k).sum() > 500 for k in range(len(seeds))) and (want[0] == -1).sum() > 0
        pool, ws = pools(words)
        steps, owner, stats = expect(pkg, ws, pool, words, MAZE_DEPTH, origin, dims, 0, seeds, want=want)
        assert stats["owner_rounds"] > 7


# ---- the field form ------------------------------------------------------------------------------------------------------------------
GROW_REGION = ((2, 0, 6), (61, 40, 12))


def test_a_label_field_is_grown_in_place_and_out_of_place(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = GROW_REGION
    cores = component_labels_words(words, 6, origin, dims, 2, False, field=distance_field_separable(words, 6, origin, dims, 2))
    want = owner_field_words(words, 6, origin, dims, 0, seed_field=cores)
    assert len(set(cores[cores >= 0].tolist())) >= 2 and ((want[1] >= 0) & (cores < 0)).sum() > 1000 and (want[0] == -2).sum() > 100
    labels = pkg.label_components(ws, pool, 6, origin, dims, 2, as_tensor=True)
    same_field(labels.cpu().numpy(), cores)
    keep = labels.clone()
    stats = {}
    steps, owner = pkg.owner_field(ws, pool, 6, origin, dims, 0, seed_field=labels, as_tensor=True, stats=stats)     # out of place
    assert owner.data_ptr() != labels.data_ptr() and torch.equal(labels, keep) and stats["seeds_used"] == want[2] == int((cores >= 0).sum())
    same_field(steps.cpu().numpy(), want[0])
    same_field(owner.cpu().numpy(), want[1])
    steps2, grown = pkg.owner_field(ws, pool, 6, origin, dims, 0, seed_field=labels, as_tensor=True, owner=labels)   # in place
    assert grown.data_ptr() == labels.data_ptr() and torch.equal(grown, owner) and torch.equal(steps2, steps)
    same_field(pkg.owner_field(ws, pool, 6, origin, dims, 0, seed_field=cores)[1], want[1])                          # an array


@pytest.mark.parametrize("door,min_core", [(1, 1), (0, 5), (0, 1), (1, 8)])
def test_segment_rooms_on_the_hand_scene(env, pools, door, min_core):
    pkg, torch = env
    words = rooms_pool()
    pool, ws = pools(words)
    want = segment_rooms_words(words, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, door, min_core)
    got = pkg.segment_rooms(ws, pool, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, door, min_core=min_core)
    assert set(got) == set(want)
    for key in ("rooms", "steps", "cores"):
        same_field(got[key], want[key])
    for key in ("labels", "core_sizes", "room_sizes", "doors"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (key, got[key].tolist())
    if (door, min_core) == (1, 1):
        a, b, rooms = rooms_scene_expected()
        same_field(got["rooms"], rooms)
        assert got["doors"].tolist() == [[a, b, 1]]
    with pytest.raises(ValueError):
        pkg.segment_rooms(ws, pool, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 1, 0)


def test_segment_rooms_on_the_fused_pool(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = (0, 0, 4), (48, 40, 14)
    want = segment_rooms_words(words, 6, origin, dims, 0, 2, 3)
    assert want["labels"].shape[0] >= 2 and want["doors"].shape[0] >= 1 and (want["rooms"] == -2).sum() > 100
    got = pkg.segment_rooms(ws, pool, 6, origin, dims, 0, 2, min_core=3)
    for key in ("rooms", "steps", "cores"):
        same_field(got[key], want[key])
    for key in ("labels", "core_sizes", "room_sizes", "doors"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (key, got[key].tolist(), want[key].tolist())


# ---- the rest ----------------------------------------------------------------------------------------------------------------------
def test_depth_16_cells_beyond_15_bits(env):
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 16, 2000, 43)
    words = pool.words()
    xyz = occupied_cells(words, 16)[0]
    anchor = xyz[np.argmax(xyz.max(1))]
    dims = [65, 9, 3]
    origin = [int(np.clip(anchor[a] - dims[a] // 2, 0, (1 << 16) - dims[a])) for a in range(3)]
    field = distance_field_separable(words, 16, origin, dims, 2)
    seeds = seeds_for(field == -1, origin, dims, 16, 3, np.random.default_rng(3))
    want = owner_field_words(words, 16, origin, dims, 2, seeds, field=field)
    assert max(origin) >= 1 << 15 and want[2] == 3 and (want[0] > 0).sum() > 100 and (want[0] == -2).sum() > 5
    expect(pkg, ws, pool, words, 16, origin, dims, 2, seeds, want=want)


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(hp.words())
    # (1,1,0) and (0,0,1) are occupied; with clearance 1 every cell has one of them as a face neighbour
    seeds = [(1, 1, 1), (0, 0, 0), (1, 1, 0)]
    steps, owner, stats = expect(pkg, ws, pool, hp.words(), 1, (0, 0, 0), (2, 2, 2), 0, seeds)
    same_field(steps, np.array([[[0, 1], [1, -2]], [[-2, 1], [1, 0]]], np.int32))
    same_field(owner, np.array([[[1, 1], [1, -2]], [[-2, 0], [0, 0]]], np.int32))
    steps, owner, stats = expect(pkg, ws, pool, hp.words(), 1, (0, 0, 0), (2, 2, 2), 1, seeds)
    assert (steps == -2).all() and (owner == -2).all() and stats["seeds_used"] == 0


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 17, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    seeds = [origin, [origin[a] + dims[a] - 1 for a in range(3)], [origin[0] + 64, origin[1] + 8, origin[2]]]
    unsynced = own(pkg, ws, pool, depth, origin, dims, 1, seeds)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want = owner_field_words(words, depth, origin, dims, 1, seeds, field=distance_field_separable(words, depth, origin, dims, 1))
    assert want[2] >= 1 and (want[0] > 0).sum() > 100 and (want[0] == -2).sum() > 100
    same_field(unsynced[0], want[0])
    same_field(unsynced[1], want[1])


def test_a_deferred_commit_is_read_in_its_old_state(env):
    """between svoslam_svo_fuse_commit_deferred and svoslam_svo_fuse_apply the fields are those of the words the pool held before
    the commit, and after the apply those of the new words; on the workspace that holds the deferred commit"""
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
    origin, dims = (0, 0, 8), (64, 40, 12)
    seeds = [(1, 1, 9), (60, 38, 18), (30, 20, 12), (5, 30, 16)]
    before = owner_field_words(old, depth, origin, dims, 1, seeds, field=distance_field_separable(old, depth, origin, dims, 1))
    expect(pkg, ws, pool, old, depth, origin, dims, 1, seeds, want=before)
    pkg.svo_fuse_apply(ws, pool)
    new = pool.words()
    want = owner_field_words(new, depth, origin, dims, 1, seeds, field=distance_field_separable(new, depth, origin, dims, 1))
    assert (want[1] != before[1]).sum() > 200                      # the commit changed the field in this region
    expect(pkg, ws, pool, new, depth, origin, dims, 1, seeds, want=want)


def test_workspace_slots_are_reused_and_two_calls_agree(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused
    ws = pkg.Workspace()
    assert ws.reach_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    seeds = [(6, 4, 8), (30, 20, 12), (63, 63, 39), (0, 0, 0)]
    want = owner_field_words(words, 6, *large, 1, seeds, field=distance_field_separable(words, 6, *large, 1))
    assert (want[0] > 0).sum() > 1000 and (want[0] == -2).sum() > 1000 and len(set(want[1][want[1] >= 0].tolist())) >= 2
    first = expect(pkg, ws, pool, words, 6, *large, 1, seeds, want=want)
    slots, field_slots = ws.reach_buffers(), ws.field_buffers()
    assert all(p != 0 and b > 0 for p, b in slots + field_slots)
    again = expect(pkg, ws, pool, words, 6, *large, 1, seeds, want=want)
    assert ws.reach_buffers() == slots and ws.field_buffers() == field_slots     # a second call of the same size allocates nothing
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert len(set(seeds)) == len(seeds)                                                       # no duplicates: as many seed cells as entries
    expect(pkg, ws, pool, words, 6, *large, 1, seed_field=field_of_list(*large, seeds), want=want)   # the field form, in the same slots
    expect(pkg, ws, pool, words, 6, *small, 1, seeds)                                          # a smaller call
    assert ws.reach_buffers() == slots and ws.field_buffers() == field_slots and ws.component_buffers() == [(0, 0)] * 2
    same_field(pkg.reach_field(ws, pool, 6, *large, 1, seeds), want[0])                        # the reach field, in the owner field's slots
    assert ws.reach_buffers() == slots
    ws.close()


def test_the_other_fields_are_unchanged_by_owner_calls_on_their_workspace(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    for case in [c for c in FIELD_FUSED_CASES if c[0] == 6][:3]:
        depth, d, shape, ox, radius = case
        origin, dims = case_region(words, d, shape, ox, radius)
        seeds = [origin, [origin[a] + dims[a] // 2 for a in range(3)]]
        dist2 = pkg.distance_field(ws, pool, d, origin, dims, radius)
        reach = pkg.reach_field(ws, pool, d, origin, dims, 1, seeds)
        labels = pkg.label_components(ws, pool, d, origin, dims, 1)
        own(pkg, ws, pool, d, origin, dims, 1, seeds)
        own(pkg, ws, pool, d, [0, 0, 0], [min(1 << d, 70), 9, 9], 3, seed_field=np.arange(min(1 << d, 70) * 81, dtype=np.int32).reshape(9, 9, -1))
        same_field(pkg.distance_field(ws, pool, d, origin, dims, radius), dist2)
        same_field(dist2, distance_field_separable(words, d, origin, dims, radius))
        same_field(pkg.reach_field(ws, pool, d, origin, dims, 1, seeds), reach)
        same_field(reach, reach_field_words(words, d, origin, dims, 1, seeds, field=distance_field_separable(words, d, origin, dims, 1)))
        same_field(pkg.label_components(ws, pool, d, origin, dims, 1), labels)


def test_as_tensor_and_seeds_as_a_tensor(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = (3, 0, 9), (61, 30, 5)
    field = distance_field_separable(words, 6, origin, dims, 1)
    seeds = seeds_for(field == -1, origin, dims, 6, 3, np.random.default_rng(5))
    want = owner_field_words(words, 6, origin, dims, 1, seeds, field=field)
    stats = {}
    steps, owner = pkg.owner_field(ws, pool, 6, origin, dims, 1, seeds=torch.from_numpy(seeds.astype(np.int32)).cuda(), as_tensor=True, stats=stats)
    for t in (steps, owner):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (5, 30, 61)
    same_field(steps.cpu().numpy(), want[0])
    same_field(owner.cpu().numpy(), want[1])
    assert stats["seeds_used"] == 3 and set(stats) == STATS
    steps, owner = pkg.owner_field(ws, pool, 6, origin, dims, 1, seeds)                    # an array, no stats
    same_field(owner, want[1])
    with pytest.raises(ValueError):
        pkg.owner_field(ws, pool, 6, origin, dims, 1, torch.zeros((1, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        pkg.owner_field(ws, pool, 6, origin, dims, 1)                                      # neither form
    with pytest.raises(ValueError):
        pkg.owner_field(ws, pool, 6, origin, dims, 1, seeds, seed_field=want[1])           # both
    with pytest.raises(ValueError):
        pkg.owner_field(ws, pool, 6, origin, dims, 1, seed_field=np.zeros((5, 30, 60), np.int32))


def test_box_to_cells_then_the_map_rooms_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    want = segment_rooms_words(words, 6, lo.tolist(), dims.tolist(), 0, 1, 2)
    assert want["labels"].shape[0] >= 1 and (want["rooms"] == -2).sum() > 20
    ckpt, out = tmp_path / "map.svopool", tmp_path / "rooms.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_rooms.py"), str(ckpt), str(out), "--clearance", "0", "--door", "1", "--min-core", "2",
           "--box"] + [repr(float(v)) for v in box]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    for key in ("rooms", "steps", "cores"):
        same_field(z[key], want[key])
    for key in ("labels", "core_sizes", "room_sizes", "doors"):
        assert np.array_equal(z[key], want[key]), key
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    assert int(z["clearance_cells"]) == 0 and int(z["door_cells"]) == 1 and int(z["min_core"]) == 2 and float(z["cell_size"]) == 2.0 * EDGE / 64
    assert "%d rooms, %d doors, %d free cells in no room" % (want["labels"].shape[0], want["doors"].shape[0], int((want["rooms"] == -1).sum())) in r.stdout


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        steps, owner, stats = own(pkg, ws, pool, 5, (1, 2, 3), dims, 4, [(1, 2, 3)])
        assert steps.shape == owner.shape == (dims[2], dims[1], dims[0]) and steps.dtype == owner.dtype == np.int32
        assert stats == dict.fromkeys(STATS, 0)
        steps, owner, stats = own(pkg, ws, pool, 5, (1, 2, 3), dims, 4, seed_field=np.zeros((dims[2], dims[1], dims[0]), np.int32))
        assert owner.shape == (dims[2], dims[1], dims[0]) and stats == dict.fromkeys(STATS, 0)
    assert ws.reach_buffers() == [(0, 0)] * 2 and ws.field_buffers() == [(0, 0)] * 3   # nothing was launched, nothing allocated
    buf, buf2 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    labels = torch.arange(64, dtype=torch.int32, device="cuda")
    seed_buf = torch.tensor([[1, 2, 3], [2, 2, 3]], dtype=torch.int32, device="cuda")
    null, ptr, ptr2, sp, fp = C.c_void_p(0), pkg._ptr(buf), pkg._ptr(buf2), pkg._ptr(seed_buf), pkg._ptr(labels)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, seeds=sp, n=2, seed_field=null,
              steps=ptr, owner=ptr2, stats=None):
        return L.svoslam_pool_owner_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, seeds, n, seed_field, steps, owner, stats,
                                          pkg._stream())
    st = pkg._OwnerStats()
    assert field() == 0 and field(stats=C.byref(st)) == 0 and st.seeds_used == 2 and st.rounds >= 1 and st.owner_rounds >= 1
    assert field(seeds=null, n=0, seed_field=fp, stats=C.byref(st)) == 0 and st.seeds_used == 16
    assert field(seeds=null, n=0, seed_field=fp, owner=fp) == 0                       # in place
    assert field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), steps=null, owner=null) == 0 and field(pool_ref=None, dims=(0, 0, 0), steps=null) == 0
    assert field(seeds=null, n=0) == 0 and field(n=0) == 0          # no seeds: allowed, with or without a pointer
    assert field(n=-1) == -1 and field(seeds=null, n=1) == -1 and field(n=-1, dims=(0, 2, 2)) == -1
    # one seed form: a field with a list, or with a count
    assert field(seed_field=fp) == -1 and field(seed_field=fp, seeds=null, n=2) == -1 and field(seed_field=fp, n=0) == -1
    assert field(seed_field=fp, dims=(0, 2, 2)) == -1
    # the outputs
    assert field(steps=null) == -1 and field(owner=null) == -1 and field(owner=ptr) == -1 and field(steps=null, owner=null) == -1
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
        origin[a] = 32 - dims[a]
        assert field(origin=origin) == 0
    assert field(radius=0) == 0 and field(radius=64) == 0
    assert field(radius=-1) == -1 and field(radius=4097) == -1 and field(radius=4097, dims=(0, 2, 2)) == -1
    assert field(pool_ref=None) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # the limits: refused before anything is allocated, the tile limit by dims alone on a fresh workspace
    fresh = pkg.Workspace()
    assert field(ws_ref=fresh._h, depth=16, origin=(0, 0, 0), dims=(1, 65536, 32767), radius=0) == -6    # 2^25 tiles
    assert field(ws_ref=fresh._h, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(ws_ref=fresh._h, depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), radius=4096) == -6
    assert fresh.reach_buffers() == [(0, 0)] * 2 and fresh.field_buffers() == [(0, 0)] * 3
    with pytest.raises(Exception):
        pkg.owner_field(ws, pool, 5, (30, 0, 0), (4, 4, 4), 3, [(0, 0, 0)])
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        _, _, stats = own(pkg, ws, pool, 6, (0, 0, 0), (64, 20, 3), 1, [(63, 19, 2), (0, 0, 0)])
        own(pkg, ws, pool, 4, (1, 2, 3), (9, 3, 3), 0, [])
        own(pkg, ws, pool, 6, (0, 0, 0), (64, 20, 3), 1, seed_field=np.arange(64 * 20 * 3, dtype=np.int32).reshape(3, 20, 64))
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 3 and ms > 0.0 and stats["rounds"] >= 1 and stats["owner_rounds"] >= 1
        own(pkg, ws, pool, 6, (0, 0, 0), (64, 0, 3), 1, [(0, 0, 0)])     # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            own(pkg, ws, pool, 6, (0, 0, 0), (65, 2, 3), 1, [(0, 0, 0)])   # refused: not bracketed either
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])
