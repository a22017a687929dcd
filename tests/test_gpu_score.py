"""svoslam_score_poses on the device: cost, near, far, outside and best equal the host restatement of the specification
(tests/test_score_cpu.py: score_poses_ref, binary32 operation by operation) bit for bit, on the pool's own words and the device's
own field, which is itself first compared with distance_field_separable -- never a second device result alone.

The host chooses between two forms of the kernel: one workgroup per pose, or the points of a pose split over workgroups that add
into a record per pose, iff n > SPLIT_ABOVE points and fewer than SPLIT_BELOW poses.  SIZES covers each n with at least two P and
each P with at least two n, and both sides of both edges of that switch; every (region, radius) case of the fused pool runs one of
the five SIZE_GROUPS, a different one at every radius, so every size runs at every radius and in three regions.  Where the region's
field holds a distance at all (in this root the cloud stays more than 3 cells from low_corner and offset_37 and more than 8 from
one_cell: there every in-region pair is FAR, whatever the pose), the cases with at least 63 points and 63 poses must pass
check_case on the reference's results before the device is asked: every class of pair the case can have, a pose that would win
were its near not below min_near, and a tie at the best cost."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, fused_regions, midpoints, region_cells
from test_gpu_query import fused_pool
from test_reach_cpu import cells_pool
from test_score_cpu import (FAR, IDENTITY, MAX_MISS, NEAR, OUT_REGION, OUT_ROOT, OUTPUTS, SIGNED_PERMUTATIONS, VOID, check_case, choose_rules,
                            classify, edge_case_poses, lattice_inputs, plane_edge_points, reduce_pairs, same_scores, score_poses_ref)
from test_surface_cpu import CENTER, EDGE, occupied_cells

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_ABOVE, SPLIT_BELOW = 1024, 512                                    # map_score.hip: kChunk, kSplitBelow
SIZE_GROUPS = [[(0, 1), (63, 63), (256, 300), (4099, 1), (SPLIT_ABOVE + 1, SPLIT_BELOW - 1)],
               [(0, 64), (64, 65), (257, 64), (1000, 300), (4099, 63)],
               [(1, 0), (65, 64), (255, 63), (64, 1), (4099, 300)],
               [(1, 2), (63, 300), (256, 65), (257, 1), (SPLIT_ABOVE, 64), (SPLIT_ABOVE + 1, 64)],
               [(65, 2), (255, 0), (1000, 2), (4099, 2), (300, 70), (SPLIT_ABOVE + 1, SPLIT_BELOW)]]
SIZES = [s for group in SIZE_GROUPS for s in group]
RADII = (0, 3, 8)
LAT_CENTER, LAT_EDGE = (0.5, -0.25, 1.0), 2.0                           # a dyadic centre and a power-of-two edge: the exact lattice


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


@pytest.fixture(scope="module")
def device_fields(env, fused):
    """(region, radius) -> the device's own field of the fused pool as an array, after it has been compared with the restatement"""
    pkg, torch = env
    pool, words, pts, ws = fused
    cache = {}

    def get(region, radius):
        if (region, radius) not in cache:
            origin, dims = fused_regions(6)[region]
            field = pkg.distance_field(ws, pool, 6, origin, dims, radius)
            assert np.array_equal(field, distance_field_separable(words, 6, origin, dims, radius))
            cache[(region, radius)] = field
        return cache[(region, radius)]
    return get


def small_motion(rng, cell, turn_deg, shift_cells):
    """a rotation by up to turn_deg about a seeded axis and a shift by up to shift_cells per axis: float64 [4, 4]"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = np.deg2rad(turn_deg) * (rng.random() * 2 - 1)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    M[:3, 3] = (rng.random(3) * 2 - 1) * shift_cells * cell
    return M


def flat(M):
    return np.asarray(M, np.float64).T.reshape(16).astype(F)           # column-major


def seeded_case(field, depth, center, edge, origin, dims, n, n_poses, seed, cloud):
    """-> (points float32 [n, 3], poses float32 [n_poses, 16]).  Points: world targets pulled back through the pose A (small, about
    the identity) -- fused points, points beside the cloud, the middles of region cells with and without a distance, points
    anywhere in the root, points outside the root -- and void points.  Poses: one that throws everything out of the root first,
    then A, small motions of A, and the exact-lattice kind (a signed permutation about the root's centre and a whole-cell shift);
    the list is followed by its own reverse, so from 2 poses on costs are tied."""
    rng = np.random.default_rng(seed)
    n_side = 1 << depth
    cell, c = 2.0 * edge / n_side, np.asarray(center, np.float64)
    A = small_motion(rng, cell, 4.0, 3.0)
    groups = [cloud[rng.integers(0, cloud.shape[0], n)], cloud[rng.integers(0, cloud.shape[0], n)] + rng.normal(scale=2 * cell, size=(n, 3))]
    mids, values = midpoints(depth, center, edge, origin, dims), np.asarray(field).reshape(-1)
    for pick in (mids[values >= 0], mids[values < 0]):
        if pick.shape[0]:
            groups.append(pick[rng.integers(0, pick.shape[0], n)])
    groups.append(c + (rng.random((n, 3)) * 2 - 1) * edge)
    beyond = c + (rng.random((n, 3)) * 2 - 1) * edge
    beyond[np.arange(n), rng.integers(0, 3, n)] = c[0] + edge * rng.choice([-1.3, 1.1, 2.0], n)
    groups.append(beyond)
    world = np.stack([groups[(i + seed) % len(groups)][i] for i in range(n)]) if n else np.zeros((0, 3))
    points = ((world - A[:3, 3]) @ A[:3, :3]).astype(F)                 # A^-1 in float64, rounded once
    if n >= 8:
        void = rng.choice(n, max(1, n // 9), replace=False)
        points[void] = np.inf
        points[void[::2], rng.integers(0, 3)] = np.nan
        points[void[1::3], 0] = F(0.25)                                 # void in two components only
    base = [np.eye(4)]
    base[0][:3, 3] = c + 5.0 * edge                                     # everything outside the root
    base.append(A)
    while len(base) < (n_poses + 1) // 2:
        if len(base) % 4 == 3:
            S = np.eye(4)
            S[:3, :3] = SIGNED_PERMUTATIONS[int(rng.integers(48))]
            S[:3, 3] = c - S[:3, :3] @ c + rng.integers(-3, 4, 3) * cell
            base.append(S @ A if len(base) % 8 == 3 else S)
        else:
            base.append(small_motion(rng, cell, 3.0, 3.0) @ A)
    poses = np.stack([flat(M) for M in (base + base[::-1])[:n_poses]]) if n_poses else np.zeros((0, 16), F)
    return points, poses


def run_on_device(pkg, ws, field, depth, center, edge, origin, dims, points, poses, radius, full_check):
    """the reference once, the device under the rules chosen for the case and under the natural ones.  -> the classes"""
    cls, v, _ = classify(field, depth, center, edge, origin, dims, points, poses)
    rules = [(radius * radius + 1, 0)]
    if full_check:
        chosen = choose_rules(cls, v, radius)
        assert chosen is not None
        check_case(cls, v, field, depth, origin, dims, *chosen)
        rules.insert(0, chosen)
    for miss, min_near in rules:
        got = pkg.score_poses(ws, field, depth, center, edge, origin, dims, points, poses, miss, min_near, want=OUTPUTS)
        same_scores(got, reduce_pairs(cls, v, miss, min_near))
    return cls


# ---- 1. the fused pool ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("region", sorted(fused_regions(6)))
def test_fused_cloud(env, fused, device_fields, region, radius):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)[region]
    field = device_fields(region, radius)
    case = 3 * sorted(fused_regions(6)).index(region) + RADII.index(radius)
    seen = set()
    for j, (n, n_poses) in enumerate(SIZE_GROUPS[(sorted(fused_regions(6)).index(region) + RADII.index(radius)) % 5]):
        points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, n, n_poses, 100 * case + j, pts)
        cls = run_on_device(pkg, ws, field, 6, CENTER, EDGE, origin, dims, points, poses, radius, n >= 63 and n_poses >= 63 and (field >= 0).any())
        seen |= set(np.unique(cls).tolist())
    assert {VOID, OUT_ROOT} <= seen and (region == "whole_root" or OUT_REGION in seen)


def test_every_size_runs_and_both_forms_of_the_kernel():
    """SIZES against the issue's lists and the host's switch (on the list alone)"""
    ns, ps = {n for n, _ in SIZES}, {p for _, p in SIZES}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099} <= ns and {0, 1, 2, 63, 64, 65, 300} <= ps
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099):
        assert len({p for m, p in SIZES if m == n}) >= 2
    for p in (0, 1, 2, 63, 64, 65, 300):
        assert len({n for n, q in SIZES if q == p}) >= 2
    split = [(n, p) for n, p in SIZES if n > SPLIT_ABOVE and 0 < p < SPLIT_BELOW]
    assert (SPLIT_ABOVE + 1, 64) in split and (SPLIT_ABOVE + 1, SPLIT_BELOW - 1) in split
    assert (SPLIT_ABOVE, 64) not in split and (SPLIT_ABOVE + 1, SPLIT_BELOW) not in split
    for group in SIZE_GROUPS:                                           # every group has both forms, and a case large enough for check_case
        assert any(s in split for s in group) and any(s not in split and s[0] >= 63 and s[1] >= 63 for s in group)


def test_the_fused_cases_are_not_empty(fused, device_fields):
    """on the reference alone: across the regions every class of pair occurs at every radius, near and far pairs included"""
    pool, words, pts, ws = fused
    for radius in RADII:
        counts = np.zeros(5, np.int64)
        for k, (region, (origin, dims)) in enumerate(sorted(fused_regions(6).items())):
            field = device_fields(region, radius)
            points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, 257, 64, 100 * (3 * k + RADII.index(radius)) + 15, pts)
            counts += np.bincount(classify(field, 6, CENTER, EDGE, origin, dims, points, poses)[0].reshape(-1), minlength=5)
        assert (counts > 50).all(), (radius, counts.tolist())
    both = [(region, radius) for region in fused_regions(6) for radius in RADII
            if (device_fields(region, radius) >= 0).any() and (device_fields(region, radius) < 0).any()]
    assert len(both) >= 6 and {"whole_root", "high_corner"} <= {region for region, _ in both}   # where check_case applies in full


# ---- 2. a root of 256 cells a side, the lattice's edges ------------------------------------------------------------------------------
def test_depth_8_region_off_the_origin_with_the_plane_edge_points(env):
    pkg, torch = env
    depth, origin, dims, radius = 8, (1, 1, 1), (200, 3, 255), 5         # 200 cells a row: not a multiple of 64; the first cell is not 0
    occupied = [(3, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 248), (199, 2, 2), (200, 3, 255), (2, 2, 0), (150, 2, 100)]
    words = cells_pool(occupied, depth)
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    field = pkg.distance_field(ws, pool, depth, origin, dims, radius)
    assert np.array_equal(field, distance_field_separable(words, depth, origin, dims, radius))
    edge_points, axes, cells = plane_edge_points(depth, CENTER, EDGE)
    rng = np.random.default_rng(8)
    mids = midpoints(depth, CENTER, EDGE, origin, dims)
    close = np.flatnonzero(field.reshape(-1) >= 0)
    more = np.concatenate([mids[rng.integers(0, mids.shape[0], 150)], mids[close[rng.integers(0, close.size, 150)]]])
    points = np.concatenate([edge_points, more, [[np.inf, 0, 0], [0, 0, np.nan], [3e38, 0.5, 0.5]]]).astype(F)
    cell = 2.0 * EDGE / 256
    poses = np.concatenate([edge_case_poses(), [flat(small_motion(rng, cell, 2.0, 2.0)) for _ in range(5)], IDENTITY[None, :]])
    cls, v, q = classify(field, depth, CENTER, EDGE, origin, dims, points, poses)
    on_edges = cls[0, :36]                                              # under the identity: the expected cells, in the root or not
    assert np.array_equal(on_edges == OUT_ROOT, cells < 0)
    assert np.array_equal(q[0, :36][cells >= 0, axes[cells >= 0]], cells[cells >= 0])
    assert {NEAR, FAR, OUT_REGION} <= set(on_edges.tolist()) and {VOID, NEAR, FAR, OUT_REGION, OUT_ROOT} == set(np.unique(cls).tolist())
    for miss, min_near in ((radius * radius + 1, 0), (0, 0), (MAX_MISS, 100), (7, 340)):
        want = reduce_pairs(cls, v, miss, min_near)
        same_scores(pkg.score_poses(ws, field, depth, CENTER, EDGE, origin, dims, points, poses, miss, min_near, want=OUTPUTS), want)
    huge = reduce_pairs(cls, v, MAX_MISS, 100)
    assert huge["cost"].max() > 1 << 32 and huge["best"][1] == 0 and (huge["cost"] == huge["best"][0]).sum() == 3   # the three identities tie
    assert want["best"].tolist() == [-1, -1]
    big_n = np.tile(points, (13, 1))                                    # the same pairs 13 times over in the split form: 4407 points
    got = pkg.score_poses(ws, field, depth, CENTER, EDGE, origin, dims, big_n, poses, MAX_MISS, 100, want=OUTPUTS)
    assert np.array_equal(got["cost"], 13 * huge["cost"]) and np.array_equal(got["near"], 13 * huge["near"]) and got["best"][1] == huge["best"][1]
    same_scores(got, score_poses_ref(field, depth, CENTER, EDGE, origin, dims, big_n, poses, MAX_MISS, 100))


# ---- 3. the outputs ------------------------------------------------------------------------------------------------------------------
def test_each_output_alone_best_alone_and_all_together(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, _ = fused
    origin, dims = fused_regions(6)["whole_root"]
    field = device_fields("whole_root", 3)
    for n, n_poses in ((300, 70), (2000, 70)):                          # one workgroup per pose, and the split form
        ws = pkg.Workspace()
        points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, n, n_poses, 77, pts)
        cls, v, _ = classify(field, 6, CENTER, EDGE, origin, dims, points, poses)
        miss, min_near = choose_rules(cls, v, 3)
        want = reduce_pairs(cls, v, miss, min_near)
        assert len(set(want["cost"].tolist())) > 5 and want["best"][1] > 0
        for names in [(name,) for name in OUTPUTS if name != "best"]:
            got = pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, miss, min_near, want=names)
            assert set(got) == set(names)
            same_scores(got, want, names)
            assert (ws.score_buffers()[0][1] > 0) == (n > SPLIT_ABOVE)  # no record is kept unless the form or `best` needs one
        got = pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, miss, min_near, want=("best",))
        assert set(got) == {"best"} and ws.score_buffers()[0][1] >= 24 * n_poses
        same_scores(got, want, ("best",))
        for names in (OUTPUTS, ("best", "near"), ("outside", "cost")):
            got = pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, miss, min_near, want=names)
            same_scores(got, want, names)
        assert set(pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, miss)) == {"cost", "near"}   # the default
        ws.close()


def test_tensors_in_tensors_out_and_nearest_fields_dist2(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)["low_corner"]
    field = device_fields("low_corner", 8)
    near = pkg.nearest_field(ws, pool, 6, origin, dims, 8, want=("dist2",), as_tensor=True)["dist2"]
    points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, 500, 20, 5, pts)
    got = pkg.score_poses(ws, near, 6, CENTER, EDGE, origin, dims, torch.from_numpy(points).cuda(), torch.from_numpy(poses).cuda(), 65, 10,
                          want=OUTPUTS, as_tensor=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got.values())
    assert got["cost"].dtype == torch.int64 and got["near"].dtype == torch.int32 and tuple(got["best"].shape) == (2,)
    same_scores({k: t.cpu().numpy() for k, t in got.items()}, score_poses_ref(field, 6, CENTER, EDGE, origin, dims, points, poses, 65, 10))
    with pytest.raises(KeyError):
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, 65, want=("steps",))
    with pytest.raises(ValueError):
        pkg.score_poses(ws, field[:-1], 6, CENTER, EDGE, origin, dims, points, poses, 65)
    with pytest.raises(ValueError):
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, torch.from_numpy(points.astype(np.float64)).cuda(), poses, 65)


# ---- 4. a second opinion on the device ---------------------------------------------------------------------------------------------------
def test_the_sums_are_transform_vertex_map_then_nearest_occupied(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)["whole_root"]
    for radius in (3, 8):
        field = device_fields("whole_root", radius)
        points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, 1500, 10, 21 + radius, pts)
        poses = poses[:5]
        miss = radius * radius + 1
        got = pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, miss, want=("cost", "near", "far", "outside"))
        same_scores(got, score_poses_ref(field, 6, CENTER, EDGE, origin, dims, points, poses, miss), ("cost", "near", "far", "outside"))
        live = np.isfinite(points).all(1)
        for k in range(5):
            moved = torch.from_numpy(points[live]).cuda()
            pkg.transform_vertex_map(moved, poses[k])
            d = pkg.nearest_occupied(pool, 6, CENTER, EDGE, moved, radius, outputs=("dist2",))["dist2"].cpu().numpy().astype(np.int64)
            assert (got["near"][k], got["far"][k], got["outside"][k]) == ((d >= 0).sum(), (d == -1).sum(), (d == -2).sum())
            assert got["cost"][k] == d[d >= 0].sum() + miss * (d < 0).sum()
        assert got["near"][1] > 100 and got["far"].max() > 100 and got["outside"][1:].max() > 50 and got["outside"][0] == live.sum()


# ---- 5. recovery -------------------------------------------------------------------------------------------------------------------------
def test_relocalize_recovers_an_exact_lattice_pose(env, fused):
    """the observation: the centres of all occupied cells, seen from a sensor that is turned by 90 degrees and shifted by whole
    cells; the prior is off by (2, -3, 1) cells.  The search steps over whole cells, then halves: the true pose, cost 0, all near."""
    pkg, torch = env
    pool, words, pts, ws = fused
    n_side, h = 64, LAT_EDGE / 64
    k = occupied_cells(words, 6)[0]
    S0 = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.int64)         # a quarter turn about y
    T0 = np.array([30, 33, 35])
    u = (2 * (k - T0) + 1) @ S0
    void = np.zeros(u.shape[0], bool)
    points, true_pose = lattice_inputs(6, LAT_CENTER, LAT_EDGE, u, void, [S0], [T0])
    cls, v, _ = classify(pkg.distance_field(ws, pool, 6, (0, 0, 0), (64, 64, 64), 3), 6, LAT_CENTER, LAT_EDGE, (0, 0, 0), (64, 64, 64), points, true_pose)
    assert (cls == NEAR).all() and not v.any() and points.shape[0] > 500           # on the reference: the true pose costs nothing
    prior = true_pose[0].copy()
    prior[12:15] += np.array([2, -3, 1], F) * F(2 * h)
    found = pkg.relocalize(ws, pool, 6, LAT_CENTER, LAT_EDGE, points, prior, (8 * h, 8 * h, 8 * h), 0.0, 3, steps=(9, 9, 9), yaw_steps=1, rounds=3)
    assert found is not None and found["cost"] == 0 and found["near"] == points.shape[0]
    assert np.array_equal(found["pose"].view(np.uint32), true_pose[0].view(np.uint32))
    assert len(found["rounds"]) == 3 and [r[0] for r in found["rounds"]] == [0, 0, 0]
    want_index = ((4 - 1) * 9 + (4 + 3)) * 9 + (4 - 2)                  # z slowest: the offsets (-2, +3, -1) cells in a grid of whole cells
    assert found["rounds"][0][1] == want_index
    with_yaw = pkg.relocalize(ws, pool, 6, LAT_CENTER, LAT_EDGE, torch.from_numpy(points).cuda(), prior, (8 * h, 8 * h, 8 * h), 0.2, 3,
                              steps=(9, 9, 9), yaw_steps=3, rounds=2)   # the unturned candidates are the same poses: found again
    assert with_yaw["cost"] == 0 and np.array_equal(with_yaw["pose"].view(np.uint32), true_pose[0].view(np.uint32))
    assert pkg.relocalize(ws, pool, 6, LAT_CENTER, LAT_EDGE, points, prior, (8 * h, 8 * h, 8 * h), 0.0, 3, yaw_steps=1, min_near_fraction=1.01) is None
    far_prior = prior.copy()
    far_prior[12] += F(40 * 2 * h)                                      # 40 cells off: nothing within 4 cells of it has half the points near
    assert pkg.relocalize(ws, pool, 6, LAT_CENTER, LAT_EDGE, points, far_prior, (8 * h, 8 * h, 8 * h), 0.0, 0, yaw_steps=1, min_near_fraction=0.9) is None


def test_the_map_relocalize_tool(env, fused, tmp_path):
    """tools/map_relocalize.py on a saved map and a file of points: the pose, its cost and the rounds of relocalize()"""
    pkg, torch = env
    pool, words, pts, ws = fused
    h = LAT_EDGE / 64
    k = occupied_cells(words, 6)[0][::3]
    S0, T0 = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.int64), np.array([31, 30, 34])
    u = (2 * (k - T0) + 1) @ S0
    points, true_pose = lattice_inputs(6, LAT_CENTER, LAT_EDGE, u, np.zeros(u.shape[0], bool), [S0], [T0])
    points = np.concatenate([points, np.full((7, 3), np.inf, F)])       # pixels without depth
    prior = true_pose[0].copy()
    prior[12:15] += np.array([-1, 0, 3], F) * F(2 * h)
    ckpt, cloud, out = tmp_path / "map.svopool", tmp_path / "points.npy", tmp_path / "found.npz"
    pool.save(ckpt, LAT_CENTER, LAT_EDGE, 6)
    np.save(cloud, points)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_relocalize.py"), str(ckpt), str(out), "--points", str(cloud), "--extent"] + [repr(8 * h)] * 3
    cmd += ["--yaw", "0", "--yaw-steps", "1", "--radius", "3", "--rounds", "2", "--prior"] + [repr(float(x)) for x in prior]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["found"]) == 1 and int(z["cost"]) == 0 and int(z["near"]) == int(z["points"]) == u.shape[0]
    assert np.array_equal(z["pose"].view(np.uint32), true_pose[0].view(np.uint32)) and z["rounds"].shape == (2, 2) and not z["rounds"][:, 0].any()
    assert int(z["depth"]) == 6 and float(z["cell_size"]) == 2 * h and int(z["radius_cells"]) == 3
    r = subprocess.run(cmd + ["--min-near", "1.01"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nothing qualified" in r.stdout and int(np.load(out)["found"]) == 0


# ---- 6. conventions ---------------------------------------------------------------------------------------------------------------------
def test_the_slot_is_reused_and_the_other_slots_are_left_alone(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, _ = fused
    ws = pkg.Workspace()
    assert ws.score_buffers() == [(0, 0)]
    small = ((5, 3, 7), (33, 20, 9))
    views = np.array([[6, 4, 8], [20, 10, 10]], np.int32)
    pkg.distance_field(ws, pool, 6, *small, 3)
    pkg.nearest_field(ws, pool, 6, *small, 3)
    pkg.visibility_field(ws, pool, 6, *small, 3, views)
    pkg.reach_field(ws, pool, 6, *small, 0, views)
    pkg.label_components(ws, pool, 6, *small, 0)
    others = lambda: (ws.field_buffers(), ws.nearest_buffers(), ws.visibility_buffers(), ws.reach_buffers(), ws.component_buffers())
    before = others()
    origin, dims = fused_regions(6)["low_corner"]
    field = device_fields("low_corner", 3)
    points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, 2000, 100, 3, pts)
    want = score_poses_ref(field, 6, CENTER, EDGE, origin, dims, points, poses, 10, 5)
    t_field, t_points, t_poses = torch.from_numpy(field).cuda(), torch.from_numpy(points).cuda(), torch.from_numpy(poses).cuda()
    first = pkg.score_poses(ws, t_field, 6, CENTER, EDGE, origin, dims, t_points, t_poses, 10, 5, want=OUTPUTS)
    slots = ws.score_buffers()
    assert slots[0][0] != 0 and 24 * 100 <= slots[0][1] < 2 * 24 * 100 + 512       # a record per pose, and the slot's headroom
    again = pkg.score_poses(ws, t_field, 6, CENTER, EDGE, origin, dims, t_points, t_poses, 10, 5, want=OUTPUTS)
    assert ws.score_buffers() == slots                                  # a second call of the same size allocates nothing
    same_scores(first, want)
    same_scores(again, want)
    same_scores(pkg.score_poses(ws, t_field, 6, CENTER, EDGE, origin, dims, t_points[:300], t_poses[:9], 10, 5, want=OUTPUTS),
                score_poses_ref(field, 6, CENTER, EDGE, origin, dims, points[:300], poses[:9], 10, 5))   # a smaller call in the larger one's slot
    assert ws.score_buffers() == slots and others() == before
    ws.close()


def test_another_stream_the_pool_and_the_abi(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)["whole_root"]
    field = device_fields("whole_root", 8)
    t_field = torch.from_numpy(field).cuda()
    for n, n_poses in ((700, 33), (3000, 33)):
        points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, n, n_poses, 9, pts)
        t_points, t_poses = torch.from_numpy(points).cuda(), torch.from_numpy(poses).cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got = pkg.score_poses(ws, t_field, 6, CENTER, EDGE, origin, dims, t_points, t_poses, 65, 20, want=OUTPUTS, as_tensor=True)
        stream.synchronize()
        same_scores({k: t.cpu().numpy() for k, t in got.items()}, score_poses_ref(field, 6, CENTER, EDGE, origin, dims, points, poses, 65, 20))
    assert np.array_equal(pool.words(), words) and pkg.lib().svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused, device_fields):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = fused_regions(6)["low_corner"]
    field = device_fields("low_corner", 3)
    points, poses = seeded_case(field, 6, CENTER, EDGE, origin, dims, 3000, 40, 4, pts)
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points[:500], poses, 10, want=("cost",))      # one launch
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points[:500], poses, 10, want=("best",))      # two
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses, 10, want=OUTPUTS)              # three: the split form
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 3 and ms > 0.0
        pkg.score_poses(ws, field, 6, CENTER, EDGE, origin, dims, points, poses[:0], 10, want=("cost",))        # nothing is launched
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws = pkg.Workspace()
    L = pkg.lib()
    field = torch.arange(4 * 2 * 2, dtype=torch.int32, device="cuda") - 3
    points = torch.tensor([[0.1, 0.1, 0.1], [0.3, -0.2, 0.4], [float("inf"), 0, 0]], dtype=torch.float32, device="cuda")
    poses = torch.from_numpy(np.tile(IDENTITY, (2, 1))).cuda()
    cost, best = [torch.full((4,), 0x55, dtype=torch.int64, device="cuda") for _ in range(2)]
    counts = [torch.full((4,), 0x55, dtype=torch.int32, device="cuda") for _ in range(3)]
    null = C.c_void_p(0)
    outs = [pkg._ptr(cost)] + [pkg._ptr(t) for t in counts] + [pkg._ptr(best)]

    def f3(v):
        return None if v is None else (C.c_float * 3)(*v)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def score(ws_ref=ws._h, d_field=pkg._ptr(field), depth=5, center=CENTER, edge=EDGE, origin=(1, 2, 3), dims=(4, 2, 2), d_points=pkg._ptr(points),
              n=3, d_poses=pkg._ptr(poses), n_poses=2, miss=10, min_near=0, out=outs):
        return L.svoslam_score_poses(ws_ref, d_field, depth, f3(center), edge, i3(origin), i3(dims), d_points, n, d_poses, n_poses, miss, min_near,
                                     *out, pkg._stream())
    nulls = [null] * 5
    assert score() == 0
    torch.cuda.synchronize()
    assert cost[:2].tolist() == [20, 20] and best[:2].tolist() == [20, 0] and counts[2][:2].tolist() == [2, 2]   # far from the root's low corner
    only_best = nulls[:4] + [outs[4]]
    assert score(n_poses=0, d_poses=null) == 0 and score(n_poses=0, d_poses=null, out=only_best) == 0 and score(n_poses=0, out=nulls) == 0
    torch.cuda.synchronize()
    assert best[:2].tolist() == [-1, -1]                                # no poses: no pose qualifies
    assert score(n=0, d_points=null) == 0 and score(dims=(4, 0, 2), d_field=null) == 0 and score(n=0, d_points=null, d_field=null) == 0
    torch.cuda.synchronize()
    assert cost[:2].tolist() == [0, 0] and counts[0][:2].tolist() == [0, 0] and best[:2].tolist() == [0, 0]
    assert score(min_near=1) == 0                                       # nothing is near: nobody qualifies
    torch.cuda.synchronize()
    assert best[:2].tolist() == [-1, -1]
    assert score(miss=MAX_MISS) == 0
    torch.cuda.synchronize()
    assert cost[:2].tolist() == [2 * MAX_MISS, 2 * MAX_MISS]
    for t in [cost, best] + counts:
        t.fill_(0x55)
    torch.cuda.synchronize()
    slots = ws.score_buffers()
    assert slots[0][1] > 0
    assert score(ws_ref=None) == -1 and score(center=None) == -1 and score(origin=None) == -1 and score(dims=None) == -1
    assert score(depth=0) == -1 and score(depth=17) == -1
    assert score(edge=0.0) == -1 and score(edge=-1.0) == -1 and score(edge=float("nan")) == -1
    assert score(dims=(-1, 2, 2)) == -1 and score(dims=(4, 2, -1)) == -1 and score(dims=(0, -1, 2)) == -1
    for a in range(3):                                                  # one cell outside the root on each side
        origin, dims = [1, 2, 3], [4, 2, 2]
        origin[a] = -1
        assert score(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert score(origin=origin) == -1
        origin[a], dims[a] = 0, 33
        assert score(origin=origin, dims=dims) == -1
    assert score(n=-1) == -1 and score(n_poses=-1) == -1 and score(n=-1, n_poses=0) == -1
    assert score(miss=-1) == -1 and score(miss=MAX_MISS + 1) == -1 and score(min_near=-1) == -1
    assert score(d_points=null) == -1 and score(d_poses=null) == -1 and score(d_field=null) == -1
    assert score(out=nulls) == -1 and score(out=nulls, n=0, d_points=null) == -1
    assert score(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6       # more than 2^31 - 1 cells
    fresh = pkg.Workspace()
    assert score(ws_ref=fresh._h, miss=-1) == -1 and score(ws_ref=fresh._h, out=nulls) == -1
    assert score(ws_ref=fresh._h, depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    torch.cuda.synchronize()
    assert fresh.score_buffers() == [(0, 0)] and ws.score_buffers() == slots
    assert all((t == 0x55).all().item() for t in [cost, best] + counts) # none of the refused calls wrote anything
    assert L.svoslam_abi_version() == 1
