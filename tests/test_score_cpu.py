"""Scoring candidate poses against a distance field (svoslam_score_poses, pose_grid; include/svoslam.h): the
specification restated in numpy, binary32 operation by operation (score_poses_ref); a second, independent restatement in integers
only for exact-lattice inputs (score_poses_lattice), the two proven equal on a pool fused by the CPU oracle and on hand-built
pools; the lattice's edges (points on planes and one ulp beside them, overflow, NaN, the largest miss cost); the host call
pose_grid; and the header's pins.  No GPU.

score_poses_ref below is what the device call must produce; tests/test_gpu_score.py compares against it bit for bit.

What a comparison needs in order not to pass empty is asserted on the reference alone (check_case): pairs of every class the case
can have -- NEAR and FAR where the field has values of that sign, OUTSIDE the region where the region is not the whole root,
OUTSIDE the root, VOID -- a pose that would win `best` were its near not below min_near, and a tie at the best cost that the lower
index wins.  choose_rules picks miss_cost and min_near for that from the reference's own results."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, fused_regions, midpoints, region_cells
from test_reach_cpu import cells_pool
from test_surface_cpu import CENTER, EDGE, load_pkg, occupied_cells
from test_volume_cpu import DEPTH, ROOT_CENTER, ROOT_EDGE, F, cell_in_block, fused, plane  # noqa: F401

I64 = np.int64
VOID, NEAR, FAR, OUT_REGION, OUT_ROOT = range(5)
CLASS_NAMES = ("void", "near", "far", "outside the region", "outside the root")
MAX_MISS = 1 << 30
OUTPUTS = ("cost", "near", "far", "outside", "best")


# ---- the specification, restated -------------------------------------------------------------------------------------------
def move(poses, points, dtype=F):
    """[P, n, 3]: w = (m0 * x + m1 * y) + (m2 * z + m3 * 1), m[c] = column c of the pose: one product or sum per operation, in
    `dtype` (binary32: mat4_mul_point's own order; float64 to prove a case exact)"""
    m = np.asarray(poses, F).reshape(-1, 4, 4).astype(dtype)
    p = np.asarray(points, F).reshape(-1, 3).astype(dtype)
    with np.errstate(all="ignore"):
        col = [m[:, c, None, :3] for c in range(4)]
        x, y, z = [p[None, :, a, None] for a in range(3)]
        return (col[0] * x + col[1] * y) + (col[2] * z + col[3] * dtype(1.0))


def classify(field, depth, center, edge, origin, dims, points, poses):
    """-> (class [P, n] uint8, value [P, n] int64 (0 unless NEAR), cell [P, n, 3]) of every (pose, point) pair"""
    p = np.asarray(points, F).reshape(-1, 3)
    n_side = 1 << depth
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    o, d = np.asarray(origin, I64), np.asarray(dims, I64)
    w = move(poses, p)
    assert w.dtype == F
    void = ~np.isfinite(p).all(1)
    zero, full = np.zeros(w.shape[:2], I64), np.full(w.shape[:2], n_side, I64)
    with np.errstate(all="ignore"):
        p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
        in_root = np.isfinite(w).all(2) & ((p0 <= w) & (w <= pn)).all(2)                # false for a NaN
        q = np.stack([cell_in_block(c[a], n_side, h, w[..., a], zero, full, False) for a in range(3)], 2)
    rel = q - o
    in_region = in_root & ((rel >= 0) & (rel < d)).all(2)
    flat = np.asarray(field, np.int32).reshape(-1)
    idx = np.where(in_region, (rel[..., 2] * d[1] + rel[..., 1]) * d[0] + rel[..., 0], 0)
    v = flat[idx].astype(I64) if flat.size else np.zeros(idx.shape, I64)
    cls = np.where(in_region, np.where(v >= 0, NEAR, FAR), np.where(in_root, OUT_REGION, OUT_ROOT)).astype(np.uint8)
    cls[:, void] = VOID
    return cls, np.where(cls == NEAR, v, 0), q


def reduce_pairs(cls, v, miss_cost, min_near):
    """per pose the cost and the counts, and the best: the specification's "Per pose" and "Best" """
    assert 0 <= miss_cost <= MAX_MISS and min_near >= 0
    near, far = (cls == NEAR).sum(1), (cls == FAR).sum(1)
    outside = (cls == OUT_REGION).sum(1) + (cls == OUT_ROOT).sum(1)
    cost = v.sum(1).astype(I64) + I64(miss_cost) * (far + outside).astype(I64)
    ok = np.flatnonzero(near >= min_near)
    best = np.array([-1, -1], I64)
    if ok.size:
        at = ok[np.argmin(cost[ok])]                                    # argmin: the first of equal costs, the lowest index
        best = np.array([cost[at], at], I64)
    return {"cost": cost, "near": near.astype(np.int32), "far": far.astype(np.int32), "outside": outside.astype(np.int32), "best": best}


def score_poses_ref(field, depth, center, edge, origin, dims, points, poses, miss_cost, min_near=0):
    """-> {"cost" int64 [P], "near", "far", "outside" int32 [P], "best" int64 [2]}: svoslam_score_poses in numpy"""
    cls, v, _ = classify(field, depth, center, edge, origin, dims, points, poses)
    return reduce_pairs(cls, v, miss_cost, min_near)


def same_scores(got, want, names=OUTPUTS):
    for name in names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, bad.size, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


# ---- what a case needs in order not to pass empty -----------------------------------------------------------------------------
def possible_classes(field, depth, origin, dims):
    """the classes a pair can have at all with this field and region"""
    flat = np.asarray(field).reshape(-1)
    out = {VOID, OUT_ROOT}
    if (flat >= 0).any():
        out.add(NEAR)
    if (flat < 0).any():
        out.add(FAR)
    if any(origin[a] > 0 or origin[a] + dims[a] < (1 << depth) for a in range(3)):
        out.add(OUT_REGION)
    return out


def choose_rules(cls, v, radius):
    """(miss_cost, min_near) under which the winner without a limit on near is disqualified, someone still qualifies, and the best
    cost among those is shared by two poses: the first miss cost of radius^2 + 1, 1, 0 that allows it.  None if none does."""
    for miss in (radius * radius + 1, 1, 0):
        free = reduce_pairs(cls, v, miss, 0)
        min_near = int(free["near"][free["best"][1]]) + 1
        res = reduce_pairs(cls, v, miss, min_near)
        if res["best"][1] >= 0 and ((res["cost"] == res["best"][0]) & (res["near"] >= min_near)).sum() >= 2:
            return miss, min_near
    return None


def check_case(cls, v, field, depth, origin, dims, miss, min_near):
    counts = np.bincount(cls.reshape(-1), minlength=5)
    for k in possible_classes(field, depth, origin, dims):
        assert counts[k] > 0, "no pair is %s" % CLASS_NAMES[k]
    free, res = reduce_pairs(cls, v, miss, 0), reduce_pairs(cls, v, miss, min_near)
    cheat, best = int(free["best"][1]), int(res["best"][1])
    assert free["near"][cheat] < min_near and best >= 0 and best != cheat        # would otherwise win
    assert (free["cost"][cheat], cheat) < (res["best"][0], best)
    tied = np.flatnonzero((res["cost"] == res["best"][0]) & (res["near"] >= min_near))
    assert tied.size >= 2 and best == tied[0]                          # a tie, resolved to the lower index


# ---- exact-lattice inputs: the specification once more, in integers only ---------------------------------------------------------
SIGNED_PERMUTATIONS = [np.array([[s[r] if perm[r] == col else 0 for col in range(3)] for r in range(3)], I64)
                       for perm in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]


def score_poses_lattice(field, depth, origin, dims, u, void, S, T, miss_cost, min_near=0):
    """Points at u * h in the sensor frame (u[n, 3] odd integers, h half a cell: cell centres of a lattice through the sensor's
    origin; void[n] marks the points without a measurement), poses (S[P] signed permutations, translation = plane 2 T - N of the
    world lattice per axis): the moved point is the centre of cell T + (S u - 1) / 2, never on a plane.  Integers throughout."""
    n_side = 1 << depth
    k = np.asarray(T, I64)[:, None, :] + (np.einsum("pab,nb->pna", np.asarray(S, I64), np.asarray(u, I64)) - 1) // 2
    in_root = ((k >= 0) & (k < n_side)).all(2)
    rel = k - np.asarray(origin, I64)
    d = np.asarray(dims, I64)
    in_region = in_root & ((rel >= 0) & (rel < d)).all(2)
    flat = np.asarray(field, np.int32).reshape(-1).astype(I64)
    cost = np.zeros(k.shape[0], I64)
    near, far, outside = np.zeros(k.shape[0], np.int32), np.zeros(k.shape[0], np.int32), np.zeros(k.shape[0], np.int32)
    for p in range(k.shape[0]):
        for i in np.flatnonzero(~np.asarray(void)):
            if not in_region[p, i]:
                outside[p] += 1
                cost[p] += miss_cost
                continue
            value = int(flat[(rel[p, i, 2] * d[1] + rel[p, i, 1]) * d[0] + rel[p, i, 0]])
            if value < 0:
                far[p] += 1
                cost[p] += miss_cost
            else:
                near[p] += 1
                cost[p] += value
    best = (-1, -1)
    for p in range(k.shape[0]):
        if near[p] >= min_near and (best[1] < 0 or cost[p] < best[0]):
            best = (int(cost[p]), p)
    return {"cost": cost, "near": near, "far": far, "outside": outside, "best": np.array(best, I64)}


def lattice_inputs(depth, center, edge, u, void, S, T):
    """-> (points float32 [n, 3], poses float32 [P, 16]) of score_poses_lattice's inputs, after proving that binary32 holds them and
    every intermediate of the move exactly (edge a power of two, centre dyadic): the same values in float64"""
    n_side = 1 << depth
    h = float(edge) / n_side
    assert np.log2(float(edge)).is_integer() and (np.asarray(u) % 2 == 1).all()
    p64 = np.asarray(u, np.float64) * h
    points = p64.astype(F)
    assert np.array_equal(points.astype(np.float64), p64)
    points[np.asarray(void)] = np.inf                                   # what the vertex map writes for a pixel without depth
    points[np.flatnonzero(void)[::2], 1] = np.nan                      # ... and the other kind of non-finite, in one component
    points[np.flatnonzero(void)[1::4], 0] = F(0.5)                     # ... and a point of which only two components are void
    M = np.zeros((len(S), 4, 4), np.float64)                           # M[p, c] = column c
    M[:, :3, :3] = np.asarray(S, np.float64).transpose(0, 2, 1)
    M[:, 3, :3] = np.asarray(center, np.float64) + (2 * np.asarray(T, np.float64) - n_side) * h
    M[:, 3, 3] = 1.0
    poses = M.reshape(-1, 16).astype(F)
    assert np.array_equal(poses.astype(np.float64), M.reshape(-1, 16))
    live = ~np.asarray(void)
    w32, w64 = move(poses, points[live]), move(poses, points[live], np.float64)
    assert w32.dtype == F and np.array_equal(w32.astype(np.float64), w64)           # every product and sum was exact
    k = np.arange(n_side + 1)
    for a in range(3):                                                  # ... and so is every plane
        assert np.array_equal(plane(center[a], k, n_side, F(edge) / F(n_side)).astype(np.float64), center[a] + (2 * k - n_side) * h)
    return points, poses


def lattice_case(words, depth, origin, dims, radius, seed, n=90):
    """-> (field, u, void, S, T) for one region of one pool: the observation is a seeded mix of cells seen through the pose
    (S0, T0) -- cells of the region with and without a distance, cells beside the region, cells outside the root, void points --
    and the poses are that pose, whole-cell shifts of it, other turns, one that throws everything out of the root; every pose
    occurs twice, so every cost is tied"""
    rng = np.random.default_rng(seed)
    n_side = 1 << depth
    field = distance_field_separable(words, depth, origin, dims, radius)
    cells = region_cells(origin, dims)
    flat = field.reshape(-1)
    S0, T0 = SIGNED_PERMUTATIONS[int(rng.integers(48))], rng.integers(0, n_side, 3)
    targets = []
    for pick in (cells[flat >= 0], cells[flat < 0]):
        if pick.shape[0]:
            targets.append(pick[rng.integers(0, pick.shape[0], n // 3)])
    anywhere = rng.integers(0, n_side, (n // 4, 3))                     # in the root, in the region or not
    beside = np.asarray(origin) + np.asarray(dims) * rng.integers(0, 2, (n // 6, 3)) + rng.integers(-2, 2, (n // 6, 3))
    beyond = rng.integers(0, n_side, (n // 6, 3))
    beyond[np.arange(n // 6), rng.integers(0, 3, n // 6)] = rng.choice([-1, -2, n_side, n_side + 3], n // 6)
    k = np.concatenate(targets + [anywhere, beside, beyond])
    u = (2 * (k - T0) + 1) @ S0                                         # S0 u = 2 (k - T0) + 1: S0's inverse is its transpose
    void = np.zeros(u.shape[0], bool)
    void[rng.choice(u.shape[0], max(2, u.shape[0] // 10), replace=False)] = True
    S, T = [S0], [T0]
    for shift in ((1, 0, 0), (0, -1, 0), (0, 0, 2), (-3, 1, 0), (0, 0, -1), (2, 2, 2)):
        S.append(S0)
        T.append(T0 + np.asarray(shift))
    for j in rng.integers(0, 48, 4):
        S.append(SIGNED_PERMUTATIONS[int(j)])
        T.append(T0 + rng.integers(-3, 4, 3))
    S.append(S0)
    T.append(T0 + 10 * n_side)                                          # everything outside the root
    S, T = S[::-1] + S, T[::-1] + T                                     # the thrown-out pose first, the true pose in the middle, twice
    return field, u, void, np.asarray(S), np.asarray(T)


def run_lattice_case(words, depth, center, edge, origin, dims, radius, seed):
    field, u, void, S, T = lattice_case(words, depth, origin, dims, radius, seed)
    points, poses = lattice_inputs(depth, center, edge, u, void, S, T)
    cls, v, _ = classify(field, depth, center, edge, origin, dims, points, poses)
    rules = choose_rules(cls, v, radius)
    assert rules is not None
    check_case(cls, v, field, depth, origin, dims, *rules)
    for miss, min_near in (rules, (radius * radius + 1, 0), (0, 0), (MAX_MISS, 3)):
        want = score_poses_lattice(field, depth, origin, dims, u, void, S, T, miss, min_near)
        same_scores(reduce_pairs(cls, v, miss, min_near), want)
        assert np.array_equal(want["near"] + want["far"] + want["outside"], np.full(len(S), (~void).sum()))
    return cls


# the radius per region: the cloud fills the low quarter of the root, so the regions away from it need a long reach to hold a distance
LATTICE_RADII = {"whole_root": 3, "low_corner": 2, "high_corner": 64, "one_cell": 8, "offset_37": 30}


@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_two_restatements_agree_on_the_fused_pool(fused, region):
    words, _ = fused
    origin, dims = fused_regions(DEPTH)[region]
    cls = run_lattice_case(words, DEPTH, ROOT_CENTER, ROOT_EDGE, origin, dims, LATTICE_RADII[region], 7 + len(region))
    if region != "one_cell":                                            # one cell has one value: near or far, not both
        assert {NEAR, FAR} <= set(np.unique(cls).tolist())


HAND_POOLS = {
    "one_cell_depth_3": ([(2, 3, 3)], 3, (0, 2, 1), (5, 4, 6), 2),
    "three_cells_depth_4": ([(2, 3, 3), (12, 13, 1), (7, 7, 8)], 4, (1, 0, 2), (14, 16, 9), 4),
    "a_wall_depth_4_whole_root": ([(x, y, 5) for x in range(3, 12) for y in range(2, 9)], 4, (0, 0, 0), (16, 16, 16), 3),
}


@pytest.mark.parametrize("name", sorted(HAND_POOLS))
def test_the_two_restatements_agree_on_hand_built_pools(name):
    occupied, depth, origin, dims, radius = HAND_POOLS[name]
    cls = run_lattice_case(cells_pool(occupied, depth), depth, (0.5, -0.25, 1.0), 2.0, origin, dims, radius, 31 + len(name))
    assert {NEAR, FAR} <= set(np.unique(cls).tolist())


# ---- the lattice's edges ------------------------------------------------------------------------------------------------------------
IDENTITY = np.eye(4, dtype=F).reshape(16)


def plane_edge_points(depth, center, edge):
    """-> (points [n, 3], axis [n], expected cell or -1 = outside the root [n]): on each axis the planes k = 0, 1, N - 1 and N
    themselves (inside: cells 0, 1, N - 1, N - 1) and one ulp either side of each; the other two coordinates in the middle of cell 2"""
    n_side = 1 << depth
    h = F(edge) / F(n_side)
    points, axes, cells = [], [], []
    for a in range(3):
        for k, on, below, above in ((0, 0, -1, 0), (1, 1, 0, 1), (n_side - 1, n_side - 1, n_side - 2, n_side - 1), (n_side, n_side - 1, n_side - 1, -1)):
            pl = plane(center[a], k, n_side, h)
            for value, cell in ((pl, on), (np.nextafter(pl, F(-np.inf)), below), (np.nextafter(pl, F(np.inf)), above)):
                p = [(plane(center[b], 2, n_side, h) + plane(center[b], 3, n_side, h)) / F(2) for b in range(3)]
                p[a] = value
                points.append(p)
                axes.append(a)
                cells.append(cell)
    return np.asarray(points, F), np.asarray(axes), np.asarray(cells)


@pytest.mark.parametrize("depth,center,edge", [(4, CENTER, EDGE), (8, CENTER, EDGE), (6, ROOT_CENTER, ROOT_EDGE), (12, (0.3, -7.1, 2.0), 3.3)])
def test_points_on_the_planes_and_one_ulp_beside_them(depth, center, edge):
    n_side = 1 << depth
    points, axes, cells = plane_edge_points(depth, center, edge)
    assert points.shape[0] == 36 and len({tuple(p) for p in points.view(np.uint32).tolist()}) == 36    # an ulp is a different number
    field = np.arange(n_side, dtype=np.int32)[None, None, :] * np.ones((1, 1, 1), np.int32)            # a row along x: value = x
    for a in range(3):                                                  # a region of one row along axis a through cell 2 of the others
        origin, dims = [2, 2, 2], [1, 1, 1]
        origin[a], dims[a] = 0, n_side
        sel = axes == a
        cls, v, q = classify(field.reshape([n_side if b == a else 1 for b in (2, 1, 0)]), depth, center, edge, origin, dims, points[sel], IDENTITY)
        assert np.array_equal(move(IDENTITY, points[sel])[0].view(np.uint32), points[sel].view(np.uint32))   # the identity moves nothing
        inside = cells[sel] >= 0
        assert np.array_equal(cls[0] == OUT_ROOT, ~inside) and np.array_equal(cls[0] == NEAR, inside)
        assert np.array_equal(q[0][inside, a], cells[sel][inside]) and np.array_equal(v[0][inside], cells[sel][inside])
        res = reduce_pairs(cls, v, 7, 0)
        assert res["near"][0] == 10 and res["outside"][0] == 2 and res["cost"][0] == cells[sel][inside].sum() + 2 * 7


def edge_case_poses():
    """identity; a translation that overflows to inf; a rotation entry whose product overflows; a NaN in the rotation; a NaN in the
    translation; a NaN in the bottom row, which the move never reads"""
    poses = np.tile(IDENTITY, (6, 1))
    poses[1, 12] = F(3e38)
    poses[2, 0] = F(1e30)
    poses[3, 5] = F(np.nan)
    poses[4, 14] = F(np.nan)
    poses[5, [3, 7, 11, 15]] = F(np.nan)
    return poses


def test_overflow_nan_and_the_miss_costs():
    depth, center, edge = 4, (0.5, -0.25, 1.0), 2.0
    field = distance_field_separable(cells_pool([(2, 3, 3), (9, 9, 9)], depth), depth, (0, 0, 0), (16, 16, 16), 3)
    mids = midpoints(depth, center, edge, (0, 0, 0), (16, 16, 16))
    points = np.concatenate([mids[:: 37], [[3e38, 0.5, 0.5], [1e20, -1e20, 0.0], [np.inf, 0, 0], [0, np.nan, 0]]]).astype(F)
    poses = edge_case_poses()
    cls, v, _ = classify(field, depth, center, edge, (0, 0, 0), (16, 16, 16), points, poses)
    live = np.isfinite(points).all(1)
    assert (cls[:, ~live] == VOID).all() and (~live).sum() == 2
    assert set(cls[0, live].tolist()) == {NEAR, FAR, OUT_ROOT}
    assert (cls[1, live] == OUT_ROOT).all() and np.isinf(move(poses[1], points[-4:-3])[0, 0, 0])           # 3e38 + 3e38: w overflows to inf
    assert np.isinf(move(poses[2], points[-4:-3])[0, 0, 0])                                               # 1e30 * 3e38
    for p in (3, 4):
        assert (cls[p, live] == OUT_ROOT).all()                        # a NaN in a pose: every non-void pair is outside
    assert np.array_equal(cls[5], cls[0])
    n_live = int(live.sum())
    assert n_live * MAX_MISS > 1 << 32
    zero, huge = reduce_pairs(cls, v, 0, 0), reduce_pairs(cls, v, MAX_MISS, 0)
    assert zero["cost"][1] == 0 and huge["cost"][1] == n_live * MAX_MISS and huge["cost"].dtype == I64
    assert zero["best"].tolist() == [0, 1] and huge["best"].tolist() == [int(huge["cost"][0]), 0]
    assert huge["cost"][0] == zero["cost"][0] + MAX_MISS * int(zero["far"][0] + zero["outside"][0]) > 1 << 32
    none = reduce_pairs(cls, v, 5, n_live + 1)
    assert none["best"].tolist() == [-1, -1] and reduce_pairs(cls[:0], v[:0], 5, 0)["best"].tolist() == [-1, -1]
    empty = score_poses_ref(field, depth, center, edge, (0, 0, 0), (16, 16, 16), points[:0], poses, 5)
    assert not empty["cost"].any() and not (empty["near"] | empty["far"] | empty["outside"]).any() and empty["best"].tolist() == [0, 0]
    gone = score_poses_ref(np.zeros((16, 0, 16), np.int32), depth, center, edge, (0, 3, 0), (16, 0, 16), points, poses[:1], 5)
    assert gone["outside"][0] == n_live and gone["cost"][0] == 5 * n_live      # a zero dimension: every non-void pair is outside


# ---- pose_grid ---------------------------------------------------------------------------------------------------------------------
def test_pose_grid_shape_order_middle_and_symmetry():
    pkg = load_pkg()
    rng = np.random.default_rng(5)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    prior = np.eye(4)
    prior[:3, :3], prior[:3, 3] = R, (0.3, -1.2, 2.0)
    prior = prior.T.reshape(16).astype(F)                               # column-major
    prior[3] = F(-0.0)                                                  # a sign that an addition of zero would lose
    steps, yaw_steps, half, yaw_half = (3, 5, 7), 9, (0.1, 0.2, 0.4), 0.3
    grid = pkg.pose_grid(prior, half, steps, yaw_half, yaw_steps)
    assert grid.dtype == F and grid.shape == (3 * 5 * 7 * 9, 16)
    g = grid.reshape(7, 5, 3, 9, 16)                                    # z slowest, then y, then x, yaw fastest
    assert np.array_equal(g[3, 2, 1, 4].view(np.uint32), prior.view(np.uint32))  # the middle candidate is the prior, bit for bit
    t = g[..., 12:15].astype(np.float64) - prior[12:15].astype(np.float64)
    for axis, a in ((2, 0), (1, 1), (0, 2)):                            # the translation of axis a varies along its own grid axis only
        line = np.moveaxis(t[..., a], axis, 0).reshape(steps[a], -1)
        assert np.allclose(line, np.linspace(-half[a], half[a], steps[a])[:, None], atol=1e-6)
        assert np.allclose(line + line[::-1], 0.0, atol=1e-6)          # symmetric offsets
    rot = g[..., :12].reshape(7, 5, 3, 9, 3, 4)[..., :3]                # [.., column, row]
    assert np.array_equal(rot, np.broadcast_to(rot[0, 0, 0], rot.shape))   # the turn does not depend on the offset
    up = R @ np.array([0.0, 1.0, 0.0])
    for k in range(9):                                                  # prior . R_y(yaw): the up axis stays, the turn is yaw_k, symmetric
        Rk = rot[0, 0, 0, k].T.astype(np.float64)
        assert np.allclose(Rk @ np.array([0.0, 1.0, 0.0]), up, atol=1e-6)
        turn = R.T @ Rk
        assert np.allclose(np.arctan2(turn[0, 2], turn[0, 0]), -0.3 + 0.075 * k, atol=1e-6)
        assert np.allclose(turn @ (R.T @ rot[0, 0, 0, 8 - k].T.astype(np.float64)), np.eye(3), atol=1e-6)
    assert (g[..., [3, 7, 11]] == 0).all() and (g[..., 15] == 1).all()
    one = pkg.pose_grid(prior, (1, 1, 1), (1, 1, 1), 0.5, 1)
    assert one.shape == (1, 16) and np.array_equal(one[0].view(np.uint32), prior.view(np.uint32))
    even = pkg.pose_grid(prior, (0.5, 0, 0), (2, 1, 1), 0.0, 1)
    assert np.allclose(even[:, 12] - prior[12], [-0.5, 0.5]) and np.array_equal(even[:, :12], np.tile(prior[:12], (2, 1)))
    other = pkg.pose_grid(prior, (0, 0, 0), (1, 1, 1), 0.2, 3, up=(0, 0, 2))
    assert np.allclose(other[0].reshape(4, 4)[:3, :3].T @ np.array([0, 0, 1.0]), R @ np.array([0, 0, 1.0]), atol=1e-6)
    with pytest.raises(ValueError):
        pkg.pose_grid(prior, half, (3, 0, 3), yaw_half, 3)


# ---- the header and the library -------------------------------------------------------------------------------------------------
def test_the_header_declares_the_calls_and_keeps_its_pins():
    pkg = load_pkg()
    header = " ".join(open(pkg.HEADER_PATH).read().split())
    assert ("int svoslam_score_poses(svoslam_workspace *ws, const int32_t *d_dist2, int32_t max_depth, const float center[3], float "
            "edge_length, const int32_t origin_cell[3], const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, "
            "int32_t n_poses, int32_t miss_cost, int32_t min_near, int64_t *d_cost, int32_t *d_near, int32_t *d_far, int32_t *d_outside, "
            "int64_t *d_best, void *stream);") in header
    assert "int svoslam_workspace_score_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);" in header
    raw = open(pkg.HEADER_PATH).read()
    assert "#define SVOSLAM_STAGE_QUERY 12" in raw and "#define SVOSLAM_STAGE_COUNT 13" in raw
    assert "#define SVOSLAM_MAX_MISS_COST (1 << 30)" in raw and pkg.MAX_MISS_COST == MAX_MISS
    assert "svoslam_score_poses" in raw[raw.index("#define SVOSLAM_STAGE_QUERY 12"):raw.index("#define SVOSLAM_STAGE_COUNT 13")]


def test_library_exports_the_score_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_score_poses", "svoslam_workspace_score_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert len(pkg.SIGNATURES["svoslam_score_poses"][1]) == 19
    for name in ("score_poses", "pose_grid", "relocalize"):
        assert hasattr(pkg, name)
    assert hasattr(pkg.Workspace, "score_buffers") and pkg.SCORE_OUTPUTS == OUTPUTS
    assert os.path.exists(os.path.join(os.path.dirname(pkg.HEADER_PATH), "..", "tools", "map_relocalize.py"))
