"""Localisation against the map: candidate poses scored on a distance field, grids of them, and the coarse-to-fine search."""
import numpy as np

from ._abi import _fa, _stream, check, lib
from ._args import Outputs, device_i32, device_rows, ptr_or_null, region, region_cells
from ._fields import box_to_cells, distance_field

MAX_MISS_COST = 1 << 30                                                 # include/svoslam.h SVOSLAM_MAX_MISS_COST
SCORE_OUTPUTS = ("cost", "near", "far", "outside", "best")


def score_poses(ws, field, max_depth, center, edge_length, origin, dims, points, poses, miss_cost, min_near=0, want=("cost", "near"),
                as_tensor=False):
    """svoslam_score_poses: every one of `points` ([n, 3] float32 in the sensor frame, e.g. a vertex map; a non-finite point counts
    nowhere) moved by every one of `poses` ([P, 16] float32, sensor to world, the layout of every trans[16]) and looked up in
    `field`, the int32 [nz, ny, nx] distance field of the region origin[3] .. origin + dims[3] (distance_field's or nearest_field's
    dist2 with the same max_depth, origin and dims).  Per pose: "cost" int64 = the sum of the field's values where it has one +
    miss_cost * the pairs where it has none or that fall outside the region, and the counts "near", "far", "outside" (int32).
    "best": int64 (cost, index) of the cheapest pose with near >= min_near, the lowest index among equals, (-1, -1) if none.
    field, points and poses may be cuda tensors (used in place) or arrays (uploaded).  `want`: the subset to compute; the others are
    passed as NULL.  -> a dict of numpy arrays, or with as_tensor cuda tensors, in which case nothing is synchronised."""
    import torch
    _, n3, o3c, n3c = region(origin, dims)
    outs = Outputs({name: (torch.int64, np.int64) if name in ("cost", "best") else (torch.int32, np.int32) for name in SCORE_OUTPUTS}, want)
    t_field = device_i32(field, "field", 1)
    cells = region_cells(n3)
    if int(t_field.shape[0]) != cells:
        raise ValueError("the field has %d values, the region %d cells" % (int(t_field.shape[0]), cells))
    t_points = device_rows(points, torch.float32, np.float32, 3, "points")
    t_poses = device_rows(poses, torch.float32, np.float32, 16, "poses")
    n, count = int(t_points.shape[0]), int(t_poses.shape[0])
    outs.alloc(count, best=2)
    check(lib().svoslam_score_poses(ws._h, ptr_or_null(t_field), int(max_depth), _fa(center, 3), float(edge_length), o3c, n3c,
                                    ptr_or_null(t_points), n, ptr_or_null(t_poses), count, int(miss_cost), int(min_near), *outs.ptrs(),
                                    _stream()))
    return outs.result(as_tensor)


def _rotation(axis, angle):
    """Rodrigues' rotation about the unit vector along `axis`, float64 [3, 3]; exactly the identity at angle 0"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _symmetric_steps(half, steps):
    """`steps` evenly spaced values from -half to half: exactly symmetric, the middle one of an odd number exactly 0"""
    steps = int(steps)
    if steps < 1:
        raise ValueError("at least one step per axis")
    if steps == 1:
        return np.zeros(1)
    return (np.arange(steps, dtype=np.float64) - (steps - 1) / 2.0) * (2.0 * float(half) / (steps - 1))


def pose_grid(prior, half_extent, steps, yaw_half, yaw_steps, up=(0, 1, 0)):
    """A grid of candidate poses around `prior` (16 floats, sensor to world, the layout of every trans[16]) for score_poses: host only.
    Candidate = T(dx, dy, dz) . prior . R_up(yaw): the sensor moved by (dx, dy, dz) in the world and turned by yaw (radians) about
    its own `up` axis.  Offsets run over steps[a] evenly spaced values in [-half_extent[a], half_extent[a]] per world axis, yaws over
    yaw_steps values in [-yaw_half, yaw_half]; both symmetric about 0, a single step is 0.  ORDER: z slowest, then y, then x, yaw
    fastest: index = ((iz * steps[1] + iy) * steps[0] + ix) * yaw_steps + iyaw.  Computed in float64 and rounded once; with odd step
    counts the middle candidate is `prior` bit for bit.  -> float32 [steps[0] * steps[1] * steps[2] * yaw_steps, 16]."""
    prior32 = np.asarray(prior, np.float32).reshape(16)
    M = prior32.astype(np.float64).reshape(4, 4).T                      # column-major storage -> M[row, col]
    offs = [_symmetric_steps(half_extent[a], steps[a]) for a in range(3)]
    yaws = _symmetric_steps(yaw_half, yaw_steps)
    turned = np.empty((len(yaws), 4, 4))
    for k, yaw in enumerate(yaws):
        R = np.eye(4)
        R[:3, :3] = _rotation(up, yaw)
        turned[k] = M @ R
    dz, dy, dx = np.meshgrid(offs[2], offs[1], offs[0], indexing="ij")
    shift = np.stack([dx, dy, dz], -1).reshape(-1, 1, 3)               # z slowest, x fastest
    out = np.broadcast_to(turned, (shift.shape[0],) + turned.shape).copy()
    out[:, :, :3, 3] += shift
    grid = np.ascontiguousarray(out.transpose(0, 1, 3, 2)).reshape(-1, 16).astype(np.float32)
    still = (np.broadcast_to(shift == 0.0, out.shape[:2] + (3,)).all(-1) & (yaws == 0.0)[None, :]).reshape(-1)
    grid[still] = prior32                                               # -0.0 + 0.0 is +0.0: the unmoved candidate is the prior's own bits
    return grid


def relocalize(ws, pool, max_depth, center, edge_length, points, prior, half_extent, yaw_half, radius_cells, steps=(9, 9, 9), yaw_steps=9,
               rounds=3, min_near_fraction=0.5, up=(0, 1, 0)):
    """Where in this map were these points seen?  A coarse-to-fine search with score_poses around `prior` (16 floats, sensor to world):
    `points` ([n, 3] float32 in the sensor frame, a cuda tensor or an array; non-finite = no measurement), half_extent[3] in metres
    per world axis and yaw_half in radians about the sensor's `up` axis are the first round's pose_grid; every round scores its
    grid, re-centres on the best pose if that is strictly cheaper than the centre it came from, and halves extents and yaw.  The
    distance field (radius_cells, miss cost radius_cells^2 + 1) is built once, over the box of cells the search can reach, and
    stays on the device; every round reads back only the two words of `best`.  A pose qualifies with near >= ceil(min_near_fraction
    * the finite points).  -> {"pose": float32 [16], "cost": int, "near": int, "rounds": [(cost, index) per round]}, or None when
    no pose of some round qualifies (the rounds so far are then lost: nothing was found)."""
    import torch
    t_points = device_rows(points, torch.float32, np.float32, 3, "points")
    prior32 = np.asarray(prior, np.float32).reshape(16)
    finite = torch.isfinite(t_points).all(1)
    n_finite = int(finite.sum().item())
    if n_finite == 0:
        return None
    # the box the search can reach: the points under the prior, moved by at most the sum of all rounds' extents (< 2 x the first)
    # and turned by at most the sum of all rounds' yaws about the sensor's origin (a chord of the farthest point's circle)
    live = t_points[finite].double()
    M = torch.from_numpy(prior32.astype(np.float64).reshape(4, 4).T.copy()).cuda()
    world = live @ M[:3, :3].T + M[:3, 3]
    chord = 2.0 * float(live.norm(dim=1).max().item()) * np.sin(min(2.0 * abs(float(yaw_half)), np.pi) / 2.0)
    cell = 2.0 * float(edge_length) / (1 << int(max_depth))
    slack = np.array([2.0 * abs(float(e)) for e in half_extent]) + chord + cell
    box = np.concatenate([world.min(0).values.cpu().numpy() - slack, world.max(0).values.cpu().numpy() + slack]).astype(np.float32)
    cells = box_to_cells(max_depth, center, edge_length, box)
    if cells is None:
        return None                                                     # the search cannot reach the root
    origin, dims = cells[0], cells[1] - cells[0] + 1
    field = distance_field(ws, pool, max_depth, origin, dims, radius_cells, as_tensor=True)
    miss, min_near = int(radius_cells) * int(radius_cells) + 1, int(np.ceil(float(min_near_fraction) * n_finite))
    pose, extent, yaw, found, best_cost = prior32, np.asarray(half_extent, np.float64), float(yaw_half), [], None
    for _ in range(int(rounds)):
        grid = pose_grid(pose, extent, steps, yaw, yaw_steps, up)
        best = score_poses(ws, field, max_depth, center, edge_length, origin, dims, t_points, grid, miss, min_near, want=("best",))["best"]
        cost, index = int(best[0]), int(best[1])
        if index < 0:
            return None
        found.append((cost, index))
        if best_cost is None or cost < best_cost:                       # an equally cheap neighbour does not move the centre
            pose, best_cost = grid[index], cost
        extent, yaw = extent / 2.0, yaw / 2.0
    last = score_poses(ws, field, max_depth, center, edge_length, origin, dims, t_points, pose.reshape(1, 16), miss, 0, want=("cost", "near"))
    return {"pose": pose.copy(), "cost": int(last["cost"][0]), "near": int(last["near"][0]), "rounds": found}
