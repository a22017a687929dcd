"""What scoring candidate poses against a distance field costs on one MI355X in one svoslam_score_poses call, beside the route the
library offered before it: per pose a copy of the points, svoslam_transform_vertex_map_dmat, svoslam_pool_nearest_occupied and a
sum on the device.

    python tools/map_score_bench.py [--frames 20] [--runs 7] [--out profiles/map_score_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker.  The field is svoslam_pool_distance_field with a radius of 16 cells on the 256 x 256 x 64 block of tools/map_field_bench.py
about the median cell of the last frame's fused points; the points are the last frame's vertex map in the sensor frame, whole
(640 x 480 = 307200 points, void ones included) and at pyramid level 3 (80 x 60 = 4800); the poses are a pose_grid about the
tracker's own pose of that frame (+-0.2 m, +-10 degrees), cut to the number wanted.  Shapes (n, P): (4800, 4096), (4800, 64),
(307200, 8), (307200, 1).  Per shape, medians of --runs runs after one warm-up each (a record, not a gate), the device synchronised
before and after every run: for svoslam_score_poses (cost + near + far + best) the HIP-event time of the call's bracket
(svoslam_stage_timing: query) and the wall clock; for the old route the wall clock of the P rounds of four steps, nothing read
back until the end.  Before anything is written the old route's sum and count under the prior are asserted equal to the new call's on
the points that the prior puts at least 2 cells inside the block (the old route knows no region: a point in the root outside the
block has a distance there and is OUTSIDE here).

The block is 64 cells (13 cm) thin, so a whole vertex map mostly misses it and few pairs read the field.  A second table therefore
times the new call alone on the same four shapes with points that stay in the block -- the middles of seeded cells of the block,
seen through the prior -- under a tighter grid of poses (+-0.02 m, +-1 degree): there almost every pair is a gather at a random
place of the 16.8 MB field."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 16
MISS = RADIUS * RADIUS + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    assert torch.cuda.is_available(), "needs a gfx950 device"
    w, h, depth, center, edge = 640, 480, 12, (0.0, 1.5, 0.0), 4.096
    P = pl.SlamPipeline(w, h, depth, center, edge, strict_reference=False)
    ks = list(range(args.frames))
    frames = [synth.render_frame(k, w, h, device="cuda") for k in ks]
    P.run_stream([f[0] for f in frames], [f[1] for f in frames], ks, [pl.ground_truth_view(k, synth) for k in ks])
    torch.cuda.synchronize()
    pool, ws = P.pool, pkg.Workspace()
    fx = fy = float(P.focal)
    full = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(frames[-1][0], full, fx, fy, w, h)
    level, tmp, lw, lh = frames[-1][0].clone(), torch.empty_like(frames[-1][0]), w, h
    for _ in range(3):
        pkg.subsample_depth(level, tmp, lw, lh)
        lw, lh = lw // 2, lh // 2
    small = torch.empty((lh, lw, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(level.reshape(-1)[: lw * lh].reshape(lh, lw), small, fx, fy, w, h)
    clouds = {w * h: full.reshape(-1, 3).contiguous(), lw * lh: small.reshape(-1, 3).contiguous()}
    # the tracker's pose of the last frame, from what it does to the origin and the three unit points
    probe = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, device="cuda")
    pkg.transform_vertex_map_dmat(probe, P.cam.fusion_transform_ptr())
    moved = probe.cpu().numpy().astype(np.float64)
    prior = np.zeros((4, 4))
    prior[:3, :3] = moved[1:] - moved[0]
    prior[3, :3], prior[3, 3] = moved[0], 1.0
    prior = prior.reshape(16).astype(np.float32)                       # rows of this array are the matrix's columns
    world = full.reshape(-1, 3).clone()
    pkg.transform_vertex_map_dmat(world, P.cam.fusion_transform_ptr())
    world = world[torch.isfinite(world).all(1)]
    about = pkg.box_to_cells(depth, center, edge, np.tile(world.median(0).values.cpu().numpy(), 2))[0]
    n_side, dims = 1 << depth, (256, 256, 64)
    origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
    field = pkg.distance_field(ws, pool, depth, origin, dims, RADIUS, as_tensor=True)
    grid = pkg.pose_grid(prior, (0.2, 0.2, 0.2), (9, 9, 9), np.deg2rad(10.0), 9)
    order = np.random.default_rng(3).permutation(grid.shape[0])       # any prefix is spread over the whole grid
    order = np.concatenate([[grid.shape[0] // 2], order[order != grid.shape[0] // 2]])   # ... and starts with the prior itself
    all_poses = torch.from_numpy(grid[order]).cuda()

    def new_call(points, poses):
        return pkg.score_poses(ws, field, depth, center, edge, origin, dims, points, poses, MISS, 0, want=("cost", "near", "far", "best"), as_tensor=True)

    def old_route(points, poses):
        cost = torch.empty(poses.shape[0], dtype=torch.int64, device="cuda")
        near = torch.empty(poses.shape[0], dtype=torch.int32, device="cuda")
        live = torch.isfinite(points).all(1)
        for k in range(poses.shape[0]):
            moved = points.clone()
            pkg.transform_vertex_map_dmat(moved, poses[k].data_ptr())
            d = pkg.nearest_occupied(pool, depth, center, edge, moved, RADIUS, outputs=("dist2",))["dist2"]
            cost[k] = torch.where(live, torch.where(d >= 0, d, MISS), 0).sum()   # no index by a mask: that would read back
            near[k] = ((d >= 0) & live).sum()
        return cost, near

    def timed(call, staged):
        def run():
            if staged:
                pkg.stage_timing([pkg.STAGE_QUERY])
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                ms = pkg.stage_timing_read(pkg.STAGE_QUERY)[0] if staged else float("nan")
            finally:
                if staged:
                    pkg.stage_timing([])
            return ms, wall
        run()                                                     # warm-up
        got = [run() for _ in range(args.runs)]
        return float(np.median([g[0] for g in got])), float(np.median([g[1] for g in got]))

    lines = [
        "scoring poses against a distance field: tools/map_score_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; field: radius %d on %d x %d x %d cells from cell %s (%.1f MB), miss cost %d" % (
            args.frames, w, h, depth, pool.size, RADIUS, dims[0], dims[1], dims[2], origin, field.numel() * 4 / 1e6, MISS),
        "points: the last frame's vertex map in the sensor frame, whole and at pyramid level 3; poses: a 9 x 9 x 9 x 9 grid of +-0.2 m and +-10 degrees about the tracker's pose, the prior first, then shuffled",
        "new: ONE svoslam_score_poses call (cost + near + far + best); kernels = HIP events around its bracket, call = wall clock incl. a device synchronisation",
        "old: per pose a copy of the points + svoslam_transform_vertex_map_dmat + svoslam_pool_nearest_occupied + a sum on the device; wall clock of all P rounds incl. one device synchronisation",
        "",
    ]
    for n, count in ((4800, 4096), (4800, 64), (307200, 8), (307200, 1)):
        points, poses = clouds[n], all_poses[:count].contiguous()
        got = new_call(points, poses)
        # the two routes on the points that the prior (pose 0) puts at least 2 cells inside the block: there no region is in play
        moved = points.clone()
        pkg.transform_vertex_map_dmat(moved, poses[0].data_ptr())
        at = (moved.double() - (torch.tensor(center, dtype=torch.float64, device="cuda") - edge)) / (2.0 * edge / n_side)
        lo, hi = torch.tensor(origin, device="cuda") + 2, torch.tensor(origin, device="cuda") + torch.tensor(dims, device="cuda") - 2
        inner = points[(torch.isfinite(at) & (at >= lo) & (at < hi)).all(1)].contiguous()
        old_cost, old_near = old_route(inner, poses[:1])
        same = new_call(inner, poses[:1])
        assert inner.shape[0] > 0 and torch.equal(same["cost"], old_cost) and torch.equal(same["near"], old_near), "the two routes disagree"
        best = got["best"].cpu().tolist()
        new_ms, new_wall = timed(lambda: new_call(points, poses), True)
        _, old_wall = timed(lambda: old_route(points, poses), False)
        lines += ["n = %6d points, P = %4d poses (%.2f M pairs, %.1f %% of them read the field): best cost %d at pose %d; the %d points the prior puts well inside the block: cost %d, %d near, by both routes" % (
            n, count, n * count / 1e6, 100.0 * float((got["near"].sum() + got["far"].sum()).item()) / (n * count), best[0], best[1], int(inner.shape[0]), int(old_cost[0].item()), int(old_near[0].item())),
            "  new   kernels %9.3f ms   %9.1f M pairs/s   call %9.3f ms" % (new_ms, n * count / new_ms / 1e3, new_wall),
            "  old                          %9.1f M pairs/s   call %9.3f ms   = %.1f x the new call" % (n * count / old_wall / 1e3, old_wall, old_wall / new_wall)]
    # the same shapes with the gather in play: the vertex map above mostly misses a block that is 64 cells (13 cm) thin, so here the
    # points are the middles of seeded cells of the block seen through the prior, and the poses a grid of +-10 cells and +-1 degree
    M = prior.astype(np.float64).reshape(4, 4).T
    tight = pkg.pose_grid(prior, (0.02, 0.02, 0.02), (9, 9, 9), np.deg2rad(1.0), 9)
    tight_poses = torch.from_numpy(tight[order]).cuda()
    rng = np.random.default_rng(11)
    lines += ["", "the same shapes with points that stay in the block: the middles of seeded cells of the block seen through the prior, poses a 9 x 9 x 9 x 9 grid of +-0.02 m and +-1 degree (new call only)"]
    for n, count in ((4800, 4096), (4800, 64), (307200, 8), (307200, 1)):
        cells = np.asarray(origin) + rng.random((n, 3)) * np.asarray(dims)
        target = np.asarray(center) - edge + cells * (2.0 * edge / n_side)
        points = torch.from_numpy(((target - M[:3, 3]) @ M[:3, :3]).astype(np.float32)).cuda()
        poses = tight_poses[:count].contiguous()
        got = new_call(points, poses)
        new_ms, new_wall = timed(lambda: new_call(points, poses), True)
        lines.append("n = %6d points, P = %4d poses (%.2f M pairs, %.1f %% of them read the field):   new   kernels %9.3f ms   %9.1f M pairs/s   call %9.3f ms" % (
            n, count, n * count / 1e6, 100.0 * float((got["near"].sum() + got["far"].sum()).item()) / (n * count), new_ms, n * count / new_ms / 1e3, new_wall))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
