"""What the owner field of a map region costs on one MI355X, beside the reach field with the same seeds on the same region (that
relaxation is phase 1 of this call, so it is the floor) and beside the way the answer was had before: one reach field per seed and
an arg-min on the host.  On the map tools/map_reach_bench.py asks.

    python tools/map_owner_bench.py [--frames 20] [--runs 7] [--out profiles/map_owner_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with clearance 0 and 4 cells, on the two regions of tools/map_reach_bench.py about the median cell of
the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

with 1, 8 and 64 seeds, spread evenly, in output order, over the region's traversable cells.  Before anything is timed the steps
are asserted to equal svoslam_pool_reach_field's, and for the 8-seed rows the owners to equal a host arg-min over the per-seed
reach fields (the smallest index on a tie).  Per row, medians of --runs runs after one warm-up each (a record, not a gate): the
HIP-event time of the call's one bracket (svoslam_stage_timing: query; it spans the per-round readbacks), the rounds and tile runs
of both phases, the same time for svoslam_pool_reach_field (unchanged code), and for the 8-seed rows the wall clock of the n reach
fields and the host arg-min."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    nodes = pool.size
    fx = fy = float(P.focal)
    vmap = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(frames[-1][0], vmap, fx, fy, w, h)
    pkg.transform_vertex_map_dmat(vmap, P.cam.fusion_transform_ptr())
    points = vmap.reshape(-1, 3)
    points = points[torch.isfinite(points).all(1)]
    median = points.median(0).values.cpu().numpy()
    about = pkg.box_to_cells(depth, center, edge, np.concatenate([median, median]))[0]
    n_side = 1 << depth

    def staged(call):
        def run():
            pkg.stage_timing([pkg.STAGE_QUERY])
            try:
                torch.cuda.synchronize()
                call()
                torch.cuda.synchronize()
                ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
            finally:
                pkg.stage_timing([])
            assert pairs == 1
            return ms
        run()                                                     # warm-up
        return float(np.median([run() for _ in range(args.runs)]))

    def wall(call):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        run()
        return float(np.median([run() for _ in range(args.runs)]))

    lines = [
        "the owner field of a map region: tools/map_owner_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "tiles of 64 x 8 x 8 cells, one workgroup of 256 per tile and round, two relaxations (steps, then owners); one 32-byte readback per round",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        for clearance in (0, 4):
            field = pkg.distance_field(ws, pool, depth, origin, dims, clearance, as_tensor=True)
            free = torch.nonzero(field.reshape(-1) == -1).reshape(-1)
            assert free.numel() >= 64, "fewer than 64 traversable cells in the region"
            lines += ["", "%s: %d x %d x %d cells from cell %s, clearance %d cells, %d traversable" % (title, dims[0], dims[1], dims[2], origin, clearance,
                                                                                                       free.numel())]
            for count in (1, 8, 64):
                at = free[((torch.arange(count, device="cuda") * 2 + 1) * free.numel()) // (2 * count)]
                seeds = torch.stack([origin[0] + at % dims[0], origin[1] + (at // dims[0]) % dims[1], origin[2] + at // (dims[0] * dims[1])], 1).to(torch.int32)
                stats = {}
                steps, owner = pkg.owner_field(ws, pool, depth, origin, dims, clearance, seeds=seeds, as_tensor=True, stats=stats)
                reach = pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds, as_tensor=True)
                assert torch.equal(steps, reach), "the steps are not the reach field's"
                assert stats["seeds_used"] == count and torch.equal(owner < 0, steps < 0) and torch.equal(owner[owner < 0], steps[steps < 0])

                def by_hand():
                    """n reach fields and a host arg-min: the smallest index at the minimum"""
                    each = np.stack([pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds[k:k + 1]) for k in range(count)]).astype(np.int64)
                    best = np.where(each >= 0, each, np.iinfo(np.int64).max)
                    return np.where(best.min(0) < np.iinfo(np.int64).max, best.argmin(0), each[0]).astype(np.int32)
                if count == 8:
                    assert np.array_equal(by_hand(), owner.cpu().numpy()), "the owners are not the host arg-min's"
                ms = staged(lambda: pkg.owner_field(ws, pool, depth, origin, dims, clearance, seeds=seeds, as_tensor=True))
                rms = staged(lambda: pkg.reach_field(ws, pool, depth, origin, dims, clearance, seeds, as_tensor=True))
                sizes = torch.bincount(owner[owner >= 0].long(), minlength=count)
                lines += ["  %2d seeds   owner_field  bracket %9.3f ms   steps: %d rounds, %d tile runs; owners: %d rounds, %d tile runs   reach_field, same seeds  bracket %9.3f ms   ratio %.2f   (%d cells reached, the largest share %d, the smallest %d)" % (
                    count, ms, stats["rounds"], stats["tile_runs"], stats["owner_rounds"], stats["owner_tile_runs"], rms, ms / rms,
                    int((steps >= 0).sum().item()), int(sizes.max().item()), int(sizes.min().item()))]
                if count == 8:
                    hms = wall(by_hand)
                    lines += ["             %d reach fields and a host arg-min  wall clock %9.3f ms   = %.1f x the owner field's bracket" % (count, hms, hms / ms)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
