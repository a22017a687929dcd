"""What the ground field of a map region and the tracing of paths down it cost on one MI355X, beside the reach field with the body
radius as clearance and the same seed on the same region (unchanged code: the yardstick), on the map tools/map_reach_bench.py asks.

    python tools/map_ground_bench.py [--frames 20] [--runs 7] [--out profiles/map_ground_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with up = +y, on the two regions of tools/map_reach_bench.py about the median cell of the last frame's
fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

Step 2 cells, height 8 cells, radius 0 and 4 cells, climb cost 0 and 3.  One seed: the median, in output order, of the region's
footholds.  Per region, radius and climb cost, medians of --runs runs after one warm-up each (a record, not a gate): the HIP-event
time of the call's bracket (svoslam_stage_timing: query; it spans the per-round readbacks), the wall clock of the call + a device
synchronisation, the rounds and tile runs of svoslam_pool_ground_field and of svoslam_pool_reach_field, the footholds, the reached
cells and the longest path, and the same two times for svoslam_field_trace_ground_paths from 1 start (the dearest cell) and from
4096 starts spread evenly over the reached cells, with room for the longest path."""
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
    up, step, height = pkg.UP_PLUS_Y, 2, 8

    def staged(call):
        def run():
            pkg.stage_timing([pkg.STAGE_QUERY])
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
            finally:
                pkg.stage_timing([])
            assert pairs == 1
            return ms, wall
        run()                                                     # warm-up
        got = [run() for _ in range(args.runs)]
        return float(np.median([g[0] for g in got])), float(np.median([g[1] for g in got]))

    lines = [
        "ground navigation in a map region: tools/map_ground_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "up +y, step %d cells, height %d cells; tiles of 64 x 8 x 8 cells, one workgroup of 256 per tile and round; one 32-byte readback per round; the trace: one lane per start" % (
            step, height),
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        cells = dims[0] * dims[1] * dims[2]
        for radius in (0, 4):
            for climb in (0, 3):
                probe = pkg.ground_field(ws, pool, depth, origin, dims, up, radius, height, step, climb, [], as_tensor=True)
                foot = torch.nonzero(probe.reshape(-1) != -2).reshape(-1)
                if foot.numel() == 0:
                    lines += ["", "%s: %d x %d x %d cells from cell %s, radius %d cells, climb cost %d: no foothold in the region, nothing measured" % (
                        title, dims[0], dims[1], dims[2], origin, radius, climb)]
                    continue
                at = int(foot[foot.numel() // 2].item())
                seed = torch.tensor([[origin[0] + at % dims[0], origin[1] + (at // dims[0]) % dims[1], origin[2] + at // (dims[0] * dims[1])]],
                                    dtype=torch.int32, device="cuda")
                stats, reach_stats = {}, {}
                cost = pkg.ground_field(ws, pool, depth, origin, dims, up, radius, height, step, climb, seed, as_tensor=True, stats=stats)
                pkg.reach_field(ws, pool, depth, origin, dims, radius, seed, as_tensor=True, stats=reach_stats)
                assert stats["seeds_used"] == 1 and stats["footholds"] == foot.numel() and int(cost.reshape(-1)[at].item()) == 0
                ms, wall = staged(lambda: pkg.ground_field(ws, pool, depth, origin, dims, up, radius, height, step, climb, seed, as_tensor=True))
                rms, rwall = staged(lambda: pkg.reach_field(ws, pool, depth, origin, dims, radius, seed, as_tensor=True))
                reached = torch.nonzero(cost.reshape(-1) >= 0).reshape(-1)
                dearest = int(cost.reshape(-1).argmax().item())
                lines += ["", "%s: %d x %d x %d cells from cell %s, radius %d cells, climb cost %d, seed %s   (%d footholds, %d reached, %d cut off; largest cost %d)" % (
                    title, dims[0], dims[1], dims[2], origin, radius, climb, seed[0].tolist(), stats["footholds"], reached.numel(),
                    int((cost == -1).sum().item()), int(cost.max().item())),
                    "  ground_field      bracket %9.3f ms  (HIP events, one bracket, readbacks included)   %9.2f M cells/s   call %9.3f ms  (wall clock incl. a device synchronisation)   %d rounds, %d tile runs" % (
                        ms, cells / ms / 1e3, wall, stats["rounds"], stats["tile_runs"]),
                    "  reach_field       bracket %9.3f ms  (HIP events, one bracket, readbacks included)   %9.2f M cells/s   call %9.3f ms  clearance = the radius, the same seed, unchanged code   %d rounds, %d tile runs" % (
                        rms, cells / rms / 1e3, rwall, reach_stats["rounds"], reach_stats["tile_runs"]),
                    "  ground_field / reach_field, event time: %.2f" % (ms / rms)]
                for count in (1, 4096):
                    pick = torch.tensor([dearest], device="cuda") if count == 1 else reached[torch.linspace(0, reached.numel() - 1, count, device="cuda").long()]
                    starts = torch.stack([origin[0] + pick % dims[0], origin[1] + (pick // dims[0]) % dims[1], origin[2] + pick // (dims[0] * dims[1])], 1).int()
                    lengths = pkg.trace_ground_paths(cost, origin, dims, up, step, climb, starts, 0, as_tensor=True)[1]
                    assert int(lengths.min().item()) >= 1
                    room = int(lengths.max().item())
                    tms, twall = staged(lambda: pkg.trace_ground_paths(cost, origin, dims, up, step, climb, starts, room, as_tensor=True))
                    lines += ["  trace_ground      kernel  %9.3f ms  (HIP events, one bracket)   call %9.3f ms  (wall clock incl. the output buffers' fill and a device synchronisation)   %d starts, longest path %d cells, %d cells in all" % (
                        tms, twall, count, room, int(lengths.sum().item()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
