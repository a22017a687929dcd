"""What asking the map by volume costs on one MI355X: svoslam_pool_count_boxes and svoslam_pool_nearest_occupied on the map
tools/map_query_bench.py asks.

    python tools/map_volume_bench.py [--frames 20] [--runs 7] [--out profiles/map_volume_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, medians of --runs runs after one warm-up each (a record, not a gate).  Per row: the HIP-event time of the kernel
(svoslam_stage_timing: query), the wall clock of the call + a device synchronisation, and steps (descents) per entry:

  columns      one box per cell of the x-z plane at depth --column-depth (default 9) over the whole footprint, -inf..+inf in y:
               the projected occupancy grid of tools/map_slice.py
  cubes        cubes of 8 cells a side at depth 12 about the last frame's fused points, stop_after = 1 (the any-hit collision
               test) and unlimited
  nearest      svoslam_pool_nearest_occupied at those points at depth 12, radius 16 and 64 cells
"""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from map_slice import slice_inputs  # noqa: E402  (tools/map_slice.py: the script's own directory is on the path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--column-depth", type=int, default=9)
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
    pool = P.pool
    nodes = pool.size
    fx = fy = float(P.focal)
    # the points the last frame fused: its vertex map carried into the map's frame, as the pipeline's back-projection does it
    vmap = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(frames[-1][0], vmap, fx, fy, w, h)
    pkg.transform_vertex_map_dmat(vmap, P.cam.fusion_transform_ptr())
    points = vmap.reshape(-1, 3)
    points = points[torch.isfinite(points).all(1)].contiguous()
    npts = int(points.shape[0])
    half = 4.0 * (2.0 * edge / (1 << depth))                      # 8 cells a side
    cubes = torch.cat([points - half, points + half], 1).contiguous()
    cd = args.column_depth
    columns = torch.from_numpy(slice_inputs(center, edge, cd, 1, -np.inf, np.inf)[0]).cuda()
    ncol = int(columns.shape[0])

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

    def mean(t):
        return float(t.to(torch.float64).mean().item())

    rows = []
    res = pkg.count_boxes(pool, cd, center, edge, columns)
    ms, wall = staged(lambda: pkg.count_boxes(pool, cd, center, edge, columns))
    rows.append(("count_boxes, %d columns (-inf..+inf in y) of the x-z plane at depth %d" % (ncol, cd), ncol, ms, wall, mean(res["steps"]),
                 "%d columns occupied, %d cells counted" % (int((res["count"] > 0).sum().item()), int(res["count"].sum().item()))))
    for stop, label in ((1, "stop_after 1 (any hit)"), (0, "unlimited")):
        res = pkg.count_boxes(pool, depth, center, edge, cubes, stop)
        ms, wall = staged(lambda: pkg.count_boxes(pool, depth, center, edge, cubes, stop))
        rows.append(("count_boxes, %d cubes of 8 cells a side about the last frame's points at depth %d, %s" % (npts, depth, label), npts, ms,
                     wall, mean(res["steps"]), "%d cubes hold a cell, %.1f cells counted per cube" % (
                         int((res["count"] > 0).sum().item()), mean(res["count"]))))
    for radius in (16, 64):
        res = pkg.nearest_occupied(pool, depth, center, edge, points, radius)
        ms, wall = staged(lambda: pkg.nearest_occupied(pool, depth, center, edge, points, radius))
        found = res["dist2"] >= 0
        rows.append(("nearest_occupied, those %d points at depth %d, radius %d cells" % (npts, depth, radius), npts, ms, wall,
                     mean(res["steps"]), "%d found, %d of them in the point's own cell" % (
                         int(found.sum().item()), int((res["dist2"] == 0).sum().item()))))
    lines = [
        "asking the map by volume: tools/map_volume_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes" % (args.frames, w, h, depth, nodes),
        "count_boxes_kernel: 28 VGPRs, nearest_occupied_kernel: 42 VGPRs, 0 bytes of scratch, no LDS (compiler's resource report)",
    ]
    for title, n, ms, wall, steps, note in rows:
        lines += ["", title,
                  "  kernel %9.3f ms  (HIP events)   %8.2f M/s" % (ms, n / ms / 1e3),
                  "  call   %9.3f ms  (wall clock incl. a device synchronisation)" % wall,
                  "  steps per entry %.2f   %s" % (steps, note)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
