"""What the distance field of a map region costs on one MI355X, beside asking svoslam_pool_nearest_occupied once per cell, on the map
tools/map_query_bench.py and tools/map_volume_bench.py ask.

    python tools/map_field_bench.py [--frames 20] [--runs 7] [--out profiles/map_field_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with radius 16 and 64 cells, on two regions about the median cell of the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane, the clearance plane of tools/map_slice.py

Per region and radius, medians of --runs runs after one warm-up each (a record, not a gate): the HIP-event time of the field's four
launches (svoslam_stage_timing: query, one bracket per call), the wall clock of the call + a device synchronisation, cells per
second, the split over the launches (svoslam_pool_distance_field_profile), and the same two times for
svoslam_pool_nearest_occupied (unchanged code) on the centres of the same cells, dist2 only.  The two dist2 arrays are asserted
equal before anything is written."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cell_centres(torch, depth, center, edge, origin, dims):
    """[nz * ny * nx, 3] float32 on the device: (P(k) + P(k + 1)) / 2 in binary32 for every cell of the region, x fastest"""
    n_side = 1 << depth
    h = np.float32(edge) / np.float32(n_side)
    axes = []
    for a in range(3):
        k = torch.arange(origin[a], origin[a] + dims[a] + 1, device="cuda", dtype=torch.int64)
        p = float(np.float32(center[a])) + (2 * k - n_side).to(torch.float32) * float(h)
        axes.append((p[:-1] + p[1:]) / 2)
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).contiguous()


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
        "the distance field of a map region: tools/map_field_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "region_raster_kernel 18 VGPRs, edt_x_kernel<false> 16, edt_pass_kernel<kLds, false> 13 (LDS) / 10 (global), 0 bytes of scratch; LDS (64 + 2 R) * 256 bytes per one-wavefront workgroup (compiler's resource report)",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        cells = dims[0] * dims[1] * dims[2]
        centres = cell_centres(torch, depth, center, edge, origin, dims)
        for radius in (16, 64):
            field = pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True)
            near = pkg.nearest_occupied(pool, depth, center, edge, centres, radius, outputs=("dist2",))["dist2"]
            assert torch.equal(field.reshape(-1), near), "the field differs from svoslam_pool_nearest_occupied at the cell centres"
            ms, wall = staged(lambda: pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True))
            split = []
            for _ in range(args.runs + 1):
                one = []
                pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True, launch_ms=one)
                split.append(one)
            split = np.median(np.array(split[1:]), 0)
            pms, pwall = staged(lambda: pkg.nearest_occupied(pool, depth, center, edge, centres, radius, outputs=("dist2",)))
            lines += ["", "%s: %d x %d x %d cells from cell %s, radius %d cells   (%d cells on occupied ones, %d with nothing within the radius)" % (
                title, dims[0], dims[1], dims[2], origin, radius, int((field == 0).sum().item()), int((field < 0).sum().item())),
                "  distance_field    kernels %9.3f ms  (HIP events, one bracket)   %9.2f M cells/s   call %9.3f ms  (wall clock incl. a device synchronisation)" % (
                    ms, cells / ms / 1e3, wall),
                "    per launch: raster %.3f ms, x pass %.3f ms, y pass %.3f ms, z pass %.3f ms" % tuple(split),
                "  nearest_occupied  kernel  %9.3f ms  (HIP events)                %9.2f M points/s  call %9.3f ms   on the centres of the same cells, dist2 only: the same values" % (
                    pms, cells / pms / 1e3, pwall),
                "  nearest_occupied / distance_field, kernel time: %.1f" % (pms / ms)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
