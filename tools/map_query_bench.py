"""What asking the map costs on one MI355X: svoslam_pool_cast_rays beside svoslam_raycast_model_depth on the same view, and
svoslam_pool_query_points on the map's own points.

    python tools/map_query_bench.py [--frames 20] [--runs 7] [--out profiles/map_query_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker -- the map tools/surface_mesh_bench.py builds -- then, medians of --runs runs after one warm-up each (a record, not a gate):

  cast_rays     the 640x480 rays of the last frame's pinhole view (pixel-row order: coherent neighbours), cast at depth 12 with
                every output written: HIP-event time of the kernel (svoslam_stage_timing: query) and the wall clock of the call +
                a device synchronisation; Mrays/s from the kernel time, hits and blocks visited per ray
  model depth   svoslam_raycast_model_depth of the same view (cone stepping, stops on A >= 254): wall clock of the call + a
                device synchronisation, and its steps per ray
  query_points  the vertex map of the last frame in the map's frame (the points that frame fused), looked up at depth 12:
                kernel time, wall clock, Mpoints/s and the share found at level 12
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


def median_of(runs, fn):
    fn()                                                          # warm-up
    return float(np.median([fn() for _ in range(runs)]))


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
    pool = P.pool
    nodes = pool.size
    # the pinhole view of the last frame: the camera-to-map matrix the fusion used (column-major, as the library takes it)
    cam = pkg.copy_from_device(P.cam.fusion_transform_ptr(), (16,), np.float32)
    fx = fy = float(P.focal)
    m = cam.reshape(4, 4).T.astype(np.float64)                    # row-major 4x4
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    d_cam = np.stack([(px - w // 2) / fx, (h // 2 - py) / fy, np.ones_like(px, np.float64)], -1).reshape(-1, 3)
    v = d_cam @ m[:3, :3].T
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rays = torch.from_numpy(np.concatenate([np.tile(m[:3, 3], (w * h, 1)), v], 1).astype(np.float32)).cuda()
    n = w * h

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

    cast_ms, cast_wall = staged(lambda: pkg.cast_rays(pool, depth, center, edge, rays))
    res = pkg.cast_rays(pool, depth, center, edge, rays)
    hits = int((res["node"] >= 0).sum().item())
    cast_steps = float(res["steps"].to(torch.float64).mean().item())
    saturated = int(((res["node"] >= 0) & (((res["color"] >> 24) & 0xFF) >= 254)).sum().item())
    depth_img = torch.zeros((h, w), dtype=torch.int16, device="cuda")   # (uint16 bit pattern, as the sensor frames)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def model():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pkg.raycast_model_depth(depth_img, fx, fy, pool.data_ptr, center, edge, cam_to_world_ptr=P.cam.fusion_transform_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    model_wall = median_of(args.runs, model)
    pkg.raycast_model_depth(depth_img, fx, fy, pool.data_ptr, center, edge, cam_to_world_ptr=P.cam.fusion_transform_ptr(), counters=cnt)
    model_steps = int(cnt[0].item()) / n
    model_hits = int((depth_img != 0).sum().item())
    # the points the last frame fused: its vertex map carried into the map's frame, as the pipeline's back-projection does it
    vmap = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(frames[-1][0], vmap, fx, fy, w, h)
    pkg.transform_vertex_map_dmat(vmap, P.cam.fusion_transform_ptr())
    points = vmap.reshape(-1, 3)
    points = points[torch.isfinite(points).all(1)].contiguous()
    npts = int(points.shape[0])
    look_ms, look_wall = staged(lambda: pkg.query_points(pool, depth, center, edge, points))
    lv = pkg.query_points(pool, depth, center, edge, points, outputs=("level",))["level"]
    at_depth = int((lv == depth).sum().item())
    lines = [
        "asking the map: tools/map_query_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes" % (args.frames, w, h, depth, nodes),
        "",
        "svoslam_pool_cast_rays, %d rays of the last frame's pinhole view at depth %d, all five outputs" % (n, depth),
        "  kernel %9.3f ms  (HIP events)   %8.1f Mrays/s" % (cast_ms, n / cast_ms / 1e3),
        "  call   %9.3f ms  (wall clock incl. a device synchronisation)" % cast_wall,
        "  hits %d of %d (%d of them on a node with A >= 254)   blocks visited per ray %.2f" % (hits, n, saturated, cast_steps),
        "  cast_rays_kernel: 39 VGPRs, 0 bytes of scratch, no LDS (compiler's resource report)",
        "",
        "svoslam_raycast_model_depth of the same view (cone stepping at the LOD's cell size, stops on A >= 254)",
        "  call   %9.3f ms  (wall clock incl. a device synchronisation)" % model_wall,
        "  pixels with a depth %d of %d   samples per ray %.2f" % (model_hits, n, model_steps),
        "",
        "svoslam_pool_query_points, the %d points of the last frame at depth %d, all four outputs" % (npts, depth),
        "  kernel %9.3f ms  (HIP events)   %8.1f Mpoints/s" % (look_ms, npts / look_ms / 1e3),
        "  call   %9.3f ms  (wall clock incl. a device synchronisation)" % look_wall,
        "  found at level %d: %d of %d" % (depth, at_depth, npts),
        "  query_points_kernel: 18 VGPRs, 0 bytes of scratch, no LDS",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
