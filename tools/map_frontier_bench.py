"""What observing a sensor frame and finding the frontier of the known cost on one MI355X, beside the gather form of the same walk:
svoslam_pool_visibility_field with the sensor's cell as its one viewpoint over the same region.

    python tools/map_frontier_bench.py [--frames 20] [--runs 7] [--level 10] [--out profiles/map_frontier_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker.  The observation is the last frame: its vertex map in the sensor frame (307200 rays, the pixels without depth void) with
the pose the frame was fused with, on the lattice of depth --level.  Two regions:

  view box     the bounding box of the sensor's cell and the cells the rays end in, at most 512 cells per axis about its middle
  slab         up to 64 layers of the view box about the median of the ends, across the viewing direction: most of every ray
               lies outside it

Per region, medians of --runs runs after one warm-up each (a record, not a gate): the HIP-event time of each call's one bracket
(svoslam_stage_timing: query) for svoslam_field_observe_rays (with rays/s, and walked crossings/s: the sum of |D_x| + |D_y| + |D_z|
over the marked rays, every one of which the plain form walks from the sensor's cell to its end whether or not it lies in the region),
for svoslam_field_observe_rays without rays (the two clears and the finish launch alone), for svoslam_pool_frontier_field, and for the
yardstick: svoslam_pool_visibility_field, count only, one viewpoint in the sensor's cell, range = the longest ray, which walks from
the viewpoint to every cell of the region in range, less the same call without viewpoints (its raster).  Its crossings/s count |D|_1
over the region cells in range, an upper bound: a blocked walk ends early.  Neither variant of DESIGN.md section 25 (entering the walk
at the region, one elected lane per word) is built, so none is timed."""
import argparse
import datetime
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--level", type=int, default=10, help="lattice depth of the observation")
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
    points = vmap.reshape(1, -1, 3).contiguous()
    # the pose the frame was fused with, read off the library's own transform: the images of the origin and the three unit points
    probe = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32, device="cuda").reshape(1, 4, 3).contiguous()
    pkg.transform_vertex_map_dmat(probe, P.cam.fusion_transform_ptr())
    moved = probe.reshape(4, 3).cpu().numpy().astype(np.float64)
    pose = np.zeros(16, np.float32)
    for col in range(3):
        pose[4 * col:4 * col + 3] = moved[1 + col] - moved[0]
    pose[12:15], pose[15] = moved[0], 1.0
    poses = pose.reshape(1, 16)
    level, n_side = args.level, 1 << args.level
    size = 2.0 * edge / n_side
    low = np.asarray(center, np.float64) - edge
    world = vmap.reshape(-1, 3).clone()
    pkg.transform_vertex_map_dmat(world, P.cam.fusion_transform_ptr())
    world = world.cpu().numpy().astype(np.float64)
    live = np.isfinite(world).all(1)
    ends = np.floor((world[live] - low) / size).astype(np.int64)        # for the regions and the crossing counts: the library has its own rule
    ends = ends[((ends >= 0) & (ends < n_side)).all(1)]
    sensor = np.floor((moved[0] - low) / size).astype(np.int64)
    assert ((sensor >= 0) & (sensor < n_side)).all(), "the sensor stands outside the root"
    reach = int(np.ceil(np.sqrt(((ends - sensor) ** 2).sum(1).max())))
    crossings = int(np.abs(ends - sensor).sum())
    lo, hi = np.minimum(ends.min(0), sensor), np.maximum(ends.max(0), sensor) + 1
    mid = (lo + hi) // 2
    lo, hi = np.maximum(lo, mid - 256), np.minimum(hi, mid + 256)
    median = np.median(ends, 0).astype(np.int64)
    axis = int(np.argmax(np.abs(median - sensor)))                      # the slab lies across the viewing direction
    slab_lo, slab_hi = lo.copy(), hi.copy()
    slab_lo[axis] = max(lo[axis], median[axis] - 32)
    slab_hi[axis] = min(hi[axis], slab_lo[axis] + 64)

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

    lines = [
        "observed space of a map region: tools/map_frontier_bench.py --frames %d --runs %d --level %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, level, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; the observation: the last frame, %d rays, %d with depth, on the lattice of depth %d" % (
            args.frames, w, h, depth, nodes, w * h, int(live.sum()), level),
        "sensor cell %s, longest ray %d cells, %d crossings over all rays (|D|_1 from cells computed in float64 on the host)" % (sensor.tolist(), reach, crossings),
        "HIP events around each call's one bracket; the plain form of observe_kernel; the kernels' resource report is in DESIGN.md section 25",
    ]
    view = torch.from_numpy(sensor.astype(np.int32).reshape(1, 3)).cuda()
    none = np.zeros((0, 3), np.int32)
    for title, a, b in (("view box", lo, hi), ("slab", slab_lo, slab_hi)):
        origin, dims = [int(v) for v in a], [int(v) for v in b - a]
        obs = torch.zeros(dims[::-1], dtype=torch.uint8, device="cuda")
        _, summary = pkg.observe_rays(ws, obs, level, center, edge, origin, dims, points, poses)
        field = pkg.frontier_field(ws, pool, level, origin, dims, obs, want=("summary",))["summary"]
        t_obs = staged(lambda: pkg.observe_rays(ws, obs, level, center, edge, origin, dims, points, poses, as_tensor=True))
        t_front = staged(lambda: pkg.frontier_field(ws, pool, level, origin, dims, obs, as_tensor=True))
        t_bare = staged(lambda: pkg.observe_rays(ws, obs, level, center, edge, origin, dims, points[:, :0], poses, as_tensor=True))
        radius = min(reach, 4096)
        t_vis = staged(lambda: pkg.visibility_field(ws, pool, level, origin, dims, radius, view, want=("count",), as_tensor=True))
        t_raster = staged(lambda: pkg.visibility_field(ws, pool, level, origin, dims, radius, none, want=("count",), as_tensor=True))
        z, y, x = torch.meshgrid(*[torch.arange(origin[k], origin[k] + dims[k], dtype=torch.int32, device="cuda") for k in (2, 1, 0)], indexing="ij")
        d = torch.stack([x, y, z], -1).reshape(-1, 3) - view
        near = (d * d).sum(1) <= radius * radius
        gather = int(d[near].abs().sum().item())
        del x, y, z, d, near
        marked = int(summary[3])
        lines += ["", "%s: %d x %d x %d cells from cell %s: rays %s (void, outside, far, marked); %d cells passed through, %d ended in; cells per state %s" % (
            title, dims[0], dims[1], dims[2], origin, summary[:4].tolist(), int(summary[4]), int(summary[5]), field.tolist()),
            "  observe_rays %9.3f ms (no rays: %.3f ms)   %.1f M rays/s, %.2f G crossings/s   frontier_field %9.3f ms" % (
                t_obs, t_bare, marked / t_obs / 1e3, crossings / t_obs / 1e6, t_front),
            "  visibility_field, one viewpoint in the sensor's cell, range %d: %9.3f ms, of which raster %.3f ms: %.2f G crossings/s at most" % (
                radius, t_vis, t_raster, gather / max(t_vis - t_raster, 1e-6) / 1e6)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
