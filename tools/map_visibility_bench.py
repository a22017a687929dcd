"""What the visibility field of a map region costs on one MI355X beside the distance field of the same region and beside one exact
ray per (cell, viewpoint) pair, on the map and the regions of tools/map_field_bench.py.

    python tools/map_visibility_bench.py [--frames 20] [--runs 7] [--out profiles/map_visibility_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with a range of 16 and 64 cells and 1 and 32 viewpoints, on two regions about the median cell of the
last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

The viewpoints are a seeded choice among the region's cells that are at least 2 cells clear of every occupied cell
(svoslam_pool_distance_field with radius 2: none, or a squared distance of 4).  Per region and range, medians of --runs runs after
one warm-up each (a record, not a gate): the HIP-event time of the call's launches (svoslam_stage_timing: query, one bracket per
call) and the wall clock of the call + a device synchronisation, for svoslam_pool_visibility_field with mask + count (also with no viewpoints: the raster of the inflated region alone), for
svoslam_pool_distance_field (unchanged code) with the range as its radius, and for svoslam_pool_cast_rays with one ray per in-range
(cell, viewpoint) pair of the first viewpoint, from the viewpoint's centre to the cell's centre.  Before anything is written count
is asserted to be the popcount of mask, and sight is asserted symmetric on a sample of pairs: 16 viewpoints and 16 clear cells
near them, the field from the one list read at the other list's cells against the field from the other list read at the one's."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTH = ("mask", "count")


def cell_centres(torch, depth, center, edge, cells):
    """[n, 3] float32 on the device: (P(k) + P(k + 1)) / 2 in binary32 per axis for the cells[n, 3]"""
    n_side = 1 << depth
    h = float(np.float32(edge) / np.float32(n_side))
    c = torch.tensor([float(np.float32(v)) for v in center], device="cuda", dtype=torch.float32)
    lo = c + (2 * cells - n_side).to(torch.float32) * h
    hi = c + (2 * (cells + 1) - n_side).to(torch.float32) * h
    return ((lo + hi) / 2).contiguous()


def popcount(torch, mask):
    m = mask.to(torch.int64) & 0xFFFFFFFF
    return sum((m >> k) & 1 for k in range(32)).to(torch.int32)


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
        "the visibility field of a map region: tools/map_visibility_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "sight_kernel in its plain form, one cell per step; the kernels' resource report is in DESIGN.md section 19",
        "kernels: HIP events around the call's one bracket; call: wall clock of the Python call + a device synchronisation",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        cells = dims[0] * dims[1] * dims[2]
        z, y, x = torch.meshgrid(*[torch.arange(origin[a], origin[a] + dims[a], device="cuda") for a in (2, 1, 0)], indexing="ij")
        q = torch.stack([x, y, z], -1).reshape(-1, 3)
        clear = pkg.distance_field(ws, pool, depth, origin, dims, 2, as_tensor=True).reshape(-1)
        free = q[(clear < 0) | (clear >= 4)]                       # at least 2 cells clear of every occupied cell
        assert free.shape[0] >= 32, "the region has fewer than 32 clear cells"
        pick = np.random.default_rng(7).choice(int(free.shape[0]), 32, replace=False)
        views = free[torch.from_numpy(np.sort(pick)).cuda()].to(torch.int32).contiguous()
        for radius in (16, 64):
            got = pkg.visibility_field(ws, pool, depth, origin, dims, radius, views, want=BOTH, as_tensor=True)
            assert torch.equal(got["count"], popcount(torch, got["mask"])), "count is not the popcount of mask"
            # symmetry: 16 viewpoints a and, for each, a clear cell b within half the range of it (seeded); then all 16 x 16 pairs, a
            # seen from b and b seen from a, each list's field read at the other list's cells
            a, others = views[:16], []
            for i in range(16):
                near = free[((free - a[i]).abs().max(1).values <= max(radius // 2, 1)) & (free != a[i]).any(1)]
                assert near.shape[0] > 0, "no clear cell near viewpoint %d" % i
                others.append(near[int(np.random.default_rng(100 + i).integers(0, near.shape[0]))])
            b = torch.stack(others).to(torch.int32).contiguous()
            lo = torch.minimum(a.min(0).values, b.min(0).values)
            span = (torch.maximum(a.max(0).values, b.max(0).values) - lo + 1).tolist()
            from_a = pkg.visibility_field(ws, pool, depth, lo.tolist(), span, radius, a, as_tensor=True)["mask"]
            from_b = pkg.visibility_field(ws, pool, depth, lo.tolist(), span, radius, b, as_tensor=True)["mask"]
            ra, rb = (a - lo).to(torch.int64), (b - lo).to(torch.int64)
            ab = (from_a[rb[:, 2], rb[:, 1], rb[:, 0]][None, :] >> torch.arange(16, device="cuda")[:, None]) & 1   # [i, j]: b_j from a_i
            ba = (from_b[ra[:, 2], ra[:, 1], ra[:, 0]][:, None] >> torch.arange(16, device="cuda")[None, :]) & 1   # [i, j]: a_i from b_j
            assert torch.equal(ab, ba), "sight is not symmetric"
            one = pkg.visibility_field(ws, pool, depth, origin, dims, radius, views[:1], want=BOTH, as_tensor=True)
            v0 = views[0].to(torch.int64)
            in_range = ((q - v0) ** 2).sum(1) <= radius * radius
            targets = q[in_range]
            o = cell_centres(torch, depth, center, edge, v0[None, :]).expand(targets.shape[0], 3)
            rays = torch.cat([o, cell_centres(torch, depth, center, edge, targets) - o], 1).contiguous()
            keep = (targets != v0).any(1)                          # the viewpoint's own cell would be a ray without a direction
            rays, t_max = rays[keep].contiguous(), torch.ones(int(keep.sum().item()), dtype=torch.float32, device="cuda")
            fms, fwall = staged(lambda: pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True))
            rows = [("visibility_field, no viewpoints (the raster)", lambda: pkg.visibility_field(ws, pool, depth, origin, dims, radius, views[:0], want=BOTH, as_tensor=True)),
                    ("visibility_field, 1 viewpoint", lambda: pkg.visibility_field(ws, pool, depth, origin, dims, radius, views[:1], want=BOTH, as_tensor=True)),
                    ("visibility_field, 32 viewpoints", lambda: pkg.visibility_field(ws, pool, depth, origin, dims, radius, views, want=BOTH, as_tensor=True)),
                    ("cast_rays, %d rays of viewpoint 0" % int(rays.shape[0]), lambda: pkg.cast_rays(pool, depth, center, edge, rays, t_max=t_max, outputs=("t",)))]
            lines += ["", "%s: %d x %d x %d cells from cell %s, range %d cells   (viewpoint 0 at %s: %d cells in range, %d of them seen; 32 viewpoints: %d (cell, viewpoint) pairs seen, %d cells seen by none; symmetric on 16 x 16 pairs, %d of them in sight)" % (
                title, dims[0], dims[1], dims[2], origin, radius, views[0].tolist(), int(in_range.sum().item()), int(one["count"].sum().item()),
                int(got["count"].sum().item()), int((got["count"] == 0).sum().item()), int(ab.sum().item())),
                "  %-44s kernels %9.3f ms  (HIP events, one bracket)   %9.2f M cells/s   call %9.3f ms  (wall clock incl. a device synchronisation)" % (
                    "distance_field", fms, cells / fms / 1e3, fwall)]
            for label, call in rows:
                ms, wall = staged(call)
                rate = "%9.2f M rays/s " % (int(rays.shape[0]) / ms / 1e3) if label.startswith("cast_rays") else "%9.2f M cells/s" % (cells / ms / 1e3)
                lines.append("  %-44s kernels %9.3f ms                               %s   call %9.3f ms   %.2f x the distance field" % (
                    label, ms, rate, wall, ms / fms))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
