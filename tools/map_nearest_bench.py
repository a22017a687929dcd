"""What the nearest-cell field of a map region costs on one MI355X beside the distance field of the same region, on the map and the
regions of tools/map_field_bench.py.

    python tools/map_nearest_bench.py [--frames 20] [--runs 7] [--out profiles/map_nearest_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with radius 16 and 64 cells, on two regions about the median cell of the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

Per region and radius, medians of --runs runs after one warm-up each (a record, not a gate): the HIP-event time of the call's
launches (svoslam_stage_timing: query, one bracket per call) and the wall clock of the call + a device synchronisation, for
svoslam_pool_nearest_field to the occupied cells with dist2 + cell, with all four outputs, and to the free cells with dist2 +
cell, and for svoslam_pool_distance_field (unchanged code) beside them, with the ratio to it.  Before anything is written the
dist2 of the nearest-cell field is asserted equal to the distance field, every witness is asserted to lie at exactly that
distance, and node / colour are asserted to be svoslam_pool_query_points' at the witness."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ("dist2", "cell", "node", "color")


def cell_centres(torch, depth, center, edge, cells):
    """[n, 3] float32 on the device: (P(k) + P(k + 1)) / 2 in binary32 per axis for the cells[n, 3]"""
    n_side = 1 << depth
    h = float(np.float32(edge) / np.float32(n_side))
    c = torch.tensor([float(np.float32(v)) for v in center], device="cuda", dtype=torch.float32)
    lo = c + (2 * cells - n_side).to(torch.float32) * h
    hi = c + (2 * (cells + 1) - n_side).to(torch.float32) * h
    return ((lo + hi) / 2).contiguous()


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
        "the nearest-cell field of a map region: tools/map_nearest_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "region_raster_kernel 18 VGPRs, edt_x_kernel<true> 17, edt_pass_kernel<kLds, true> 18 (LDS) / 14 (global), nearest_resolve_kernel 15 (node / colour) / 11, 0 bytes of scratch; LDS (64 + 2 R) * 256 bytes per one-wavefront workgroup (compiler's resource report)",
        "kernels: HIP events around the call's one bracket; call: wall clock of the Python call + a device synchronisation, which for nearest_field includes the binding's unpacking of cell into cell_xyz (torch kernels outside the bracket)",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        cells = dims[0] * dims[1] * dims[2]
        z, y, x = torch.meshgrid(*[torch.arange(origin[a], origin[a] + dims[a], device="cuda") for a in (2, 1, 0)], indexing="ij")
        q = torch.stack([x, y, z], -1)
        for radius in (16, 64):
            field = pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True)
            got = pkg.nearest_field(ws, pool, depth, origin, dims, radius, want=ALL, as_tensor=True)
            free = pkg.nearest_field(ws, pool, depth, origin, dims, radius, which=pkg.NEAREST_FREE, as_tensor=True)
            assert torch.equal(got["dist2"], field), "dist2 differs from svoslam_pool_distance_field"
            for f in (got, free):
                ok = f["dist2"] >= 0
                assert torch.equal(((f["cell_xyz"].to(torch.int64) - q) ** 2).sum(-1)[ok], f["dist2"][ok].to(torch.int64)), "a witness is not at its distance"
                assert bool((f["cell_xyz"][~ok] == -1).all())
            ok = got["dist2"] >= 0
            there = pkg.query_points(pool, depth, center, edge, cell_centres(torch, depth, center, edge, got["cell_xyz"][ok].to(torch.int64)),
                                     outputs=("node", "level", "color"))
            assert bool((there["level"] == depth).all()) and torch.equal(there["node"], got["node"][ok]) and torch.equal(there["color"], got["color"][ok]), \
                "node / colour differ from svoslam_pool_query_points at the witness"
            assert bool(((free["dist2"] == 0) == (field != 0)).all()), "the free cells are not the distance field's non-zero cells"
            fms, fwall = staged(lambda: pkg.distance_field(ws, pool, depth, origin, dims, radius, as_tensor=True))
            rows = [("nearest_field, dist2 + cell", lambda: pkg.nearest_field(ws, pool, depth, origin, dims, radius, as_tensor=True)),
                    ("nearest_field, all four", lambda: pkg.nearest_field(ws, pool, depth, origin, dims, radius, want=ALL, as_tensor=True)),
                    ("nearest_field, FREE, dist2 + cell", lambda: pkg.nearest_field(ws, pool, depth, origin, dims, radius, which=pkg.NEAREST_FREE, as_tensor=True))]
            lines += ["", "%s: %d x %d x %d cells from cell %s, radius %d cells   (%d cells on occupied ones, %d with nothing within the radius; inside: %d cells with no free cell within the radius)" % (
                title, dims[0], dims[1], dims[2], origin, radius, int((field == 0).sum().item()), int((field < 0).sum().item()),
                int((free["dist2"] < 0).sum().item())),
                "  %-34s kernels %9.3f ms  (HIP events, one bracket)   %9.2f M cells/s   call %9.3f ms  (wall clock incl. a device synchronisation)" % (
                    "distance_field", fms, cells / fms / 1e3, fwall)]
            for label, call in rows:
                ms, wall = staged(call)
                lines.append("  %-34s kernels %9.3f ms                               %9.2f M cells/s   call %9.3f ms   %.2f x the distance field" % (
                    label, ms, cells / ms / 1e3, wall, ms / fms))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
