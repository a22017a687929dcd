"""What the component labels of a map region cost on one MI355X, beside the distance field with the same radius on the same region
(that call is part of this one, so it is the floor) and beside the reach field from one seed (the blocking way to get ONE
component without this call), on the map tools/map_field_bench.py asks.

    python tools/map_components_bench.py [--frames 20] [--runs 7] [--out profiles/map_components_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with clearance 0 and 4 cells, for the free and the solid set, on the two regions of
tools/map_field_bench.py and tools/map_reach_bench.py about the median cell of the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

Per region, clearance and set, medians of --runs runs after one warm-up each (a record, not a gate): the HIP-event time of the
call's bracket (svoslam_stage_timing: query) and the wall clock of the call + a device synchronisation, for labels alone without
stats (asynchronous), and for labels + sizes + stats (one readback); the components, the largest, the tile passes and the unions;
the same two times for svoslam_pool_distance_field and for svoslam_pool_reach_field seeded at the median traversable cell (both
unchanged code).  Before anything is written the labels are asserted canonical, the set to be the distance field's, and the reach
field's support to be the seed's component."""
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
        "the component labels of a map region: tools/map_components_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "tiles of 64 x 8 x 8 cells, one workgroup of 256 per tile; no readback without stats, one of 32 bytes with them",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        cells = dims[0] * dims[1] * dims[2]
        index = torch.arange(cells, dtype=torch.int32, device="cuda")
        for clearance in (0, 4):
            field = pkg.distance_field(ws, pool, depth, origin, dims, clearance, as_tensor=True)
            free = torch.nonzero(field.reshape(-1) == -1).reshape(-1)
            assert free.numel() > 0, "no traversable cell in the region"
            at = int(free[free.numel() // 2].item())
            seed = torch.tensor([[origin[0] + at % dims[0], origin[1] + (at // dims[0]) % dims[1], origin[2] + at // (dims[0] * dims[1])]],
                                dtype=torch.int32, device="cuda")
            steps = pkg.reach_field(ws, pool, depth, origin, dims, clearance, seed, as_tensor=True)
            fms, fwall = staged(lambda: pkg.distance_field(ws, pool, depth, origin, dims, clearance, as_tensor=True))
            rms, rwall = staged(lambda: pkg.reach_field(ws, pool, depth, origin, dims, clearance, seed, as_tensor=True))
            lines += ["", "%s: %d x %d x %d cells from cell %s, clearance %d cells" % (title, dims[0], dims[1], dims[2], origin, clearance)]
            for solid in (False, True):
                stats = {}
                labels, sizes = pkg.label_components(ws, pool, depth, origin, dims, clearance, solid=solid, sizes=True, as_tensor=True, stats=stats)
                flat = labels.reshape(-1)
                in_set = flat >= 0
                assert torch.equal(in_set, (field.reshape(-1) == -1) != solid), "the set is not the distance field's"
                assert bool((flat[in_set] <= index[in_set]).all()) and torch.equal(flat[flat[in_set].long()], flat[in_set]), "labels are not canonical"
                assert int((flat == index).sum().item()) == stats["components"] and int(sizes.max().item()) == stats["largest"]
                if not solid:
                    assert torch.equal(steps.reshape(-1) >= 0, flat == flat[at]), "the reach field's support is not the seed's component"
                ms, wall = staged(lambda: pkg.label_components(ws, pool, depth, origin, dims, clearance, solid=solid, as_tensor=True))
                sms, swall = staged(lambda: pkg.label_components(ws, pool, depth, origin, dims, clearance, solid=solid, sizes=True, as_tensor=True, stats={}))
                lines += [
                    "  %-5s label_components                  bracket %9.3f ms  (HIP events, one bracket, asynchronous)   %9.2f M cells/s   call %9.3f ms  (wall clock incl. a device synchronisation)   / distance_field %.2f" % (
                        "solid" if solid else "free", ms, cells / ms / 1e3, wall, ms / fms),
                    "        label_components + sizes + stats  bracket %9.3f ms  (one readback, inside the bracket)        %9.2f M cells/s   call %9.3f ms   %d cells in %d components, the largest %d; %d tile passes over %d tiles, %d unions" % (
                        sms, cells / sms / 1e3, swall, int(in_set.sum().item()), stats["components"], stats["largest"], stats["tile_passes"],
                        -(-dims[0] // 64) * -(-dims[1] // 8) * -(-dims[2] // 8), stats["unions"])]
            lines += [
                "  distance_field                           kernels %9.3f ms  (HIP events, one bracket)                  %9.2f M cells/s   call %9.3f ms   the same region and radius: part of every call above" % (
                    fms, cells / fms / 1e3, fwall),
                "  reach_field, one seed %-18s bracket %9.3f ms  (readbacks included; it blocks)             %9.2f M cells/s   call %9.3f ms   ONE free component: %d cells reached" % (
                    seed[0].tolist(), rms, cells / rms / 1e3, rwall, int((steps >= 0).sum().item()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
