"""What safe corridors along traced paths cost on one MI355X, beside the tracing and the straightening of the same paths
(svoslam_field_trace_paths and svoslam_field_shorten_paths, unchanged code: the yardsticks), on the map and the regions
tools/map_paths_bench.py asks.

    python tools/map_corridor_bench.py [--frames 20] [--runs 7] [--out profiles/map_corridor_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with clearance 0 and 4 cells, on the two regions of tools/map_paths_bench.py about the median cell of
the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

The comfort radius is the clearance + 4 cells and the ring costs the ramp 12 9 6 3; one seed, the median in output order of the
region's traversable cells; paths are traced down the cost field from 1 start (the dearest cell) and from 4096 starts spread evenly
over the reached cells.  Per region, clearance and start count, medians of --runs runs after one warm-up each (a record, not a
gate): the HIP-event time of the call's bracket (svoslam_stage_timing: query) and the wall clock of the call + a device
synchronisation, for svoslam_field_trace_paths, for svoslam_field_shorten_paths with max_lookahead 64, for
svoslam_field_path_corridors with max_extent 4, 16 and 64 against the distance field with the comfort radius, and for
svoslam_field_grow_boxes at the same extents over the single cells at those corridors' anchors; with them the box counts and the
cells a box holds.  Before anything is written the device's corridors are asserted equal to a host restatement of the rule on a
sample of the paths, every path's gaps to be 0, and on that sample every cell of every box to be free and consecutive boxes to
share the next anchor's cell."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grow_on_the_host(mask, lo, hi, E):
    """grow(box) of include/svoslam_corridor.h over a mask of the free cells, relative cells: -x +x -y +y -z +z round by round"""
    lo, hi, grown, shape = list(lo), list(hi), [0] * 6, mask.shape[::-1]
    grew = True
    while grew:
        grew = False
        for d in range(6):
            axis, high = d >> 1, d & 1
            at = hi[axis] + 1 if high else lo[axis] - 1
            if grown[d] >= E or not 0 <= at < shape[axis]:
                continue
            cut = [slice(lo[k], hi[k] + 1) for k in range(3)]
            cut[axis] = slice(at, at + 1)
            if mask[cut[2], cut[1], cut[0]].all():
                (hi if high else lo)[axis] = at
                grown[d] += 1
                grew = True
    return lo, hi, sum(grown)


def corridors_on_the_host(mask, origin, cells, E):
    """svoslam_field_path_corridors for one path of free face neighbours -> (boxes, anchors), absolute cells"""
    o = np.asarray(origin, np.int64)
    p = np.asarray(cells, np.int64) - o
    L, boxes, anchors, a = p.shape[0], [], [], 0
    while True:
        assert mask[p[a, 2], p[a, 1], p[a, 0]]
        q = p[min(a + 1, L - 1)]
        lo, hi, _ = grow_on_the_host(mask, np.minimum(p[a], q).tolist(), np.maximum(p[a], q).tolist(), E)
        out = ~((p[a:] >= lo) & (p[a:] <= hi)).all(1)
        e = a + (int(np.argmax(out)) if out.any() else L - a) - 1
        boxes.append((np.array(lo) + o).tolist() + (np.array(hi) + o).tolist())
        anchors.append(a)
        if e == L - 1:
            return boxes, anchors
        assert e > a
        a = e


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
        "safe corridors along paths in a map region: tools/map_corridor_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "the trace: one lane per start; shorten_paths, path_corridors: one wavefront per path; grow_boxes: one wavefront per seed",
    ]
    checked = 0
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        for clearance in (0, 4):
            comfort = clearance + 4
            ring = [3 * (comfort - clearance - k) for k in range(comfort - clearance)]
            near = pkg.distance_field(ws, pool, depth, origin, dims, clearance, as_tensor=True)
            free = torch.nonzero(near.reshape(-1) == -1).reshape(-1)
            assert free.numel() > 0, "no traversable cell in the region"
            at = int(free[free.numel() // 2].item())
            seed = torch.tensor([[origin[0] + at % dims[0], origin[1] + (at // dims[0]) % dims[1], origin[2] + at // (dims[0] * dims[1])]],
                                dtype=torch.int32, device="cuda")
            cost = pkg.cost_field(ws, pool, depth, origin, dims, clearance, comfort, ring, seed, as_tensor=True)
            field = pkg.distance_field(ws, pool, depth, origin, dims, comfort, as_tensor=True)
            h_field = field.cpu().numpy()
            mask = (h_field < 0) | (h_field > clearance * clearance)
            lines += ["", "%s: %d x %d x %d cells from cell %s, clearance %d cells, comfort %d cells (the distance field's radius), ring cost %s, seed %s; %.3f of the cells are free" % (
                title, dims[0], dims[1], dims[2], origin, clearance, comfort, ring, seed[0].tolist(), float(mask.mean()))]
            reached = torch.nonzero(cost.reshape(-1) >= 0).reshape(-1)
            dearest = int(cost.reshape(-1).argmax().item())
            for count in (1, 4096):
                pick = torch.tensor([dearest], device="cuda") if count == 1 else reached[torch.linspace(0, reached.numel() - 1, count, device="cuda").long()]
                starts = torch.stack([origin[0] + pick % dims[0], origin[1] + (pick // dims[0]) % dims[1], origin[2] + pick // (dims[0] * dims[1])], 1).int()
                lengths = pkg.trace_paths(cost, origin, dims, starts, 0, as_tensor=True)[1]
                assert int(lengths.min().item()) >= 1
                room = int(lengths.max().item())
                paths, lengths = pkg.trace_paths(cost, origin, dims, starts, room, as_tensor=True)
                tms, twall = staged(lambda: pkg.trace_paths(cost, origin, dims, starts, room, as_tensor=True))
                total = int(lengths.sum().item())
                lines += ["  %d starts, longest path %d cells, %d path cells in all" % (count, room, total),
                          "    trace_paths              kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms  (wall clock incl. the output buffers' fill and a device synchronisation)" % (
                              tms, twall)]
                most = int(pkg.shorten_paths(field, origin, dims, clearance, paths, lengths, max_lookahead=64, as_tensor=True)[1].max().item())
                sms, swall = staged(lambda: pkg.shorten_paths(field, origin, dims, clearance, paths, lengths, max_lookahead=64, max_vertices=most,
                                                              as_tensor=True))
                lines += ["    shorten_paths W = 64     kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms" % (sms, swall)]
                h_paths, h_lengths = paths.cpu().numpy(), lengths.cpu().numpy()
                for extent in (4, 16, 64):
                    boxes, anchors, counts, gaps = pkg.corridors.path_corridors(field, origin, dims, clearance, extent, paths, lengths, as_tensor=True)
                    assert int(gaps.max().item()) == 0, "a traced path's chain is broken"
                    most = int(counts.max().item())
                    cms, cwall = staged(lambda: pkg.corridors.path_corridors(field, origin, dims, clearance, extent, paths, lengths, max_boxes=most,
                                                                             as_tensor=True))
                    h_boxes, h_anchors, h_counts = boxes.cpu().numpy(), anchors.cpu().numpy(), counts.cpu().numpy()
                    # a sample against the host restatement: the shortest of a few evenly spread paths
                    sample = sorted(sorted(set(np.linspace(0, count - 1, min(count, 24)).astype(int).tolist()), key=lambda k: int(h_lengths[k]))[:6])
                    for k in sample:
                        cells = h_paths[k, :h_lengths[k]]
                        want_boxes, want_anchors = corridors_on_the_host(mask, origin, cells, extent)
                        n = int(h_counts[k])
                        assert n == len(want_boxes) and h_boxes[k, :n].tolist() == want_boxes and h_anchors[k, :n].tolist() == want_anchors, (
                            title, clearance, count, extent, k)
                        for i in range(n):
                            lo, hi = h_boxes[k, i, :3] - origin, h_boxes[k, i, 3:] - origin
                            assert mask[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].all()
                            if i:
                                c = cells[h_anchors[k, i]]
                                assert (h_boxes[k, i - 1, :3] <= c).all() and (c <= h_boxes[k, i - 1, 3:]).all()
                        checked += 1
                    kept = np.nonzero(np.arange(most)[None, :] < h_counts[:, None])
                    sizes = (h_boxes[kept][:, 3:] - h_boxes[kept][:, :3] + 1).astype(np.int64).prod(1)
                    # the single cells at the anchors, one wavefront each
                    seeds = h_paths[kept[0], h_anchors[kept]]
                    t_seeds = torch.from_numpy(np.ascontiguousarray(np.concatenate([seeds, seeds], 1).astype(np.int32))).cuda()
                    layers = pkg.corridors.grow_boxes(field, origin, dims, clearance, extent, t_seeds, as_tensor=True)[1]
                    assert int(layers.min().item()) >= 0
                    gms, gwall = staged(lambda: pkg.corridors.grow_boxes(field, origin, dims, clearance, extent, t_seeds, as_tensor=True))
                    lines += ["    path_corridors E = %-3d   kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms   %d boxes in all, at most %d on a path; a box holds %.0f cells in the mean, %d at most" % (
                        extent, cms, cwall, int(h_counts.sum()), most, float(sizes.mean()), int(sizes.max())),
                        "    grow_boxes     E = %-3d   kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms   %d single-cell seeds, the cells at those anchors; %.1f layers a seed in the mean" % (
                            extent, gms, gwall, int(t_seeds.shape[0]), float(layers.float().mean().item()))]
            print("... %s, clearance %d done" % (title, clearance), file=sys.stderr, flush=True)
    lines += ["", "%d paths' corridors were equal to the host restatement before this was written" % checked]
    assert checked > 20
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
