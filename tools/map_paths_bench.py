"""What straightening traced paths and checking segments against a distance field cost on one MI355X, beside the tracing of the same
paths (svoslam_field_trace_paths, unchanged code: the yardstick), on the map and the regions tools/map_plan_bench.py asks.

    python tools/map_paths_bench.py [--frames 20] [--runs 7] [--out profiles/map_paths_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with clearance 0 and 4 cells, on the two regions of tools/map_plan_bench.py about the median cell of
the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

The comfort radius is the clearance + 4 cells and the ring costs the ramp 12 9 6 3; one seed, the median in output order of the
region's traversable cells; paths are traced down the cost field from 1 start (the dearest cell) and from 4096 starts spread evenly
over the reached cells.  Per region, clearance and start count, medians of --runs runs after one warm-up each (a record, not a
gate): the HIP-event time of the call's bracket (svoslam_stage_timing: query) and the wall clock of the call + a device
synchronisation, for svoslam_field_trace_paths, for svoslam_field_shorten_paths against the distance field with the comfort radius
with max_lookahead 0 (unlimited) and 64, and for svoslam_field_segment_clearance over the segments between the vertices; with
them the vertex counts and the Manhattan and Euclidean lengths in cells.  Before anything is written the device's vertices are
asserted equal to a host restatement of the rule, cell by cell, on a sample of the paths, and every segment between two vertices
more than one cell apart to keep the clearance by svoslam_field_segment_clearance."""
import argparse
import datetime
import importlib
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INF = 1 << 40


def walk_order(D):
    """the cells of the supercover of the segment from cell 0 to cell D, without the two, in walk order (include/svoslam.h)"""
    n = [abs(d) for d in D]
    s = [(d > 0) - (d < 0) for d in D]
    i, c, left = [0, 0, 0], [0, 0, 0], sum(n)
    while left:
        live = [a for a in range(3) if i[a] < n[a]]
        first = [a for a in live if all((2 * i[a] + 1) * n[b] <= (2 * i[b] + 1) * n[a] for b in live)]
        if len(first) > 1:
            for k in range(1, len(first)):
                for sub in itertools.combinations(first, k):
                    yield tuple(c[a] + (s[a] if a in sub else 0) for a in range(3))
        for a in first:
            c[a] += s[a]
            i[a] += 1
        left -= len(first)
        if left:
            yield tuple(c)


def shorten_on_the_host(field, origin, r, cells, lookahead):
    """svoslam_field_shorten_paths for one path, every j of the window tried"""
    nz, ny, nx = field.shape

    def g(c):
        x, y, z = c[0] - origin[0], c[1] - origin[1], c[2] - origin[2]
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
            return 0
        v = int(field[z, y, x])
        return INF if v < 0 else v
    own = [g(c) for c in cells]
    out, a, L = [0], 0, len(cells)
    while a < L - 1:
        hi = L - 1 if lookahead == 0 else min(L - 1, a + lookahead)
        best, m = a + 1, own[a]
        for j in range(a + 1, hi + 1):
            m = min(m, own[j])
            floor = max(r * r + 1, m)
            if j > a + 1 and own[a] >= floor and own[j] >= floor and all(
                    g(tuple(cells[a][k] + c[k] for k in range(3))) >= floor for c in walk_order(tuple(cells[j][k] - cells[a][k] for k in range(3)))):
                best = j
        a = best
        out.append(a)
    return out


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
        "straightening paths in a map region: tools/map_paths_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; nothing was tuned against this record)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "the trace: one lane per start; shorten_paths: one wavefront per path, 64 candidates per batch; segment_clearance: one lane per segment",
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
            lines += ["", "%s: %d x %d x %d cells from cell %s, clearance %d cells, comfort %d cells (the distance field's radius), ring cost %s, seed %s" % (
                title, dims[0], dims[1], dims[2], origin, clearance, comfort, ring, seed[0].tolist())]
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
                moves = int((lengths - 1).sum().item())
                lines += ["  %d starts, longest path %d cells, %d moves in all (the Manhattan length in cells)" % (count, room, moves),
                          "    trace_paths           kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms  (wall clock incl. the output buffers' fill and a device synchronisation)" % (
                              tms, twall)]
                h_paths, h_lengths = paths.cpu().numpy(), lengths.cpu().numpy()
                for lookahead in (0, 64):
                    vertices, counts = pkg.shorten_paths(field, origin, dims, clearance, paths, lengths, max_lookahead=lookahead, as_tensor=True)
                    most = int(counts.max().item())
                    sms, swall = staged(lambda: pkg.shorten_paths(field, origin, dims, clearance, paths, lengths, max_lookahead=lookahead,
                                                                  max_vertices=most, as_tensor=True))
                    h_vertices, h_counts = vertices.cpu().numpy(), counts.cpu().numpy()
                    # a sample against the host restatement: the shortest paths of a few evenly spread ones (the host walks cell by cell)
                    sample = sorted(sorted(set(np.linspace(0, count - 1, min(count, 24)).astype(int).tolist()), key=lambda k: int(h_lengths[k]))[:6])
                    for k in sample:
                        if lookahead == 0 and h_lengths[k] > 260:
                            continue
                        want = shorten_on_the_host(h_field, origin, clearance, [tuple(c) for c in h_paths[k, :h_lengths[k]].tolist()], lookahead)
                        assert h_counts[k] == len(want) and h_vertices[k, :len(want)].tolist() == want, (title, clearance, count, lookahead, k)
                        checked += 1
                    # the segments between the vertices, and their Euclidean length
                    rows = np.nonzero(np.arange(most - 1)[None, :] < (h_counts - 1)[:, None])
                    a = h_paths[rows[0], h_vertices[rows[0], rows[1]]]
                    b = h_paths[rows[0], h_vertices[rows[0], rows[1] + 1]]
                    straight = float(np.sqrt(((b - a).astype(np.float64) ** 2).sum(1)).sum())
                    segments = torch.from_numpy(np.concatenate([a, b], 1).astype(np.int32)).cuda()
                    cms, cwall = 0.0, 0.0
                    if segments.shape[0]:
                        low = pkg.segment_clearance(field, origin, dims, segments, as_tensor=True).cpu().numpy()
                        long_ones = np.abs(b - a).sum(1) > 1
                        assert ((low[long_ones] < 0) | (low[long_ones] > clearance * clearance)).all(), "a segment between two vertices comes within the clearance"
                        cms, cwall = staged(lambda: pkg.segment_clearance(field, origin, dims, segments, want_cell=True, as_tensor=True))
                    lines += ["    shorten_paths W = %-3d  kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms   %d vertices in all, at most %d on a path; Euclidean length %.1f cells, %.3f of the moves" % (
                        lookahead, sms, swall, int(h_counts.sum()), most, straight, straight / max(moves, 1)),
                        "    segment_clearance     kernel %9.3f ms  (HIP events, one bracket)   call %9.3f ms   %d segments between those vertices, minimum and first cell" % (
                            cms, cwall, int(segments.shape[0]))]
            print("... %s, clearance %d done" % (title, clearance), file=sys.stderr, flush=True)
    lines += ["", "%d paths' vertices were equal to the host restatement before this was written" % checked]
    assert checked > 20
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
