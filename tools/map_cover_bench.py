"""What choosing viewpoints that cover a map region costs on one MI355X, beside the route the library offered before
svoslam_pool_cover_views: the visibility field once per 32 candidates, a dense mask read back per call, and the set cover in numpy.
On the map and the regions of tools/map_field_bench.py.

    python tools/map_cover_bench.py [--frames 20] [--runs 7] [--out profiles/map_cover_bench.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then, at depth 12 with surface targets, a range of 16 and 64 cells, 64 / 1024 / 4096 candidates and k_max = 16, on two
regions about the median cell of the last frame's fused points:

  block        256 x 256 x 64 cells
  mid-plane    512 x 1 x 512 cells: one x-z plane

The candidates are a seeded choice among the region's cells that are at least 2 cells clear of every occupied cell
(svoslam_pool_distance_field with radius 2: none, or a squared distance of 4).  Per region, range and candidate count, medians of
--runs runs after one warm-up each (a record, not a gate): the HIP-event time of the call's one bracket (svoslam_stage_timing:
query; it holds the call's one readback of T) and the wall clock of the call + a device synchronisation.  The stages are differences
of such medians: the raster is svoslam_pool_visibility_field without viewpoints at the same inflation; targets = cover_views without
candidates - raster; matrix = cover_views with k_max = 0 and no d_seen (the matrix and the OR over its rows) - cover_views without
candidates; rounds = the whole call - that (the scores and 16 rounds of two launches).  The other route is timed once per case, by
the wall clock: svoslam_pool_visibility_field with mask per 32 candidates, each mask read back, the surface cells gathered on the
host from svoslam_pool_distance_field's zeros on the region inflated by 1, the greedy cover in numpy over packed bits.  Before
anything is written the two routes are asserted equal: seen, chosen, gain, round and summary."""
import argparse
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_MAX = 16
POPCOUNT8 = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def other_route(pkg, ws, pool, depth, origin, dims, radius, cands, k_max):
    """the same outputs without svoslam_pool_cover_views -> a dict of numpy arrays"""
    n_side = 1 << depth
    o, n = np.asarray(origin), np.asarray(dims)
    lo, hi = np.maximum(o - 1, 0), np.minimum(o + n + 1, n_side)
    occ = pkg.distance_field(ws, pool, depth, lo, hi - lo, 0) == 0      # [z, y, x] of the region inflated by 1
    solid = np.ones(tuple(n[::-1] + 2), bool)                           # what lies outside the root is no free neighbour
    at = tuple(slice(lo[a] - (o[a] - 1), lo[a] - (o[a] - 1) + hi[a] - lo[a]) for a in (2, 1, 0))
    solid[at] = occ
    inner = solid[1:-1, 1:-1, 1:-1]
    open_side = np.zeros_like(inner)
    for axis in range(3):
        for step in (0, 2):
            cut = [slice(1, -1)] * 3
            cut[axis] = slice(step, step + inner.shape[axis])
            open_side |= ~solid[tuple(cut)]
    flags = (inner & open_side).reshape(-1)
    targets = np.nonzero(flags)[0]
    T = targets.size
    rows = np.zeros((cands.shape[0], (T + 7) // 8), np.uint8)
    for s in range(0, cands.shape[0], 32):
        mask = pkg.visibility_field(ws, pool, depth, origin, dims, radius, cands[s:s + 32])["mask"].reshape(-1)[targets]
        for c in range(min(32, cands.shape[0] - s)):
            rows[s + c] = np.packbits(((mask >> np.uint32(c)) & 1).astype(np.uint8))
    seen = POPCOUNT8[rows].sum(1, dtype=np.int64).astype(np.int32)
    covered = np.zeros(rows.shape[1], np.uint8)
    chosen, gain = np.full(k_max, -1, np.int32), np.zeros(k_max, np.int32)
    first = np.full(T, -2, np.int32)
    for j in range(k_max):
        gains = POPCOUNT8[rows & ~covered].sum(1, dtype=np.int64)
        if gains.size == 0 or gains.max() < 1:
            break
        c = int(np.argmax(gains))
        chosen[j], gain[j] = c, gains[c]
        first[np.unpackbits(rows[c] & ~covered)[:T] == 1] = j
        covered |= rows[c]
    rounds = np.full(flags.size, -1, np.int32)
    rounds[targets] = first
    any_row = np.bitwise_or.reduce(rows, 0) if rows.shape[0] else covered
    summary = np.array([T, (chosen >= 0).sum(), POPCOUNT8[covered].sum(dtype=np.int64), POPCOUNT8[any_row].sum(dtype=np.int64)], np.int32)
    return {"seen": seen, "chosen": chosen, "gain": gain, "round": rounds.reshape(dims[2], dims[1], dims[0]), "summary": summary}


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
        "viewpoints that cover a map region: tools/map_cover_bench.py --frames %d --runs %d   (%s, %s; medians of %d runs after a warm-up; measured once, a record and not a gate)" % (
            args.frames, args.runs, pkg.device_arch(), datetime.date.today().isoformat(), args.runs),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes; regions about cell %s, the median of the last frame's fused points" % (
            args.frames, w, h, depth, nodes, about.tolist()),
        "surface targets, k_max = %d, min_gain = 1; two launches a round (the plain form); the kernels' resource report is in DESIGN.md section 24" % K_MAX,
        "cover_views: HIP events around the call's one bracket, which holds the readback of T; stages: differences of such medians (see the tool's header)",
        "other route: svoslam_pool_visibility_field with mask per 32 candidates + readbacks + the cover in numpy, wall clock of one run; both routes asserted equal before this was written",
    ]
    for title, dims in (("block", (256, 256, 64)), ("mid-plane", (512, 1, 512))):
        origin = [int(np.clip(about[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
        z, y, x = torch.meshgrid(*[torch.arange(origin[a], origin[a] + dims[a], device="cuda") for a in (2, 1, 0)], indexing="ij")
        q = torch.stack([x, y, z], -1).reshape(-1, 3)
        clear = pkg.distance_field(ws, pool, depth, origin, dims, 2, as_tensor=True).reshape(-1)
        free = q[(clear < 0) | (clear >= 4)]                       # at least 2 cells clear of every occupied cell
        for radius in (16, 64):
            raster, _ = staged(lambda: pkg.visibility_field(ws, pool, depth, origin, dims, max(radius, 1), np.zeros((0, 3), np.int32), want=("count",), as_tensor=True))
            bare, _ = staged(lambda: pkg.cover_views(ws, pool, depth, origin, dims, radius, np.zeros((0, 3), np.int32), 0, want=("summary",), as_tensor=True))
            lines += ["", "%s: %d x %d x %d cells from cell %s, range %d cells, %d clear cells to draw from" % (
                title, dims[0], dims[1], dims[2], origin, radius, int(free.shape[0]))]
            for n_cands in (64, 1024, 4096):
                count = min(n_cands, int(free.shape[0]))
                pick = np.random.default_rng(7).choice(int(free.shape[0]), count, replace=False)
                cands = free[torch.from_numpy(np.sort(pick)).cuda()].to(torch.int32).contiguous()
                got = pkg.cover_views(ws, pool, depth, origin, dims, radius, cands, K_MAX)
                t0 = time.perf_counter()
                other = other_route(pkg, ws, pool, depth, origin, dims, radius, cands.cpu().numpy(), K_MAX)
                other_ms = (time.perf_counter() - t0) * 1e3
                for name in got:
                    assert np.array_equal(got[name], other[name]), "the two routes differ in %s" % name
                T, n_chosen, covered, coverable = got["summary"].tolist()
                matrix_only, _ = staged(lambda: pkg.cover_views(ws, pool, depth, origin, dims, radius, cands, 0, want=("summary",), as_tensor=True))
                whole, wall = staged(lambda: pkg.cover_views(ws, pool, depth, origin, dims, radius, cands, K_MAX, as_tensor=True))
                lines.append("  %4d candidates: T %d, matrix %d bytes, %d chosen cover %d of %d coverable   cover_views %9.3f ms (raster %.3f, targets %.3f, matrix %.3f, rounds %.3f)   call %9.3f ms   other route %10.1f ms, %.0f x" % (
                    count, T, count * ((T + 63) // 64) * 8, n_chosen, covered, coverable, whole, raster, bare - raster, matrix_only - bare,
                    whole - matrix_only, wall, other_ms, other_ms / wall))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
