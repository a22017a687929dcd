"""What svoslam_pool_compact costs and what it does to the ray march, on one MI355X, on a map of BASELINE config 3's class
(depth 12, 640x480 frames of the synthetic stream through the frame loop), after one populated root octant was paged out.

    python tools/pool_compact_bench.py [--frames 100] [--runs 7] [--out profiles/pool_compact_bench.json]

Prints ONE JSON object.  All times are taken in this process, as medians of --runs (>= 5) runs after a warm-up:

  compact_keep_ms / compact_shrink_ms   wall clock of the blocking call (allocation of the new pool and release of the old one
                                        included), capacity kept / shrunk to fit (the latter adds the trimming device copy)
  copy_ms                               svoslam_pool_copy of the same pool into an allocation that is already large enough: the
                                        same nodes moved once by a plain device copy -- the yardstick
  march_ms_before / march_ms_after      kernel time of one fixed 640x480 reference-mode view (brick march), from
                                        svoslam_cone_trace_timing, on the paged-out map before and after compaction

Algorithmic bytes of a compaction of N surviving nodes in T = N / 8 tiles ("Pool compaction"):
  16 N   every surviving node read once by the emit pass and written once
   8 N   the count pass's re-read of the same tiles
  28 T   4-byte entries per tile: the frontier written once and read twice (count, emit), the counts written, scanned in
         place (read + write) and read by the emit pass
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.frames >= 1 and args.runs >= 5
    import importlib
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    assert torch.cuda.is_available(), "needs a gfx950 device"
    w, h, depth, center, edge = 640, 480, 12, (0.0, 1.5, 0.0), 4.096
    P = pl.SlamPipeline(w, h, depth, center, edge)
    chunk = 25
    for first in range(0, args.frames, chunk):
        ks = list(range(first, min(first + chunk, args.frames)))
        frames = [synth.render_frame(k, w, h, device="cuda") for k in ks]
        P.run_stream([f[0] for f in frames], [f[1] for f in frames], ks, [pl.ground_truth_view(k, synth) for k in ks])
        torch.cuda.synchronize()
    M = P.pool
    nodes_map = M.size
    root = M.words()[:16:2]
    octant = next(k for k in range(8) if root[k] & pkg.FLAG_CHILDREN)
    with tempfile.TemporaryDirectory() as tmp:
        M.evict_subtree([octant], os.path.join(tmp, "octant.svosub"))
    view = pl.ground_truth_view(args.frames - 1, synth)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    W = pkg.Pool()

    def march_ms(pool):
        pkg.cone_trace_timing(True)
        try:
            out = []
            for k in range(2 + args.runs):
                pkg.cone_trace_svo(img, 45.0, view, pool.data_ptr, center, edge, pkg.RENDER_REFERENCE)
                ms, launches = pkg.cone_trace_timing_read()
                if k >= 2:
                    out.append(ms)
            return statistics.median(out), pool.march_accel()
        finally:
            pkg.cone_trace_timing(False)

    W.copy_from(M)
    march_before, accel_before = march_ms(W)
    reference_image = img.clone()
    copy, keep, shrink = [], [], []
    stats = None
    for k in range(1 + args.runs):
        c = timed(lambda: W.copy_from(M))
        a = timed(lambda: W.compact(0))
        W.copy_from(M)
        holder = {}
        b = timed(lambda: holder.update(W.compact(1)))
        stats = holder
        if k >= 1:
            copy.append(c); keep.append(a); shrink.append(b)
        if k < args.runs:
            W.reserve(M.capacity)      # the copy that follows is timed into an allocation that is large enough already
    march_after, accel_after = march_ms(W)
    same_image = bool(torch.equal(img, reference_image))
    n_after, t_after = stats["size_after"], stats["size_after"] // 8
    alg_bytes = 16 * n_after + 8 * n_after + 28 * t_after
    copy_ms, keep_ms, shrink_ms = statistics.median(copy), statistics.median(keep), statistics.median(shrink)
    rec = {
        "what": "svoslam_pool_compact after paging one root octant out of a cfg3-class map (tools/pool_compact_bench.py)",
        "device": pkg.device_arch(), "date": datetime.date.today().isoformat(),
        "frames": args.frames, "width": w, "height": h, "depth": depth, "runs": args.runs,
        "nodes_map": nodes_map, "evicted_root_octant": octant,
        "nodes_before": stats["size_before"], "nodes_after": n_after, "tiles_dropped": stats["tiles_dropped"], "levels": stats["levels"],
        "capacity_before": stats["capacity_before"], "capacity_after_shrink": stats["capacity_after"],
        "compact_keep_ms": round(keep_ms, 4), "compact_shrink_ms": round(shrink_ms, 4), "copy_ms": round(copy_ms, 4),
        "ratio_keep_to_copy": round(keep_ms / copy_ms, 3), "ratio_shrink_to_copy": round(shrink_ms / copy_ms, 3),
        "copy_bytes": 16 * stats["size_before"], "copy_GBs": round(16 * stats["size_before"] / copy_ms / 1e6, 2),
        "algorithmic_bytes": alg_bytes, "compact_keep_GBs": round(alg_bytes / keep_ms / 1e6, 2),
        "march_ms_before": round(march_before, 4), "march_ms_after": round(march_after, 4),
        "march_accel_before": accel_before, "march_accel_after": accel_after, "image_unchanged": same_image,
        "samples_ms": {"copy": [round(v, 4) for v in copy], "compact_keep": [round(v, 4) for v in keep],
                       "compact_shrink": [round(v, 4) for v in shrink]},
    }
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
