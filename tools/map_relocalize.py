"""Where in a saved map (svoslam_pool_save checkpoint) was this depth frame taken?  A coarse-to-fine pose search on one MI355X.

    python tools/map_relocalize.py CHECKPOINT OUT.npz (--depth DEPTH.png --fx FX --fy FY | --points PTS.npy)
        (--prior 16 floats | --prior-file POSE.txt) --extent MX MY MZ --yaw DEG --radius CELLS
        [--depth-level D] [--subsample K] [--steps 9 9 9] [--yaw-steps 9] [--rounds 3] [--min-near 0.5]

The observation is a 16-bit depth image in millimetres (PNG / PGM: svoslam_image_load), halved --subsample times as the tracker's
pyramid halves it (svoslam_subsample_depth_u16) and turned into a vertex map (svoslam_generate_vertex_map), or an [n, 3] float32
array of points in the sensor frame (a non-finite point = no measurement).  The prior is a sensor-to-world matrix, 16 floats
column-major as every trans[16] of include/svoslam.h (a file holds them separated by white space).  The search covers +-extent
metres per world axis and +-yaw degrees about the sensor's y axis: relocalize() builds the distance field of the box the search can
reach once (svoslam_pool_distance_field, --radius cells, at --depth-level, default the map's stored depth), scores a grid of poses
against it (svoslam_score_poses), re-centres on the best and halves the extents, --rounds times.  A pose qualifies if at least
--min-near of the measured points land within the radius of an occupied cell.  OUT.npz holds

  found            1 if a pose qualified in every round, else 0 (then only the inputs are stored)
  pose             float32 [16], the pose found
  cost, near       its cost (the sum of squared cell distances + (radius^2 + 1) per point without one) and its inlier count
  rounds           int64 [rounds, 2]: the (cost, grid index) of every round's best
  points           the number of measured points, and prior, extent, yaw_deg, radius_cells, depth, center, edge_length, cell_size"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--depth", default=None, help="16-bit depth image in millimetres")
    ap.add_argument("--points", default=None, help=".npy, [n, 3] float32 in the sensor frame")
    ap.add_argument("--fx", type=float, default=None)
    ap.add_argument("--fy", type=float, default=None)
    ap.add_argument("--prior", type=float, nargs=16, default=None)
    ap.add_argument("--prior-file", default=None)
    ap.add_argument("--extent", type=float, nargs=3, required=True, metavar=("MX", "MY", "MZ"), help="metres either side of the prior")
    ap.add_argument("--yaw", type=float, required=True, help="degrees either side of the prior")
    ap.add_argument("--radius", type=int, required=True, help="cells (0 .. 4096)")
    ap.add_argument("--depth-level", type=int, default=None, help="lattice depth (default: the stored depth)")
    ap.add_argument("--subsample", type=int, default=0, help="halvings of the depth image")
    ap.add_argument("--steps", type=int, nargs=3, default=(9, 9, 9))
    ap.add_argument("--yaw-steps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-near", type=float, default=0.5, help="fraction of the measured points")
    args = ap.parse_args()
    if (args.depth is None) == (args.points is None):
        sys.exit("give either --depth (with --fx and --fy) or --points")
    if (args.prior is None) == (args.prior_file is None):
        sys.exit("give either --prior or --prior-file")
    prior = np.asarray(args.prior if args.prior is not None else np.loadtxt(args.prior_file).reshape(-1), np.float32)
    if prior.shape != (16,):
        sys.exit("the prior is 16 floats")
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    if args.points is not None:
        points = torch.from_numpy(np.ascontiguousarray(np.load(args.points), np.float32).reshape(-1, 3)).cuda()
    else:
        if args.fx is None or args.fy is None:
            sys.exit("a depth image needs --fx and --fy")
        image = pkg.image_load(args.depth)
        if image.ndim != 2 or image.dtype != np.uint16:
            sys.exit("the depth image is one channel of 16 bits")
        h, w = image.shape
        depth = torch.from_numpy(image.view(np.int16).copy()).cuda()
        tmp = torch.empty_like(depth)
        lw, lh = w, h
        for _ in range(args.subsample):
            pkg.subsample_depth(depth, tmp, lw, lh)
            lw, lh = lw // 2, lh // 2
        level = depth.reshape(-1)[: lw * lh].reshape(lh, lw)
        vmap = torch.empty((lh, lw, 3), dtype=torch.float32, device="cuda")
        pkg.generate_vertex_map(level, vmap, args.fx, args.fy, w, h)
        points = vmap.reshape(-1, 3)
    pool, ws = pkg.Pool(), pkg.Workspace()
    center, edge, stored = pool.load(args.checkpoint)
    depth_level = stored if args.depth_level is None else args.depth_level
    measured = int(torch.isfinite(points).all(1).sum().item())
    found = pkg.relocalize(ws, pool, depth_level, center, edge, points, prior, args.extent, np.deg2rad(args.yaw), args.radius,
                           steps=tuple(args.steps), yaw_steps=args.yaw_steps, rounds=args.rounds, min_near_fraction=args.min_near)
    common = dict(points=measured, prior=prior, extent=np.asarray(args.extent, np.float32), yaw_deg=np.float32(args.yaw),
                  radius_cells=args.radius, depth=depth_level, center=np.asarray(center, np.float32), edge_length=np.float32(edge),
                  cell_size=2.0 * float(edge) / (1 << depth_level))
    if found is None:
        np.savez_compressed(args.out, found=0, **common)
        print("nothing qualified: no pose of the search has %.0f %% of the %d measured points within %d cells of the map -> %s" % (
            100.0 * args.min_near, measured, args.radius, args.out))
        return
    np.savez_compressed(args.out, found=1, pose=found["pose"], cost=np.int64(found["cost"]), near=np.int32(found["near"]),
                        rounds=np.asarray(found["rounds"], np.int64).reshape(-1, 2), **common)
    print("depth %d, radius %d cells: cost %d, %d of %d measured points within the radius, after %d rounds (best per round: %s) -> %s" % (
        depth_level, args.radius, found["cost"], found["near"], measured, len(found["rounds"]),
        ", ".join("%d at %d" % r for r in found["rounds"]), args.out))
    print("pose: " + " ".join(repr(float(v)) for v in found["pose"]))


if __name__ == "__main__":
    main()
