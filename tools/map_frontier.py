"""What have these sensor frames seen of a box of a saved map (svoslam_pool_save checkpoint), where does the known end, and from
where to look next -- on one MI355X.

    python tools/map_frontier.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1
        (--points PTS.npy --poses POSES.npy | --frame DEPTH.png POSE.txt [--frame ...] --fx FX --fy FY [--subsample K])
        [--range CELLS] [--obs PREVIOUS.npz] [--depth D] [--views K --grid STEP --clearance CELLS --view-range CELLS]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth).  The frames are either PTS.npy, [F, n, 3] float32 points in the sensor frame (a non-finite point
= no measurement), with POSES.npy, [F, 16] float32 sensor-to-world matrices, column-major as every trans[16] of include/svoslam.h;
or 16-bit depth images in millimetres (PNG / PGM: svoslam_image_load) of one size, each with a file of its pose's 16 floats
separated by white space, halved --subsample times (svoslam_subsample_depth_u16) and turned into vertex maps
(svoslam_generate_vertex_map), as tools/map_relocalize.py reads its observation.  svoslam_field_observe_rays marks every cell of
the box a ray passed through or ended in; a ray longer than --range cells is skipped (default 0: no limit).  --obs PREVIOUS.npz
continues an earlier result of this tool over the same cells: the new marks are added to its obs.  svoslam_pool_frontier_field then
holds the observation against the map.  OUT.npz holds

  obs[z, y, x]        uint8: bit 1 a ray passed through the cell, bit 2 a ray ended in it
  state[z, y, x]      uint8: 0 unknown, 1 free, 2 frontier (free beside an unknown cell of the box), 3 occupied, 4 vacated (occupied,
                      rays passed through and none ended), 5 unmapped (a ray ended where the map has nothing)
  frontier[z, y, x]   uint8: 1 where the state is 2
  ray_summary         int64 [6]: rays void, outside the root, beyond the range, marked; cells with bit 1, cells with bit 2
  state_summary       int32 [6]: the cells per state
  origin, dims        the first cell and the cells per axis (x, y, z) at `depth`
  cell_size           metres per cell, and depth, center, edge_length, range_cells, box

With --views K it also chooses up to K viewpoints for the frontier (svoslam_pool_cover_views with the free cells selected by
`frontier` as targets, seen within --view-range cells): the candidates are every STEP-th cell of the box per axis, counted from its
first cell, that has no occupied cell within --clearance cells, as tools/map_cover.py takes them, and OUT.npz also holds
candidate_cells, seen, chosen, gain, round, cover_summary, chosen_cells (int32 [K, 3], -1 past the end) and chosen_centres (float64
[K, 3] metres, NaN past the end).

Prints the ray counts, the cells per state and what each chosen view adds."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_from_images(pkg, torch, frames, fx, fy, subsample):
    """-> (points [F, n, 3] cuda float32, poses [F, 16] float32): the vertex maps of the depth images"""
    maps, poses = [], []
    for image_path, pose_path in frames:
        image = pkg.image_load(image_path)
        if image.ndim != 2 or image.dtype != np.uint16:
            sys.exit("%s: a depth image is one channel of 16 bits" % image_path)
        h, w = image.shape
        depth = torch.from_numpy(image.view(np.int16).copy()).cuda()
        tmp = torch.empty_like(depth)
        lw, lh = w, h
        for _ in range(subsample):
            pkg.subsample_depth(depth, tmp, lw, lh)
            lw, lh = lw // 2, lh // 2
        level = depth.reshape(-1)[: lw * lh].reshape(lh, lw)
        vmap = torch.empty((lh, lw, 3), dtype=torch.float32, device="cuda")
        pkg.generate_vertex_map(level, vmap, fx, fy, w, h)
        maps.append(vmap.reshape(-1, 3))
        pose = np.asarray(np.loadtxt(pose_path).reshape(-1), np.float32)
        if pose.shape != (16,):
            sys.exit("%s: a pose is 16 floats" % pose_path)
        poses.append(pose)
    if len({int(m.shape[0]) for m in maps}) != 1:
        sys.exit("the depth images are of one size")
    return torch.stack(maps), np.stack(poses)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--box", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="metres: min xyz, max xyz")
    ap.add_argument("--points", default=None, metavar="PTS.npy", help="[F, n, 3] float32 in the sensor frame")
    ap.add_argument("--poses", default=None, metavar="POSES.npy", help="[F, 16] float32, sensor to world")
    ap.add_argument("--frame", nargs=2, action="append", default=None, metavar=("DEPTH.png", "POSE.txt"), help="a 16-bit depth image in millimetres and its pose")
    ap.add_argument("--fx", type=float, default=None)
    ap.add_argument("--fy", type=float, default=None)
    ap.add_argument("--subsample", type=int, default=0, help="halvings of the depth images")
    ap.add_argument("--range", type=int, default=0, dest="range_cells", help="rays longer than this many cells are skipped (0: no limit)")
    ap.add_argument("--obs", default=None, metavar="PREVIOUS.npz", help="an earlier result over the same cells to add to")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    ap.add_argument("--views", type=int, default=None, metavar="K", help="choose up to K viewpoints for the frontier")
    ap.add_argument("--grid", type=int, default=4, metavar="STEP", help="with --views: candidates are every STEP-th cell of the box that is clear")
    ap.add_argument("--clearance", type=int, default=1, metavar="CELLS", help="with --views: no occupied cell within CELLS cells of a candidate")
    ap.add_argument("--view-range", type=int, default=None, metavar="CELLS", help="with --views: cells a candidate sees far (default: --range)")
    args = ap.parse_args()
    if (args.points is None) == (args.frame is None):
        sys.exit("give either --points PTS.npy --poses POSES.npy or --frame DEPTH.png POSE.txt")
    if args.points is not None and args.poses is None:
        sys.exit("--points needs --poses")
    if args.frame is not None and (args.fx is None or args.fy is None):
        sys.exit("a depth image needs --fx and --fy")
    if args.views is not None and args.grid < 1:
        sys.exit("--grid STEP is at least 1")
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    pool, ws = pkg.Pool(), pkg.Workspace()
    center, edge, stored = pool.load(args.checkpoint)
    depth = stored if args.depth is None else args.depth
    cells = pkg.box_to_cells(depth, center, edge, args.box)
    if cells is None:
        sys.exit("the box is empty: a NaN, min > max, or outside the root cube")
    lo, hi = cells
    dims = hi - lo + 1
    if args.points is not None:
        poses = np.ascontiguousarray(np.load(args.poses), np.float32).reshape(-1, 16)
        points = torch.from_numpy(np.ascontiguousarray(np.load(args.points), np.float32).reshape(poses.shape[0], -1, 3)).cuda()
    else:
        points, poses = frames_from_images(pkg, torch, args.frame, args.fx, args.fy, args.subsample)
    previous = None
    if args.obs is not None:
        z = np.load(args.obs)
        if z["origin"].tolist() != lo.tolist() or z["dims"].tolist() != dims.tolist() or int(z["depth"]) != depth:
            sys.exit("%s holds other cells than this box at depth %d" % (args.obs, depth))
        previous = z["obs"]
    obs, ray_summary = pkg.observe_rays(ws, previous, depth, center, edge, lo, dims, points, poses, args.range_cells,
                                        accumulate=previous is not None, as_tensor=True)
    cell_size = 2.0 * float(edge) / (1 << depth)
    extra = {}
    if args.views is None:
        field = pkg.frontier_field(ws, pool, depth, lo, dims, obs)
    else:
        clear = pkg.distance_field(ws, pool, depth, lo, dims, args.clearance)[::args.grid, ::args.grid, ::args.grid] == -1
        cz, cy, cx = np.nonzero(clear)                                  # region order: x fastest
        cand_cells = (np.stack([cx, cy, cz], 1) * args.grid + lo).astype(np.int32)
        view_range = args.range_cells if args.view_range is None else args.view_range
        field, cover = pkg.explore_views(ws, pool, depth, lo, dims, obs, cand_cells, view_range, args.views)
        n_chosen = int(cover["summary"][1])
        chosen_cells = np.full((args.views, 3), -1, np.int32)
        chosen_centres = np.full((args.views, 3), np.nan)
        chosen_cells[:n_chosen] = cand_cells[cover["chosen"][:n_chosen]]
        chosen_centres[:n_chosen] = (np.asarray(center, np.float64) - float(edge)) + (chosen_cells[:n_chosen] + 0.5) * cell_size
        extra = dict(candidate_cells=cand_cells, seen=cover["seen"], chosen=cover["chosen"], gain=cover["gain"], round=cover["round"],
                     cover_summary=cover["summary"], chosen_cells=chosen_cells, chosen_centres=chosen_centres, view_range_cells=view_range)
    ray_summary = ray_summary.cpu().numpy()
    np.savez_compressed(args.out, obs=obs.cpu().numpy(), state=field["state"], frontier=field["frontier"], ray_summary=ray_summary,
                        state_summary=field["summary"], origin=lo.astype(np.int32), dims=dims.astype(np.int32), cell_size=cell_size, depth=depth,
                        center=np.asarray(center, np.float32), edge_length=np.float32(edge), range_cells=args.range_cells,
                        box=np.asarray(args.box, np.float32), **extra)
    print("depth %d, cells %s + %s, %d frames: rays %d void, %d outside, %d beyond %d cells, %d marked; cells %d passed through, %d ended in -> %s" % (
        depth, lo.tolist(), dims.tolist(), poses.shape[0], ray_summary[0], ray_summary[1], ray_summary[2], args.range_cells, ray_summary[3],
        ray_summary[4], ray_summary[5], args.out))
    print("  cells: " + ", ".join("%d %s" % (count, name) for name, count in zip(pkg.STATE_NAMES, field["summary"].tolist())))
    if args.views is not None:
        for j in range(n_chosen):
            print("  view %d: candidate %d at cell %s sees %d more frontier cells" % (j, cover["chosen"][j], chosen_cells[j].tolist(), cover["gain"][j]))


if __name__ == "__main__":
    main()
