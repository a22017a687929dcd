"""Viewpoints that cover a box of a saved map (svoslam_pool_save checkpoint): which few of many candidate cells see the most of
the box's surface, and what stays unseen after them, on one MI355X.

    python tools/map_cover.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --range CELLS
        (--candidates PTS.npy | --grid STEP --clearance CELLS) --views K [--min-gain G] [--targets surface|free|all] [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth).  The candidates are either the points of PTS.npy ([n, 3] metres; each becomes the cell that holds
it, by the same rule; a point outside the root cube becomes -1 -1 -1 and sees nothing), or every STEP-th cell of the box per axis,
counted from its first cell, that has no occupied cell within CELLS cells (svoslam_pool_distance_field with that radius gives -1
there), in the box's cell order, x fastest.  svoslam_pool_cover_views then scores every candidate by the targets it sees within
--range cells (the visibility field's sight rule: edges and corners block) and covers the targets greedily in at most K rounds, each
round taking the candidate that sees the most targets not yet covered, the lowest index among equals, until a round would gain less
than G (default 1).  OUT.npz holds

  chosen, gain        int32 [K]: the candidate of each round and the targets it added (-1 / 0 past the end)
  chosen_cells        int32 [K, 3]: the cells of the chosen candidates (-1 -1 -1 past the end)
  chosen_centres      float64 [K, 3]: their centres in metres (NaN past the end)
  seen                int32 [n]: the targets each candidate sees
  round[z, y, x]      int32: -1 not a target, -2 a target no chosen candidate sees, else the round that first covered the cell
  summary             int32 [4]: targets, chosen, covered, coverable (seen by at least one candidate)
  candidate_cells     int32 [n, 3]
  origin, dims        the first cell and the cells per axis (x, y, z) at `depth`
  cell_size           metres per cell, and depth, center, edge_length, range_cells, min_gain, targets, box

Prints the targets, how many of them any candidate sees, and what each round added."""
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
    ap.add_argument("--box", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="metres: min xyz, max xyz")
    ap.add_argument("--range", type=int, required=True, dest="range_cells", help="cells a candidate sees far (0 .. 4096)")
    ap.add_argument("--candidates", default=None, metavar="PTS.npy", help="[n, 3] points in metres")
    ap.add_argument("--grid", type=int, default=None, metavar="STEP", help="candidates: every STEP-th cell of the box that is clear")
    ap.add_argument("--clearance", type=int, default=0, metavar="CELLS", help="with --grid: no occupied cell within CELLS cells")
    ap.add_argument("--views", type=int, required=True, metavar="K", help="rounds of the cover at most (0 .. 1024)")
    ap.add_argument("--min-gain", type=int, default=1, metavar="G", help="stop when a round would add fewer targets")
    ap.add_argument("--targets", choices=("surface", "free", "all"), default="surface")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    args = ap.parse_args()
    if (args.candidates is None) == (args.grid is None):
        sys.exit("give either --candidates PTS.npy or --grid STEP")
    if args.grid is not None and args.grid < 1:
        sys.exit("--grid STEP is at least 1")
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
    if args.candidates is not None:
        points = np.asarray(np.load(args.candidates), np.float32).reshape(-1, 3)
        cand_cells = np.full((points.shape[0], 3), -1, np.int32)
        for k, p in enumerate(points):
            at = pkg.box_to_cells(depth, center, edge, list(p) + list(p))
            if at is not None:
                cand_cells[k] = at[0]
    else:
        clear = pkg.distance_field(ws, pool, depth, lo, dims, args.clearance)[::args.grid, ::args.grid, ::args.grid] == -1
        z, y, x = np.nonzero(clear)                                     # region order: x fastest
        cand_cells = (np.stack([x, y, z], 1) * args.grid + lo).astype(np.int32)
    got = pkg.cover_views(ws, pool, depth, lo, dims, args.range_cells, cand_cells, args.views, args.min_gain, args.targets)
    cell_size = 2.0 * float(edge) / (1 << depth)
    n_chosen = int(got["summary"][1])
    chosen_cells = np.full((args.views, 3), -1, np.int32)
    chosen_centres = np.full((args.views, 3), np.nan)
    chosen_cells[:n_chosen] = cand_cells[got["chosen"][:n_chosen]]
    chosen_centres[:n_chosen] = (np.asarray(center, np.float64) - float(edge)) + (chosen_cells[:n_chosen] + 0.5) * cell_size
    np.savez_compressed(args.out, origin=lo.astype(np.int32), dims=dims.astype(np.int32), candidate_cells=cand_cells, chosen_cells=chosen_cells,
                        chosen_centres=chosen_centres, cell_size=cell_size, depth=depth, center=np.asarray(center, np.float32),
                        edge_length=np.float32(edge), range_cells=args.range_cells, min_gain=args.min_gain, targets=args.targets,
                        box=np.asarray(args.box, np.float32), **got)
    T, _, covered, coverable = got["summary"].tolist()
    print("depth %d, cells %s + %s, range %d cells, %s targets: %d targets, %d seen by at least one of %d candidates, %d covered by %d -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.range_cells, args.targets, T, coverable, cand_cells.shape[0], covered, n_chosen, args.out))
    for j in range(n_chosen):
        print("  round %d: candidate %d at cell %s adds %d" % (j, got["chosen"][j], chosen_cells[j].tolist(), got["gain"][j]))


if __name__ == "__main__":
    main()
