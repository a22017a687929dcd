"""The reach field (cost-to-go, navigation function) of a box of a saved map (svoslam_pool_save checkpoint), on one MI355X.

    python tools/map_reach.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --clearance CELLS --seed x y z [--seed ...] [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth), and every --seed (metres) the cell that holds it, by the same rule.  svoslam_pool_reach_field
gives every cell of the box the number of face-neighbour moves of the shortest path from a seed that stays in the box and at least
--clearance cells clear of every occupied cell of the map.  OUT.npz holds

  steps[z, y, x]   int32, -1 = no path from any seed, -2 = blocked (an occupied cell within the clearance)
  metres[z, y, x]  float32, steps * cell_size, +inf where steps is negative
  origin, dims     the first cell and the cells per axis (x, y, z) at `depth`
  seed_cells       int32 [n, 3], the cells of the seeds (a seed outside the root cube: -1 -1 -1)
  cell_size        metres per cell, and depth, center, edge_length, clearance_cells, box, seeds

Prints how many seeds counted, the cells reached, cut off and blocked, and the longest path."""
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
    ap.add_argument("--clearance", type=int, required=True, help="cells every path keeps from occupied cells (0 .. 4096)")
    ap.add_argument("--seed", type=float, nargs=3, action="append", required=True, metavar=("X", "Y", "Z"), help="metres; may be repeated")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    args = ap.parse_args()
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
    seed_cells = np.full((len(args.seed), 3), -1, np.int32)
    for k, s in enumerate(args.seed):
        at = pkg.box_to_cells(depth, center, edge, list(s) + list(s))
        if at is not None:
            seed_cells[k] = at[0]
    stats = {}
    steps = pkg.reach_field(ws, pool, depth, lo, dims, args.clearance, seed_cells, stats=stats)
    cell_size = 2.0 * float(edge) / (1 << depth)
    metres = np.where(steps >= 0, steps.astype(np.float64) * cell_size, np.inf).astype(np.float32)
    np.savez_compressed(args.out, steps=steps, metres=metres, origin=lo.astype(np.int32), dims=dims.astype(np.int32), seed_cells=seed_cells,
                        cell_size=cell_size, depth=depth, center=np.asarray(center, np.float32), edge_length=np.float32(edge),
                        clearance_cells=args.clearance, box=np.asarray(args.box, np.float32), seeds=np.asarray(args.seed, np.float32))
    print("depth %d, cells %s + %s, clearance %d cells: %d of %d seeds counted, %d cells reached, %d cut off, %d blocked%s -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.clearance, stats["seeds_used"], len(args.seed), int((steps >= 0).sum()),
        int((steps == -1).sum()), int((steps == -2).sum()),
        ", longest path %d steps = %.3f m" % (int(steps.max()), int(steps.max()) * cell_size) if (steps >= 0).any() else "", args.out))


if __name__ == "__main__":
    main()
