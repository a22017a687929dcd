"""The distance field (ESDF-style clearance block) of a box of a saved map (svoslam_pool_save checkpoint), on one MI355X.

    python tools/map_esdf.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --radius CELLS [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth); svoslam_pool_distance_field gives every cell of it the squared distance, in cells, to the nearest
occupied cell of the map within --radius cells -- occupied cells outside the box count too.  OUT.npz holds

  dist2[z, y, x]   int32, -1 = nothing within the radius
  metres[z, y, x]  float32, sqrt(dist2) * cell_size, +inf where dist2 is -1
  origin, dims     the first cell and the cells per axis (x, y, z) at `depth`
  cell_size        metres per cell, and depth, center, edge_length, radius_cells, box

Prints the share of occupied cells and the largest finite clearance."""
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
    ap.add_argument("--radius", type=int, required=True, help="truncation radius in cells (0 .. 4096)")
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
    dist2 = pkg.distance_field(ws, pool, depth, lo, dims, args.radius)
    cell_size = 2.0 * float(edge) / (1 << depth)
    metres = np.where(dist2 >= 0, np.sqrt(np.maximum(dist2, 0).astype(np.float64)) * cell_size, np.inf).astype(np.float32)
    np.savez_compressed(args.out, dist2=dist2, metres=metres, origin=lo.astype(np.int32), dims=dims.astype(np.int32), cell_size=cell_size,
                        depth=depth, center=np.asarray(center, np.float32), edge_length=np.float32(edge), radius_cells=args.radius,
                        box=np.asarray(args.box, np.float32))
    near = metres[np.isfinite(metres)]
    print("depth %d, cells %s + %s, radius %d cells: %d of %d cells occupied, %d with nothing within the radius%s -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.radius, int((dist2 == 0).sum()), dist2.size, int((dist2 < 0).sum()),
        ", largest clearance %.3f m" % near.max() if near.size else "", args.out))


if __name__ == "__main__":
    main()
