"""The connected components of the free or the solid cells of a box of a saved map (svoslam_pool_save checkpoint), on one MI355X.

    python tools/map_components.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --clearance CELLS [--solid] [--depth D] [--min-size K]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth).  svoslam_pool_label_components labels the 6-connected components, inside the box, of the cells
at least --clearance cells clear of every occupied cell of the map -- "is B reachable from A at all" is labels[a] == labels[b] --
or with --solid of the box's other cells: at clearance 0 the clusters of occupied cells, whose sizes tell depth-noise floaters
from structure.  Cells that touch only by an edge or a corner are not connected; --solid --clearance 1 clusters more loosely.
OUT.npz holds

  labels[z, y, x]  int32, -1 = not in the set, else the smallest index (z * ny + y) * nx + x of the cell's component
  sizes[z, y, x]   int32, the cells of the component, 0 where labels is -1
  keep[z, y, x]    bool, only with --min-size: the cells of components of at least K cells
  origin, dims     the first cell and the cells per axis (x, y, z) at `depth`
  components       how many components there are, and largest, the cells of the largest
  cell_size        metres per cell, and depth, center, edge_length, clearance_cells, solid, box

Prints the number of components, the largest, and with --min-size what is kept."""
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
    ap.add_argument("--clearance", type=int, required=True, help="cells the free set keeps from occupied cells (0 .. 4096)")
    ap.add_argument("--solid", action="store_true", help="label the cells that are NOT clear instead (clearance 0: the occupied cells)")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    ap.add_argument("--min-size", type=int, default=None, metavar="K", help="also write the mask of components of at least K cells")
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
    stats = {}
    labels, sizes = pkg.label_components(ws, pool, depth, lo, dims, args.clearance, solid=args.solid, sizes=True, stats=stats)
    cell_size = 2.0 * float(edge) / (1 << depth)
    extra = {}
    kept = ""
    if args.min_size is not None:
        extra["keep"] = sizes >= max(args.min_size, 1)
        extra["min_size"] = args.min_size
        roots = labels.reshape(-1) == np.arange(labels.size)
        kept = ", %d components of at least %d cells keep %d cells" % (int((roots & extra["keep"].reshape(-1)).sum()), args.min_size,
                                                                       int(extra["keep"].sum()))
    np.savez_compressed(args.out, labels=labels, sizes=sizes, origin=lo.astype(np.int32), dims=dims.astype(np.int32),
                        components=stats["components"], largest=stats["largest"], cell_size=cell_size, depth=depth,
                        center=np.asarray(center, np.float32), edge_length=np.float32(edge), clearance_cells=args.clearance,
                        solid=bool(args.solid), box=np.asarray(args.box, np.float32), **extra)
    print("depth %d, cells %s + %s, clearance %d cells, %s: %d components in %d cells, the largest %d cells%s -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.clearance, "solid" if args.solid else "free", stats["components"], int((labels >= 0).sum()),
        stats["largest"], kept, args.out))


if __name__ == "__main__":
    main()
