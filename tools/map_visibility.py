"""The visibility field (which viewpoints have a line of sight to which cells) of a box of a saved map (svoslam_pool_save
checkpoint), on one MI355X.

    python tools/map_visibility.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --range CELLS --view x y z [--view ...] [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth), and every --view (metres) the cell that holds it, by the same rule.  svoslam_pool_visibility_field
gives every cell of the box the viewpoints within --range cells whose segment to it, cell centre to cell centre, touches no occupied
cell other than the two ends -- edges and corners block.  A viewpoint may lie outside the box.  OUT.npz holds

  mask[z, y, x]    uint32, bit k set = viewpoint k sees the cell (written for at most 32 viewpoints)
  count[z, y, x]   int32, the viewpoints that see the cell
  origin, dims     the first cell and the cells per axis (x, y, z) at `depth`
  view_cells       int32 [n, 3], the cells of the viewpoints (a viewpoint outside the root cube: -1 -1 -1; it sees nothing)
  cell_size        metres per cell, and depth, center, edge_length, range_cells, box, views

Prints how many viewpoints counted, the cells seen by at least one, and the cells seen by all that counted."""
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
    ap.add_argument("--range", type=int, required=True, dest="range_cells", help="cells a viewpoint sees far (0 .. 4096)")
    ap.add_argument("--view", type=float, nargs=3, action="append", required=True, metavar=("X", "Y", "Z"), help="metres; may be repeated")
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
    view_cells = np.full((len(args.view), 3), -1, np.int32)
    for k, v in enumerate(args.view):
        at = pkg.box_to_cells(depth, center, edge, list(v) + list(v))
        if at is not None:
            view_cells[k] = at[0]
    want = ("mask", "count") if len(args.view) <= pkg.MAX_VIEWS_MASK else ("count",)
    got = pkg.visibility_field(ws, pool, depth, lo, dims, args.range_cells, view_cells, want=want)
    cell_size = 2.0 * float(edge) / (1 << depth)
    counted = int((view_cells >= 0).all(1).sum())
    np.savez_compressed(args.out, origin=lo.astype(np.int32), dims=dims.astype(np.int32), view_cells=view_cells, cell_size=cell_size,
                        depth=depth, center=np.asarray(center, np.float32), edge_length=np.float32(edge), range_cells=args.range_cells,
                        box=np.asarray(args.box, np.float32), views=np.asarray(args.view, np.float32), **got)
    count = got["count"]
    print("depth %d, cells %s + %s, range %d cells: %d of %d viewpoints counted, %d of %d cells seen by at least one, %d by all of them -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.range_cells, counted, len(args.view), int((count > 0).sum()), count.size,
        int((count == counted).sum()) if counted else 0, args.out))


if __name__ == "__main__":
    main()
