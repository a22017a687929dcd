"""The signed distance field of a box of a saved map (svoslam_pool_save checkpoint) with the witness cell behind every distance and the
direction away from it -- what a trajectory optimiser pushes a way-point along -- on one MI355X.

    python tools/map_gradient.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --radius CELLS [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth).  svoslam_pool_nearest_field is called twice: for the nearest occupied cell of every cell of the
box, and for the nearest cell that is not occupied; cells outside the box count as targets, and among equally near cells the one
with the smallest z, then y, then x is the witness.  OUT.npz holds

  dist2_occupied[z, y, x], dist2_free[z, y, x]   int32, squared cells, -1 = nothing within the radius
  witness_occupied[z, y, x, 3], witness_free     int32, the x, y, z of the witness cell, -1 where there is none
  signed_metres[z, y, x]   float32: +sqrt(dist2_occupied) * cell_size at a cell that is not occupied, -sqrt(dist2_free) * cell_size
                           at an occupied one; +inf / -inf where there is nothing within the radius
  direction[z, y, x, 3]    float32: the unit vector from the witness (the occupied one outside, the free one inside) to the cell,
                           zero where there is none
  origin, dims             the first cell and the cells per axis (x, y, z) at `depth`
  cell_size                metres per cell, and depth, center, edge_length, radius_cells, box

Prints the share of occupied cells and the largest finite distance on either side."""
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
    occ = pkg.nearest_field(ws, pool, depth, lo, dims, args.radius, which=pkg.NEAREST_OCCUPIED)
    free = pkg.nearest_field(ws, pool, depth, lo, dims, args.radius, which=pkg.NEAREST_FREE)
    cell_size = 2.0 * float(edge) / (1 << depth)
    inside = occ["dist2"] == 0
    dist2 = np.where(inside, free["dist2"], occ["dist2"])
    none = dist2 < 0
    metres = np.where(inside, -1.0, 1.0) * np.sqrt(np.maximum(dist2, 0).astype(np.float64)) * cell_size
    signed = np.where(none, np.where(inside, -np.inf, np.inf), metres).astype(np.float32)
    z, y, x = np.meshgrid(*[np.arange(lo[a], lo[a] + dims[a]) for a in (2, 1, 0)], indexing="ij")
    witness = np.where(inside[..., None], free["cell_xyz"], occ["cell_xyz"])
    away = np.where(none[..., None], 0, np.stack([x, y, z], -1) - witness).astype(np.float64)
    norm = np.sqrt((away ** 2).sum(-1, keepdims=True))
    direction = np.where(norm > 0, away / np.maximum(norm, 1e-30), 0.0).astype(np.float32)
    np.savez_compressed(args.out, dist2_occupied=occ["dist2"], dist2_free=free["dist2"], witness_occupied=occ["cell_xyz"],
                        witness_free=free["cell_xyz"], signed_metres=signed, direction=direction, origin=lo.astype(np.int32),
                        dims=dims.astype(np.int32), cell_size=cell_size, depth=depth, center=np.asarray(center, np.float32),
                        edge_length=np.float32(edge), radius_cells=args.radius, box=np.asarray(args.box, np.float32))
    out, deep = signed[np.isfinite(signed) & ~inside], signed[np.isfinite(signed) & inside]
    print("depth %d, cells %s + %s, radius %d cells: %d of %d cells occupied, %d with nothing within the radius%s%s -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.radius, int(inside.sum()), inside.size, int(none.sum()),
        ", largest clearance %.3f m" % out.max() if out.size else "", ", largest depth %.3f m" % -deep.min() if deep.size else "", args.out))


if __name__ == "__main__":
    main()
