"""A 2-D navigation slice of a saved map (svoslam_pool_save checkpoint), on one MI355X.

    python tools/map_slice.py CHECKPOINT OUT.npz --axis y --lo M --hi M [--depth D] [--radius CELLS]

The slab --lo .. --hi (metres along --axis) is projected onto the plane of the other two axes (u, v: x z for --axis y, y z for x,
x y for z), cell by cell at depth D (default: the map's stored depth, at most 10 -- the grids hold 4^D cells):

  occupancy[v, u]  the occupied cells in the column over plane cell (u, v) between --lo and --hi (svoslam_pool_count_boxes, one
                   column box per plane cell, its faces on the cell's lattice planes): 0 = the column is free
  clearance[v, u]  metres from the centre of the slab's mid-plane cell (u, v) to the nearest occupied cell's centre, by
                   svoslam_pool_nearest_occupied within --radius cells (default 64): inf = nothing within the radius

OUT.npz also holds axis, lo, hi, depth, center, edge_length, radius_cells and cell_size.  Prints how many columns are occupied and
the smallest clearance over the free ones."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
ROWS_PER_CALL = 1 << 20     # boxes or points per launch: bounds the device arrays at a few tens of MB


def planes(center, depth, edge):
    """P(k), k = 0 .. N, of one axis: center + (float)(2k - N) * (edge / (float)N) in binary32, as the library computes them"""
    n_side = 1 << depth
    return (F(center) + (2 * np.arange(n_side + 1, dtype=np.int64) - n_side).astype(F) * (F(edge) / F(n_side))).astype(F)


def slice_inputs(center, edge, depth, axis, lo, hi):
    """(boxes[N*N, 6], points[N*N, 3]) in v-major order: the column over each plane cell, and the centre of its mid-plane cell"""
    n_side = 1 << depth
    u, v = [a for a in range(3) if a != axis]
    pu, pv = planes(center[u], depth, edge), planes(center[v], depth, edge)
    iv, iu = np.meshgrid(np.arange(n_side), np.arange(n_side), indexing="ij")
    iu, iv = iu.reshape(-1), iv.reshape(-1)
    boxes = np.empty((n_side * n_side, 6), F)
    boxes[:, u], boxes[:, 3 + u] = pu[iu], pu[iu + 1]             # a face ON a lattice plane does not take in the cell beyond
    boxes[:, v], boxes[:, 3 + v] = pv[iv], pv[iv + 1]
    boxes[:, axis], boxes[:, 3 + axis] = lo, hi
    points = np.empty((n_side * n_side, 3), F)
    points[:, u] = ((pu[iu].astype(np.float64) + pu[iu + 1]) / 2).astype(F)
    points[:, v] = ((pv[iv].astype(np.float64) + pv[iv + 1]) / 2).astype(F)
    points[:, axis] = (float(lo) + float(hi)) / 2
    return boxes, points


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--axis", choices="xyz", default="y", help="the axis the slab is projected along")
    ap.add_argument("--lo", type=float, required=True, help="lower face of the slab in metres")
    ap.add_argument("--hi", type=float, required=True, help="upper face of the slab in metres")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth, at most 10)")
    ap.add_argument("--radius", type=int, default=64, help="clearance search radius in cells (0 .. 4096)")
    args = ap.parse_args()
    if not args.lo <= args.hi:
        ap.error("--lo must not exceed --hi")
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    pool = pkg.Pool()
    center, edge, stored = pool.load(args.checkpoint)
    depth = min(stored, 10) if args.depth is None else args.depth
    axis = "xyz".index(args.axis)
    n_side = 1 << depth
    boxes, points = slice_inputs(center, edge, depth, axis, args.lo, args.hi)
    count, dist2 = np.empty(n_side * n_side, np.uint64), np.empty(n_side * n_side, np.int32)
    for s in range(0, n_side * n_side, ROWS_PER_CALL):
        e = s + ROWS_PER_CALL
        count[s:e] = pkg.count_boxes(pool, depth, center, edge, boxes[s:e], outputs=("count",))["count"]
        dist2[s:e] = pkg.nearest_occupied(pool, depth, center, edge, points[s:e], args.radius, outputs=("dist2",))["dist2"]
    cell_size = 2.0 * float(edge) / n_side
    clearance = np.where(dist2 >= 0, np.sqrt(np.maximum(dist2, 0).astype(np.float64)) * cell_size, np.where(dist2 == -1, np.inf, np.nan))
    occupancy = count.astype(np.uint32).reshape(n_side, n_side)
    clearance = clearance.astype(F).reshape(n_side, n_side)
    np.savez_compressed(args.out, occupancy=occupancy, clearance=clearance, axis=args.axis, lo=args.lo, hi=args.hi, depth=depth,
                        center=np.asarray(center, F), edge_length=F(edge), radius_cells=args.radius, cell_size=cell_size)
    free = occupancy == 0
    near = clearance[free & np.isfinite(clearance)]
    print("depth %d, slab %s %.3f .. %.3f m: %d of %d columns occupied%s -> %s" % (
        depth, args.axis, args.lo, args.hi, int((~free).sum()), n_side * n_side,
        ", smallest clearance over a free column %.3f m" % near.min() if near.size else "", args.out))


if __name__ == "__main__":
    main()
