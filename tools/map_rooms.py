"""The rooms of a box of a saved map (svoslam_pool_save checkpoint) and the doors between them, on one MI355X.

    python tools/map_rooms.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --clearance CELLS --door CELLS [--min-core K] [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth).  Free space is eroded to the cells at least --door cells clear of every occupied cell of the map;
the connected components of what remains (svoslam_pool_label_components) are the cores, those of fewer than --min-core cells are
dropped; svoslam_pool_owner_field then grows every core back through the cells at least --clearance cells clear (--door >=
--clearance): a cell belongs to the core nearest by path, on a tie to the smaller label.  OUT.npz holds

  rooms[z, y, x]   int32, the room's label = the smallest index (z * ny + y) * nx + x of its core; -1 = free but reached by no
                   core, -2 = blocked
  steps[z, y, x]   int32, the moves to the room's core (0 in the core), -1, -2 as rooms
  cores[z, y, x]   int32, the core's label, -1 elsewhere
  labels[k]        the rooms' labels, ascending, with core_sizes[k] and room_sizes[k] in cells
  doors[m, 3]      (a, b, faces) for every pair a < b of rooms that are face neighbours, and how many cell faces they share
  origin, dims     the first cell and the cells per axis (x, y, z) at `depth`
  cell_size        metres per cell, and depth, center, edge_length, clearance_cells, door_cells, min_core, box

Prints the number of rooms and doors, and the cells no room reaches."""
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
    ap.add_argument("--clearance", type=int, required=True, help="cells a room keeps from occupied cells (0 .. 4096)")
    ap.add_argument("--door", type=int, required=True, help="cells a core keeps from occupied cells: half the widest opening that still parts two rooms")
    ap.add_argument("--min-core", type=int, default=1, metavar="K", help="drop cores of fewer than K cells (default 1)")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    args = ap.parse_args()
    if args.door < args.clearance:
        sys.exit("--door is at least --clearance")
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
    r = pkg.segment_rooms(ws, pool, depth, lo, dims, args.clearance, args.door, min_core=args.min_core)
    cell_size = 2.0 * float(edge) / (1 << depth)
    np.savez_compressed(args.out, origin=lo.astype(np.int32), dims=dims.astype(np.int32), cell_size=cell_size, depth=depth,
                        center=np.asarray(center, np.float32), edge_length=np.float32(edge), clearance_cells=args.clearance,
                        door_cells=args.door, min_core=args.min_core, box=np.asarray(args.box, np.float32), **r)
    print("depth %d, cells %s + %s, clearance %d cells, door %d cells: %d rooms, %d doors, %d free cells in no room -> %s" % (
        depth, lo.tolist(), dims.tolist(), args.clearance, args.door, r["labels"].shape[0], r["doors"].shape[0],
        int((r["rooms"] == -1).sum()), args.out))


if __name__ == "__main__":
    main()
