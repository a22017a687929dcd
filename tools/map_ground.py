"""Paths over the ground of a box of a saved map (svoslam_pool_save checkpoint) for a robot that stands on surfaces, on one MI355X.

    python tools/map_ground.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --up {+y,-y,+z,-z} --radius CELLS --height CELLS
           --step CELLS --climb-cost C --snap CELLS --goal x y z --start x y z [--start ...] [--depth D]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth), and the goal and every --start (metres) the cell that holds it, by the same rule; each is then
snapped downwards by at most --snap cells to its foothold.  A cell is a foothold when the cell under it is occupied, --height cells
from it upwards are free, and from --step cells above it upwards nothing occupied lies within --radius cells of it horizontally.
svoslam_pool_ground_field, seeded at the goal, gives every foothold of the box the cost of the cheapest way to the goal: a move goes
one cell horizontally and at most --step cells up or down and costs 1, plus --climb-cost per cell climbed or descended.
svoslam_field_trace_ground_paths then walks from every start down the field.  OUT.npz holds

  cost[z, y, x]     int32, the cost to the goal; -1 = a foothold without a way, -2 = no foothold
  origin, dims      the first cell and the cells per axis (x, y, z) at `depth`
  goal_cell         int32 [3], and start_cells int32 [n, 3], before snapping (a point outside the root cube: -1 -1 -1)
  lengths, costs    int32 [n]: the cells of each start's path, both footholds included, and its cost (0 and -1: no path)
  climbs            int32 [n]: the cells climbed and descended along each path in all
  cells_K           int32 [lengths[K], 3], the cells of start K's path from its foothold to the goal's
  polyline_K        float64 [lengths[K], 3], their centres in metres
  footholds         the number of footholds in the box
  cell_size         metres per cell, and depth, center, edge_length, up, radius_cells, height_cells, step_cells, climb_cost,
                    snap_cells, box, goal, starts

Prints, per start, the cells and metres of its path, its cost and its climb."""
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
    ap.add_argument("--up", choices=("+y", "-y", "+z", "-z"), default="+y", help="the direction away from the ground (default +y)")
    ap.add_argument("--radius", type=int, required=True, help="cells of body radius above the step height (0 .. 4096)")
    ap.add_argument("--height", type=int, required=True, help="cells of headroom (1 .. 256)")
    ap.add_argument("--step", type=int, required=True, help="cells the robot climbs in one move (0 .. min(height - 1, 4))")
    ap.add_argument("--climb-cost", type=int, default=0, help="extra cost per cell climbed or descended (0 .. 65534)")
    ap.add_argument("--snap", type=int, default=0, help="cells the goal and the starts may be above their foothold (0 .. 256)")
    ap.add_argument("--goal", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"), help="metres")
    ap.add_argument("--start", type=float, nargs=3, action="append", required=True, metavar=("X", "Y", "Z"), help="metres; may be repeated")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    args = ap.parse_args()
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    pool, ws = pkg.Pool(), pkg.Workspace()
    center, edge, stored = pool.load(args.checkpoint)
    depth = stored if args.depth is None else args.depth
    plan = pkg.plan_ground_paths(ws, pool, depth, center, edge, args.box, args.goal, args.start, args.up, args.radius, args.height,
                                 args.step, args.climb_cost, args.snap)
    if plan is None:
        sys.exit("the box is empty: a NaN, min > max, or outside the root cube")
    none = np.full(3, -1, np.int32)
    paths = plan["paths"]
    out = dict(cost=plan["cost"], origin=plan["origin"].astype(np.int32), dims=plan["dims"].astype(np.int32),
               goal_cell=none if plan["goal_cell"] is None else plan["goal_cell"],
               start_cells=np.array([none if p["cell"] is None else p["cell"] for p in paths], np.int32).reshape(-1, 3),
               lengths=np.array([p["length"] or 0 for p in paths], np.int32),
               costs=np.array([-1 if p["cost"] is None else p["cost"] for p in paths], np.int32),
               climbs=np.array([p["climb"] or 0 for p in paths], np.int32), footholds=plan["footholds"],
               cell_size=plan["cell_size"], depth=depth, center=np.asarray(center, np.float32), edge_length=np.float32(edge),
               up=args.up, radius_cells=args.radius, height_cells=args.height, step_cells=args.step, climb_cost=args.climb_cost,
               snap_cells=args.snap, box=np.asarray(args.box, np.float32), goal=np.asarray(args.goal, np.float32),
               starts=np.asarray(args.start, np.float32))
    for k, p in enumerate(paths):
        out["cells_%d" % k] = p["cells"] if p["cells"] is not None else np.zeros((0, 3), np.int32)
        out["polyline_%d" % k] = p["polyline"] if p["polyline"] is not None else np.zeros((0, 3), np.float64)
    np.savez_compressed(args.out, **out)
    print("depth %d, cells %s + %s, up %s, radius %d, height %d, step %d, climb cost %d, snap %d, %d footholds -> %s" % (
        depth, plan["origin"].tolist(), plan["dims"].tolist(), args.up, args.radius, args.height, args.step, args.climb_cost, args.snap,
        plan["footholds"], args.out))
    for k, p in enumerate(paths):
        if p["length"] is None:
            print("start %d: no path" % k)
        else:
            print("start %d: %d cells, %.3f m, cost %d, climb %d cells" % (k, p["length"], (p["length"] - 1) * plan["cell_size"], p["cost"],
                                                                          p["climb"]))


if __name__ == "__main__":
    main()
