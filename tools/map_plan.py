"""Paths through a box of a saved map (svoslam_pool_save checkpoint) that keep away from obstacles where they can, on one MI355X.

    python tools/map_plan.py CHECKPOINT OUT.npz --box x0 y0 z0 x1 y1 z1 --clearance CELLS --comfort CELLS
           (--penalty P | --ring-cost c1 c2 ...) --goal x y z --start x y z [--start ...] [--depth D]
           [--straighten [--lookahead K]] [--corridor EXTENT]

The box (metres, min xyz then max xyz) becomes the cell range svoslam_pool_count_boxes would count (svoslam_box_to_cells) at depth D
(default: the map's stored depth), and the goal and every --start (metres) the cell that holds it, by the same rule.
svoslam_pool_cost_field, seeded at the goal's cell, gives every cell of the box the cost of the cheapest path to the goal that stays
in the box and at least --clearance cells clear of every occupied cell of the map: entering a cell costs 1, plus ring_cost[j -
clearance - 1] when its nearest occupied cell is in ring j, (j - 1)^2 < squared distance <= j^2, clearance < j <= comfort.
--ring-cost gives the comfort - clearance costs, nearest ring first; --penalty P is the linear ramp ring_cost[k] = P * (comfort -
clearance - k).  svoslam_field_trace_paths then walks from every start down the field.  OUT.npz holds

  cost[z, y, x]     int32, the cost to the goal; -1 = no path, -2 = blocked (an occupied cell within the clearance)
  origin, dims      the first cell and the cells per axis (x, y, z) at `depth`
  goal_cell         int32 [3], and start_cells int32 [n, 3] (a point outside the root cube: -1 -1 -1)
  lengths, costs    int32 [n]: the cells of each start's path, start and goal included, and its cost (0 and -1: no path)
  cells_K           int32 [lengths[K], 3], the cells of start K's path from the start to the goal
  polyline_K        float64 [lengths[K], 3], their centres in metres
  cell_size         metres per cell, and depth, center, edge_length, clearance_cells, comfort_cells, ring_cost, box, goal, starts

With --straighten every path is also pruned by svoslam_field_shorten_paths into waypoints joined by straight segments that keep the
clearance and come no nearer to an occupied cell than the stretch of the path they replace did, judged on the distance field with
the comfort radius; --lookahead K looks at most K cells ahead of a waypoint (default 0: the whole path, which costs up to
length^2 segment walks per path).  OUT.npz then also holds

  vertices_K            int32 [k], indices into cells_K: the waypoints of start K's path, first and last cell included
  waypoints_K           int32 [k, 3], the cells at them, and waypoint_polyline_K float64 [k, 3], their centres in metres
  straight_lengths      float64 [n], the Euclidean length of each waypoint polyline in metres (0: no path), and lookahead

With --corridor EXTENT every path also gets a safe corridor (svoslam_field_path_corridors): a chain of overlapping axis-aligned
boxes of cells that are all more than --clearance cells from every occupied cell, each grown at most EXTENT (0 .. 65536) layers a
direction from a cell of the path and its successor, judged on the distance field with the comfort radius.  OUT.npz then also holds

  boxes_K               int32 [k, 6], the boxes of start K's path in cells, lo xyz then hi xyz, both inclusive
  boxes_m_K             float64 [k, 6], the same in metres: the lo corner and the hi corner, the outer faces of the cubes
  anchors_K             int32 [k], indices into cells_K: the cell each box was grown from; consecutive boxes share the next one's
  corridor_gaps         int32 [n], the places where a path's chain is broken (0 for every path this tool traces), and corridor_extent

Prints, per start, the cells and metres of its path and its cost, with --straighten its waypoints and their metres, and with
--corridor its boxes."""
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
    ap.add_argument("--comfort", type=int, required=True, help="cells within which being near an occupied cell costs extra (clearance .. 4096)")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--penalty", type=int, help="linear ramp: ring k costs P * (comfort - clearance - k) extra")
    how.add_argument("--ring-cost", type=int, nargs="*", help="comfort - clearance extra costs, nearest ring first (0 .. 65534 each)")
    ap.add_argument("--goal", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"), help="metres")
    ap.add_argument("--start", type=float, nargs=3, action="append", required=True, metavar=("X", "Y", "Z"), help="metres; may be repeated")
    ap.add_argument("--depth", type=int, default=None, help="lattice depth (default: the stored depth)")
    ap.add_argument("--straighten", action="store_true", help="also prune every path into waypoints joined by straight segments")
    ap.add_argument("--lookahead", type=int, default=0, help="with --straighten: cells a waypoint looks ahead (0: the whole path)")
    ap.add_argument("--corridor", type=int, default=None, metavar="EXTENT", help="also a chain of free boxes along every path, grown at most EXTENT layers a direction")
    args = ap.parse_args()
    if args.corridor is not None and not 0 <= args.corridor <= 65536:
        sys.exit("--corridor is 0 .. 65536")
    if args.lookahead and not args.straighten:
        sys.exit("--lookahead goes with --straighten")
    if args.lookahead < 0:
        sys.exit("--lookahead is 0 or more")
    rings = args.comfort - args.clearance
    if rings < 0:
        sys.exit("--comfort is at least --clearance")
    ring_cost = [args.penalty * (rings - k) for k in range(rings)] if args.penalty is not None else list(args.ring_cost)
    if len(ring_cost) != rings:
        sys.exit("--ring-cost takes comfort - clearance = %d values" % rings)
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    pool, ws = pkg.Pool(), pkg.Workspace()
    center, edge, stored = pool.load(args.checkpoint)
    depth = stored if args.depth is None else args.depth
    more = dict(straighten=True, max_lookahead=args.lookahead) if args.straighten else {}
    if args.corridor is None:
        plan = pkg.plan_paths(ws, pool, depth, center, edge, args.box, args.goal, args.start, args.clearance, args.comfort, ring_cost, **more)
    else:
        plan = pkg.corridors.plan_corridors(ws, pool, depth, center, edge, args.box, args.goal, args.start, args.clearance, args.comfort,
                                            ring_cost, args.corridor, **more)
    if plan is None:
        sys.exit("the box is empty: a NaN, min > max, or outside the root cube")
    none = np.full(3, -1, np.int32)
    paths = plan["paths"]
    out = dict(cost=plan["cost"], origin=plan["origin"].astype(np.int32), dims=plan["dims"].astype(np.int32),
               goal_cell=none if plan["goal_cell"] is None else plan["goal_cell"],
               start_cells=np.array([none if p["cell"] is None else p["cell"] for p in paths], np.int32).reshape(-1, 3),
               lengths=np.array([p["length"] or 0 for p in paths], np.int32),
               costs=np.array([-1 if p["cost"] is None else p["cost"] for p in paths], np.int32),
               cell_size=plan["cell_size"], depth=depth, center=np.asarray(center, np.float32), edge_length=np.float32(edge),
               clearance_cells=args.clearance, comfort_cells=args.comfort, ring_cost=np.array(ring_cost, np.int32),
               box=np.asarray(args.box, np.float32), goal=np.asarray(args.goal, np.float32), starts=np.asarray(args.start, np.float32))
    for k, p in enumerate(paths):
        out["cells_%d" % k] = p["cells"] if p["cells"] is not None else np.zeros((0, 3), np.int32)
        out["polyline_%d" % k] = p["polyline"] if p["polyline"] is not None else np.zeros((0, 3), np.float64)
    if args.straighten:
        out["lookahead"] = args.lookahead
        out["straight_lengths"] = np.array([p["straight_length"] or 0.0 for p in paths], np.float64)
        for k, p in enumerate(paths):
            out["vertices_%d" % k] = p["vertices"] if p["vertices"] is not None else np.zeros(0, np.int32)
            out["waypoints_%d" % k] = p["waypoints"] if p["waypoints"] is not None else np.zeros((0, 3), np.int32)
            out["waypoint_polyline_%d" % k] = p["waypoint_polyline"] if p["waypoint_polyline"] is not None else np.zeros((0, 3), np.float64)
    if args.corridor is not None:
        out["corridor_extent"] = args.corridor
        out["corridor_gaps"] = np.array([p["gaps"] or 0 for p in paths], np.int32)
        for k, p in enumerate(paths):
            out["boxes_%d" % k] = p["boxes"] if p["boxes"] is not None else np.zeros((0, 6), np.int32)
            out["boxes_m_%d" % k] = p["boxes_m"] if p["boxes_m"] is not None else np.zeros((0, 6), np.float64)
            out["anchors_%d" % k] = p["anchors"] if p["anchors"] is not None else np.zeros(0, np.int32)
    np.savez_compressed(args.out, **out)
    print("depth %d, cells %s + %s, clearance %d, comfort %d, ring cost %s -> %s" % (
        depth, plan["origin"].tolist(), plan["dims"].tolist(), args.clearance, args.comfort, ring_cost, args.out))
    for k, p in enumerate(paths):
        if p["length"] is None:
            print("start %d: no path" % k)
        else:
            print("start %d: %d cells, %.3f m, cost %d" % (k, p["length"], (p["length"] - 1) * plan["cell_size"], p["cost"]))
            if args.straighten:
                print("start %d: %d waypoints, %.3f m" % (k, len(p["vertices"]), p["straight_length"]))
            if args.corridor is not None:
                print("start %d: %d boxes, %d gaps" % (k, len(p["boxes"]), p["gaps"]))


if __name__ == "__main__":
    main()
