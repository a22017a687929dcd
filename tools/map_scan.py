"""A simulated spinning range sensor in a saved map (svoslam_pool_save checkpoint), on one MI355X.

    python tools/map_scan.py CHECKPOINT OUT.npy --origin x y z [--az A] [--el E] [--fov-el deg] [--t-max m]

A x E rays leave one origin -- A azimuths round the full circle about the y axis, E elevations spread over --fov-el degrees about
the horizontal -- and are cast into the map at its stored depth with svoslam_pool_cast_rays (exact traversal of the occupied
cells: nothing thin is jumped).  OUT.npy holds a structured array [E, A] with the fields range (metres along the unit ray; inf =
nothing within --t-max), cell (x | y << 16 | z << 32 | face << 48) and color (the hit node's colour word R | G << 8 | B << 16 |
A << 24).  Prints how many rays hit and the nearest and farthest range."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scan_rays(origin, n_az, n_el, fov_el_deg):
    """[n_el * n_az, 6] float32: elevation-major, unit directions"""
    az = (np.arange(n_az) / n_az) * 2.0 * np.pi
    half = np.radians(fov_el_deg) / 2.0
    el = np.linspace(-half, half, n_el) if n_el > 1 else np.zeros(1)
    el, az = np.meshgrid(el, az, indexing="ij")
    v = np.stack([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)], -1).reshape(-1, 3)
    return np.concatenate([np.tile(np.asarray(origin, np.float64), (v.shape[0], 1)), v], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--origin", type=float, nargs=3, required=True, metavar=("X", "Y", "Z"))
    ap.add_argument("--az", type=int, default=1024, help="azimuth steps round the circle")
    ap.add_argument("--el", type=int, default=32, help="elevation rings")
    ap.add_argument("--fov-el", type=float, default=30.0, help="vertical field of view in degrees")
    ap.add_argument("--t-max", type=float, default=None, help="range limit in metres (default: none)")
    args = ap.parse_args()
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    pool = pkg.Pool()
    center, edge, depth = pool.load(args.checkpoint)
    rays = scan_rays(args.origin, args.az, args.el, args.fov_el)
    t_max = None if args.t_max is None else np.full(rays.shape[0], args.t_max, np.float32)
    res = pkg.cast_rays(pool, depth, center, edge, rays, t_max, outputs=("t", "cell", "color"))
    out = np.empty((args.el, args.az), dtype=[("range", np.float32), ("cell", np.uint64), ("color", np.uint32)])
    out["range"], out["cell"], out["color"] = (res[k].reshape(args.el, args.az) for k in ("t", "cell", "color"))
    np.save(args.out, out)
    hit = np.isfinite(out["range"])
    print("depth %d: %d x %d rays, %d hit%s -> %s" % (
        depth, args.az, args.el, int(hit.sum()),
        ", range %.3f .. %.3f m" % (out["range"][hit].min(), out["range"][hit].max()) if hit.any() else "", args.out))


if __name__ == "__main__":
    main()
