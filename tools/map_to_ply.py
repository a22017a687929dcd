"""A saved map (svoslam_pool_save checkpoint) as a surface mesh in a PLY file, on one MI355X.

    python tools/map_to_ply.py CHECKPOINT OUT.ply [--depth D] [--triangulate]

Loads the checkpoint (Pool.load), extracts the surface of the occupied cells at depth D (default: the depth stored in the
checkpoint; smaller gives a coarser surface from the mip levels) with svoslam_extract_surface_mesh and writes it with
svoslam_mesh_write_ply: welded vertices, one coloured quad per exposed cell face, or two triangles per quad with --triangulate.
Prints the numbers of cells, faces and vertices and the size of the file."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--depth", type=int, default=0, help="extraction depth (default: the checkpoint's)")
    ap.add_argument("--triangulate", action="store_true", help="two triangles per quad")
    args = ap.parse_args()
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    ws, pool = pkg.Workspace(), pkg.Pool()
    center, edge, depth = pool.load(args.checkpoint)
    if args.depth > 0:
        depth = args.depth
    vertices, quads, colors, stats = pkg.extract_surface_mesh(ws, pool, depth, center, edge)
    pkg.write_ply(args.out, vertices, quads, colors, triangulate=args.triangulate)
    print("depth %d: %d cells, %d faces, %d vertices -> %s (%d bytes%s)" % (
        depth, stats["cells"], stats["faces"], stats["vertices"], args.out, os.path.getsize(args.out),
        ", triangulated" if args.triangulate else ""))


if __name__ == "__main__":
    main()
