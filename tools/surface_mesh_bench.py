"""What svoslam_extract_surface_mesh costs on one MI355X, beside the cube-per-voxel mesh it replaces as a hand-over format.

    python tools/surface_mesh_bench.py [--frames 20] [--out profiles/surface_mesh.txt]

Fuses the first --frames frames of the synthetic stream (640x480, depth 12, root cube of BASELINE config 3) with the corrected
tracker, then on that pool, once each after one warm-up call (a record, not a gate):

  surface   cells / faces / vertices, output bytes (12 per vertex, 16 + 4 per face), and the HIP-event time of its three stages
            (svoslam_stage_timing: surface_bfs, surface_faces, surface_weld; the readbacks between their launches included) and the
            wall clock of the blocking call
  cubes     svoslam_extract_voxel_grid + svoslam_voxel_grid_to_mesh with a unit cube mesh (24 vertices, 36 indices): wall clock of
            the two blocking calls and the bytes of the four output arrays
"""
import argparse
import ctypes as C
import datetime
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cube_mesh():
    """a cube of half edge 1 with per-face vertices: 24 x 3 positions and normals, 36 indices"""
    v, n, idx = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            base = len(v)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0.0, 0.0, 0.0]
                p[axis], p[u], p[w] = sign, a, b
                v.append(p)
                nn = [0.0, 0.0, 0.0]
                nn[axis] = sign
                n.append(nn)
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return np.array(v, np.float32).reshape(-1), np.array(idx, np.int32), np.array(n, np.float32).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    assert torch.cuda.is_available(), "needs a gfx950 device"
    w, h, depth, center, edge = 640, 480, 12, (0.0, 1.5, 0.0), 4.096
    P = pl.SlamPipeline(w, h, depth, center, edge, strict_reference=False)
    ks = list(range(args.frames))
    frames = [synth.render_frame(k, w, h, device="cuda") for k in ks]
    P.run_stream([f[0] for f in frames], [f[1] for f in frames], ks, [pl.ground_truth_view(k, synth) for k in ks])
    torch.cuda.synchronize()
    ws, pool = pkg.Workspace(), P.pool
    nodes = pool.size
    stages = (("bfs", pkg.STAGE_SURFACE_BFS), ("faces", pkg.STAGE_SURFACE_FACES), ("weld", pkg.STAGE_SURFACE_WELD))
    pkg.extract_surface_mesh(ws, pool, depth, center, edge)          # warm-up: the workspace's buffers are allocated here
    pkg.stage_timing([s for _, s in stages])
    try:
        # the library call alone (the binding's copies to the host are not part of it)
        pv, pq, pc, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), pkg.SurfaceStats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pkg.check(pkg.lib().svoslam_extract_surface_mesh(ws._h, C.byref(pool._p), depth, pkg._fa(center, 3), float(edge), C.byref(pv),
                                                         C.byref(pq), C.byref(pc), C.byref(st), pkg._stream()))
        surface_ms = (time.perf_counter() - t0) * 1e3
        stage_ms = {name: pkg.stage_timing_read(s) for name, s in stages}
        for p in (pv, pq, pc):
            pkg.lib().svoslam_free(p)
    finally:
        pkg.stage_timing([])
    surface_bytes = 12 * st.vertices + 20 * st.faces
    # the parent's way: voxel list, then one cube per voxel
    cv, ci, cn = cube_mesh()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pc_, pk_, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    pkg.check(pkg.lib().svoslam_extract_voxel_grid(ws._h, C.byref(pool._p), depth, pkg._fa(center, 3), float(edge), C.byref(pc_),
                                                   C.byref(pk_), C.byref(n), pkg._stream()))
    grid_ms = (time.perf_counter() - t0) * 1e3
    nvox = int(n.value)
    cube_bytes = nvox * (3 * cv.size * 4 + ci.size * 4)
    assert nvox * ci.size <= 0x7FFFFFFF, "svoslam_voxel_grid_to_mesh takes at most (2^31 - 1) / 36 voxels of this cube"
    vbo = torch.empty(nvox * cv.size, dtype=torch.float32, device="cuda")
    nbo, cbo = torch.empty_like(vbo), torch.empty_like(vbo)
    ibo = torch.empty(nvox * ci.size, dtype=torch.int32, device="cuda")
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pkg.check(pkg.lib().svoslam_voxel_grid_to_mesh(ws._h, pc_, pk_, nvox, float(edge) / (1 << depth), cv.ctypes.data_as(f32p), cv.size,
                                                   ci.ctypes.data_as(i32p), ci.size, cn.ctypes.data_as(f32p), pkg._ptr(vbo), pkg._ptr(ibo),
                                                   pkg._ptr(nbo), pkg._ptr(cbo), pkg._stream()))
    cubes_ms = (time.perf_counter() - t0) * 1e3
    pkg.lib().svoslam_free(pc_)
    pkg.lib().svoslam_free(pk_)
    lines = [
        "surface mesh of a map: tools/surface_mesh_bench.py --frames %d   (%s, %s; measured once)" % (
            args.frames, pkg.device_arch(), datetime.date.today().isoformat()),
        "map: %d frames of the synthetic stream, %dx%d, depth %d, corrected tracker: %d nodes" % (args.frames, w, h, depth, nodes),
        "",
        "svoslam_extract_surface_mesh at depth %d" % depth,
        "  cells %d   faces %d   vertices %d" % (st.cells, st.faces, st.vertices),
        "  output bytes %d  (12 per vertex, 16 + 4 per face)" % surface_bytes,
    ] + ["  %-6s %9.3f ms  (HIP events, %d bracket%s)" % (name, stage_ms[name][0], stage_ms[name][1], "" if stage_ms[name][1] == 1 else "s")
         for name, _ in stages] + [
        "  call   %9.3f ms  (wall clock of the blocking call: the three stages, output allocation, host work between them)" % surface_ms,
        "",
        "svoslam_extract_voxel_grid + svoslam_voxel_grid_to_mesh (24-vertex cube, 36 indices) on the same pool",
        "  voxels %d" % nvox,
        "  output bytes %d  (%d per voxel: positions, normals, colours, indices)" % (cube_bytes, cube_bytes // max(nvox, 1)),
        "  voxel grid %9.3f ms   cubes %9.3f ms  (wall clock of the blocking calls; the outputs of the second are allocated before)" % (
            grid_ms, cubes_ms),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
