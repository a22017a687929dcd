"""The surface mesh of a map (svoslam_extract_surface_mesh, include/svoslam.h): the specification restated on
host words, hand-built pools with their expected arrays written out, invariants of a closed surface on a pool fused by the CPU
oracle, and the PLY writer (host code of the library: runs here).  No GPU.

surface_words below is what the device call must produce; tests/test_gpu_surface.py compares against it bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from util import surface_cloud

FLAG, MASK = 0x40000000, 0x3FFFFFFF

# corners of the face in direction -x +x -y +y -z +z as lattice offsets, counter-clockwise seen from outside
CORNERS = np.array([
    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],
    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],
    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],
    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],
    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],
    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]], dtype=np.int64)
STEP = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], dtype=np.int64)


def occupied_cells(words, depth):
    """(xyz[n,3], node[n]) of the occupied set at `depth`, in ascending cell-key order: level by level, a node stays iff its
    alpha is > 127, and only nodes with the children flag are descended"""
    words = np.asarray(words, dtype=np.uint32)
    w0, w1 = words[0::2].astype(np.int64), words[1::2].astype(np.int64)
    oct_xyz = np.array([(o & 1, (o >> 1) & 1, (o >> 2) & 1) for o in range(8)], dtype=np.int64)
    node, xyz = np.arange(8, dtype=np.int64), oct_xyz.copy()
    for level in range(1, depth + 1):
        keep = (w1[node] >> 24) > 127
        node, xyz = node[keep], xyz[keep]
        if level == depth:
            break
        keep = (w0[node] & FLAG) != 0
        node, xyz = node[keep], xyz[keep]
        child = w0[node] & MASK
        node = (child[:, None] + np.arange(8)[None, :]).reshape(-1)
        xyz = (2 * xyz[:, None, :] + oct_xyz[None, :, :]).reshape(-1, 3)
    return xyz, node


def cell_keys(xyz, depth):
    key = np.ones(xyz.shape[0], dtype=np.int64)
    for level in range(depth - 1, -1, -1):
        key = (key << 3) | ((xyz[:, 0] >> level) & 1) | (((xyz[:, 1] >> level) & 1) << 1) | (((xyz[:, 2] >> level) & 1) << 2)
    return key


def surface_face_masks(words, depth):
    """per occupied cell, in key order: bit d set iff the face in direction d (-x +x -y +y -z +z) is part of the surface"""
    face = exposed_faces(occupied_cells(words, depth)[0], depth)
    return (face * (1 << np.arange(6))).sum(1).astype(np.uint8)


def exposed_faces(xyz, depth):
    n_side = 1 << depth
    code = (xyz[:, 2] * n_side + xyz[:, 1]) * n_side + xyz[:, 0]
    sorted_code = np.sort(code)
    face = np.zeros((xyz.shape[0], 6), dtype=bool)
    for d in range(6):
        nb = xyz + STEP[d]
        inside = ((nb >= 0) & (nb < n_side)).all(1)
        nb_code = (nb[:, 2] * n_side + nb[:, 1]) * n_side + nb[:, 0]
        pos = np.clip(np.searchsorted(sorted_code, nb_code), 0, max(sorted_code.size - 1, 0))
        present = inside & (sorted_code[pos] == nb_code) if sorted_code.size else inside & False
        face[:, d] = ~present
    return face


def surface_lattice(words, depth):
    """(lattice corner of every vertex [nv,3] int64, quads [nf,4] uint32, colours [nf] uint32, cells xyz)"""
    words = np.asarray(words, dtype=np.uint32)
    xyz, node = occupied_cells(words, depth)
    face = exposed_faces(xyz, depth)
    cell, d = np.nonzero(face)                                   # row-major: (cell, direction) ascending
    corners = xyz[cell][:, None, :] + CORNERS[d]                 # [nf, 4, 3]
    s = depth + 1
    vkey = (corners[:, :, 2] << (2 * s)) | (corners[:, :, 1] << s) | corners[:, :, 0]
    uniq, inverse = np.unique(vkey.reshape(-1), return_inverse=True)
    lattice = np.stack([uniq & ((1 << s) - 1), (uniq >> s) & ((1 << s) - 1), uniq >> (2 * s)], 1)
    colors = words[1::2][node][cell].astype(np.uint32)
    return lattice, inverse.reshape(-1, 4).astype(np.uint32), colors, xyz


def lattice_positions(lattice, depth, center, edge):
    """center + (float)(2 i - N) * (edge / (float)N), binary32 operation by operation"""
    n_side = 1 << depth
    step = np.float32(edge) / np.float32(n_side)
    return (np.asarray(center, np.float32)[None, :] + (2 * lattice - n_side).astype(np.float32) * step).astype(np.float32)


def surface_words(words, depth, center, edge):
    """-> (vertices[nv,3] float32, quads[nf,4] uint32, colors[nf] uint32, stats) of the pool words: the specification of
    svoslam_extract_surface_mesh in numpy"""
    lattice, quads, colors, xyz = surface_lattice(words, depth)
    stats = {"cells": int(xyz.shape[0]), "faces": int(quads.shape[0]), "vertices": int(lattice.shape[0])}
    return lattice_positions(lattice, depth, center, edge).reshape(-1, 3), quads.reshape(-1, 4), colors, stats


# ---- hand-built pools ----------------------------------------------------------------------------------------------------
class HandPool:
    """nodes set along octant paths; a tile of 8 zeroed children is appended whenever a path has to go below a node"""

    def __init__(self):
        self.w = [0] * 16

    def children(self, node):
        if not self.w[2 * node] & FLAG:
            self.w[2 * node] = FLAG | (len(self.w) // 2)
            self.w += [0] * 16
        return self.w[2 * node] & MASK

    def put(self, path, colors):
        """path: one octant per level; colors: word1 per level (None leaves the node's word alone).  Returns the last node"""
        base = 0
        for k, (o, c) in enumerate(zip(path, colors)):
            node = base + o
            if c is not None:
                self.w[2 * node + 1] = c
            if k + 1 < len(path):
                base = self.children(node)
        return node

    def words(self):
        return np.array(self.w, dtype=np.uint32)


def path_of(x, y, z, depth):
    return [((x >> l) & 1) | (((y >> l) & 1) << 1) | (((z >> l) & 1) << 2) for l in range(depth - 1, -1, -1)]


def rgba(r, g, b, a):
    return r | (g << 8) | (b << 16) | (a << 24)


OPAQUE = rgba(10, 20, 30, 255)
# an isolated cell: its 8 corners sort as ix + 2 iy + 4 iz, and the six quads are the corner table in those indices
CUBE_QUADS = np.array([[0, 4, 6, 2], [1, 3, 7, 5], [0, 1, 5, 4], [2, 6, 7, 3], [0, 2, 3, 1], [4, 5, 7, 6]], dtype=np.uint32)


def cube_lattice(x, y, z):
    return np.array([(x + dx, y + dy, z + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], dtype=np.int64)


def hand_pools():
    """name -> (words, depth, expected lattice corners, expected quads, expected colours, expected cells)"""
    out = {}
    for o in (0, 7):                                              # one cell at depth 1
        p = HandPool()
        p.put([o], [rgba(1, 2, 3, 200)])
        out["one_cell_octant_%d" % o] = (p.words(), 1, cube_lattice(o & 1, (o >> 1) & 1, o >> 2), CUBE_QUADS,
                                         np.full(6, rgba(1, 2, 3, 200), np.uint32), 1)
    # two cells either side of the level-1 boundary x = 3 | 4 at depth 3: the face between them is not part of the surface
    p = HandPool()
    ca, cb = rgba(200, 0, 0, 255), rgba(0, 0, 200, 128)
    p.put(path_of(3, 2, 5, 3), [OPAQUE, OPAQUE, ca])
    p.put(path_of(4, 2, 5, 3), [OPAQUE, OPAQUE, cb])
    lat = np.array([(x, y, z) for z in (5, 6) for y in (2, 3) for x in (3, 4, 5)], dtype=np.int64)
    quads = np.array([[0, 6, 9, 3], [0, 1, 7, 6], [3, 9, 10, 4], [0, 3, 4, 1], [6, 7, 10, 9],               # cell (3,2,5): all but +x
                      [2, 5, 11, 8], [1, 2, 8, 7], [4, 10, 11, 5], [1, 4, 5, 2], [7, 8, 11, 10]], np.uint32)  # cell (4,2,5): all but -x
    out["two_cells_across_level_1"] = (p.words(), 3, lat, quads, np.array([ca] * 5 + [cb] * 5, np.uint32), 2)
    # a cell in the cube's corner: the faces on the boundary are emitted, lattice coordinate N included
    p = HandPool()
    p.put(path_of(7, 0, 7, 3), [OPAQUE, OPAQUE, OPAQUE])
    out["boundary_cell"] = (p.words(), 3, cube_lattice(7, 0, 7), CUBE_QUADS, np.full(6, OPAQUE, np.uint32), 1)
    # alpha 127 is empty, alpha 128 is occupied: the 128 cell keeps its face towards the 127 sibling
    p = HandPool()
    p.put(path_of(2, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 128)])
    p.put(path_of(3, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 127)])
    out["alpha_127_128"] = (p.words(), 2, cube_lattice(2, 2, 2), CUBE_QUADS, np.full(6, rgba(5, 5, 5, 128), np.uint32), 1)
    # an opaque node under a parent of alpha <= 127 is not a cell (3,3,3 below); its neighbour (4,3,3) is isolated
    p = HandPool()
    p.put(path_of(3, 3, 3, 3), [OPAQUE, rgba(9, 9, 9, 127), OPAQUE])
    p.put(path_of(4, 3, 3, 3), [OPAQUE, OPAQUE, OPAQUE])
    out["opaque_under_transparent"] = (p.words(), 3, cube_lattice(4, 3, 3), CUBE_QUADS, np.full(6, OPAQUE, np.uint32), 1)
    # an opaque CHILDLESS level-2 node (covering x 2..3, y 2..3, z 2..3) contributes nothing at depth 3; (4,3,3) beside it keeps -x
    p = HandPool()
    p.put(path_of(3, 3, 3, 3)[:2], [OPAQUE, OPAQUE])
    p.put(path_of(4, 3, 3, 3), [OPAQUE, OPAQUE, OPAQUE])
    out["childless_above_depth"] = (p.words(), 3, cube_lattice(4, 3, 3), CUBE_QUADS, np.full(6, OPAQUE, np.uint32), 1)
    # a level-d node that has children (transparent ones, even) is still a cell
    p = HandPool()
    p.put(path_of(1, 2, 3, 2) + [5], [OPAQUE, rgba(7, 8, 9, 255), 0])
    out["cell_with_children"] = (p.words(), 2, cube_lattice(1, 2, 3), CUBE_QUADS, np.full(6, rgba(7, 8, 9, 255), np.uint32), 1)
    return out


HAND = hand_pools()
CENTER, EDGE = (0.05, -0.02, 0.01), 1.0


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_pools(name):
    words, depth, lat, quads, colors, cells = HAND[name]
    v, q, c, stats = surface_words(words, depth, CENTER, EDGE)
    assert stats == {"cells": cells, "faces": quads.shape[0], "vertices": lat.shape[0]}
    assert np.array_equal(q, quads) and np.array_equal(c, colors)
    n_side = 1 << depth
    want = np.empty(lat.shape, np.float32)
    for k in range(lat.shape[0]):
        for a in range(3):                                         # scalar by scalar: one division, one product, one sum
            want[k, a] = np.float32(CENTER[a]) + np.float32(2 * int(lat[k, a]) - n_side) * (np.float32(EDGE) / np.float32(n_side))
    assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), want.view(np.uint32))


def test_hand_built_counts_and_positions_spelled_out():
    v, q, c, stats = surface_words(HAND["one_cell_octant_0"][0], 1, CENTER, EDGE)
    assert stats == {"cells": 1, "faces": 6, "vertices": 8}
    lo, mid = np.asarray(CENTER, np.float32) - np.float32(EDGE), np.asarray(CENTER, np.float32)
    assert np.array_equal(v[0], lo) and np.array_equal(v[7], mid)                 # center - edge ... center
    v7 = surface_words(HAND["one_cell_octant_7"][0], 1, CENTER, EDGE)[0]
    assert np.array_equal(v7[0], mid) and np.array_equal(v7[7], mid + np.float32(EDGE))
    assert surface_words(HAND["two_cells_across_level_1"][0], 3, CENTER, EDGE)[3] == {"cells": 2, "faces": 10, "vertices": 12}
    vb = surface_words(HAND["boundary_cell"][0], 3, CENTER, EDGE)[0]
    assert vb[:, 0].max() == np.float32(CENTER[0]) + np.float32(EDGE) and vb[:, 1].min() == np.float32(CENTER[1]) - np.float32(EDGE)
    # shallower than the tree: the level above answers
    assert surface_words(HAND["two_cells_across_level_1"][0], 2, CENTER, EDGE)[3] == {"cells": 2, "faces": 10, "vertices": 12}
    assert surface_words(HAND["childless_above_depth"][0], 2, CENTER, EDGE)[3] == {"cells": 2, "faces": 10, "vertices": 12}
    assert surface_words(np.zeros(16, np.uint32), 4, CENTER, EDGE)[3] == {"cells": 0, "faces": 0, "vertices": 0}


# ---- a fused pool ----------------------------------------------------------------------------------------------------------
DEPTH = 6


@pytest.fixture(scope="module")
def fused(oracle):
    rng = np.random.default_rng(41)
    pts, col = surface_cloud(rng, 15000)
    pool = oracle.Pool()
    for _ in range(2):
        pool.insert_cloud(pts, col, DEPTH, CENTER, EDGE)
    return pool, pool.words()


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
def test_restatement_on_a_fused_pool(fused, depth):
    pool, words = fused
    lattice, quads, colors, xyz = surface_lattice(words, depth)
    keys = cell_keys(xyz, depth)
    assert xyz.shape[0] > 256 and (np.diff(keys) > 0).all()                      # ascending cell keys
    # the cells and their colours are the voxel extraction's
    ce, co = pool.extract(depth, CENTER, EDGE)
    assert ce.shape[0] == xyz.shape[0]
    node = occupied_cells(words, depth)[1]
    w1 = words[1::2][node]
    mine = np.stack([(w1 >> s & 0xFF).astype(np.float32) / np.float32(255.0) for s in (0, 8, 16, 24)], 1)
    assert np.array_equal(mine, co)
    corner = lattice[quads.astype(np.int64)]                                      # [nf, 4, 3]
    e1, e2 = corner[:, 1] - corner[:, 0], corner[:, 3] - corner[:, 0]
    normal = np.cross(e1, e2)
    assert (np.abs(normal).sum(1) == 1).all()                                     # unit squares, axis-aligned
    axis = np.abs(normal).argmax(1)
    sign = normal[np.arange(normal.shape[0]), axis]
    along = corner[np.arange(corner.shape[0]), 0, axis]
    assert (corner[np.arange(corner.shape[0]), :, axis] == along[:, None]).all()  # planar
    # divergence theorem in lattice units: the flux of (x, 0, 0) -- sign of the normal x coordinate along it, over the faces
    # normal to x -- is the enclosed volume, the number of cells; likewise for y and z (so three times that over all faces)
    for a in range(3):
        assert int((sign * along)[axis == a].sum()) == xyz.shape[0]
    # every directed edge occurs as often as its reverse: the surface is closed
    a = quads.astype(np.int64)
    b = np.roll(a, -1, axis=1)
    nv = lattice.shape[0]
    fwd, rev = np.sort((a * nv + b).reshape(-1)), np.sort((b * nv + a).reshape(-1))
    assert np.array_equal(fwd, rev)
    # welded: no duplicate vertex, no unused vertex, ascending vertex keys
    s = depth + 1
    vkey = (lattice[:, 2] << (2 * s)) | (lattice[:, 1] << s) | lattice[:, 0]
    assert (np.diff(vkey) > 0).all()
    assert np.array_equal(np.unique(quads), np.arange(nv))
    v = lattice_positions(lattice, depth, CENTER, EDGE)
    assert np.unique(v.view(np.uint32).reshape(-1, 3), axis=0).shape[0] == nv


# ---- the PLY writer ----------------------------------------------------------------------------------------------------------
def read_ply(path):
    """-> (vertices[n,3] float32, faces: list of index tuples, colours[m,4] uint8) of a binary little-endian PLY as
    svoslam_mesh_write_ply writes it; every header line is checked"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    lines = [ln for ln in lines[2:-1] if not ln.startswith("comment")]
    nv, nf = int(lines[0].split()[2]), int(lines[4].split()[2])
    assert lines == ["element vertex %d" % nv, "property float x", "property float y", "property float z", "element face %d" % nf,
                     "property list uchar uint vertex_indices", "property uchar red", "property uchar green", "property uchar blue",
                     "property uchar alpha"]
    v = np.frombuffer(blob, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    pos = end + 12 * nv
    faces, colors = [], []
    for _ in range(nf):
        k = blob[pos]
        faces.append(tuple(np.frombuffer(blob, dtype="<u4", count=k, offset=pos + 1).tolist()))
        colors.append(tuple(blob[pos + 1 + 4 * k:pos + 5 + 4 * k]))
        pos += 5 + 4 * k
    assert pos == len(blob)
    return v, faces, np.array(colors, dtype=np.uint8).reshape(-1, 4)


def load_pkg():
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    return pkg


def test_library_exports_the_surface_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_extract_surface_mesh", "svoslam_mesh_write_ply"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert [n for n, _ in pkg.SurfaceStats._fields_] == ["cells", "faces", "vertices"] and C.sizeof(pkg.SurfaceStats) == 12
    assert hasattr(pkg, "extract_surface_mesh") and hasattr(pkg, "write_ply")


@pytest.mark.parametrize("name", ["two_cells_across_level_1", "fused"])
def test_write_ply_round_trip(tmp_path, fused, name):
    pkg = load_pkg()
    words, depth = (fused[1], DEPTH) if name == "fused" else HAND[name][:2]
    v, q, c, stats = surface_words(words, depth, CENTER, EDGE)
    rgba8 = np.stack([(c >> s) & 0xFF for s in (0, 8, 16, 24)], 1).astype(np.uint8)
    quad_file, tri_file = tmp_path / "quads.ply", tmp_path / "tris.ply"
    pkg.write_ply(quad_file, v, q, c)
    pkg.write_ply(tri_file, v, q, c, triangulate=True)
    pv, pf, pc = read_ply(quad_file)
    assert np.array_equal(pv.view(np.uint32), v.view(np.uint32))
    assert pf == [tuple(r) for r in q.tolist()] and np.array_equal(pc, rgba8)
    tv, tf, tc = read_ply(tri_file)
    assert np.array_equal(tv.view(np.uint32), v.view(np.uint32))
    want = []
    for r in q.tolist():
        want += [(r[0], r[1], r[2]), (r[0], r[2], r[3])]
    assert tf == want and np.array_equal(tc, np.repeat(rgba8, 2, axis=0))
    assert os.path.getsize(quad_file) == len(open(quad_file, "rb").read()) > 12 * stats["vertices"] + 21 * stats["faces"]


def test_write_ply_empty_mesh_and_refusals(tmp_path):
    pkg = load_pkg()
    empty = tmp_path / "empty.ply"
    pkg.write_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint32), np.zeros(0, np.uint32))
    v, f, c = read_ply(empty)
    assert v.shape == (0, 3) and f == [] and c.shape == (0, 4)
    v, q, c, _ = surface_words(HAND["one_cell_octant_0"][0], 1, CENTER, EDGE)
    with pytest.raises(pkg.SvoslamError, match=r"status -8 \("):                  # SVOSLAM_ERR_IO
        pkg.write_ply(tmp_path / "no_such_directory" / "x.ply", v, q, c)
    bad = q.copy()
    bad[3, 2] = 8                                                               # 8 vertices: indices 0..7
    target = tmp_path / "bad.ply"
    with pytest.raises(pkg.SvoslamError, match=r"status -1 \(invalid argument"):  # SVOSLAM_ERR_INVALID_ARG
        pkg.write_ply(target, v, bad, c)
    assert not target.exists()
    with pytest.raises(ValueError):
        pkg.write_ply(target, v, q, c[:5])
