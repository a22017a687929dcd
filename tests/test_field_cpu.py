"""The distance field of a map region (svoslam_pool_distance_field, svoslam_box_to_cells; include/svoslam.h):
the definition restated as brute force over the occupied set; a second, separable restatement that follows the device's three
passes; the two proven equal on a pool fused by the CPU oracle; the tie to svoslam_pool_nearest_occupied's restatement through
the midpoints of the cells; hand-built pools with every output value written out; and the host call svoslam_box_to_cells against
the plane-by-plane count.  No GPU.

distance_field_words (the definition) and distance_field_separable (for the larger cases) below are what the device call must
produce; tests/test_gpu_field.py compares against them bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from test_query_cpu import F, plane
from test_surface_cpu import CENTER, EDGE, HAND, HandPool, OPAQUE, load_pkg, occupied_cells, path_of, rgba
from test_volume_cpu import (DEPTH, MAX_RADIUS, ROOT_CENTER, ROOT_EDGE, count_cells, fused, nearest_occupied_words,  # noqa: F401
                             seeded_boxes)

I64 = np.int64
NONE = 1 << 30                                                          # "nothing within reach so far" of the separable passes
FAR = np.iinfo(I64).max                                                 # no occupied cell at all


# ---- the specification, restated -------------------------------------------------------------------------------------------
def region_cells(origin, dims):
    """[nz * ny * nx, 3] the cells of the region in output order: x fastest"""
    z, y, x = np.meshgrid(*[np.arange(origin[a], origin[a] + dims[a], dtype=I64) for a in (2, 1, 0)], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)


def min_dist2_to(cells, q, chunk=1 << 22):
    """per row of q[n,3] the minimum over cells[m,3] of the squared distance (FAR when there are no cells): chunked brute force"""
    out = np.full(q.shape[0], FAR, I64)
    if cells.shape[0] == 0:
        return out
    rows = max(1, chunk // cells.shape[0])
    c, q = cells.astype(np.int32), q.astype(np.int32)                   # 3 * 65535^2 overflows an int32: the sum is taken in int64
    for s in range(0, q.shape[0], rows):
        d2 = np.zeros((min(rows, q.shape[0] - s), c.shape[0]), I64)
        for a in range(3):
            d = q[s:s + rows, None, a] - c[None, :, a]
            d2 += d.astype(I64) * d
        out[s:s + rows] = d2.min(1)
    return out


def distance_field_words(words, depth, origin, dims, radius, cells=None):
    """-> int32 [nz, ny, nx]: svoslam_pool_distance_field by its definition -- for every cell of the region the minimum squared
    distance over ALL occupied cells of the root, -1 where that exceeds radius^2.  (`cells`: the occupied set to use instead of
    occupied_cells(words, depth), for what the field would be without some of them.)"""
    assert 0 <= radius <= MAX_RADIUS and all(v >= 0 for v in dims)
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) for a in range(3))
    if cells is None:
        cells = occupied_cells(words, depth)[0]
    near = min_dist2_to(cells, region_cells(origin, dims))
    return np.where(near <= radius * radius, near, -1).astype(np.int32).reshape(dims[2], dims[1], dims[0])


def _pass(g, axis, off, out_len, radius):
    """g'(i) = min over |k| <= radius of g(i + off + k) + k^2 along `axis`, i in 0 .. out_len; above radius^2: NONE"""
    g = np.moveaxis(g, axis, 0)
    in_len = g.shape[0]
    out = np.full((out_len,) + g.shape[1:], NONE, I64)
    for k in range(-radius, radius + 1):
        lo, hi = max(0, -(off + k)), min(out_len, in_len - off - k)
        if lo < hi:
            out[lo:hi] = np.minimum(out[lo:hi], g[lo + off + k:hi + off + k] + k * k)
    return np.moveaxis(np.where(out <= radius * radius, out, NONE), 0, axis)


def distance_field_separable(words, depth, origin, dims, radius):
    """the same field by the device's route: the occupancy of the region inflated by `radius` and clipped to the root, the distance
    to the nearest occupied cell along x (scans from both sides), then the y and the z pass"""
    n_side = 1 << depth
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    if (n == 0).any():
        return np.zeros((dims[2], dims[1], dims[0]), np.int32)
    lo, hi = np.maximum(o - radius, 0), np.minimum(o + n + radius, n_side)
    xyz = occupied_cells(words, depth)[0]
    c = xyz[((xyz >= lo) & (xyz < hi)).all(1)] - lo
    occ = np.zeros(tuple(hi - lo)[::-1], bool)
    occ[c[:, 2], c[:, 1], c[:, 0]] = True
    idx = np.arange(occ.shape[2], dtype=I64)
    below = np.maximum.accumulate(np.where(occ, idx, -NONE), axis=2)             # the nearest occupied x at or below
    above = np.minimum.accumulate(np.where(occ, idx, NONE)[:, :, ::-1], axis=2)[:, :, ::-1]
    dist = np.minimum(idx - below, above - idx)
    off = o - lo
    g = np.where(dist <= radius, dist * dist, NONE)[:, :, off[0]:off[0] + n[0]]
    g = _pass(g, 1, int(off[1]), int(n[1]), radius)
    g = _pass(g, 0, int(off[2]), int(n[2]), radius)
    return np.where(g <= radius * radius, g, -1).astype(np.int32)


def midpoints(depth, center, edge, origin, dims):
    """[nz * ny * nx, 3] float32: (P(k) + P(k + 1)) / 2 in binary32 for every cell of the region, in output order"""
    n_side = 1 << depth
    h = F(edge) / F(n_side)
    q = region_cells(origin, dims)
    return np.stack([((plane(center[a], q[:, a], n_side, h) + plane(center[a], q[:, a] + 1, n_side, h)) / F(2)).astype(F)
                     for a in range(3)], 1)


# ---- a pool fused by the oracle: the two restatements, and the existing call's -------------------------------------------------
RADII = (0, 1, 3, 64)


def fused_regions(depth):
    """name -> (origin, dims) at `depth` (the cloud fills the low quarter of each axis of test_volume_cpu's root)"""
    n = 1 << depth
    far = (37 * n) // 64                                                # x 37 at depth 6: inside a row word, beyond the cloud
    out = {"whole_root": ((0, 0, 0), (n, n, n)),
           "low_corner": ((0, 0, 0), (n // 2 + 1, n // 4 - 1, 5)),      # touches the three low faces, cuts through the cloud
           "high_corner": ((n - n // 4 - 1, n - 3, n - n // 2), (n // 4 + 1, 3, n // 2)),
           "one_cell": ((n // 8, n // 8 + 1, n // 8), (1, 1, 1)),
           "offset_37": ((far, n // 16, n // 8), (min(20, n - far), 7, 3))}
    return out


def truncated(full, radius):
    return np.where((full >= 0) & (full <= radius * radius), full, -1).astype(np.int32)


@pytest.fixture(scope="module")
def fields(fused):
    """(depth, region name, radius, alone=False) -> the field by its definition, computed once per (depth, region) with the largest
    radius and truncated per radius; `alone`: the field the region would have if the occupied cells outside it did not exist"""
    words, _ = fused
    cache = {}

    def get(depth, name, radius, alone=False):
        key = (depth, name, alone and name != "whole_root")
        if key not in cache:
            origin, dims = fused_regions(depth)[name]
            xyz = occupied_cells(words, depth)[0]
            inside = ((xyz >= np.asarray(origin)) & (xyz < np.asarray(origin) + np.asarray(dims))).all(1)
            cache[key] = distance_field_words(words, depth, origin, dims, MAX_RADIUS, cells=xyz[inside] if key[2] else None)
        return truncated(cache[key], radius)
    return get


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_separable_passes_are_the_definition(fused, fields, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    assert all(0 <= origin[a] and dims[a] >= 1 and origin[a] + dims[a] <= (1 << depth) for a in range(3))
    for radius in RADII:
        want = fields(depth, region, radius)
        assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
        if region == "one_cell":                                        # the truncation of the cache is the definition's own
            assert np.array_equal(want, distance_field_words(words, depth, origin, dims, radius))
        assert np.array_equal(distance_field_separable(words, depth, origin, dims, radius), want), radius


@pytest.mark.parametrize("radius", [3, 64])
def test_the_fused_cases_are_not_empty(fused, fields, radius):
    """the conditions a comparison needs in order not to pass empty, on the definition's result at depth 6 (at depth 4 the cloud
    has fewer than 100 cells and, 3 * 15^2 < 64^2, nothing is farther than 64 cells from anything)"""
    zero = positive = none = from_outside = 0
    for name in fused_regions(DEPTH):
        f = fields(DEPTH, name, radius)
        zero, positive, none = zero + int((f == 0).sum()), positive + int((f > 0).sum()), none + int((f == -1).sum())
        from_outside += int((f != fields(DEPTH, name, radius, alone=True)).sum())
    assert zero > 100 and positive > 100 and none > 20 and from_outside >= 1, (zero, positive, none, from_outside)


def sample_cells(origin, dims, count, seed):
    """indices into the region's output order: all of it when small, else its eight corners, a face of the border and a seeded
    sample"""
    total = dims[0] * dims[1] * dims[2]
    if total <= count:
        return np.arange(total)
    rng = np.random.default_rng(seed)
    q = region_cells((0, 0, 0), dims)
    border = np.nonzero(((q == 0) | (q == np.asarray(dims) - 1)).any(1))[0]
    corners = np.nonzero(((q == 0) | (q == np.asarray(dims) - 1)).all(1))[0]
    pick = np.concatenate([corners, rng.choice(border, min(border.size, count // 2), replace=False),
                           rng.choice(total, count // 2, replace=False)])
    return np.unique(pick)


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
def test_the_field_is_nearest_occupied_at_the_cell_midpoints(fused, fields, depth):
    """an independent route: the existing call's restatement (the walk, from the float midpoint of each cell) gives the field's
    value, also where the nearest occupied cell lies outside the region"""
    words, _ = fused
    from_outside = 0
    for k, (name, (origin, dims)) in enumerate(sorted(fused_regions(depth).items())):
        at = sample_cells(origin, dims, 500, 60 + k)
        points = midpoints(depth, ROOT_CENTER, ROOT_EDGE, origin, dims)[at]
        assert np.array_equal(count_cells(ROOT_CENTER, ROOT_EDGE, depth, points, False), region_cells(origin, dims)[at])
        for radius in RADII:
            want = fields(depth, name, radius).reshape(-1)[at]
            got = nearest_occupied_words(words, depth, ROOT_CENTER, ROOT_EDGE, points, radius)["dist2"]
            assert np.array_equal(got, want), (name, radius)
            from_outside += int((fields(depth, name, radius, alone=True).reshape(-1)[at] != want).sum())
    assert from_outside >= 1


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def one_cell_field(c, origin, dims, radius):
    """the field of ONE occupied cell c, by the formula itself: (cx - qx)^2 + (cy - qy)^2 + (cz - qz)^2, -1 above radius^2"""
    out = np.zeros((dims[2], dims[1], dims[0]), np.int32)
    for z in range(dims[2]):
        for y in range(dims[1]):
            for x in range(dims[0]):
                d2 = (c[0] - origin[0] - x) ** 2 + (c[1] - origin[1] - y) ** 2 + (c[2] - origin[2] - z) ** 2
                out[z, y, x] = d2 if d2 <= radius * radius else -1
    return out


def field_cases():
    """name -> (words, depth, origin, dims, radius, expected int32 [nz, ny, nx])"""
    out = {}
    # one leaf at depth 1, 2 and 3 (test_volume_cpu's), the whole root
    leaves = {1: (1, 0, 1), 2: (2, 1, 3), 3: (5, 2, 6)}
    pools = {}
    for depth, xyz in leaves.items():
        pool = HandPool()
        pool.put(path_of(*xyz, depth), [OPAQUE] * (depth - 1) + [rgba(40 + depth, 2, 3, 255)])
        pools[depth] = pool.words()
    n = -1
    out["one_leaf_depth_1"] = (pools[1], 1, (0, 0, 0), (2, 2, 2), 1,                  # (1,0,1): [z][y][x]
                               np.array([[[n, 1], [n, n]], [[1, 0], [n, 1]]], np.int32))
    out["one_leaf_depth_1_radius_2"] = (pools[1], 1, (0, 0, 0), (2, 2, 2), 2, np.array([[[2, 1], [3, 2]], [[1, 0], [2, 1]]], np.int32))
    out["one_leaf_depth_2"] = (pools[2], 2, (0, 0, 0), (4, 4, 4), 2,                  # (2,1,3)
                               np.array([[[n, n, n, n], [n, n, n, n], [n, n, n, n], [n, n, n, n]],
                                         [[n, n, n, n], [n, n, 4, n], [n, n, n, n], [n, n, n, n]],
                                         [[n, 3, 2, 3], [n, 2, 1, 2], [n, 3, 2, 3], [n, n, n, n]],
                                         [[n, 2, 1, 2], [4, 1, 0, 1], [n, 2, 1, 2], [n, n, 4, n]]], np.int32))
    out["one_leaf_depth_3"] = (pools[3], 3, (0, 0, 0), (8, 8, 8), 4, one_cell_field(leaves[3], (0, 0, 0), (8, 8, 8), 4))
    # R = 0: the occupied cells themselves
    want = np.full((4, 4, 4), -1, np.int32)
    want[3, 1, 2] = 0
    out["radius_0"] = (pools[2], 2, (0, 0, 0), (4, 4, 4), 0, want)
    # a cell at offset (3, 4, 0) from the only occupied one: 25 = 5^2 exactly; R = 5 takes it, R = 4 does not
    pool = HandPool()
    pool.put(path_of(1, 1, 5, 3), [OPAQUE] * 3)
    out["offset_3_4_0_radius_5"] = (pool.words(), 3, (4, 5, 5), (1, 1, 1), 5, np.array([[[25]]], np.int32))
    out["offset_3_4_0_radius_4"] = (pool.words(), 3, (4, 5, 5), (1, 1, 1), 4, np.array([[[-1]]], np.int32))
    # the occupied cell two cells outside the region x, y, z 3..4 of depth 3, on each of its six sides, R = 3:
    # -x: (1,3,3) -> for (x, y, z): (x - 1)^2 + (y - 3)^2 + (z - 3)^2, -1 above 9
    sides = {"minus_x": ((1, 3, 3), [[[4, 9], [5, n]], [[5, n], [6, n]]]), "plus_x": ((6, 3, 3), [[[9, 4], [n, 5]], [[n, 5], [n, 6]]]),
             "minus_y": ((3, 1, 3), [[[4, 5], [9, n]], [[5, 6], [n, n]]]), "plus_y": ((3, 6, 3), [[[9, n], [4, 5]], [[n, n], [5, 6]]]),
             "minus_z": ((3, 3, 1), [[[4, 5], [5, 6]], [[9, n], [n, n]]]), "plus_z": ((3, 3, 6), [[[9, n], [n, n]], [[4, 5], [5, 6]]])}
    for name, (xyz, want) in sides.items():
        pool = HandPool()
        pool.put(path_of(*xyz, 3), [OPAQUE] * 3)
        assert np.array_equal(np.array(want, np.int32), one_cell_field(xyz, (3, 3, 3), (2, 2, 2), 3))
        out["outside_the_region_%s" % name] = (pool.words(), 3, (3, 3, 3), (2, 2, 2), 3, np.array(want, np.int32))
    # regions in the root's corners: the inflation by R = 2 is clipped at three faces
    pool = HandPool()
    pool.put(path_of(0, 0, 0, 2), [OPAQUE] * 2)
    pool.put(path_of(3, 3, 3, 2), [OPAQUE] * 2)
    out["root_corner_low"] = (pool.words(), 2, (0, 0, 0), (2, 2, 2), 2, np.array([[[0, 1], [1, 2]], [[1, 2], [2, 3]]], np.int32))
    out["root_corner_high"] = (pool.words(), 2, (2, 2, 2), (2, 2, 2), 2, np.array([[[3, 2], [2, 1]], [[2, 1], [1, 0]]], np.int32))
    # alpha 127 beside 128 at depth 2: (2,2,2) is occupied, (3,2,2) is not
    out["alpha_127_128"] = (HAND["alpha_127_128"][0], 2, (0, 2, 2), (4, 1, 1), 3, np.array([[[4, 1, 0, 1]]], np.int32))
    # a saturated CHILDLESS level-2 node over x, y, z 2..3 contributes nothing at depth 3: only (4,3,3) is occupied
    out["childless_above_depth"] = (HAND["childless_above_depth"][0], 3, (0, 3, 3), (8, 1, 1), 8,
                                    np.array([[[16, 9, 4, 1, 0, 1, 4, 9]]], np.int32))
    # d one below the leaf depth: the leaf (5,2,6) of depth 3 is cell (2,1,3) at depth 2 (the mip alpha: the path is opaque)
    out["one_level_above_the_leaf"] = (pools[3], 2, (0, 0, 0), (4, 4, 4), 4, one_cell_field((2, 1, 3), (0, 0, 0), (4, 4, 4), 4))
    # an empty pool
    out["empty_pool"] = (HandPool().words(), 2, (0, 0, 0), (4, 4, 4), 2, np.full((4, 4, 4), -1, np.int32))
    return out


FIELD_CASES = field_cases()


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, radius, want = FIELD_CASES[name]
    assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
    for restatement in (distance_field_words, distance_field_separable):
        got = restatement(words, depth, origin, dims, radius)
        assert got.dtype == np.int32 and np.array_equal(got, want), (restatement.__name__, got.tolist())
        if depth > 1:                                                   # the level above, from the same words
            up = ([v // 2 for v in origin], [(origin[a] + dims[a] + 1) // 2 - origin[a] // 2 for a in range(3)])
            assert np.array_equal(distance_field_separable(words, depth - 1, *up, radius),
                                  distance_field_words(words, depth - 1, *up, radius))


def test_a_zero_dimension_is_an_empty_field():
    words = FIELD_CASES["one_leaf_depth_2"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        for restatement in (distance_field_words, distance_field_separable):
            got = restatement(words, 2, (0, 0, 0), dims, 2)
            assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32


# ---- svoslam_box_to_cells: host code of the library, runs here --------------------------------------------------------------------
def lattice_boxes(depth):
    """boxes whose faces lie ON lattice planes (a max face on a plane does not take in the cell beyond, a min face does), point
    boxes on planes, the whole root from plane 0 to plane N, and a NaN, an inverted and two outside boxes"""
    n_side = 1 << depth
    h = F(ROOT_EDGE) / F(n_side)
    rng = np.random.default_rng(31)
    k = np.sort(rng.integers(0, n_side + 1, (120, 2, 3)), axis=1)
    boxes = np.concatenate([np.stack([plane(ROOT_CENTER[a], k[:, 0, a], n_side, h) for a in range(3)], 1),
                            np.stack([plane(ROOT_CENTER[a], k[:, 1, a], n_side, h) for a in range(3)], 1)], 1).astype(F)
    lo_face, hi_face = [float(plane(ROOT_CENTER[a], 0, n_side, h)) for a in range(3)], [float(plane(ROOT_CENTER[a], n_side, n_side, h)) for a in range(3)]
    inf = float("inf")
    extra = np.array([lo_face + hi_face, [-inf] * 3 + [inf] * 3, lo_face + lo_face, hi_face + hi_face,
                      [np.nan] + lo_face[1:] + hi_face, hi_face + lo_face,
                      [-inf] * 3 + [float(np.nextafter(F(lo_face[0]), F(-inf)))] + hi_face[1:],
                      lo_face[:1] + [float(np.nextafter(F(hi_face[1]), F(inf)))] + lo_face[2:] + [inf] * 3], F)
    return np.concatenate([boxes, extra])


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2, 1])
def test_box_to_cells_is_count_boxes_box_to_cells(fused, depth):
    """lo = c(min), hi = max(lo, strict c(max)) with the planes compared one by one (test_volume_cpu.count_cells), and `empty`,
    bit for bit: this pins the host arithmetic to binary32 with nothing fused"""
    pkg = load_pkg()
    _, pts = fused
    boxes = np.concatenate([seeded_boxes(pts), lattice_boxes(depth)])
    n_side = 1 << depth
    h = F(ROOT_EDGE) / F(n_side)
    c = np.asarray(ROOT_CENTER, F)
    p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
    mn, mx = boxes[:, :3], boxes[:, 3:]
    with np.errstate(all="ignore"):
        empty = (~(mn <= mx) | (mx < p0[None, :]) | (mn > pn[None, :])).any(1)
    lo = count_cells(ROOT_CENTER, ROOT_EDGE, depth, mn, False)
    hi = np.maximum(lo, count_cells(ROOT_CENTER, ROOT_EDGE, depth, mx, True))
    assert empty.sum() > 5 and (~empty).sum() > 300 and (hi > lo).any(1).sum() > 100
    L = C.CDLL(pkg.LIB_PATH)
    fn = L.svoslam_box_to_cells
    fn.restype, fn.argtypes = pkg.SIGNATURES["svoslam_box_to_cells"]
    for k in range(boxes.shape[0]):
        got_lo, got_hi, got_empty = (C.c_int32 * 3)(), (C.c_int32 * 3)(), C.c_int32(-1)
        assert fn(depth, pkg._fa(ROOT_CENTER, 3), ROOT_EDGE, pkg._fa(boxes[k], 6), got_lo, got_hi, C.byref(got_empty)) == 0
        assert (got_lo[:], got_hi[:], got_empty.value) == (lo[k].tolist(), hi[k].tolist(), int(empty[k])), (k, boxes[k])
        cells = pkg.box_to_cells(depth, ROOT_CENTER, ROOT_EDGE, boxes[k])
        assert (cells is None) == bool(empty[k])
        if cells is not None:
            assert cells[0].tolist() == lo[k].tolist() and cells[1].tolist() == hi[k].tolist()
    # argument errors
    ctr, box, i3, e = pkg._fa(ROOT_CENTER, 3), pkg._fa(boxes[0], 6), (C.c_int32 * 3)(), C.c_int32(0)
    assert fn(0, ctr, 1.0, box, i3, i3, C.byref(e)) == -1 and fn(17, ctr, 1.0, box, i3, i3, C.byref(e)) == -1
    assert fn(5, ctr, 0.0, box, i3, i3, C.byref(e)) == -1 and fn(5, ctr, float("nan"), box, i3, i3, C.byref(e)) == -1
    assert fn(5, None, 1.0, box, i3, i3, C.byref(e)) == -1 and fn(5, ctr, 1.0, None, i3, i3, C.byref(e)) == -1
    assert fn(5, ctr, 1.0, box, None, i3, C.byref(e)) == -1 and fn(5, ctr, 1.0, box, i3, None, C.byref(e)) == -1
    assert fn(5, ctr, 1.0, box, i3, i3, None) == -1 and fn(5, ctr, 1.0, box, i3, i3, C.byref(e)) == 0


def test_library_exports_the_field_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_distance_field", "svoslam_box_to_cells"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "distance_field") and hasattr(pkg, "box_to_cells")
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_distance_field(" in header and "int svoslam_box_to_cells(" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header and "#define SVOSLAM_MAX_RADIUS_CELLS %d" % MAX_RADIUS in header
