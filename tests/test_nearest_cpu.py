"""The nearest-cell field of a map region (svoslam_pool_nearest_field; include/svoslam.h): the definition
restated as brute force with the (z, y, x) tie rule; a second, separable restatement that keeps one argmin per pass and follows
the three indices; the two proven equal on a pool fused by the CPU oracle, for both target sets, and on hand-built pools with
every value written out; the ties to svoslam_pool_distance_field's and svoslam_pool_nearest_occupied's restatements.  No GPU.

nearest_field_words (the definition) and nearest_field_separable below are what the device call must produce;
tests/test_gpu_nearest.py compares against them bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from test_field_cpu import NONE, RADII, distance_field_words, fused_regions, midpoints, region_cells, sample_cells
from test_reach_cpu import cells_pool
from test_surface_cpu import HandPool, OPAQUE, load_pkg, occupied_cells, path_of, rgba
from test_volume_cpu import DEPTH, MAX_RADIUS, ROOT_CENTER, ROOT_EDGE, fused, nearest_occupied_words  # noqa: F401

I64 = np.int64
OCCUPIED, FREE = 0, 1                                                   # include/svoslam.h SVOSLAM_NEAREST_*
NO_CELL = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the specification, restated -------------------------------------------------------------------------------------------
def pack(xyz):
    xyz = np.asarray(xyz, I64)
    return (xyz[..., 0] | (xyz[..., 1] << 16) | (xyz[..., 2] << 32)).astype(np.uint64)


def unpack(cell):
    """uint64 [...] -> int64 [..., 3], -1 where the cell is all ones"""
    c = np.asarray(cell, np.uint64)
    xyz = np.stack([(c >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32)], -1).astype(I64)
    return np.where((c == NO_CELL)[..., None], -1, xyz)


def target_cells(words, depth, which):
    """the target set A in (z, y, x) order -- z slowest, x fastest -- and the level-`depth` node of each cell (-1 for a free one)"""
    xyz, node = occupied_cells(words, depth)
    n_side = 1 << depth
    code = (xyz[:, 2] * n_side + xyz[:, 1]) * n_side + xyz[:, 0]
    if which == FREE:
        free = np.ones(n_side ** 3, bool)
        free[code] = False
        code = np.nonzero(free)[0]
        return np.stack([code % n_side, (code // n_side) % n_side, code // (n_side * n_side)], 1).astype(I64), np.full(code.size, -1, I64)
    order = np.argsort(code)
    return xyz[order].astype(I64), node[order].astype(I64)


def nearest_in(cells, q, chunk=1 << 22):
    """per row of q[n,3]: (the minimum over cells[m,3] of the squared distance, the FIRST row of `cells` that attains it) -- the
    tie rule in one line, for cells in (z, y, x) order.  (-1, -1) when there are no cells.  Chunked brute force."""
    best, at = np.full(q.shape[0], -1, I64), np.full(q.shape[0], -1, I64)
    if cells.shape[0] == 0 or q.shape[0] == 0:
        return best, at
    rows = max(1, chunk // cells.shape[0])
    c, q = cells.astype(np.int32), q.astype(np.int32)
    for s in range(0, q.shape[0], rows):
        d2 = np.zeros((min(rows, q.shape[0] - s), c.shape[0]), I64)
        for a in range(3):
            d = q[s:s + rows, None, a] - c[None, :, a]
            d2 += d.astype(I64) * d
        at[s:s + rows] = np.argmin(d2, 1)                               # numpy: the first occurrence of the minimum
        best[s:s + rows] = d2[np.arange(d2.shape[0]), at[s:s + rows]]
    return best, at


def nearest_untruncated(words, depth, origin, dims, which):
    """(D int64 [n], witness xyz int64 [n, 3], node int64 [n]) per region cell in output order, for an unlimited radius; D = -1 where
    A is empty.  A region cell that is itself in A is its own witness at D = 0 (nothing else is at distance 0), which spares the
    brute force the cells where it has nothing to decide."""
    cells, node = target_cells(words, depth, which)
    q = region_cells(origin, dims)
    n_side = 1 << depth
    code = lambda c: (c[:, 2] * n_side + c[:, 1]) * n_side + c[:, 0]    # noqa: E731
    pos = np.searchsorted(code(cells), code(q))                         # cells are in code order
    own = np.zeros(q.shape[0], bool)
    if cells.shape[0]:
        ok = pos < cells.shape[0]
        own[ok] = code(cells)[pos[ok]] == code(q)[ok]
    best, at = np.full(q.shape[0], -1, I64), np.full(q.shape[0], -1, I64)
    best[own], at[own] = 0, pos[own]
    best[~own], at[~own] = nearest_in(cells, q[~own])
    if cells.shape[0] == 0:
        return best, np.full(q.shape, -1, I64), np.full(q.shape[0], -1, I64)
    return best, cells[at], node[at]


def truncate(words, dims, radius, best, wit, node):
    """the outputs of the call from the untruncated answer: none above radius^2"""
    ok = (best >= 0) & (best <= radius * radius)
    shape = (dims[2], dims[1], dims[0])
    color = np.where(ok & (node >= 0), np.asarray(words, np.uint32)[2 * np.maximum(node, 0) + 1], 0)
    return {"dist2": np.where(ok, best, -1).astype(np.int32).reshape(shape),
            "cell": np.where(ok, pack(wit * ok[:, None]), NO_CELL).astype(np.uint64).reshape(shape),
            "node": np.where(ok, node, -1).astype(np.int32).reshape(shape),
            "color": color.astype(np.uint32).reshape(shape)}


def nearest_field_words(words, depth, origin, dims, radius, which=OCCUPIED):
    """-> {"dist2" int32, "cell" uint64, "node" int32, "color" uint32}, each [nz, ny, nx]: svoslam_pool_nearest_field by its
    definition (node and color: -1 and 0 throughout for FREE, where the call takes no such outputs)"""
    assert 0 <= radius <= MAX_RADIUS and all(v >= 0 for v in dims) and which in (OCCUPIED, FREE)
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) for a in range(3))
    return truncate(words, dims, radius, *nearest_untruncated(words, depth, origin, dims, which))


def _pass_argmin(g, axis, off, out_len, radius):
    """g'(i) = min over |k| <= radius of g(i + off + k) + k^2 along `axis` and the SMALLEST i + off + k that attains it: the
    candidates are taken in ascending order and only a strictly smaller sum replaces what is there.  Above radius^2: NONE."""
    g = np.moveaxis(g, axis, 0)
    in_len = g.shape[0]
    out = np.full((out_len,) + g.shape[1:], NONE, I64)
    arg = np.zeros(out.shape, I64)
    for k in range(-radius, radius + 1):
        lo, hi = max(0, -(off + k)), min(out_len, in_len - off - k)
        if lo < hi:
            cand = g[lo + off + k:hi + off + k] + k * k
            better = cand < out[lo:hi]
            out[lo:hi] = np.where(better, cand, out[lo:hi])
            arg[lo:hi] = np.where(better, np.arange(lo + off + k, hi + off + k).reshape((-1,) + (1,) * (g.ndim - 1)), arg[lo:hi])
    return np.moveaxis(np.where(out <= radius * radius, out, NONE), 0, axis), np.moveaxis(arg, 0, axis)


def nearest_field_separable(words, depth, origin, dims, radius, which=OCCUPIED):
    """the same outputs by the device's route: the target set on the region inflated by `radius` and clipped to the root; along x
    the nearest target cell on either side, the lower one on a tie; the y and the z pass with their argmin; then z' from the z
    pass, y' from the y pass at (x, y, z'), x' from the x pass at (x, y', z')"""
    n_side = 1 << depth
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    shape = (dims[2], dims[1], dims[0])
    if (n == 0).any():
        return {"dist2": np.zeros(shape, np.int32), "cell": np.zeros(shape, np.uint64), "node": np.zeros(shape, np.int32),
                "color": np.zeros(shape, np.uint32)}
    lo, hi = np.maximum(o - radius, 0), np.minimum(o + n + radius, n_side)
    xyz, node = occupied_cells(words, depth)
    inside = ((xyz >= lo) & (xyz < hi)).all(1)
    c = xyz[inside] - lo
    occ = np.zeros(tuple(hi - lo)[::-1], bool)
    occ[c[:, 2], c[:, 1], c[:, 0]] = True
    node_at = np.full(occ.shape, -1, I64)
    node_at[c[:, 2], c[:, 1], c[:, 0]] = node[inside]
    tgt = occ if which == OCCUPIED else ~occ                             # the inflated region is clipped to the root: all of it are cells
    idx = np.arange(tgt.shape[2], dtype=I64)
    below = np.maximum.accumulate(np.where(tgt, idx, -NONE), axis=2)             # the nearest target x at or below
    above = np.minimum.accumulate(np.where(tgt, idx, NONE)[:, :, ::-1], axis=2)[:, :, ::-1]
    take_below = idx - below <= above - idx                              # the lower one on a tie
    dist, wx = np.where(take_below, idx - below, above - idx), np.where(take_below, below, above)
    off = o - lo
    g1 = np.where(dist <= radius, dist * dist, NONE)[:, :, off[0]:off[0] + n[0]]
    wx = wx[:, :, off[0]:off[0] + n[0]]
    g2, ay = _pass_argmin(g1, 1, int(off[1]), int(n[1]), radius)
    g3, az = _pass_argmin(g2, 0, int(off[2]), int(n[2]), radius)
    ok = g3 <= radius * radius
    x = np.broadcast_to(np.arange(n[0]), g3.shape)
    y = np.broadcast_to(np.arange(n[1])[:, None], g3.shape)
    zr = np.where(ok, az, 0)
    yr = np.where(ok, ay[zr, y, x], 0)
    xr = np.where(ok, wx[zr, yr, x], 0)
    wit = np.stack([xr + lo[0], yr + lo[1], zr + lo[2]], -1)
    nd = np.where(ok & (which == OCCUPIED), node_at[zr, yr, xr], -1)
    return {"dist2": np.where(ok, g3, -1).astype(np.int32), "cell": np.where(ok, pack(wit), NO_CELL).astype(np.uint64),
            "node": nd.astype(np.int32),
            "color": np.where(nd >= 0, np.asarray(words, np.uint32)[2 * np.maximum(nd, 0) + 1], 0).astype(np.uint32)}


FIELDS = ("dist2", "cell", "node", "color")


def same_outputs(got, want, names=FIELDS):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape)
        bad = np.argwhere(got[name] != want[name])
        assert bad.shape[0] == 0, (name, bad.shape[0], bad[:5].tolist(), got[name][tuple(bad[:5].T)].tolist(),
                                   want[name][tuple(bad[:5].T)].tolist())


# ---- a pool fused by the oracle: the two restatements ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def answers(fused):
    """(region name, which) -> the untruncated answer by the definition at depth 6, computed once"""
    words, _ = fused
    cache = {}

    def get(name, which):
        if (name, which) not in cache:
            cache[(name, which)] = nearest_untruncated(words, DEPTH, *fused_regions(DEPTH)[name], which)
        return cache[(name, which)]
    return get


@pytest.mark.parametrize("which", [OCCUPIED, FREE])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_separable_passes_are_the_definition(fused, answers, region, which):
    words, _ = fused
    origin, dims = fused_regions(DEPTH)[region]
    for radius in RADII:
        want = truncate(words, dims, radius, *answers(region, which))
        if region == "one_cell":                                        # the truncation of the cache is the definition's own
            same_outputs(want, nearest_field_words(words, DEPTH, origin, dims, radius, which))
        same_outputs(nearest_field_separable(words, DEPTH, origin, dims, radius, which), want)


def test_the_fused_cases_are_not_empty(fused, answers):
    """what a comparison needs in order not to pass empty: found and not found, witnesses outside the region, and cells with more
    than one nearest cell, where the tie rule decides"""
    words, _ = fused
    tied = outside = none = found = 0
    occ = occupied_cells(words, DEPTH)[0]
    for name, (origin, dims) in fused_regions(DEPTH).items():
        best, wit, _ = answers(name, OCCUPIED)
        ok = (best >= 0) & (best <= 9)
        found, none = found + int(ok.sum()), none + int((~ok).sum())
        outside += int((ok & ((wit < np.asarray(origin)) | (wit >= np.asarray(origin) + np.asarray(dims))).any(1)).sum())
        q = region_cells(origin, dims)[ok][:400]
        d2 = ((q[:, None, :] - occ[None, :, :]) ** 2).sum(2)
        tied += int(((d2 == d2.min(1)[:, None]).sum(1) > 1).sum())
    assert found > 1000 and none > 1000 and outside >= 1 and tied > 50, (found, none, outside, tied)
    best, wit, _ = answers("whole_root", FREE)
    assert (best == 0).sum() > 1000 and (best > 0).sum() > 100          # occupied cells have a positive depth


@pytest.mark.parametrize("which", [OCCUPIED, FREE])
def test_the_witness_is_a_target_cell_at_exactly_that_distance(fused, answers, which):
    words, _ = fused
    n_side = 1 << DEPTH
    occ = np.zeros((n_side,) * 3, bool)
    xyz = occupied_cells(words, DEPTH)[0]
    occ[xyz[:, 2], xyz[:, 1], xyz[:, 0]] = True
    for name, (origin, dims) in fused_regions(DEPTH).items():
        for radius in RADII:
            got = nearest_field_separable(words, DEPTH, origin, dims, radius, which)
            wit, ok = unpack(got["cell"]).reshape(-1, 3), got["dist2"].reshape(-1) >= 0
            assert np.array_equal(ok, (wit >= 0).all(1)) and np.array_equal(ok, got["cell"].reshape(-1) != NO_CELL)
            w, q = wit[ok], region_cells(origin, dims)[ok]
            assert ((w >= 0) & (w < n_side)).all() and (occ[w[:, 2], w[:, 1], w[:, 0]] == (which == OCCUPIED)).all()
            assert np.array_equal(((w - q) ** 2).sum(1), got["dist2"].reshape(-1)[ok])
            assert (got["dist2"].reshape(-1)[ok] <= radius * radius).all()
            if which == OCCUPIED:
                assert np.array_equal(got["node"].reshape(-1) >= 0, ok)
                assert (got["color"].reshape(-1)[ok] >> 24 > 127).all() and (got["color"].reshape(-1)[~ok] == 0).all()


def test_dist2_is_the_distance_field_and_nearest_occupied_at_the_midpoints(fused, answers):
    words, _ = fused
    for k, (name, (origin, dims)) in enumerate(sorted(fused_regions(DEPTH).items())):
        full = distance_field_words(words, DEPTH, origin, dims, MAX_RADIUS)
        at = sample_cells(origin, dims, 300, 80 + k)
        points = midpoints(DEPTH, ROOT_CENTER, ROOT_EDGE, origin, dims)[at]
        for radius in RADII:
            got = truncate(words, dims, radius, *answers(name, OCCUPIED))
            assert np.array_equal(got["dist2"], np.where((full >= 0) & (full <= radius * radius), full, -1))
            near = nearest_occupied_words(words, DEPTH, ROOT_CENTER, ROOT_EDGE, points, radius)
            assert np.array_equal(near["dist2"], got["dist2"].reshape(-1)[at])
            # the other call's cell (lowest Morton code) is another cell only among the equally near
            theirs, ours, q = unpack(near["cell"]), unpack(got["cell"].reshape(-1)[at]), region_cells(origin, dims)[at]
            ok = near["dist2"] >= 0
            assert np.array_equal(((theirs - q) ** 2).sum(1)[ok], ((ours - q) ** 2).sum(1)[ok])
            assert ((theirs == -1).all(1) == ~ok).all() and ((ours == -1).all(1) == ~ok).all()


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def colored_pool(cells, depth):
    """words with the given cells occupied, each with a colour word of its own (alpha 255), and cell -> (node, colour word)"""
    pool, where = HandPool(), {}
    for k, xyz in enumerate(cells):
        word = rgba(k + 1, 2 * k + 1, 7, 255)
        where[tuple(xyz)] = (pool.put(path_of(*xyz, depth), [OPAQUE] * (depth - 1) + [word]), word)
    return pool.words(), where


def expected(dims, values, where=None):
    """values: per cell in output order (dist2, witness xyz) or None -> the four outputs"""
    shape = (dims[2], dims[1], dims[0])
    assert len(values) == dims[0] * dims[1] * dims[2]
    out = {"dist2": np.full(len(values), -1, np.int32), "cell": np.full(len(values), NO_CELL, np.uint64),
           "node": np.full(len(values), -1, np.int32), "color": np.zeros(len(values), np.uint32)}
    for k, v in enumerate(values):
        if v is not None:
            out["dist2"][k], out["cell"][k] = v[0], v[1][0] | (v[1][1] << 16) | (v[1][2] << 32)
            if where is not None:
                out["node"][k], out["color"][k] = where[tuple(v[1])]
    return {name: a.reshape(shape) for name, a in out.items()}


def nearest_cases():
    """name -> (words, depth, origin, dims, radius, which, expected outputs)"""
    out = {}
    a, b, lowy, lowz = (1, 3, 3), (5, 3, 3), (3, 1, 3), (3, 3, 1)
    # occupied at x - 2 and x + 2 of (3,3,3): the witness is x - 2.  The row y = 3, z = 3, x 0..6
    words, where = colored_pool([a, b], 3)
    row = [(1, a), (0, a), (1, a), (4, a), (1, b), (0, b), (1, b)]
    out["tie_in_x"] = (words, 3, (0, 3, 3), (7, 1, 1), 3, OCCUPIED, expected((7, 1, 1), row, where))
    out["tie_in_x_radius_1"] = (words, 3, (0, 3, 3), (7, 1, 1), 1, OCCUPIED,
                                expected((7, 1, 1), [(1, a), (0, a), (1, a), None, (1, b), (0, b), (1, b)], where))
    # ... and a cell 2 lower in y with g = 0: the cell's own row gives 4, the lower row gives 0 + 4: the lower y wins; the higher y
    # (3,5,3) never does
    words, where = colored_pool([a, b, lowy, (3, 5, 3)], 3)
    out["tie_in_y"] = (words, 3, (3, 3, 3), (1, 1, 1), 2, OCCUPIED, expected((1, 1, 1), [(4, lowy)], where))
    # the same in z, alone and with all three at once: z wins
    words, where = colored_pool([a, b, lowz, (3, 3, 5)], 3)
    out["tie_in_z"] = (words, 3, (3, 3, 3), (1, 1, 1), 2, OCCUPIED, expected((1, 1, 1), [(4, lowz)], where))
    words, where = colored_pool([a, b, lowy, (3, 5, 3), lowz, (3, 3, 5)], 3)
    out["tie_in_all_three"] = (words, 3, (3, 3, 3), (1, 1, 1), 2, OCCUPIED, expected((1, 1, 1), [(4, lowz)], where))
    # the region x 2..4, y 3..4, z 3: every winning witness lies outside it, within R = 2.  (3,3,3): all six at 4, z wins; (2,4,3):
    # a and (3,5,3) at 2, the lower y wins; (4,4,3): b and (3,5,3) likewise
    block = [(1, a), (4, lowz), (1, b),
             (2, a), (1, (3, 5, 3)), (2, b)]
    out["witness_outside_the_region"] = (words, 3, (2, 3, 3), (3, 2, 1), 2, OCCUPIED, expected((3, 2, 1), block, where))
    # two diagonal neighbours at distance 2 in one plane: (2,2,3) and (4,2,3), (2,4,3) and (4,4,3) about (3,3,3): smallest y, then x
    words, where = colored_pool([(4, 4, 3), (2, 4, 3), (4, 2, 3), (2, 2, 3)], 3)
    out["four_diagonals"] = (words, 3, (3, 3, 3), (1, 1, 1), 2, OCCUPIED, expected((1, 1, 1), [(2, (2, 2, 3))], where))
    # an empty pool: nothing for OCCUPIED; for FREE every cell is its own witness
    empty = HandPool().words()
    out["empty_pool"] = (empty, 2, (0, 0, 0), (2, 2, 2), 2, OCCUPIED, expected((2, 2, 2), [None] * 8))
    own = [(0, (x, y, z)) for z in (1, 2) for y in (0, 1) for x in (2, 3)]
    out["empty_pool_free"] = (empty, 2, (2, 0, 1), (2, 2, 2), 2, FREE, expected((2, 2, 2), own))
    # a fully occupied depth-1 root: A is empty for FREE, nothing outside the root is a cell
    full = cells_pool([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], 1)
    out["full_root_free"] = (full, 1, (0, 0, 0), (2, 2, 2), 3, FREE, expected((2, 2, 2), [None] * 8))
    # a solid 4 x 4 x 4 root with the pocket (2,1,1): the depths of the row y = 1, z = 1 and of the column x = 2, z = 1
    pocket = (2, 1, 1)
    solid = cells_pool([(x, y, z) for z in range(4) for y in range(4) for x in range(4) if (x, y, z) != pocket], 2)
    out["pocket_row"] = (solid, 2, (0, 1, 1), (4, 1, 1), 2, FREE, expected((4, 1, 1), [(4, pocket), (1, pocket), (0, pocket), (1, pocket)]))
    out["pocket_column"] = (solid, 2, (2, 0, 1), (1, 4, 1), 1, FREE, expected((1, 4, 1), [(1, pocket), (0, pocket), (1, pocket), None]))
    # two pockets equally deep below (1,1,1): (1,1,0) wins over (1,0,1) and (0,1,1) -- z first
    three = cells_pool([(x, y, z) for z in range(4) for y in range(4) for x in range(4) if (x, y, z) not in ((1, 1, 0), (1, 0, 1), (0, 1, 1))], 2)
    out["three_pockets"] = (three, 2, (1, 1, 1), (1, 1, 1), 1, FREE, expected((1, 1, 1), [(1, (1, 1, 0))]))
    return out


NEAREST_CASES = nearest_cases()


@pytest.mark.parametrize("name", sorted(NEAREST_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, radius, which, want = NEAREST_CASES[name]
    for restatement in (nearest_field_words, nearest_field_separable):
        same_outputs(restatement(words, depth, origin, dims, radius, which), want)
    if which == OCCUPIED:
        assert np.array_equal(want["dist2"], distance_field_words(words, depth, origin, dims, radius))


@pytest.mark.parametrize("which", [OCCUPIED, FREE])
def test_the_restatements_agree_at_the_level_above_and_on_odd_regions(which):
    """the hand-built words one level up, and regions that touch the root's faces, for radii on both sides of every size"""
    for name in ("tie_in_all_three", "four_diagonals", "three_pockets", "pocket_row"):
        words, depth = NEAREST_CASES[name][:2]
        n_side = 1 << depth
        for d, origin, dims in ((depth, (0, 0, 0), (n_side,) * 3), (depth - 1, (0, 0, 0), (n_side // 2,) * 3), (depth, (1, 0, 2), (2, 3, 2))):
            for radius in (0, 1, 2, 5):
                same_outputs(nearest_field_separable(words, d, origin, dims, radius, which), nearest_field_words(words, d, origin, dims, radius, which))


def test_a_zero_dimension_is_an_empty_field():
    words = NEAREST_CASES["tie_in_x"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        for restatement in (nearest_field_words, nearest_field_separable):
            got = restatement(words, 3, (0, 0, 0), dims, 2)
            assert all(got[name].shape == (dims[2], dims[1], dims[0]) for name in FIELDS)


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_nearest_field_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_nearest_field", "svoslam_workspace_nearest_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "nearest_field") and hasattr(pkg.Workspace, "nearest_buffers")
    assert (pkg.NEAREST_OCCUPIED, pkg.NEAREST_FREE) == (OCCUPIED, FREE)
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_nearest_field(" in header and "int svoslam_workspace_nearest_buffers(" in header
    assert "#define SVOSLAM_NEAREST_OCCUPIED 0" in header and "#define SVOSLAM_NEAREST_FREE     1" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
    text = " ".join(header.split())
    assert "dist2 equals svoslam_pool_nearest_occupied's" in text and "only among equally near" in text
