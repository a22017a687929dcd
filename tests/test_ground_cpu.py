"""Ground navigation in a map region (svoslam_pool_ground_field, svoslam_field_trace_ground_paths; include/svoslam.h, DESIGN.md
section 23): the foothold set restated by its definition, body offset by body offset on the occupied cells, and the field as
Dijkstra's algorithm with a heap; a second restatement that takes the body from the distance transform's pass along the two
horizontal axes only and relaxes all cells at once to a fixed point; the path rule restated cell by cell.  The two field
restatements are proven equal on a pool fused by the CPU oracle, on hand-built pools with every value written out and on the two
worlds tests/test_gpu_ground.py runs on the device.  No GPU.

ground_field_words (the definition) and trace_ground_path are what the device calls must produce; tests/test_gpu_ground.py compares
against them value for value."""
import ctypes as C
import heapq
import os

import numpy as np
import pytest

from test_field_cpu import NONE, _pass, fused_regions
from test_surface_cpu import HandPool, OPAQUE, load_pkg, occupied_cells, path_of, rgba
from test_volume_cpu import DEPTH, fused  # noqa: F401

I64 = np.int64
MAX_RADIUS, MAX_HEIGHT, MAX_STEP, MAX_CLIMB_COST, MAX_SNAP = 4096, 256, 4, 65534, 256
UP = {"+y": 2, "-y": 3, "+z": 4, "-z": 5}


# ---- the specification, restated -------------------------------------------------------------------------------------------
def up_vector(up):
    """-> (axis, sign, u): axis up >> 1, towards smaller coordinates if up & 1"""
    assert up in (2, 3, 4, 5)
    axis, sign = up >> 1, -1 if up & 1 else 1
    u = np.zeros(3, I64)
    u[axis] = sign
    return axis, sign, u


def check_parameters(r, H, S, c, snap, step_below_height=True):
    """the call's limits.  step_below_height=False leaves out S <= H - 1 alone: the definition is well formed without it (a body with
    no cylinder part), the call refuses it"""
    assert 0 <= r <= MAX_RADIUS and 1 <= H <= MAX_HEIGHT and 0 <= S <= MAX_STEP and 0 <= c <= MAX_CLIMB_COST
    assert S <= H - 1 or not step_below_height
    assert 0 <= snap <= MAX_SNAP


def footholds_words(words, depth, origin, dims, up, r, H, S, cells=None):
    """-> bool [nz, ny, nx]: G by its definition.  A candidate is a region cell above an occupied cell; every cell of its body --
    the column k < H, and for S <= k < H the disc of radius r in the layer of q + k u -- is then looked up in the occupied set,
    offset by offset.  Cells outside the root are in no set."""
    n_side = 1 << depth
    axis, sign, u = up_vector(up)
    flat = [a for a in range(3) if a != axis]
    if cells is None:
        cells = occupied_cells(words, depth)[0]
    cells = np.asarray(cells, I64).reshape(-1, 3)
    keys = np.unique((cells[:, 2] * n_side + cells[:, 1]) * n_side + cells[:, 0])

    def occupied(q):
        inside = ((q >= 0) & (q < n_side)).all(1)
        return inside & np.isin((q[:, 2] * n_side + q[:, 1]) * n_side + q[:, 0], keys)
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    q = cells + u                                                       # 1: q - u is a cell of the root and is occupied
    q = q[((q >= o) & (q < o + n)).all(1)]
    for k in range(H):
        offsets = [(0, 0)]
        if k >= S:
            offsets = [(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1) if a * a + b * b <= r * r]
        for a, b in offsets:
            d = k * u
            d[flat[0]], d[flat[1]] = a, b
            q = q[~occupied(q + d)]
    out = np.zeros((dims[2], dims[1], dims[0]), bool)
    rel = q - o
    out[rel[:, 2], rel[:, 1], rel[:, 0]] = True
    return out


def snapped(G, origin, up, snap, entries):
    """-> int64 [m, 3]: the region-relative footholds of the entries that have one, in order, duplicates each: going from the entry
    against u, the entry itself first, at most `snap` further cells, never leaving the region"""
    axis, sign, u = up_vector(up)
    nz, ny, nx = G.shape
    out = []
    for e in np.asarray(entries, I64).reshape(-1, 3).tolist():
        q = [int(e[a]) - int(origin[a]) for a in range(3)]
        for _ in range(snap + 1):
            if not (0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz):
                break
            if G[q[2], q[1], q[0]]:
                out.append(list(q))
                break
            q[axis] -= sign
    return np.array(out, I64).reshape(-1, 3)


def ground_field_words(words, depth, origin, dims, up, r, H, S, c, seeds, snap=0, G=None, step_below_height=True):
    """-> (int32 [nz, ny, nx], stats): svoslam_pool_ground_field by its definition: G, the seeds snapped, then Dijkstra's algorithm
    with a heap over the moves q -> q + e + j u, |j| <= S, at 1 + c |j| each.  stats: footholds and seeds_used."""
    check_parameters(r, H, S, c, snap, step_below_height)
    assert all(v >= 0 for v in dims) and all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) for a in range(3))
    nx, ny, nz = dims
    if nx * ny * nz == 0:
        return np.zeros((nz, ny, nx), np.int32), dict(footholds=0, seeds_used=0)
    if G is None:
        G = footholds_words(words, depth, origin, dims, up, r, H, S)
    axis = up >> 1
    size, stride = (nx, ny, nz), (1, nx, nx * ny)
    flat = [a for a in range(3) if a != axis]
    ok = G.reshape(-1).tolist()
    best = [NONE] * len(ok)
    start = snapped(G, origin, up, snap, seeds)
    heap = []
    for x, y, z in start.tolist():
        at = (z * ny + y) * nx + x
        if best[at]:
            best[at] = 0
            heap.append((0, at))
    heapq.heapify(heap)
    while heap:
        v, at = heapq.heappop(heap)
        if v > best[at]:
            continue
        q = (at % nx, (at // nx) % ny, at // (nx * ny))
        for a in flat:
            for step in (-1, 1):
                if not 0 <= q[a] + step < size[a]:
                    continue
                for j in range(-S, S + 1):
                    if not 0 <= q[axis] + j < size[axis]:
                        continue
                    to, price = at + step * stride[a] + j * stride[axis], v + 1 + c * abs(j)
                    if ok[to] and price < best[to]:
                        best[to] = price
                        heapq.heappush(heap, (price, to))
    best = np.array(best, I64).reshape(G.shape)
    assert best[best < NONE].max(initial=0) < NONE
    out = np.where(G, np.where(best < NONE, best, -1), -2).astype(np.int32)
    return out, dict(footholds=int(G.sum()), seeds_used=int(start.shape[0]))


def footholds_planar(words, depth, origin, dims, up, r, H, S):
    """G by the device's route: the occupancy of the region inflated by r horizontally, 1 below and H - 1 above and clipped to the
    root; the distance transform's pass (test_field_cpu._pass) along the two horizontal axes only gives D = "an occupied cell
    within r in this layer"; then G = O(q - u) and, over k < H, not O(q + k u) and, over S <= k < H, not D(q + k u), layer by layer"""
    n_side = 1 << depth
    axis, sign, u = up_vector(up)
    flat = [a for a in range(3) if a != axis]
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    grow_lo, grow_hi = np.full(3, r, I64), np.full(3, r, I64)
    grow_lo[axis], grow_hi[axis] = (1, H - 1) if sign > 0 else (H - 1, 1)
    lo, hi = np.maximum(o - grow_lo, 0), np.minimum(o + n + grow_hi, n_side)
    xyz = occupied_cells(words, depth)[0]
    c = xyz[((xyz >= lo) & (xyz < hi)).all(1)] - lo
    occ = np.zeros(tuple(hi - lo)[::-1], bool)
    occ[c[:, 2], c[:, 1], c[:, 0]] = True
    off = o - lo
    g = np.where(occ, 0, NONE).astype(I64)
    for a in flat:                                                      # array axes are z, y, x
        g = _pass(g, 2 - a, int(off[a]), int(n[a]), r)
    body = g <= r * r
    cut = [slice(None)] * 3
    for a in flat:
        cut[2 - a] = slice(int(off[a]), int(off[a] + n[a]))
    centre = occ[tuple(cut)]

    def layer(rows, k):
        """rows at q + k u for the region's layers along up; a layer outside the inflated range is outside the root: nothing"""
        rows = np.moveaxis(rows, 2 - axis, 0)
        out = np.zeros((int(n[axis]),) + rows.shape[1:], bool)
        at = np.arange(n[axis]) + off[axis] + sign * k
        inside = (at >= 0) & (at < rows.shape[0])
        out[inside] = rows[at[inside]]
        return np.moveaxis(out, 0, 2 - axis)
    G = layer(centre, -1)
    for k in range(H):
        G &= ~layer(centre, k)
        if k >= S:
            G &= ~layer(body, k)
    return G


def ground_field_relaxed(words, depth, origin, dims, up, r, H, S, c, seeds, snap=0):
    """the same field by another route: G from the planar transform, then s(q) = min(s(q), s(q - e - j u) + 1 + c |j|) for every e
    and j with shifted arrays, all cells at once, repeated until nothing changes"""
    check_parameters(r, H, S, c, snap)
    nx, ny, nz = dims
    if nx * ny * nz == 0:
        return np.zeros((nz, ny, nx), np.int32), dict(footholds=0, seeds_used=0)
    G = footholds_planar(words, depth, origin, dims, up, r, H, S)
    axis = up >> 1
    flat = [a for a in range(3) if a != axis]
    start = snapped(G, origin, up, snap, seeds)
    whole, stats = G, dict(footholds=int(G.sum()), seeds_used=int(start.shape[0]))
    if not G.any():
        return np.full(G.shape, -2, np.int32), stats
    box = tuple(slice(int(np.flatnonzero(G.any(axis=tuple(b for b in range(3) if b != a)))[0]),
                      int(np.flatnonzero(G.any(axis=tuple(b for b in range(3) if b != a)))[-1]) + 1) for a in range(3))
    G = G[box]                                                          # nothing outside the footholds' bounding box takes part
    s = np.full(G.shape, NONE, I64)
    s[start[:, 2] - box[0].start, start[:, 1] - box[1].start, start[:, 0] - box[2].start] = 0

    def window(a, step, j):
        """(to, from) index tuples of the move by `step` along axis a and j along up"""
        to, frm = [slice(None)] * 3, [slice(None)] * 3
        for ax, d in ((a, step), (axis, j)):
            if d > 0:
                to[2 - ax], frm[2 - ax] = slice(d, None), slice(None, -d)
            elif d < 0:
                to[2 - ax], frm[2 - ax] = slice(None, d), slice(-d, None)
        return tuple(to), tuple(frm)
    moves = [(window(a, step, j), 1 + c * abs(j)) for a in flat for step in (-1, 1) for j in range(-S, S + 1)
             if abs(j) < G.shape[2 - axis] or j == 0]
    while True:
        t = s.copy()
        for (to, frm), price in moves:
            if t[to].size:
                t[to] = np.where(G[to], np.minimum(t[to], t[frm] + price), NONE)   # what this sweep has lowered already counts
        t = np.where(G, np.minimum(t, NONE), NONE)
        if np.array_equal(t, s):
            break
        s = t
    out = np.full(whole.shape, -2, np.int32)
    out[box] = np.where(~G, -2, np.where(s >= NONE, -1, s))
    return out, stats


def candidates(up, S):
    """the walk's order: e first (-x, +x, then - and + along the other horizontal axis), within one e j = 0, -1, +1, -2, +2, ..."""
    axis, sign, u = up_vector(up)
    other = 3 - axis
    out = []
    for a, step in ((0, -1), (0, 1), (other, -1), (other, 1)):
        for j in [0] + [v for k in range(1, S + 1) for v in (-k, k)]:
            d = [0, 0, 0]
            d[a], d[axis] = step, sign * j
            out.append((tuple(d), abs(j)))
    return out


def trace_ground_path(field, origin, up, S, c, start, max_cells, snap=0):
    """-> (cells int32 [min(|length|, max_cells), 3] absolute, length): svoslam_field_trace_ground_paths for one start, cell by
    cell.  The start is snapped to the first value other than -2 against u; length 0 outside the region, without such a cell or on
    -1; from a value v > 0 to the first candidate with v' >= 0 and v' + 1 + c |j| == v; without one the walk stops and the length
    is minus the cells walked."""
    axis, sign, u = up_vector(up)
    nz, ny, nx = field.shape
    q = [int(start[a]) - int(origin[a]) for a in range(3)]

    def inside(p):
        return 0 <= p[0] < nx and 0 <= p[1] < ny and 0 <= p[2] < nz
    found = False
    for _ in range(snap + 1):
        if not inside(q):
            break
        if field[q[2], q[1], q[0]] != -2:
            found = True
            break
        q[axis] -= sign
    cells, length = [], 0
    if found and field[q[2], q[1], q[0]] >= 0:
        order = candidates(up, S)
        while True:
            v = int(field[q[2], q[1], q[0]])
            if length < max_cells:
                cells.append([q[a] + int(origin[a]) for a in range(3)])
            length += 1
            if v == 0:
                break
            to = None
            for d, climbed in order:
                p = [q[a] + d[a] for a in range(3)]
                if inside(p) and field[p[2], p[1], p[0]] >= 0 and int(field[p[2], p[1], p[0]]) + 1 + c * climbed == v:
                    to = p
                    break
            if to is None:
                length = -length
                break
            q = to
    return np.array(cells, np.int32).reshape(-1, 3), length


def check_ground_path(field, origin, up, S, c, start, snap=0):
    """the facts of a traced path on a ground field: legal moves through G, the prices sum to the value at its first cell, and it
    ends on a cell of value 0.  -> (cells, cells climbed in all)"""
    axis = up >> 1
    cells, length = trace_ground_path(field, origin, up, S, c, start, field.size, snap)
    rel = cells.astype(I64) - np.asarray(origin, I64)
    assert length == cells.shape[0] >= 1
    value = field[rel[:, 2], rel[:, 1], rel[:, 0]].astype(I64)
    assert (value >= 0).all() and value[-1] == 0
    step = np.abs(np.diff(rel, axis=0))
    climbed = step[:, axis]
    flat = step.sum(1) - climbed
    assert (flat == 1).all() and (climbed <= S).all()
    assert np.array_equal(value[:-1] - value[1:], 1 + c * climbed)
    assert int((1 + c * climbed).sum()) == int(value[0])
    return cells, int(climbed.sum())


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
PARAMETERS = ((0, 1, 0, 0), (0, 3, 1, 0), (1, 4, 2, 5), (3, 6, 4, 1))     # r, H, S, c


def ground_seeds(G, origin, dims, depth, count, rng):
    """`count` footholds of the region (absolute), then a cell of it that is none if there is one, a cell of the root outside the
    region if there is one, and cells outside the root"""
    o = np.asarray(origin, I64)
    at = np.argwhere(G)[:, ::-1]
    pick = at[rng.choice(at.shape[0], min(count, at.shape[0]), replace=False)] + o if at.shape[0] else np.zeros((0, 3), I64)
    extra = [(-1, int(o[1]), int(o[2])), (int(o[0]), 1 << depth, int(o[2])), (int(o[0]), int(o[1]), (1 << 31) - 1),
             (-(1 << 31), int(o[1]), int(o[2]))]
    blocked = np.argwhere(~G)[:, ::-1]
    if blocked.shape[0]:
        extra.append(tuple(int(v) for v in blocked[blocked.shape[0] // 2] + o))
    for a in range(3):
        if o[a] > 0:
            outside = o.copy()
            outside[a] -= 1
            extra.append(tuple(int(v) for v in outside))
    return np.concatenate([pick, np.array(extra, I64)]).astype(I64)


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_relaxation_is_dijkstra(fused, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    rng = np.random.default_rng(23)
    cells = occupied_cells(words, depth)[0]
    footholds = reached = walked = 0
    for up in (2, 3, 4, 5):
        for r, H, S, c in PARAMETERS:
            G = footholds_words(words, depth, origin, dims, up, r, H, S, cells=cells)
            assert np.array_equal(G, footholds_planar(words, depth, origin, dims, up, r, H, S)), (up, r, H, S)
            for count in (1, 7):
                seeds = ground_seeds(G, origin, dims, depth, count, rng)
                want, stats = ground_field_words(words, depth, origin, dims, up, r, H, S, c, seeds, G=G)
                assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
                got, again = ground_field_relaxed(words, depth, origin, dims, up, r, H, S, c, seeds)
                assert np.array_equal(got, want) and again == stats, (up, r, H, S, c, count)
                assert np.array_equal(want == -2, ~G) and stats["footholds"] == int(G.sum())
                assert stats["seeds_used"] == (want == 0).sum() == min(count, int(G.sum()))
                for q in np.argwhere(want > 0)[:, ::-1][::97]:
                    check_ground_path(want, origin, up, S, c, q + np.asarray(origin, I64))
                    walked += 1
                footholds, reached = footholds + int(G.sum()), reached + int((want > 0).sum())
    if region in ("whole_root", "low_corner"):
        assert footholds > 100 and reached > 20 and walked > 5, (footholds, reached, walked)


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def cells_pool(cells, depth, alpha=None):
    """a pool with `cells` occupied at `depth`; alpha: cell -> the alpha of its leaf instead of 255"""
    pool = HandPool()
    for xyz in cells:
        leaf = OPAQUE if not alpha or tuple(xyz) not in alpha else rgba(10, 20, 30, alpha[tuple(xyz)])
        pool.put(path_of(*xyz, depth), [OPAQUE] * (depth - 1) + [leaf])
    return pool.words()


def rows(*values):
    """the rows of one z plane -> int32 [1, ny, nx]"""
    return np.array([values], np.int32)


def ground_cases():
    """name -> dict(words, depth, origin, dims, up, r, H, S, c, snap, seeds, want int32 [nz, ny, nx], footholds, seeds_used).  Depth
    3 unless said; a strip is the floor cells (x, 0, 0), x = 0 .. 7, under the region's row y = 1."""
    no = [-2] * 8
    strip = [(x, 0, 0) for x in range(8)]
    out = {}

    def case(name, cells, origin, dims, params, seeds, want, footholds, used, up=2, depth=3, snap=0, alpha=None):
        r, H, S, c = params
        out[name] = dict(words=cells_pool(cells, depth, alpha), depth=depth, origin=origin, dims=dims, up=up, r=r, H=H, S=S, c=c, snap=snap,
                         seeds=seeds, want=np.asarray(want, np.int32), footholds=footholds, seeds_used=used)
    # a flat floor just below the region: the Manhattan distance in the plane
    floor = [(x, 0, z) for z in range(8) for x in range(8)]
    flat = np.array([[[abs(x - 2) + abs(z - 3) for x in range(8)]] for z in range(8)], np.int32)
    case("flat_floor_below_the_region", floor, (0, 1, 0), (8, 1, 8), (0, 2, 0, 0), [(2, 1, 3)], flat, 64, 1)
    # the same floor as a ceiling for -y, and as a wall at z = 7 for -z
    case("flat_floor_minus_y", [(x, 7, z) for x, _, z in floor], (0, 6, 0), (8, 1, 8), (0, 2, 0, 0), [(2, 6, 3)], flat, 64, 1, up=3)
    case("flat_floor_minus_z", [(x, z, 7) for x, _, z in floor], (0, 0, 6), (8, 8, 1), (0, 2, 1, 9), [(2, 3, 6)], flat.reshape(1, 8, 8), 64, 1,
         up=5)
    case("flat_floor_plus_z", [(x, z, 0) for x, _, z in floor], (0, 0, 1), (8, 8, 1), (0, 2, 1, 9), [(2, 3, 1)], flat.reshape(1, 8, 8), 64, 1,
         up=4)
    # a strip along z, one cell wide, seeded where a tile of 8 begins: the tile before it holds the seed in its halo only, and the
    # seed's own tile lowers no cell on that face
    case("seed_on_a_tile_face", [(0, 0, z) for z in range(16)], (0, 1, 0), (1, 1, 16), (0, 1, 0, 0), [(0, 1, 8)],
         np.array([[[abs(z - 8)]] for z in range(16)], np.int32), 16, 1, depth=4)
    case("seed_under_a_tile_top", [(x, 0, 0) for x in range(8)] + [(x, y, 0) for x in range(4, 8) for y in range(1, 8)], (0, 0, 0), (8, 10, 1),
         (0, 2, 1, 0), [(0, 1, 0)], rows(no, [0, 1, 2, 3, -2, -2, -2, -2], no, no, no, no, no, no, [-2, -2, -2, -2, -1, -1, -1, -1], no), 8, 1,
         depth=4)
    # a riser of 1 at x = 4, climbed at 1 + c = 4; a riser of S + 1 = 2 is not
    riser = strip + [(x, 1, 0) for x in range(4, 8)]
    case("riser_of_one", riser, (0, 1, 0), (8, 4, 1), (0, 2, 1, 3), [(0, 1, 0)],
         rows([0, 1, 2, 3, -2, -2, -2, -2], [-2, -2, -2, -2, 7, 8, 9, 10], no, no), 8, 1)
    case("riser_of_one_from_above", riser, (0, 1, 0), (8, 4, 1), (0, 2, 1, 3), [(7, 2, 0)],
         rows([10, 9, 8, 7, -2, -2, -2, -2], [-2, -2, -2, -2, 3, 2, 1, 0], no, no), 8, 1)
    case("riser_of_two", riser + [(x, 2, 0) for x in range(4, 8)], (0, 1, 0), (8, 4, 1), (0, 2, 1, 3), [(0, 1, 0)],
         rows([0, 1, 2, 3, -2, -2, -2, -2], no, [-2, -2, -2, -2, -1, -1, -1, -1], no), 8, 1)
    # a beam over x = 3: at height H = 3 above the foothold it is clear, at H - 1 it blocks -- from outside the region, above
    case("beam_at_headroom", strip + [(3, 4, 0)], (0, 1, 0), (8, 1, 1), (0, 3, 0, 0), [(0, 1, 0)], rows(list(range(8))), 8, 1)
    case("beam_below_headroom", strip + [(3, 3, 0)], (0, 1, 0), (8, 1, 1), (0, 3, 0, 0), [(0, 1, 0)], rows([0, 1, 2, -2, -1, -1, -1, -1]), 7, 1)
    # a post beside the strip, outside the region (z = 2; the region is z = 1): at height S - 1 the body is a column and passes, at
    # S it is a disc of radius 2 and the post, 1 away in z, blocks |dx| <= 1
    wide = [(x, 0, z) for z in range(3) for x in range(8)]
    case("post_below_the_step", wide + [(4, 1, 2)], (0, 1, 1), (8, 1, 1), (2, 3, 1, 0), [(0, 1, 1)], rows(list(range(8))), 8, 1)
    case("post_at_the_step", wide + [(4, 2, 2)], (0, 1, 1), (8, 1, 1), (2, 3, 1, 0), [(0, 1, 1)], rows([0, 1, 2, -2, -2, -2, -1, -1]), 5, 1)
    case("post_at_the_step_radius_one", wide + [(4, 2, 2)], (0, 1, 1), (8, 1, 1), (1, 3, 1, 0), [(0, 1, 1)], rows([0, 1, 2, 3, -2, -1, -1, -1]),
         7, 1)
    # the root's bottom layer holds no foothold: nothing is under it
    case("root_bottom_layer", [(0, 0, 0), (1, 0, 0)], (0, 0, 0), (4, 2, 1), (0, 1, 0, 0), [(0, 1, 0), (2, 0, 0)],
         rows([-2, -2, -2, -2], [0, 1, -2, -2]), 2, 1)
    # headroom through the root's top face: nothing is occupied out there
    case("headroom_through_the_top", [(x, 6, 0) for x in range(4)], (0, 7, 0), (4, 1, 1), (0, 4, 0, 0), [(0, 7, 0)], rows([0, 1, 2, 3]), 4, 1)
    # two footholds in one column: a floor at y = 0 and a slab at y = 3
    two = [(x, y, 0) for y in (0, 3) for x in range(4)]
    n4, top, cut = [-2] * 4, [0, 1, 2, 3], [-1] * 4
    case("two_in_a_column", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [(0, 4, 0)], rows(n4, cut, n4, n4, top, n4), 8, 1)
    case("snap_zero_misses", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [(0, 5, 0)], rows(n4, cut, n4, n4, cut, n4), 8, 0)
    case("snap_three_lands", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [(0, 5, 0)], rows(n4, cut, n4, n4, top, n4), 8, 1, snap=3)
    case("snap_through_the_slab", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [(3, 3, 0)], rows(n4, top[::-1], n4, n4, cut, n4), 8, 1, snap=3)
    case("snap_leaves_the_region", two, (0, 2, 0), (4, 4, 1), (0, 2, 1, 0), [(0, 3, 0)], rows(n4, n4, cut, n4), 4, 0, snap=3)
    case("duplicates", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [(0, 4, 0), (0, 4, 0), (3, 5, 0)], rows(n4, cut, n4, n4, [0, 1, 1, 0], n4), 8, 3,
         snap=1)
    case("no_seeds", two, (0, 0, 0), (4, 6, 1), (0, 2, 1, 0), [], rows(n4, cut, n4, n4, cut, n4), 8, 0)
    # alpha 127 is not occupied: no support at x = 2
    case("alpha_127_beside_128", strip[:4], (0, 1, 0), (4, 1, 1), (0, 1, 0, 0), [(0, 1, 0)], rows([0, 1, -2, -1]), 3, 1,
         alpha={(2, 0, 0): 127, (3, 0, 0): 128})
    # asked one level above the leaves: the cells (x, 0, 0) of depth 4, x = 0 .. 7, are the cells x = 0 .. 3 of depth 3
    out["one_below_the_leaf_depth"] = dict(out["alpha_127_beside_128"], words=cells_pool(strip, 4), dims=(8, 1, 1),
                                           want=rows([0, 1, 2, 3, -2, -2, -2, -2]), footholds=4)
    return out


GROUND_CASES = ground_cases()


@pytest.mark.parametrize("name", sorted(GROUND_CASES))
def test_hand_built_pools(name):
    k = GROUND_CASES[name]
    args = (k["words"], k["depth"], k["origin"], k["dims"], k["up"], k["r"], k["H"], k["S"], k["c"], k["seeds"], k["snap"])
    got, stats = ground_field_words(*args)
    assert np.array_equal(got, k["want"]), (got.tolist(), k["want"].tolist())
    assert stats == dict(footholds=k["footholds"], seeds_used=k["seeds_used"])
    again, also = ground_field_relaxed(*args)
    assert np.array_equal(again, got) and also == stats
    o = np.asarray(k["origin"], I64)
    counted = {tuple(int(v) for v in q + o) for q in snapped(got != -2, k["origin"], k["up"], k["snap"], k["seeds"])}
    for q in np.argwhere(got >= 0)[:, ::-1]:
        cells, _ = check_ground_path(got, k["origin"], k["up"], k["S"], k["c"], q + o)
        assert tuple(int(v) for v in cells[-1]) in counted


def test_a_zero_dimension_is_an_empty_field():
    for dims in ((0, 3, 3), (3, 0, 3), (3, 3, 0)):
        for call in (ground_field_words, ground_field_relaxed):
            got, stats = call(HandPool().words(), 3, (1, 1, 1), dims, 2, 0, 1, 0, 0, [(1, 1, 1)])
            assert got.shape == (dims[2], dims[1], dims[0]) and got.size == 0 and stats == dict(footholds=0, seeds_used=0)


def test_the_tie_break_order_on_the_flat_floor():
    """e before j, -x before +x before the other axis: along x first, then along z"""
    k = GROUND_CASES["flat_floor_below_the_region"]
    cells, length = trace_ground_path(k["want"], k["origin"], 2, 0, 0, (4, 1, 5), 64)
    assert length == 5 and cells.tolist() == [[4, 1, 5], [3, 1, 5], [2, 1, 5], [2, 1, 4], [2, 1, 3]]
    cells, length = trace_ground_path(k["want"], k["origin"], 2, 0, 0, (0, 1, 1), 3)
    assert length == 5 and cells.tolist() == [[0, 1, 1], [1, 1, 1], [2, 1, 1]]
    assert trace_ground_path(k["want"], k["origin"], 2, 0, 0, (2, 1, 3), 64)[1] == 1
    for start in ((2, 0, 3), (2, 2, 3), (-1, 1, 3), (8, 1, 3), (2, 1, 8)):   # outside the region
        assert trace_ground_path(k["want"], k["origin"], 2, 0, 0, start, 64, snap=2)[1] == 0
    k = GROUND_CASES["flat_floor_minus_z"]                              # the other horizontal axis is y
    cells, length = trace_ground_path(k["want"], k["origin"], 5, 1, 9, (4, 5, 6), 64)
    assert length == 5 and cells.tolist() == [[4, 5, 6], [3, 5, 6], [2, 5, 6], [2, 4, 6], [2, 3, 6]]


# not a ground field.  up = +y, S = 1, c = 2; planes z = 0, rows y = 0 .. 2.  (1, 1): 5 with 4 at -x below (j = -1: 4 + 1 + 2 is not
# 5) and 2 at -x above (2 + 3 == 5); (2, 1): 6 beside the 5 at j = 0; (3, 1): 9 with nothing that fits
PLATEAU = np.array([[[4, -2, -2, -2], [-2, 5, 6, 9], [2, -2, 3, -1]]], np.int32)
PLATEAU_TRACES = {                                                      # start, snap -> (cells walked, length)
    ((1, 1, 0), 0): ([(1, 1, 0), (0, 2, 0)], -2),                       # the 2 has no predecessor
    ((2, 1, 0), 0): ([(2, 1, 0), (1, 1, 0), (0, 2, 0)], -3),
    ((3, 1, 0), 0): ([(3, 1, 0)], -1),
    ((0, 0, 0), 0): ([(0, 0, 0)], -1),
    ((1, 2, 0), 0): ([], 0), ((1, 2, 0), 1): ([(1, 1, 0), (0, 2, 0)], -2),   # snapped down by one
    ((3, 2, 0), 1): ([], 0),                                            # -1 is a foothold: the snap stops on it
    ((1, 0, 0), 2): ([], 0), ((4, 1, 0), 0): ([], 0),                   # the walk leaves the region; outside
}


def test_the_trace_stops_on_a_plateau():
    for (start, snap), (cells, length) in PLATEAU_TRACES.items():
        got, n = trace_ground_path(PLATEAU, (0, 0, 0), 2, 1, 2, start, 64, snap)
        assert n == length and [tuple(c) for c in got.tolist()] == cells, (start, snap)
    assert trace_ground_path(PLATEAU, (0, 0, 0), 2, 1, 2, (2, 1, 0), 1)[0].tolist() == [[2, 1, 0]]
    # j = 0, -1, +1: with c = 0 the 4 below at -x (j = -1) comes before the 4 that would stand above
    both = np.array([[[4, -2], [-2, 5], [4, -2]]], np.int32)
    assert trace_ground_path(both, (0, 0, 0), 2, 1, 0, (1, 1, 0), 64)[0].tolist()[:2] == [[1, 1, 0], [0, 0, 0]]
    assert trace_ground_path(both, (0, 0, 0), 3, 1, 0, (1, 1, 0), 64)[0].tolist()[:2] == [[1, 1, 0], [0, 2, 0]]   # -y: "below" is y + 1


# ---- the worlds tests/test_gpu_ground.py runs on the device: their facts, on the restatement ---------------------------------------
WORLD_DEPTH = 7


def ground_routes_cells():
    """floor y 3; platform x 64 .. 127, y 4 .. 7; two staircases x 56 .. 63 of heights 1 1 2 2 3 3 4 4 at z 8 .. 13 and z 34 .. 39; a
    hump x 30 .. 33, y 4 .. 5, z 0 .. 29; a bridge slab x 20 .. 28 at y 12; a wall x 45 .. 46, y 4 .. 11 with doors at z 10 .. 12 and
    z 30 .. 36; a beam x 80 .. 89 at y 11, z 0 .. 19"""
    zs = range(40)
    cells = [(x, 3, z) for z in zs for x in range(128)]
    cells += [(x, y, z) for z in zs for y in range(4, 8) for x in range(64, 128)]
    for z in list(range(8, 14)) + list(range(34, 40)):
        cells += [(56 + i, 4 + k, z) for i, h in enumerate((1, 1, 2, 2, 3, 3, 4, 4)) for k in range(h)]
    cells += [(x, y, z) for z in range(30) for y in (4, 5) for x in range(30, 34)]
    cells += [(x, 12, z) for z in zs for x in range(20, 29)]
    cells += [(x, y, z) for z in zs if not (10 <= z <= 12 or 30 <= z <= 36) for y in range(4, 12) for x in (45, 46)]
    cells += [(x, 11, z) for z in range(20) for x in range(80, 90)]
    return cells


GROUND_ROUTES = dict(origin=(0, 0, 0), dims=(128, 16, 40), up=2, seed=(10, 4, 5), start=(100, 8, 5))
# r, H, S, c -> |G|, reached (the seed's own cell included), cut off, cost at the start, path cells
GROUND_ROUTES_ROWS = {
    (0, 4, 2, 0): (5480, 4860, 620, 120, 121),                          # over the hump, door z 10 .. 12, near stairs, round the beam
    (0, 4, 2, 20): (5480, 4860, 620, 228, 149),                         # round the hump, door z 30 .. 36, far stairs
    (2, 4, 2, 0): (5165, 4545, 620, 148, 149),                          # the narrow door is closed to the body
    (0, 3, 2, 0): (5680, 5060, 620, 100, 101),                          # under the beam
    (0, 4, 4, 0): (5480, 5060, 420, 100, 101),                          # straight up the 4-cell kerb
    # no climbing at all.  By the definition 2284 cells are reached, counted by hand: x 0 .. 29 (1200), round the hump at z 30 .. 39
    # (40), x 34 .. 44 (440), the two doors (6 + 14), x 47 .. 55 (360), and x 56 .. 63 beside the staircases (8 * 28 = 224).
    (0, 4, 0, 0): (5480, 2284, 3196, -1, 0),
}
# the fifth row has S = 4 > H - 1 = 3, outside the call's limits: its figures hold on the definition, the call refuses the row
REFUSED_ROW = (0, 4, 4, 0)
_WORLDS = {}


def ground_routes():
    """-> dict: words, and per row of GROUND_ROUTES_ROWS the field of the definition; computed once and left unchanged"""
    if "routes" not in _WORLDS:
        w = dict(GROUND_ROUTES, words=cells_pool(ground_routes_cells(), WORLD_DEPTH), fields={})
        for r, H, S, c in GROUND_ROUTES_ROWS:
            w["fields"][r, H, S, c] = ground_field_words(w["words"], WORLD_DEPTH, w["origin"], w["dims"], w["up"], r, H, S, c, [w["seed"]],
                                                         step_below_height=(r, H, S, c) != REFUSED_ROW)[0]
        _WORLDS["routes"] = w
    return _WORLDS["routes"]


@pytest.mark.parametrize("row", sorted(GROUND_ROUTES_ROWS))
def test_ground_routes(row):
    w = ground_routes()
    r, H, S, c = row
    footholds, reached, cut, value, length = GROUND_ROUTES_ROWS[row]
    field = w["fields"][row]
    at = w["start"]
    assert ((field != -2).sum(), (field >= 0).sum(), (field == -1).sum()) == (footholds, reached, cut)
    assert field[at[2], at[1], at[0]] == value
    cells, n = trace_ground_path(field, w["origin"], w["up"], S, c, at, 400)
    assert n == length
    if length:
        path, climbed = check_ground_path(field, w["origin"], w["up"], S, c, at)
        assert np.array_equal(path, cells) and tuple(path[-1]) == w["seed"] and climbed >= 4
        x, z = path[:, 0], path[:, 2]
        over_hump = bool(((x >= 30) & (x <= 33) & (path[:, 1] == 6)).any())
        door = set(z[(x == 45) | (x == 46)].tolist())
        stairs = set(z[(x >= 56) & (x <= 63) & (path[:, 1] > 4)].tolist())
        if row == (0, 4, 2, 0):
            assert over_hump and door <= {10, 11, 12} and stairs <= set(range(8, 14)) and z[(x >= 80) & (x <= 89)].min() == 20
        if row in ((0, 4, 2, 20), (2, 4, 2, 0)):
            assert door and door <= set(range(30, 37)) and stairs and stairs <= set(range(34, 40))
        if row == (0, 4, 2, 20):
            assert not over_hump
        if row == (0, 3, 2, 0):
            assert ((x >= 80) & (x <= 89) & (z < 20)).any()
    if row in ((0, 4, 2, 20), (2, 4, 2, 0)):
        got, _ = ground_field_relaxed(w["words"], WORLD_DEPTH, w["origin"], w["dims"], w["up"], r, H, S, c, [w["seed"]])
        assert np.array_equal(got, field)


CORNER_STAIRS = dict(origin=(0, 0, 0), dims=(96, 96, 96), H=2, S=1, treads=80)


def corner_stairs(offset, up=2):
    """-> (words, seed, top_x, top_z): a floor at height `offset` over x, z = 0 .. 95; a solid staircase 4 wide (z 0 .. 3) rising one
    cell per cell along x from x = 9, 80 treads; the same along z (x 92 .. 95) from z = 9.  up = 5 (-z): the same world with (x, y,
    z) -> (x, z, 95 - y), inside the same region.  The seed stands on the floor at (6, 6); the tops are the last treads' cells."""
    cells = [(x, offset, z) for z in range(96) for x in range(96)]
    for i in range(1, CORNER_STAIRS["treads"] + 1):
        cells += [(8 + i, offset + k, z) for z in range(4) for k in range(1, i + 1)]
        cells += [(x, offset + k, 8 + i) for x in range(92, 96) for k in range(1, i + 1)]
    seed, top_x, top_z = (6, offset + 1, 6), (88, offset + 81, 1), (93, offset + 81, 88)
    if up == 5:
        turn = lambda p: (p[0], p[2], 95 - p[1])                        # noqa: E731
        cells, seed, top_x, top_z = [turn(p) for p in cells], turn(seed), turn(top_x), turn(top_z)
    return cells_pool(cells, WORLD_DEPTH), seed, top_x, top_z


def corner_stairs_costs(c):
    """the approach over the floor to the foot of each staircase, then 80 treads at 1 + c: from (6, 6) to x = 8 at z = 3 (2 + 3),
    and to z = 8 at x = 92 (86 + 2); the tops lie at z = 1 (2 more sideways) and x = 93 (1 more)"""
    return 5 + 80 * (1 + c) + 2, 88 + 80 * (1 + c) + 1


@pytest.mark.parametrize("offset", range(8))
def test_corner_stairs(offset):
    """whatever tile is chosen, at some offset a riser meets a tile corner in (x, up) and in (z, up)"""
    words, seed, top_x, top_z = corner_stairs(offset)
    k = CORNER_STAIRS
    for c in (0, 3):
        field, stats = ground_field_words(words, WORLD_DEPTH, k["origin"], k["dims"], 2, 0, k["H"], k["S"], c, [seed])
        assert stats["seeds_used"] == 1 and (field == -1).sum() == 0
        assert (field[top_x[2], top_x[1], top_x[0]], field[top_z[2], top_z[1], top_z[0]]) == corner_stairs_costs(c)
        assert check_ground_path(field, k["origin"], 2, k["S"], c, top_x)[1] == 80
    if offset == 5:                                                     # the slab z 0 .. 7: the floor and the staircase along x
        got, _ = ground_field_relaxed(words, WORLD_DEPTH, k["origin"], (96, 96, 8), 2, 0, k["H"], k["S"], 3, [seed])
        assert np.array_equal(got, ground_field_words(words, WORLD_DEPTH, k["origin"], (96, 96, 8), 2, 0, k["H"], k["S"], 3, [seed])[0])
        assert got[top_x[2], top_x[1], top_x[0]] == corner_stairs_costs(3)[0]


def test_corner_stairs_minus_z():
    words, seed, top_x, top_z = corner_stairs(3, up=5)
    k = CORNER_STAIRS
    field, stats = ground_field_words(words, WORLD_DEPTH, k["origin"], k["dims"], 5, 0, k["H"], k["S"], 3, [seed])
    assert stats["seeds_used"] == 1
    assert (field[top_x[2], top_x[1], top_x[0]], field[top_z[2], top_z[1], top_z[0]]) == corner_stairs_costs(3)


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_ground_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_ground_field", "svoslam_field_trace_ground_paths", "svoslam_workspace_ground_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    for name in ("ground_field", "trace_ground_paths", "plan_ground_paths"):
        assert callable(getattr(pkg, name, None)), name
    assert hasattr(pkg.Workspace, "ground_buffers")
    assert (pkg.UP_PLUS_Y, pkg.UP_MINUS_Y, pkg.UP_PLUS_Z, pkg.UP_MINUS_Z) == (2, 3, 4, 5) == tuple(UP[k] for k in ("+y", "-y", "+z", "-z"))
    assert (pkg.MAX_STEP_CELLS, pkg.MAX_HEIGHT_CELLS, pkg.MAX_SNAP_CELLS, pkg.MAX_RING_COST) == (MAX_STEP, MAX_HEIGHT, MAX_SNAP, MAX_CLIMB_COST)
    assert [f[0] for f in pkg._GroundStats._fields_] == ["footholds", "seeds_used", "rounds", "tile_runs"]
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_ground_field(" in header and "int svoslam_field_trace_ground_paths(" in header
    assert "typedef struct { int32_t footholds, seeds_used, rounds, tile_runs; } svoslam_ground_stats;" in header
    assert "#define SVOSLAM_MAX_STEP_CELLS %d" % MAX_STEP in header
    assert "int svoslam_workspace_ground_buffers(const svoslam_workspace *ws, void *d_ptrs[6], uint64_t bytes[6]);" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
