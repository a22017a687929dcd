"""Asking the map by volume (svoslam_pool_count_boxes, svoslam_pool_nearest_occupied; include/svoslam.h): the
specification restated in numpy on pool words, walk included; next_in by its definition beside the fast form the restatement
uses; hand-built pools with every output written out; and brute force over the occupied set, without the walk, on a pool fused by
the CPU oracle.  No GPU.

count_boxes_words and nearest_occupied_words below are what the device calls must produce; tests/test_gpu_volume.py compares
against them bit for bit, `steps` included."""
import ctypes as C
import os

import numpy as np
import pytest

from test_query_cpu import F, FLAG, MASK, NO_CELL, P, cell_in_block, mid, plane
from test_surface_cpu import CENTER, EDGE, HAND, HandPool, OPAQUE, occupied_cells, path_of, rgba
from util import surface_cloud

I64 = np.int64
BOX_FIELDS = ("count", "first_cell", "first_node", "steps")
NEAR_FIELDS = ("dist2", "cell", "node", "color", "steps")
MAX_RADIUS = 4096


# ---- the specification, restated -------------------------------------------------------------------------------------------
def morton_by_bits(x, y, z, depth):
    """bits of x, y, z interleaved, x lowest: the definition, bit by bit"""
    x, y, z = (np.asarray(v, I64) for v in (x, y, z))
    m = np.zeros(np.broadcast(x, y, z).shape, I64)
    for b in range(depth):
        m |= (((x >> b) & 1) | (((y >> b) & 1) << 1) | (((z >> b) & 1) << 2)) << (3 * b)
    return m


def unmorton_by_bits(m, depth):
    m = np.asarray(m, I64)
    x, y, z = np.zeros(m.shape, I64), np.zeros(m.shape, I64), np.zeros(m.shape, I64)
    for b in range(depth):
        t = m >> (3 * b)
        x |= (t & 1) << b
        y |= ((t >> 1) & 1) << b
        z |= ((t >> 2) & 1) << b
    return x, y, z


SPREAD = ((16, 0x0000FF0000FF), (8, 0x00F00F00F00F), (4, 0x0C30C30C30C3), (2, 0x249249249249))


def spread3(v):
    """bit i of v (i < 16) moved to bit 3i, by doubling shifts (the same codes as morton_by_bits, in a few operations)"""
    v = np.asarray(v, I64) & 0xFFFF
    for sh, mask in SPREAD:
        v = (v | (v << sh)) & mask
    return v


def compact3(m):
    m = np.asarray(m, I64) & SPREAD[-1][1]
    for sh, mask in ((2, SPREAD[2][1]), (4, SPREAD[1][1]), (8, SPREAD[0][1]), (16, 0xFFFF)):
        m = (m | (m >> sh)) & mask
    return m


def morton(x, y, z, depth=16):
    return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2)


def unmorton(m, depth=16):
    xyz = cells_of(m)
    return xyz[..., 0], xyz[..., 1], xyz[..., 2]


def cells_of(m):
    """[..., 3]: the cell coordinates of Morton codes"""
    m = np.asarray(m, I64)
    return compact3(np.stack([m, m >> 1, m >> 2], -1))


def next_in_by_definition(lo, hi, depth):
    """for every cursor m in 0 .. 8^depth: the smallest Morton code >= m whose cell lies in [lo, hi], 8^depth when there is none --
    every code of the lattice is tested against the range, then the minimum is taken over the codes from m on"""
    codes = np.arange(8 ** depth + 1)
    xyz = np.stack(unmorton_by_bits(codes, depth), -1)
    inside = ((xyz >= lo) & (xyz <= hi)).all(1) & (codes < 8 ** depth)
    return np.minimum.accumulate(np.where(inside, codes, 8 ** depth)[::-1])[::-1]


def highest_bit(v):
    """position of the highest set bit of v >= 0 (v < 2^52), -1 for 0"""
    return np.frexp(np.asarray(v, np.float64))[1].astype(I64) - 1


def next_in(m, lo, hi, depth):
    """next_in for arrays of cursors m[n] and ranges lo[n,3], hi[n,3]: a cursor outside its range skips the coarsest block around
    it that is disjoint from the range -- per violating axis the 2^b cells that share the coordinate's bits above b, b the highest
    bit in which it differs from the bound it violates, lie on its side of the bound -- until it is inside or past the lattice"""
    m = np.array(m, I64)
    end = I64(8) ** depth
    at = np.arange(m.size)                                            # the cursors not yet known to be inside
    while at.size:
        xyz = cells_of(m[at])
        diff = np.where(xyz < lo[at], xyz ^ lo[at], np.where(xyz > hi[at], xyz ^ hi[at], 0))
        s = highest_bit(diff.max(-1))                                 # of the largest difference: the highest bit of the three
        out = (s >= 0) & (m[at] < end)
        at, s = at[out], s[out]
        m[at] = ((m[at] >> (3 * s)) + 1) << (3 * s)
    return np.minimum(m, end)


def _walk(words, depth, lo, hi, live, stop_after=0, q=None, radius=0):
    """the walk of the specification over the ranges [lo, hi] of the entries `live`; q is None: the visit of count_boxes,
    otherwise that of nearest_occupied about the cells q with the prune"""
    words = np.asarray(words, dtype=np.uint32)
    w0, w1 = words[0::2].astype(I64), words[1::2].astype(I64)
    n = lo.shape[0]
    m, mhi = morton(lo[:, 0], lo[:, 1], lo[:, 2], depth), morton(hi[:, 0], hi[:, 1], hi[:, 2], depth)
    steps, count = np.zeros(n, np.uint32), np.zeros(n, I64)
    cell, node, color = np.full(n, NO_CELL, np.uint64), np.full(n, -1, np.int32), np.zeros(n, np.uint32)
    best = np.full(n, radius * radius + 1, I64)
    idx = np.nonzero(live)[0]
    while idx.size:
        mm = next_in(m[idx], lo[idx], hi[idx], depth)                 # step 2
        go = mm <= mhi[idx]                                           # step 3
        idx, mm = idx[go], mm[go]
        if idx.size == 0:
            break
        steps[idx] += 1                                               # step 4: one descent
        xyz = cells_of(mm)
        k = idx.size
        child, nd, lvl = np.zeros(k, I64), np.zeros(k, I64), np.zeros(k, I64)
        walking, hit = np.ones(k, bool), np.zeros(k, bool)
        for l in range(1, depth + 1):
            sh = depth - l
            if q is not None:                                         # before the load: the block's distance against the best
                blo = (xyz >> sh) << sh
                gap = np.maximum(np.maximum(blo - q[idx], q[idx] - (blo + (1 << sh) - 1)), 0)
                pruned = walking & ((gap * gap).sum(1) >= best[idx])
                lvl, walking = np.where(pruned, l, lvl), walking & ~pruned
            nd = np.where(walking, child + ((mm >> (3 * sh)) & 7), nd)
            free = walking & ((w1[nd] >> 24) <= 127)
            hit_now = walking & ~free & (l == depth)
            free |= walking & ~free & ~hit_now & ((w0[nd] & FLAG) == 0)
            stop = free | hit_now
            lvl, hit = np.where(stop, l, lvl), hit | hit_now
            walking = walking & ~stop
            child = np.where(walking, w0[nd] & MASK, child)
            if not walking.any():
                break
        at = idx[hit]
        packed = (xyz[hit, 0] | (xyz[hit, 1] << 16) | (xyz[hit, 2] << 32)).astype(np.uint64)
        if q is None:
            first = count[at] == 0
            cell[at[first]], node[at[first]] = packed[first], nd[hit][first].astype(np.int32)
            count[at] += 1
            done = hit & (stop_after > 0) & (count[idx] == stop_after)
        else:
            d2 = ((xyz[hit] - q[at]) ** 2).sum(1)
            assert (d2 < best[at]).all()                              # the prune guarantees it
            best[at], cell[at], node[at], color[at] = d2, packed, nd[hit].astype(np.int32), w1[nd[hit]].astype(np.uint32)
            done = hit & (best[idx] == 0)
        s = depth - lvl
        m[idx] = ((mm >> (3 * s)) + 1) << (3 * s)                     # the block's end; m + 1 after a visit (lvl == depth)
        idx = idx[~done]
    return steps, count, cell, node, color, best


def count_boxes_words(words, depth, center, edge, boxes, stop_after=0):
    """-> {"count" uint64, "first_cell" uint64, "first_node" int32, "steps" uint32}: svoslam_pool_count_boxes in numpy"""
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 6)
    n, n_side = boxes.shape[0], 1 << depth
    mn, mx = boxes[:, :3], boxes[:, 3:]
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    zero, full = np.zeros(n, I64), np.full(n, n_side, I64)
    with np.errstate(all="ignore"):
        p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
        empty = (~(mn <= mx) | (mx < p0[None, :]) | (mn > pn[None, :])).any(1)      # a NaN: not (mn <= mx)
        lo = np.stack([cell_in_block(c[a], n_side, h, mn[:, a], zero, full, False) for a in range(3)], 1)
        hi = np.stack([cell_in_block(c[a], n_side, h, mx[:, a], zero, full, True) for a in range(3)], 1)
    hi = np.maximum(lo, hi)
    steps, count, cell, node, _, _ = _walk(words, depth, lo, hi, ~empty, stop_after=int(stop_after))
    return {"count": count.astype(np.uint64), "first_cell": cell, "first_node": node, "steps": steps}


def nearest_occupied_words(words, depth, center, edge, points, radius_cells):
    """-> {"dist2" int32, "cell" uint64, "node" int32, "color" uint32, "steps" uint32}: svoslam_pool_nearest_occupied in numpy"""
    assert 0 <= radius_cells <= MAX_RADIUS
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    n, n_side = p.shape[0], 1 << depth
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    zero, full = np.zeros(n, I64), np.full(n, n_side, I64)
    with np.errstate(all="ignore"):
        p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
        inside = ((p0[None, :] <= p) & (p <= pn[None, :])).all(1)                    # false for a NaN
        q = np.stack([cell_in_block(c[a], n_side, h, p[:, a], zero, full, False) for a in range(3)], 1)
    lo, hi = np.maximum(q - radius_cells, 0), np.minimum(q + radius_cells, n_side - 1)
    steps, _, cell, node, color, best = _walk(words, depth, lo, hi, inside, q=q, radius=int(radius_cells))
    dist2 = np.where(inside, np.where(node >= 0, best, -1), -2).astype(np.int32)
    return {"dist2": dist2, "cell": cell, "node": node, "color": color, "steps": steps}


# ---- next_in ----------------------------------------------------------------------------------------------------------------
def test_next_in_fast_form_is_the_definition():
    rng = np.random.default_rng(14)
    depth, cursors = 3, np.arange(8 ** 3 + 1)
    for k in range(40):
        a, b = rng.integers(0, 8, 3), rng.integers(0, 8, 3)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        if k % 8 == 0:
            hi = lo.copy()                                            # a single cell
        if k % 8 == 1:
            lo, hi = np.array([0, lo[1], lo[2]]), np.array([7, lo[1], lo[2]])   # a row
        want = next_in_by_definition(lo, hi, depth).tolist()
        got = next_in(cursors, np.tile(lo, (cursors.size, 1)), np.tile(hi, (cursors.size, 1)), depth)
        assert got.tolist() == want, (lo, hi)
        assert want[0] == int(morton_by_bits(*lo, depth)) and want[int(morton_by_bits(*hi, depth))] == int(morton_by_bits(*hi, depth))
        assert want[int(morton_by_bits(*hi, depth)) + 1] == 8 ** depth       # nothing of the range lies beyond morton(hi)


def test_morton_round_trip_and_octants():
    rng = np.random.default_rng(2)
    xyz = rng.integers(0, 1 << 16, (200, 3))
    xyz[:4] = [(0, 0, 0), (65535, 65535, 65535), (65535, 0, 0), (0, 0, 65535)]
    m = morton_by_bits(xyz[:, 0], xyz[:, 1], xyz[:, 2], 16)
    assert np.array_equal(np.stack(unmorton_by_bits(m, 16), -1), xyz) and int(m.max()) == 8 ** 16 - 1
    assert np.array_equal(morton(xyz[:, 0], xyz[:, 1], xyz[:, 2]), m) and np.array_equal(np.stack(unmorton(m), -1), xyz)
    for k in range(0, 200, 17):
        path = path_of(*[int(v) for v in xyz[k]], 16)
        assert path == [(int(m[k]) >> (3 * (16 - l))) & 7 for l in range(1, 17)]


# ---- hand-built pools --------------------------------------------------------------------------------------------------------
INF = float("inf")
EMPTY = dict(count=0, first_cell=int(NO_CELL), first_node=-1, steps=0)
NOTHING = dict(first_cell=int(NO_CELL), first_node=-1)
OUTSIDE = dict(dist2=-2, cell=int(NO_CELL), node=-1, color=0, steps=0)
NONE_NEAR = dict(dist2=-1, cell=int(NO_CELL), node=-1, color=0)


def pack(x, y, z):
    return x | (y << 16) | (z << 32)


def inner(a, x, depth):
    """(min, max) strictly inside cell x of axis a"""
    lo, hi = float(P(a, x, depth)), float(P(a, x + 1, depth))
    return F(lo + 0.25 * (hi - lo)), F(hi - 0.25 * (hi - lo))


def box_of(spans):
    return [s[0] for s in spans] + [s[1] for s in spans]


def single_leaf_boxes():
    """one leaf at depth 1, 2 and 3.  A box that is one cell costs one step; the whole root costs 7 free siblings per level + the leaf.
    The axis of each plane test is one on which that plane is not a root face (there the count clamps and the cell is taken in)."""
    out = {}
    leaves = {1: ((1, 0, 1), 0, 1), 2: ((2, 1, 3), 0, 0), 3: ((5, 2, 6), 0, 0)}      # cell, axis of the lower-plane tests, of the upper
    for depth, (xyz, al, au) in leaves.items():
        pool = HandPool()
        col = rgba(40 + depth, 2, 3, 255)
        node = pool.put(path_of(*xyz, depth), [OPAQUE] * (depth - 1) + [col])
        own = [inner(a, xyz[a], depth) for a in range(3)]
        found = dict(count=1, first_cell=pack(*xyz), first_node=node, steps=1)
        free = dict(NOTHING, count=0, steps=1)

        def on(a, span):
            s = list(own)
            s[a] = span
            return box_of(s)
        boxes, want = [], []
        boxes.append(box_of(own)); want.append(found)                                                      # contains it
        boxes.append(box_of([(-INF, INF)] * 3)); want.append(dict(found, steps=7 * depth + 1))             # the whole root
        boxes.append(on(al, (P(al, xyz[al], depth), own[al][0]))); want.append(found)                      # min ON the lower plane
        boxes.append(on(au, (own[au][1], P(au, xyz[au] + 1, depth)))); want.append(found)                  # max ON the upper plane
        below = inner(al, xyz[al] - 1, depth)
        boxes.append(on(al, (below[0], P(al, xyz[al], depth)))); want.append(free)                         # max ON the lower plane
        above = inner(au, xyz[au] + 1, depth)
        boxes.append(on(au, (P(au, xyz[au] + 1, depth), above[1]))); want.append(free)                     # min ON the upper plane
        pt = [(mid(a, xyz[a], depth),) * 2 for a in range(3)]
        pt[al] = (P(al, xyz[al], depth),) * 2
        boxes.append(box_of(pt)); want.append(found)                                                       # a point-box on the lower plane
        pt = [(mid(a, xyz[a], depth),) * 2 for a in range(3)]
        pt[au] = (P(au, xyz[au] + 1, depth),) * 2
        boxes.append(box_of(pt)); want.append(free)                                                        # ... on the upper: the next cell
        boxes.append(on(al, below)); want.append(free)                                                     # misses: the cell beside
        nan, inv, off_lo, off_hi = box_of(own), box_of(own), box_of(own), box_of(own)
        nan[4] = np.nan
        inv[2], inv[5] = inv[5], inv[2]
        off_lo[0], off_lo[3] = -INF, np.nextafter(P(0, 0, depth), F(-INF))                                  # max below P(0)
        off_hi[1], off_hi[4] = np.nextafter(P(1, 1 << depth, depth), F(INF)), INF                           # min above P(N)
        for b in (nan, inv, off_lo, off_hi, [np.nan] * 6):
            boxes.append(b); want.append(EMPTY)
        out["single_leaf_depth_%d" % depth] = ("boxes", pool.words(), depth, np.array(boxes, F), 0, want)
    return out


def hand_cases():
    """name -> (kind, words, depth, boxes[n,6] or points[n,3], stop_after or radius, expected: one dict per entry)"""
    out = single_leaf_boxes()
    # a column -inf..+inf along y through (2, ., 3) at depth 2 with (2,1,3) and (2,3,3) occupied.  In Morton order: (2,0,3) free
    # cell, (2,1,3) hit, then the level-1 octant above: (2,2,3) free cell, (2,3,3) hit -- four steps, nothing else is in the range
    pool = HandPool()
    na = pool.put(path_of(2, 1, 3, 2), [OPAQUE, rgba(1, 1, 1, 255)])
    nb = pool.put(path_of(2, 3, 3, 2), [OPAQUE, rgba(2, 2, 2, 255)])
    col = box_of([inner(0, 2, 2), (-INF, INF), inner(2, 3, 2)])
    empty_col = box_of([inner(0, 1, 2), (-INF, INF), inner(2, 3, 2)])         # x = 1: two free level-1 blocks
    want = [dict(count=2, first_cell=pack(2, 1, 3), first_node=na, steps=4), dict(NOTHING, count=0, steps=2),
            dict(count=1, first_cell=pack(2, 1, 3), first_node=na, steps=2)]
    out["column"] = ("boxes", pool.words(), 2, np.array([col, empty_col], F), 0, want[:2])
    out["column_any_hit"] = ("boxes", pool.words(), 2, np.array([col], F), 1, want[2:])
    # alpha 127 beside 128 at depth 2: (2,2,2) counts, (3,2,2) is a free cell
    words = HAND["alpha_127_128"][0]
    hp = HandPool()
    node = hp.put(path_of(2, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 128)])
    hp.put(path_of(3, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 127)])
    assert np.array_equal(hp.words(), words)
    box = box_of([(inner(0, 2, 2)[0], inner(0, 3, 2)[1]), inner(1, 2, 2), inner(2, 2, 2)])
    out["alpha_127_128"] = ("boxes", words, 2, np.array([box], F), 0, [dict(count=1, first_cell=pack(2, 2, 2), first_node=node, steps=2)])
    # a saturated CHILDLESS level-2 node over x, y, z 2..3 contributes nothing at depth 3: from (2,3,3) it is one free block of 8
    # cells, which ends at the level-1 octant that holds (4,3,3), the only other cell of the range
    words = HAND["childless_above_depth"][0]
    hp = HandPool()
    hp.put(path_of(3, 3, 3, 3)[:2], [OPAQUE, OPAQUE])
    node = hp.put(path_of(4, 3, 3, 3), [OPAQUE] * 3)
    assert np.array_equal(hp.words(), words)
    box = box_of([(inner(0, 2, 3)[0], inner(0, 4, 3)[1]), inner(1, 3, 3), inner(2, 3, 3)])
    out["childless_above_depth"] = ("boxes", words, 3, np.array([box], F), 0,
                                    [dict(count=1, first_cell=pack(4, 3, 3), first_node=node, steps=2)])
    # three occupied cells at depth 2, the whole root: octant 0 holds (0,0,0), (1,0,0) and 6 free cells, octants 1..6 are free
    # blocks, octant 7 holds 7 free cells and (3,3,3): 8 + 6 + 8 steps unlimited
    pool = HandPool()
    n0 = pool.put(path_of(0, 0, 0, 2), [OPAQUE, rgba(1, 0, 0, 255)])
    pool.put(path_of(1, 0, 0, 2), [OPAQUE, rgba(2, 0, 0, 255)])
    pool.put(path_of(3, 3, 3, 2), [OPAQUE, rgba(3, 0, 0, 255)])
    root = np.array([box_of([(-INF, INF)] * 3)], F)
    for stop, (count, steps) in {1: (1, 1), 2: (2, 2), 0: (3, 22), -1: (3, 22), 3: (3, 22)}.items():
        out["stop_after_%d" % stop] = ("boxes", pool.words(), 2, root, stop, [dict(count=count, first_cell=pack(0, 0, 0), first_node=n0, steps=steps)])
    # ---- nearest ----
    # the point's own cell is occupied; a point ON the root's +x face is inside, in cell N-1.  R = 0: the range is that cell, one
    # step.  R = 2: the walk starts at morton(lo) = (0,0,0), and the five cells before (1,0,1) in Morton order, at D 2, 1, 3, 2, 1
    # (all below best = 5), are loaded and free: the hit is the sixth step, and best == 0 ends the walk there
    pool = HandPool()
    col = rgba(41, 2, 3, 255)
    node = pool.put([5], [col])                                       # (1,0,1) at depth 1
    own = [mid(a, v, 1) for a, v in enumerate((1, 0, 1))]
    face = [P(0, 2, 1), own[1], own[2]]
    beyond = [np.nextafter(P(0, 2, 1), F(INF)), own[1], own[2]]
    pts = np.array([own, face, beyond, [np.nan, own[1], own[2]], [own[0], -INF, own[2]]], F)
    for r, steps in ((0, 1), (2, 6)):
        here = dict(dist2=0, cell=pack(1, 0, 1), node=node, color=col, steps=steps)
        out["nearest_own_cell_radius_%d" % r] = ("points", pool.words(), 1, pts, r, [here, here, OUTSIDE, OUTSIDE, OUTSIDE])
    # from (0,0,1) the leaf (1,0,1) is at distance exactly 1.  R = 1: the range is the whole root, best starts at 2; in Morton order
    # (0,0,0) D 1 loaded and free, (1,0,0) D 2, (0,1,0) D 2, (1,1,0) D 3 pruned, (0,0,1) D 0 free, (1,0,1) D 1 the hit, then
    # (0,1,1) D 1 and (1,1,1) D 2 pruned against best = 1: 8 steps.  R = 0: the own cell alone, free: 1 step, nothing found
    pt = np.array([[mid(0, 0, 1), mid(1, 0, 1), mid(2, 1, 1)]], F)
    out["nearest_at_exactly_radius"] = ("points", pool.words(), 1, pt, 1, [dict(dist2=1, cell=pack(1, 0, 1), node=node, color=col, steps=8)])
    out["nearest_radius_minus_1"] = ("points", pool.words(), 1, pt, 0, [dict(NONE_NEAR, steps=1)])
    # depth 2, leaf (2,1,3), from (2,1,1): distance exactly 2.  R = 2: the range is the whole root, best starts at 5.  Level-1
    # octants 0..4 are nearer than that and free: 5 steps; octant 5 holds the leaf: its cells (2,0,2) D 2, (3,0,2) D 3, (2,1,2)
    # D 1, (3,1,2) D 2 are loaded and free, (2,0,3) D 5 and (3,0,3) D 6 pruned, (2,1,3) D 4 the hit, (3,1,3) D 5 pruned: 8 steps;
    # octants 6 (D 3) and 7 (D 2) are nearer than 4, loaded and free: 2 steps
    pool = HandPool()
    col = rgba(42, 2, 3, 255)
    node = pool.put(path_of(2, 1, 3, 2), [OPAQUE, col])
    pt = np.array([[mid(0, 2, 2), mid(1, 1, 2), mid(2, 1, 2)]], F)
    out["nearest_at_radius_2"] = ("points", pool.words(), 2, pt, 2, [dict(dist2=4, cell=pack(2, 1, 3), node=node, color=col, steps=15)])
    # R = 1: x 1..3, y 0..2, z 0..2, best starts at 2.  Octant 0 D 1 free, 1 D 0 free, 2 D 2 pruned, 3 D 1 free, 4 D 2 pruned: 5
    # steps; octant 5 (D 1) is loaded, its cells in the range: (2,0,2) D 2, (3,0,2) D 3 pruned, (2,1,2) D 1 free, (3,1,2) D 2
    # pruned: 4 steps; octants 6 (D 3) and 7 (D 2) pruned: 2 steps
    out["nearest_radius_1_misses"] = ("points", pool.words(), 2, pt, 1, [dict(NONE_NEAR, steps=11)])
    # two cells at the same distance 1 from (3,3,3) at depth 3: (2,3,3) lies in level-1 octant 0, (4,3,3) in octant 1: the lower
    # Morton code wins.  R = 1, best starts at 2: in octant 0 the range is the level-2 block 2..3 cubed: (2,2,2) D 3, (3,2,2) D 2,
    # (2,3,2) D 2 pruned, (3,3,2) D 1 free, (2,2,3) D 2 pruned, (3,2,3) D 1 free, (2,3,3) D 1 the hit, (3,3,3) D 0 free: 8 steps;
    # each of the other seven level-1 octants holds cells of the range and is at D >= 1 = best: pruned at level 1, 7 steps
    pool = HandPool()
    ca, cb = rgba(7, 7, 7, 255), rgba(8, 8, 8, 255)
    pool.put(path_of(4, 3, 3, 3), [OPAQUE, OPAQUE, cb])
    na = pool.put(path_of(2, 3, 3, 3), [OPAQUE, OPAQUE, ca])
    pt = np.array([[mid(0, 3, 3), mid(1, 3, 3), mid(2, 3, 3)]], F)
    out["nearest_tie_lowest_morton"] = ("points", pool.words(), 3, pt, 1, [dict(dist2=1, cell=pack(2, 3, 3), node=na, color=ca, steps=15)])
    return out


CASES = hand_cases()


def run_case(case, call_boxes, call_points, depth=None):
    kind, words, d, inputs, param, _ = case
    return (call_boxes if kind == "boxes" else call_points)(words, d if depth is None else depth, CENTER, EDGE, inputs, param)


def check_expected(got, want):
    for k, w in enumerate(want):
        for name, value in w.items():
            assert int(got[name][k]) == value, (k, name, int(got[name][k]), value)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_pools(name):
    case = CASES[name]
    got = run_case(case, count_boxes_words, nearest_occupied_words)
    fields = BOX_FIELDS if case[0] == "boxes" else NEAR_FIELDS
    assert set(got) == set(fields) and all(set(w) == set(fields) for w in case[5]) and len(case[5]) == case[3].shape[0]
    if case[0] == "boxes":
        assert got["count"].dtype == np.uint64 and got["first_cell"].dtype == np.uint64 and got["first_node"].dtype == np.int32
    else:
        assert got["dist2"].dtype == np.int32 and got["cell"].dtype == np.uint64 and got["node"].dtype == np.int32 and got["color"].dtype == np.uint32
    assert got["steps"].dtype == np.uint32
    check_expected(got, case[5])


# ---- against brute force over the occupied set, without the walk -------------------------------------------------------------------
DEPTH = 6
# the cloud (within +-1 of the origin) sits in one corner of this root, so that cells farther than 64 cells from every occupied one
# exist at depth 6 (the far corner is about 85 cells away) and the radius-64 query can come back empty
ROOT_CENTER, ROOT_EDGE = (3.0, 3.0, 3.0), 4.0


@pytest.fixture(scope="module")
def fused(oracle):
    pts, col = surface_cloud(np.random.default_rng(41), 15000)
    pool = oracle.Pool()
    for _ in range(2):
        pool.insert_cloud(pts, col, DEPTH, ROOT_CENTER, ROOT_EDGE)
    return pool.words(), pts


def count_cells(center, edge, depth, p, strict):
    """c_a(p) for p[n,3] as the specification words it: planes compared one by one"""
    n_side = 1 << depth
    h = F(edge) / F(n_side)
    with np.errstate(all="ignore"):
        return np.stack([((plane(center[a], np.arange(1, n_side), n_side, h)[None, :] < p[:, a, None]) if strict else
                          (plane(center[a], np.arange(1, n_side), n_side, h)[None, :] <= p[:, a, None])).sum(1) for a in range(3)], 1)


def seeded_boxes(pts, depth=DEPTH):
    """400 boxes with sides from one cell to half the root -- half of them about a fused point, the others anywhere in a cube a
    little larger than the root, so some poke out of it or lie outside -- and 64 columns of the whole height (y)"""
    rng = np.random.default_rng(23)
    cell = 2.0 * ROOT_EDGE / (1 << depth)
    c = np.asarray(ROOT_CENTER)
    mid_ = c + (rng.random((400, 3)) * 2 - 1) * ROOT_EDGE * 1.1
    mid_[:200] = pts[rng.integers(0, pts.shape[0], 200)] + rng.normal(scale=2 * cell, size=(200, 3))
    side = cell * (ROOT_EDGE / cell) ** rng.random((400, 3))             # log-uniform between one cell and half the root
    boxes = np.concatenate([mid_ - side / 2, mid_ + side / 2], 1)
    col_mid = c - ROOT_EDGE + rng.random((64, 3)) * np.array([2.5, 0, 2.5])  # over and beside the cloud's footprint
    w = cell * rng.integers(1, 4, (64, 1))
    cols = np.concatenate([col_mid - w / 2, col_mid + w / 2], 1)
    cols[:, 1], cols[:, 4] = -np.inf, np.inf
    return np.concatenate([boxes, cols]).astype(F)


def seeded_points(pts, depth=DEPTH):
    """2000 points: 1000 fused points moved by up to 3 cells per axis, 1000 anywhere in a cube a little larger than the root"""
    rng = np.random.default_rng(29)
    cell = 2.0 * ROOT_EDGE / (1 << depth)
    near = pts[rng.integers(0, pts.shape[0], 1000)] + (rng.random((1000, 3)) * 2 - 1) * 3 * cell
    far = np.asarray(ROOT_CENTER) + (rng.random((1000, 3)) * 2 - 1) * ROOT_EDGE * 1.02
    return np.concatenate([near, far]).astype(F)


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
def test_count_boxes_against_brute_force(fused, depth):
    words, pts = fused
    boxes = seeded_boxes(pts)
    xyz, nodes = occupied_cells(words, depth)
    code = morton(xyz[:, 0], xyz[:, 1], xyz[:, 2], depth)
    n_side = 1 << depth
    h = F(ROOT_EDGE) / F(n_side)
    p0, pn = plane(np.asarray(ROOT_CENTER, F), np.zeros(3, I64), n_side, h), plane(np.asarray(ROOT_CENTER, F), np.full(3, n_side), n_side, h)
    mn, mx = boxes[:, :3], boxes[:, 3:]
    empty = (mn > mx).any(1) | (mx < p0).any(1) | (mn > pn).any(1)
    lo = count_cells(ROOT_CENTER, ROOT_EDGE, depth, mn, False)
    hi = np.maximum(lo, count_cells(ROOT_CENTER, ROOT_EDGE, depth, mx, True))
    want_count, want_cell, want_node = np.zeros(boxes.shape[0], np.uint64), np.full(boxes.shape[0], NO_CELL, np.uint64), np.full(boxes.shape[0], -1, np.int32)
    for k in np.nonzero(~empty)[0]:
        inside = ((xyz >= lo[k]) & (xyz <= hi[k])).all(1)
        want_count[k] = inside.sum()
        if inside.any():
            first = np.nonzero(inside)[0][np.argmin(code[inside])]
            want_cell[k], want_node[k] = pack(*[int(v) for v in xyz[first]]), nodes[first]
    assert (want_count > 0).sum() > 50 and (want_count == 0).sum() > 50 and empty.sum() > 5 and (want_count[400:] > 0).sum() > 10
    assert (mn < p0).any() and (mx > pn).any() and (want_count[(mn < p0).any(1) | (mx > pn).any(1)] > 0).any()   # some poke out and still count
    got = count_boxes_words(words, depth, ROOT_CENTER, ROOT_EDGE, boxes)
    assert np.array_equal(got["count"], want_count) and np.array_equal(got["first_cell"], want_cell)
    assert np.array_equal(got["first_node"], want_node) and (got["steps"][empty] == 0).all() and (got["steps"][~empty] >= 1).all()
    for stop in (1, 5):
        lim = count_boxes_words(words, depth, ROOT_CENTER, ROOT_EDGE, boxes, stop)
        assert np.array_equal(lim["count"], np.minimum(want_count, np.uint64(stop))) and np.array_equal(lim["first_cell"], want_cell)
        assert np.array_equal(lim["first_node"], want_node) and (lim["steps"] <= got["steps"]).all()


def brute_nearest(words, depth, points, radius):
    xyz, nodes = occupied_cells(words, depth)
    code = morton(xyz[:, 0], xyz[:, 1], xyz[:, 2], depth)
    order = np.argsort(code)                                          # ties: argmin takes the first, the lowest Morton code
    xyz, nodes = xyz[order], nodes[order]
    n_side = 1 << depth
    h = F(ROOT_EDGE) / F(n_side)
    c = np.asarray(ROOT_CENTER, F)
    p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
    with np.errstate(all="ignore"):
        inside = ((p0 <= points) & (points <= pn)).all(1)
    q = count_cells(ROOT_CENTER, ROOT_EDGE, depth, points, False)
    d2 = ((xyz[None, :, :] - q[:, None, :]) ** 2).sum(2)
    at = d2.argmin(1)
    near = d2[np.arange(q.shape[0]), at]
    found = inside & (near <= radius * radius)
    dist2 = np.where(inside, np.where(found, near, -1), -2).astype(np.int32)
    cell = np.where(found, xyz[at, 0] | (xyz[at, 1] << 16) | (xyz[at, 2] << 32), -1).astype(np.uint64)
    return dist2, cell, np.where(found, nodes[at], -1).astype(np.int32), np.where(found, words[1::2][nodes[at]], 0).astype(np.uint32)


@pytest.mark.parametrize("radius", [0, 3, 64])
def test_nearest_occupied_against_brute_force(fused, radius):
    words, pts = fused
    points = seeded_points(pts)
    positive = none = 0
    for depth in (DEPTH, DEPTH - 2):
        dist2, cell, node, color = brute_nearest(words, depth, points, radius)
        got = nearest_occupied_words(words, depth, ROOT_CENTER, ROOT_EDGE, points, radius)
        assert np.array_equal(got["dist2"], dist2) and np.array_equal(got["cell"], cell)
        assert np.array_equal(got["node"], node) and np.array_equal(got["color"], color)
        assert ((got["steps"] == 0) == (dist2 == -2)).all() and (dist2 == -2).sum() > 10 and (dist2 == 0).sum() > 50
        positive, none = positive + int((dist2 > 0).sum()), none + int((dist2 == -1).sum())
        # at depth 4 every cell of the lattice is within 64 cells of every other (3 * 15^2 < 64^2): -1 cannot occur there
        if radius >= 3 and radius * radius < 3 * ((1 << depth) - 1) ** 2:
            assert (dist2 > 0).sum() > 100 and (dist2 == -1).sum() > 20, (depth, (dist2 > 0).sum(), (dist2 == -1).sum())
    if radius >= 3:
        assert positive > 100 and none > 20


def test_radius_limit_is_what_an_int32_holds():
    assert 3 * MAX_RADIUS * MAX_RADIUS < 2 ** 31 and MAX_RADIUS * MAX_RADIUS + 1 < 2 ** 31


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_library_exports_the_volume_calls():
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_count_boxes", "svoslam_pool_nearest_occupied"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "count_boxes") and hasattr(pkg, "nearest_occupied")
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "svoslam_pool_count_boxes(" in header and "svoslam_pool_nearest_occupied(" in header
    assert "#define SVOSLAM_STAGE_COUNT 13" in header and "#define SVOSLAM_MAX_RADIUS_CELLS %d" % MAX_RADIUS in header
