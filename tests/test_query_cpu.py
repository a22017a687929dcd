"""Asking the map (svoslam_pool_cast_rays, svoslam_pool_query_points; include/svoslam.h): the specification
restated in numpy on pool words, hand-built pools with their expected outputs written out, and checks that do not go through the
restatement's own geometry (float64 slab tests against the occupied set) on a pool fused by the CPU oracle.  No GPU.

cast_rays_words and query_points_words below are what the device calls must produce; tests/test_gpu_query.py compares against them
bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from test_oracle_second_opinion import walk as second_opinion_walk
from test_surface_cpu import CENTER, EDGE, HAND, HandPool, OPAQUE, occupied_cells, path_of, rgba, surface_face_masks
from util import surface_cloud

F = np.float32
FLAG, MASK = 0x40000000, 0x3FFFFFFF
NO_CELL = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the specification, restated -------------------------------------------------------------------------------------------
def plane(c, k, n_side, h):
    """P(k) = c + (float)(2k - N) * h: one conversion, one product, one sum, each binary32"""
    return (F(c) + (2 * np.asarray(k, np.int64) - n_side).astype(F) * F(h)).astype(F)


def cell_in_block(c, n_side, h, p, lo, size, strict):
    """lo + the number of k in lo+1 .. lo+size-1 with P(k) <= p (< p where `strict`), per element: the count c_a(p) of the
    specification clamped to the block [lo, lo + size - 1] (size a power of two; the whole axis is lo = 0, size = N).  Planes
    ascend with k, so probing finds the count; a NaN counts nothing."""
    k, s = np.array(lo, np.int64), np.array(size, np.int64) >> 1
    while (s > 0).any():
        pl = plane(c, k + s, n_side, h)
        ok = (s > 0) & np.where(strict, pl < p, pl <= p)
        k = np.where(ok, k + s, k)
        s = s >> 1
    return k


def count_by_comparison(c, n_side, h, p, strict):
    """c_a(p) exactly as the specification words it (for the test of cell_in_block)"""
    pl = plane(c, np.arange(1, n_side), n_side, h)
    return int((pl < p).sum() if strict else (pl <= p).sum())


def cast_rays_words(words, depth, center, edge, rays, t_max=None):
    """-> {"t" float32, "node" int32, "cell" uint64, "color" uint32, "steps" uint32}: svoslam_pool_cast_rays in numpy"""
    words = np.asarray(words, dtype=np.uint32)
    w0, w1 = words[0::2].astype(np.int64), words[1::2].astype(np.int64)
    rays = np.asarray(rays, dtype=F).reshape(-1, 6)
    n, n_side = rays.shape[0], 1 << depth
    o, v = rays[:, :3], rays[:, 3:]
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    tmax = np.full(n, np.inf, F) if t_max is None else np.asarray(t_max, F).reshape(n)
    t = np.full(n, np.nan, F)
    node, cell = np.full(n, -1, np.int32), np.full(n, NO_CELL, np.uint64)
    color, steps = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    valid = np.isfinite(rays).all(1) & (v != 0).any(1)
    t[valid] = np.inf
    pos, neg, nz = v > 0, v < 0, v != 0
    zero, full = np.zeros(n, np.int64), np.full(n, n_side, np.int64)
    with np.errstate(all="ignore"):
        r = np.where(nz, F(1.0) / np.where(nz, v, F(1.0)), F(0.0)).astype(F)
        p0, pn = plane(c, np.zeros(3, np.int64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
        in_slab = (p0[None, :] <= o) & (o <= pn[None, :])
        inside = valid & in_slab.all(1)
        q_in = np.stack([cell_in_block(c[a], n_side, h, o[:, a], zero, full, neg[:, a]) for a in range(3)], 1)
        tn = ((np.where(pos, p0[None, :], pn[None, :]) - o) * r).astype(F)
        tx = ((np.where(pos, pn[None, :], p0[None, :]) - o) * r).astype(F)
        te, tf, ax = np.full(n, -np.inf, F), np.full(n, np.inf, F), np.full(n, -1, np.int64)
        for a in range(3):
            m = nz[:, a] & (tn[:, a] > te)                       # strictly greater: the lowest axis that attains the largest
            te, ax = np.where(m, tn[:, a], te), np.where(m, a, ax)
            m = nz[:, a] & (tx[:, a] < tf)
            tf = np.where(m, tx[:, a], tf)
        miss = (~nz & ~in_slab).any(1) | (ax < 0) | (te < 0) | (te > tf)
        axc = np.maximum(ax, 0)
        q_out = np.stack([cell_in_block(c[a], n_side, h, (o[:, a] + te * v[:, a]).astype(F), zero, full, neg[:, a]) for a in range(3)], 1)
        for a in range(3):
            q_out[:, a] = np.where(ax == a, np.where(pos[:, a], 0, n_side - 1), q_out[:, a])
        v_ax = v[np.arange(n), axc]
        q = np.where(inside[:, None], q_in, q_out)
        face = np.where(inside, 6, 2 * axc + np.where(v_ax > 0, 0, 1))
        tc = np.where(inside, F(0.0), te).astype(F)
        live = valid & (inside | ~miss)
        live &= ~(tc > tmax)
        idx = np.nonzero(live)[0]
        for _ in range(3 * n_side):
            if idx.size == 0:
                break
            steps[idx] += 1
            qq, m = q[idx], idx.size
            child, nd, lvl = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
            walking, hit = np.ones(m, bool), np.zeros(m, bool)
            for l in range(1, depth + 1):
                sh = depth - l
                octant = ((qq[:, 0] >> sh) & 1) | (((qq[:, 1] >> sh) & 1) << 1) | (((qq[:, 2] >> sh) & 1) << 2)
                nd = np.where(walking, child + octant, nd)
                free = walking & ((w1[nd] >> 24) <= 127)
                hit_now = walking & ~free & (l == depth)
                free |= walking & ~free & ~hit_now & ((w0[nd] & FLAG) == 0)
                stop = free | hit_now
                lvl, hit = np.where(stop, l, lvl), hit | hit_now
                walking = walking & ~stop
                child = np.where(walking, w0[nd] & MASK, child)
                if not walking.any():
                    break
            hi = idx[hit]
            t[hi], node[hi], color[hi] = tc[hi], nd[hit].astype(np.int32), w1[nd[hit]].astype(np.uint32)
            cell[hi] = (q[hi, 0] | (q[hi, 1] << 16) | (q[hi, 2] << 32) | (face[hi] << 48)).astype(np.uint64)
            go = ~hit
            idx, qq, lvl = idx[go], qq[go], lvl[go]
            if idx.size == 0:
                break
            sh = depth - lvl
            size, lo = 1 << sh, (qq >> sh[:, None]) << sh[:, None]
            oo, vv, rr = o[idx], v[idx], r[idx]
            tl, ax = np.full(idx.size, np.inf, F), np.full(idx.size, -1, np.int64)
            for a in range(3):
                kp = np.where(pos[idx, a], lo[:, a] + size, lo[:, a])
                tp = ((plane(c[a], kp, n_side, h) - oo[:, a]) * rr[:, a]).astype(F)
                m = nz[idx, a] & (tp < tl)                       # strictly smaller: the lowest axis on a tie
                tl, ax = np.where(m, tp, tl), np.where(m, a, ax)
            new_q = np.empty_like(qq)
            for a in range(3):
                k = cell_in_block(c[a], n_side, h, (oo[:, a] + tl * vv[:, a]).astype(F), lo[:, a], size, neg[idx, a])
                k = np.where(pos[idx, a], np.maximum(k, qq[:, a]), np.where(neg[idx, a], np.minimum(k, qq[:, a]), k))
                new_q[:, a] = np.where(ax == a, np.where(pos[idx, a], lo[:, a] + size, lo[:, a] - 1), k)
            left = ((new_q < 0) | (new_q >= n_side)).any(1)
            axc = np.maximum(ax, 0)
            new_t = np.where(tl > tc[idx], tl, tc[idx]).astype(F)
            keep = (ax >= 0) & ~left & ~(new_t > tmax[idx])
            ik = idx[keep]
            q[ik], tc[ik] = new_q[keep], new_t[keep]
            face[ik] = (2 * axc + np.where(vv[np.arange(idx.size), axc] > 0, 0, 1))[keep]
            idx = ik
    return {"t": t, "node": node, "cell": cell, "color": color, "steps": steps}


def query_points_words(words, depth, center, edge, points):
    """-> {"node" int32, "level" int32, "key" uint64, "color" uint32}: svoslam_pool_query_points in numpy"""
    words = np.asarray(words, dtype=np.uint32)
    w0, w1 = words[0::2].astype(np.int64), words[1::2].astype(np.int64)
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    c = np.tile(np.asarray(center, F), (n, 1))
    e = F(edge)
    with np.errstate(all="ignore"):
        inside = ((c - e <= p) & (p <= c + e)).all(1)
    node, level = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    key, color = np.where(inside, 1, 0).astype(np.int64), np.zeros(n, np.int64)
    child, walking = np.zeros(n, np.int64), inside.copy()
    for l in range(1, depth + 1):
        gt = p > c
        octant = gt[:, 0].astype(np.int64) + 2 * gt[:, 1] + 4 * gt[:, 2]
        node = np.where(walking, child + octant, node)
        key = np.where(walking, (key << 3) + octant, key)
        level = np.where(walking, l, level)
        at = np.maximum(node, 0)
        color = np.where(walking, w1[at], color)
        walking = walking & ((w0[at] & FLAG) != 0) & (l < depth)
        child = np.where(walking, w0[at] & MASK, child)
        e = e / F(2.0)
        c = np.where(walking[:, None], c + np.where(gt, e, -e), c).astype(F)
        if not walking.any():
            break
    return {"node": node.astype(np.int32), "level": level.astype(np.int32), "key": key.astype(np.uint64), "color": color.astype(np.uint32)}


def test_cell_in_block_is_the_count_by_comparison():
    rng = np.random.default_rng(5)
    for depth in (1, 3, 6):
        n_side = 1 << depth
        h = F(EDGE) / F(n_side)
        planes = plane(F(CENTER[0]), np.arange(0, n_side + 1), n_side, h)
        ps = np.concatenate([planes, np.nextafter(planes, F(np.inf)), np.nextafter(planes, F(-np.inf)),
                             (rng.random(40) * 2.4 - 1.2).astype(F), np.array([np.nan, np.inf, -np.inf], F)]).astype(F)
        for strict in (False, True):
            got = cell_in_block(F(CENTER[0]), n_side, h, ps, np.zeros(ps.size, np.int64), np.full(ps.size, n_side), np.full(ps.size, strict))
            assert got.tolist() == [count_by_comparison(F(CENTER[0]), n_side, h, p, strict) for p in ps]
            if depth == 6:                                         # clamped to a block: the count, clamped
                lo = np.full(ps.size, 24, np.int64)
                blk = cell_in_block(F(CENTER[0]), n_side, h, ps, lo, np.full(ps.size, 8), np.full(ps.size, strict))
                assert np.array_equal(blk, np.clip(got, 24, 31))


# ---- hand-built pools --------------------------------------------------------------------------------------------------------
def P(a, k, depth, center=CENTER, edge=EDGE):
    """plane k of axis a, scalar by scalar"""
    n_side = 1 << depth
    return F(F(center[a]) + F(2 * k - n_side) * (F(edge) / F(n_side)))


def mid(a, x, depth, center=CENTER, edge=EDGE):
    return F((float(P(a, x, depth, center, edge)) + float(P(a, x + 1, depth, center, edge))) / 2)


def pack(x, y, z, face):
    return x | (y << 16) | (z << 32) | (face << 48)


MISS = dict(t=F(np.inf), node=-1, cell=int(NO_CELL), color=0)
INVALID = dict(t=F(np.nan), node=-1, cell=int(NO_CELL), color=0, steps=0)


def single_leaf_cases():
    """a single occupied leaf at depth 1, 2 and 3, from each of the six sides along an axis and from inside.  Along an axis the
    free blocks in front of cell coordinate x are one per set bit of x coming from below and one per clear bit coming from above
    (the siblings of the path's nodes): the steps below are those counts + 1, written out."""
    out = {}
    leaves = {1: ((1, 0, 1), [(2, 1), (1, 2), (2, 1)]),              # per axis: (steps from the low side, from the high side)
              2: ((2, 1, 3), [(2, 2), (2, 2), (3, 1)]),
              3: ((5, 2, 6), [(3, 2), (2, 3), (3, 2)])}
    for depth, (xyz, steps) in leaves.items():
        pool = HandPool()
        col = rgba(40 + depth, 2, 3, 255)
        node = pool.put(path_of(*xyz, depth), [OPAQUE] * (depth - 1) + [col])
        rays, want = [], []
        centre = [mid(a, xyz[a], depth) for a in range(3)]
        for a in range(3):
            for side in (0, 1):                                    # 0: from below, moving up, entering through the - face
                o, v = list(centre), [0.0, 0.0, 0.0]
                o[a] = F(centre[a] + (-3.0 if side == 0 else 3.0))
                v[a] = 1.0 if side == 0 else -1.0
                rays.append(o + v)
                t_hit = F(F(P(a, xyz[a] + side, depth) - o[a]) * F(v[a]))   # (plane - o) * (1 / v)
                want.append(dict(t=t_hit, node=node, cell=pack(*xyz, 2 * a + side), color=col, steps=steps[a][side]))
        rays.append(centre + [0.3, -0.5, 0.8])
        want.append(dict(t=F(0.0), node=node, cell=pack(*xyz, 6), color=col, steps=1))
        out["single_leaf_depth_%d" % depth] = (pool.words(), depth, CENTER, EDGE, np.array(rays, F), None, want)
    return out


def hand_cases():
    """name -> (words, depth, center, edge, rays[n,6], t_max or None, expected: one dict per ray)"""
    out = single_leaf_cases()
    # only (7,7,7) is occupied at depth 3: the row y = 1, z = 1 crosses two level-1 octants, one step each, and leaves the root
    pool = HandPool()
    pool.put(path_of(7, 7, 7, 3), [OPAQUE] * 3)
    ray = [F(-3.0), mid(1, 1, 3), mid(2, 1, 3), 1.0, 0.0, 0.0]
    out["free_coarse_blocks"] = (pool.words(), 3, CENTER, EDGE, np.array([ray], F), None, [dict(MISS, steps=2)])
    # a saturated CHILDLESS level-2 node covers x, y, z in 2..3: at depth 3 it is one free block; (4,3,3) behind it is the hit
    words = HAND["childless_above_depth"][0]
    hp = HandPool()
    hp.put(path_of(3, 3, 3, 3)[:2], [OPAQUE, OPAQUE])
    node = hp.put(path_of(4, 3, 3, 3), [OPAQUE] * 3)
    assert np.array_equal(hp.words(), words)
    o = [F(-3.0), mid(1, 3, 3), mid(2, 3, 3)]
    want = dict(t=F(P(0, 4, 3) - o[0]), node=node, cell=pack(4, 3, 3, 0), color=OPAQUE, steps=3)   # blocks x 0..1, 2..3, then 4
    out["childless_above_depth"] = (words, 3, CENTER, EDGE, np.array([o + [1.0, 0.0, 0.0]], F), None, [want])
    # alpha 127 is free, alpha 128 is occupied: coming down x, (3,2,2) is passed and (2,2,2) is hit through its +x face
    words = HAND["alpha_127_128"][0]
    hp = HandPool()
    node = hp.put(path_of(2, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 128)])
    hp.put(path_of(3, 2, 2, 2), [OPAQUE, rgba(5, 5, 5, 127)])
    assert np.array_equal(hp.words(), words)
    o = [F(3.0), mid(1, 2, 2), mid(2, 2, 2)]
    want = dict(t=F(F(P(0, 3, 2) - o[0]) * F(-1.0)), node=node, cell=pack(2, 2, 2, 1), color=rgba(5, 5, 5, 128), steps=2)
    out["alpha_127_128"] = (words, 2, CENTER, EDGE, np.array([o + [-1.0, 0.0, 0.0]], F), None, [want])
    # rays in the lattice plane y = P(2) between B = (2,1,3) and A = (2,2,3): with v_y == 0 the comparison is <=, the ray runs in
    # the row y = 2 whichever way it goes along x.  An origin ON the plane x = P(2): moving up it is in cell 2 (A, at t = 0), moving
    # down it is in cell 1 (free: the level-1 block x 0..1 in one step, then out of the root)
    pool = HandPool()
    ca, cb = rgba(1, 1, 1, 255), rgba(2, 2, 2, 255)
    na = pool.put(path_of(2, 2, 3, 2), [OPAQUE, ca])
    pool.put(path_of(2, 1, 3, 2), [OPAQUE, cb])
    y, z = P(1, 2, 2), mid(2, 3, 2)
    rays = [[F(-3.0), y, z, 1.0, 0.0, 0.0], [F(3.0), y, z, -1.0, 0.0, 0.0],
            [P(0, 2, 2), mid(1, 2, 2), z, 1.0, 0.0, 0.0], [P(0, 2, 2), mid(1, 2, 2), z, -1.0, 0.0, 0.0]]
    want = [dict(t=F(P(0, 2, 2) - F(-3.0)), node=na, cell=pack(2, 2, 3, 0), color=ca, steps=2),      # block x 0..1, then A
            dict(t=F(F(P(0, 3, 2) - F(3.0)) * F(-1.0)), node=na, cell=pack(2, 2, 3, 1), color=ca, steps=2),   # (3,2,3), then A
            dict(t=F(0.0), node=na, cell=pack(2, 2, 3, 6), color=ca, steps=1),
            dict(MISS, steps=1)]
    out["along_a_lattice_plane"] = (pool.words(), 2, CENTER, EDGE, np.array(rays, F), None, want)
    # the diagonal through the root's centre (a root with exactly representable planes): every parameter ties, the lowest axis
    # goes first -- (0,0,0), (1,0,0), (1,1,0), then the occupied (1,1,1) through its -z face, all at t = 2 after the entry at t = 1
    pool = HandPool()
    node = pool.put([7], [OPAQUE])
    rays = [[-2.0, -2.0, -2.0, 1.0, 1.0, 1.0]]
    want = [dict(t=F(2.0), node=node, cell=pack(1, 1, 1, 4), color=OPAQUE, steps=4)]
    out["corner_tie_lowest_axis"] = (pool.words(), 1, (0.0, 0.0, 0.0), 1.0, np.array(rays, F), None, want)
    # origins outside: a zero component outside its slab; slabs that do not overlap; the root behind the origin
    pool = HandPool()
    pool.put([0], [OPAQUE])
    pool.put([7], [OPAQUE])
    rays = [[-3.0, 5.0, 0.0, 1.0, 0.0, 0.0], [-3.0, -3.0, 0.0, 1.0, -0.1, 0.0], [3.0, 0.3, 0.3, 1.0, 0.0, 0.0]]
    out["origin_outside_misses"] = (pool.words(), 1, CENTER, EDGE, np.array(rays, F), None, [dict(MISS, steps=0)] * 3)
    # t_max just below the hit parameter is a miss (the block in front was visited), at it and just above it is the hit
    words, depth, _, _, rays, _, want = out["single_leaf_depth_3"]
    ray, hit = rays[0], want[0]                                    # from -x: 3 steps, the third is the leaf
    tm = np.array([np.nextafter(hit["t"], F(-np.inf)), hit["t"], np.nextafter(hit["t"], F(np.inf)), -1.0], F)
    out["t_max"] = (words, depth, CENTER, EDGE, np.tile(ray, (4, 1)), tm, [dict(MISS, steps=2), hit, hit, dict(MISS, steps=0)])
    # invalid rays do no traversal
    rays = [[np.nan, 0, 0, 1, 0, 0], [0, 0, 0, np.inf, 0, 0], [0, 0, 0, 0, 0, 0], [0, -np.inf, 0, 0, 1, 0], [0, 0, 0, 1, np.nan, 0]]
    out["invalid_rays"] = (words, depth, CENTER, EDGE, np.array(rays, F), None, [INVALID] * 5)
    return out


CASES = hand_cases()


def check_expected(got, want):
    for k, w in enumerate(want):
        assert F(got["t"][k]).view(np.uint32) == F(w["t"]).view(np.uint32) or (np.isnan(w["t"]) and np.isnan(got["t"][k])), (k, got["t"][k], w["t"])
        assert int(got["node"][k]) == w["node"] and int(got["cell"][k]) == w["cell"], (k, int(got["node"][k]), hex(int(got["cell"][k])))
        assert int(got["color"][k]) == w["color"] and int(got["steps"][k]) == w["steps"], (k, int(got["color"][k]), int(got["steps"][k]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_pools(name):
    words, depth, center, edge, rays, t_max, want = CASES[name]
    got = cast_rays_words(words, depth, center, edge, rays, t_max)
    assert got["t"].dtype == F and got["node"].dtype == np.int32 and got["cell"].dtype == np.uint64
    assert got["color"].dtype == np.uint32 and got["steps"].dtype == np.uint32 and len(want) == rays.shape[0]
    check_expected(got, want)


# ---- a fused pool: checks that do not use the restatement's geometry ------------------------------------------------------------
DEPTH = 6
EPS = 2.0 ** -16          # absolute; |center| + edge <= 2 and unit directions: 128 ulp at magnitude 1, a depth-6 cell is 2^-5 wide


@pytest.fixture(scope="module")
def fused(oracle):
    pts, col = surface_cloud(np.random.default_rng(41), 15000)
    pool = oracle.Pool()
    for _ in range(2):
        pool.insert_cloud(pts, col, DEPTH, CENTER, EDGE)
    return pool.words(), pts


def seeded_rays(n, seed=7):
    """half from inside the root, half from outside aimed at a point in it; unit directions (rounded to binary32)"""
    rng = np.random.default_rng(seed)
    c = np.asarray(CENTER, np.float64)
    o = c + (rng.random((n, 3)) * 2 - 1) * EDGE * 0.999
    v = rng.normal(size=(n, 3))
    k = n // 2
    far = rng.normal(size=(n - k, 3))
    o[k:] = c + far / np.linalg.norm(far, axis=1, keepdims=True) * (2.0 + rng.random((n - k, 1)))
    v[k:] = c + (rng.random((n - k, 3)) * 2 - 1) * EDGE * 0.9 - o[k:]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([o, v], 1).astype(F)


def slab(rays, lo, hi):
    """float64 slab test of every ray against every box: (t_in, t_out)[n, m]; the ray meets the box iff t_out >= max(t_in, 0)"""
    o, v = rays[:, None, :3].astype(np.float64), rays[:, None, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        t1, t2 = (lo[None] - o) / v, (hi[None] - o) / v
        para = v == 0
        ok = (lo[None] <= o) & (o <= hi[None])
        near = np.where(para, np.where(ok, -np.inf, np.inf), np.minimum(t1, t2))
        far = np.where(para, np.where(ok, np.inf, -np.inf), np.maximum(t1, t2))
    return near.max(2), far.min(2)


def check_against_the_occupied_set(words, depth, rays, t_max, res, geometry=True):
    """properties (a) - (d) of a cast's result ((a) and (b) alone with geometry=False: (c) and (d) take unit directions);
    returns the number of hits and of those the exact ray meets"""
    xyz, nodes = occupied_cells(words, depth)
    masks = surface_face_masks(words, depth)
    n_side = 1 << depth
    code = (xyz[:, 2] * n_side + xyz[:, 1]) * n_side + xyz[:, 0]
    order = np.argsort(code)
    cell = res["cell"].astype(np.uint64)
    hit = res["node"] >= 0
    assert np.array_equal(hit, np.isfinite(res["t"])) and not np.isnan(res["t"]).any()
    x, y, z, face = (int(0xFFFF) & cell).astype(np.int64), ((cell >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64), \
        ((cell >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64), (cell >> np.uint64(48)).astype(np.int64)
    hc = (z[hit] * n_side + y[hit]) * n_side + x[hit]
    at = np.clip(np.searchsorted(code[order], hc), 0, code.size - 1)
    assert (code[order][at] == hc).all()                                             # (a) every hit cell is occupied
    which = order[at]
    assert np.array_equal(nodes[which], res["node"][hit]) and np.array_equal(words[1::2][nodes[which]], res["color"][hit])
    fh = face[hit]
    assert ((fh >= 0) & (fh <= 6)).all()
    ext = fh < 6
    assert ((masks[which][ext] >> fh[ext]) & 1).all()                               # (b) the face entered is exposed
    assert (cell[~hit] == NO_CELL).all() and (res["color"][~hit] == 0).all()
    if not geometry:
        return int(hit.sum()), 0
    planes = np.stack([plane(CENTER[a], np.arange(n_side + 1), n_side, F(EDGE) / F(n_side)) for a in range(3)], 1).astype(np.float64)
    lo = np.stack([planes[xyz[:, a], a] for a in range(3)], 1)
    hi = np.stack([planes[xyz[:, a] + 1, a] for a in range(3)], 1)
    t = res["t"].astype(np.float64)
    limit = np.full(t.shape, np.inf) if t_max is None else np.asarray(t_max, np.float64)
    hits_at = np.nonzero(hit)[0]
    for s in range(0, rays.shape[0], 128):
        rr, tt = rays[s:s + 128], t[s:s + 128]
        # (d) no occupied cell, deflated by eps, is met before t - eps; for a miss none is met within t_max
        t_in, t_out = slab(rr, lo + EPS, hi - EPS)
        met = t_out >= np.maximum(t_in, 0.0)
        first = np.where(met, np.maximum(t_in, 0.0), np.inf).min(1)
        bound = np.where(np.isfinite(tt), tt - EPS, limit[s:s + 128])
        assert (first >= bound).all(), (s, np.nonzero(first < bound)[0][:5])
    # (c) the ray meets the hit cell inflated by eps, and enters it within eps of t
    o, v = rays[hits_at, :3].astype(np.float64), rays[hits_at, 3:].astype(np.float64)

    def own_cell(grow):
        with np.errstate(all="ignore"):
            t1, t2 = (lo[which] - grow - o) / v, (hi[which] + grow - o) / v
            ok = (lo[which] - grow <= o) & (o <= hi[which] + grow)
            near = np.where(v == 0, np.where(ok, -np.inf, np.inf), np.minimum(t1, t2)).max(1)
            far = np.where(v == 0, np.where(ok, np.inf, -np.inf), np.maximum(t1, t2)).min(1)
        return np.maximum(near, 0.0), far
    th = t[hits_at]
    a_in, a_out = own_cell(EPS)
    assert (a_out >= a_in).all()                                                     # met
    assert ((a_in - EPS <= th) & (th <= a_out + EPS)).all()                          # the point at t lies in it
    e_in, e_out = own_cell(0.0)
    exact = e_out >= e_in                                                            # where the exact ray meets the exact cell:
    assert (np.abs(e_in - th)[exact] <= EPS).all(), np.abs(e_in - th)[exact].max()   # its entry parameter is t, within eps
    d_in, d_out = own_cell(-EPS)
    deep = d_out >= d_in
    assert (d_in[deep] >= th[deep] - EPS).all()                                      # (the deflated hit cell: not before t - eps)
    return int(hit.sum()), int(exact.sum())


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
def test_restatement_against_the_occupied_set(fused, depth):
    words, _ = fused
    rays = seeded_rays(2000)
    for t_max in (None, (np.random.default_rng(3).random(2000) * 3.0).astype(F)):
        res = cast_rays_words(words, depth, CENTER, EDGE, rays, t_max)
        hits, exact = check_against_the_occupied_set(words, depth, rays, t_max, res)
        assert hits > 400 and exact > 0.99 * hits and (res["steps"][res["node"] >= 0] >= 1).all()
        assert int(res["steps"].max()) <= 3 * (1 << depth)


# ---- point lookup ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 6, 9])
def test_fused_points_are_found_in_their_leaf(oracle, depth):
    pts, col = surface_cloud(np.random.default_rng(41), 15000)
    pts[5] = np.nan
    pool = oracle.Pool()
    pool.insert_cloud(pts, col, depth, CENTER, EDGE)
    words = pool.words()
    got = query_points_words(words, depth, CENTER, EDGE, pts)
    fin = np.isfinite(pts).all(1)
    assert fin.sum() == pts.shape[0] - 1 and got["node"][5] == -1 and got["level"][5] == 0 and got["key"][5] == 0 and got["color"][5] == 0
    keys = oracle.compute_keys(pts, depth, CENTER, EDGE)
    assert (got["level"][fin] == depth).all() and np.array_equal(got["key"][fin].astype(np.int64), keys[fin])
    octree = words.tolist()
    for k in np.nonzero(fin)[0][::37]:
        assert second_opinion_walk(octree, int(keys[k]))[0] == got["node"][k]
    assert np.array_equal(got["color"][fin], words[1::2][got["node"][fin]])
    # above the fused depth the lookup stops at the leaf, below it at the mip node on the same path
    deeper = query_points_words(words, depth + 3, CENTER, EDGE, pts)
    for name in ("node", "level", "key", "color"):
        assert np.array_equal(deeper[name], got[name])
    if depth > 1:
        above = query_points_words(words, depth - 1, CENTER, EDGE, pts)
        assert (above["level"][fin] == depth - 1).all() and np.array_equal(above["key"][fin], got["key"][fin] >> np.uint64(3))


def test_points_outside_on_the_faces_and_nan():
    pool = HandPool()
    n0 = pool.put([0, 7], [rgba(1, 1, 1, 200), rgba(2, 2, 2, 255)])
    words = pool.words()
    c, e = np.asarray(CENTER, F), F(EDGE)
    lo, hi = c - e, c + e
    pts = np.array([lo, hi, c,                                                       # two corners of the root (inside), its centre
                    [np.nextafter(hi[0], F(np.inf)), c[1], c[2]], [c[0], np.nextafter(lo[1], F(-np.inf)), c[2]],
                    [np.nan, c[1], c[2]], [c[0], c[1], np.inf], [lo[0], hi[1], lo[2]]], F)
    got = query_points_words(words, 2, CENTER, EDGE, pts)
    # the low corner: octant 0 at level 1, which has children, then octant 0 of its tile; the centre is not > the centre: octant 0,
    # then it is above the level-2 centre on every axis: octant 7, the put node; the high corner: octant 7, childless: level 1;
    # the last point is above the centre on y alone: octant 2, childless
    assert got["node"].tolist() == [8, 7, n0, -1, -1, -1, -1, 2]
    assert got["level"].tolist() == [2, 1, 2, 0, 0, 0, 0, 1]
    assert got["key"].tolist() == [0o100, 0o17, 0o107, 0, 0, 0, 0, 0o12]
    assert got["color"].tolist() == [0, 0, rgba(2, 2, 2, 255), 0, 0, 0, 0, 0]


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_library_exports_the_query_calls():
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_cast_rays", "svoslam_pool_query_points"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "cast_rays") and hasattr(pkg, "query_points")
    assert pkg.STAGE_QUERY == 12 and pkg.STAGE_NAMES[12] == "query" and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
