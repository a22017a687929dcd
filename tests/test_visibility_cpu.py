"""The visibility field of a map region (svoslam_pool_visibility_field; include/svoslam.h): the definition
restated as brute force -- for every cell of the bounding box of v and q an exact closed-cube / segment test with
fractions.Fraction; the integer walk from v towards q as a second restatement, as a scalar walk that lists the cells it tests and
as a numpy walk vectorised over the (viewpoint, cell) pairs; the restatements proven equal on every target of [-7, 7]^3, on a pool
fused by the CPU oracle and on hand-built pools with every value written out.  No GPU.

visibility_field_walk below is what the device call must produce; tests/test_gpu_visibility.py compares against it bit for bit."""
import ctypes as C
import itertools
import os
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

from test_field_cpu import fused_regions, region_cells
from test_reach_cpu import cells_pool
from test_surface_cpu import HandPool, load_pkg, occupied_cells
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
MAX_VIEWS_MASK = 32                                                     # include/svoslam.h SVOSLAM_MAX_VIEWS_MASK
CPU_RANGES = (0, 1, 3, 8)


# ---- the specification, restated -------------------------------------------------------------------------------------------
def occupancy(words, depth):
    """bool [N, N, N], indexed [z, y, x]: the occupied set at `depth`"""
    n_side = 1 << depth
    occ = np.zeros((n_side,) * 3, bool)
    xyz = occupied_cells(words, depth)[0]
    occ[xyz[:, 2], xyz[:, 1], xyz[:, 0]] = True
    return occ


@lru_cache(maxsize=None)
def _slab(d, c):
    """the closed interval of the parameter t over which the point 1/2 + t d of one axis lies in [c, c + 1] (d != 0): in doubled
    coordinates 2 c <= 1 + 2 t d <= 2 c + 2"""
    a, b = Fraction(2 * c - 1, 2 * d), Fraction(2 * c + 1, 2 * d)
    return (a, b) if a <= b else (b, a)


@lru_cache(maxsize=None)
def supercover_brute(D):
    """S(0, D) by its definition: the cells c of the bounding box of 0 and D, other than the two, whose closed cube meets the closed
    segment from the centre of cell 0 to the centre of cell D.  -> int64 [m, 3].  (The definition is geometric, so S(v, q) is
    v + S(0, q - v).)"""
    out = []
    spans = [range(min(0, d), max(0, d) + 1) for d in D]
    for c in itertools.product(*spans):
        if c == (0, 0, 0) or c == D:
            continue
        lo, hi = Fraction(0), Fraction(1)
        for a in range(3):
            if D[a] == 0:                                               # the coordinate stays 1/2: in [c, c + 1] iff c == 0, which the span says
                continue
            s_lo, s_hi = _slab(D[a], c[a])
            lo, hi = max(lo, s_lo), min(hi, s_hi)
        if lo <= hi:                                                    # closed against closed: a touch counts
            out.append(c)
    return np.asarray(out, I64).reshape(-1, 3)


def walk_cells(D):
    """the integer walk of the specification from cell 0 towards cell D: the cells it tests, in order (never 0, never D).  Axis a
    has made i_a of its |D_a| crossings; its next one is at (2 i_a + 1) / (2 |D_a|); two of them compare by cross-multiplication.
    Where two or three axes cross at once the side cells are tested before the diagonal step."""
    n = [abs(d) for d in D]
    s = [(d > 0) - (d < 0) for d in D]
    i, c, out = [0, 0, 0], [0, 0, 0], []
    while c != list(D):
        live = [a for a in range(3) if i[a] < n[a]]
        first = [a for a in live if all((2 * i[a] + 1) * n[b] <= (2 * i[b] + 1) * n[a] for b in live)]
        assert first and all((2 * i[a] + 1) * n[b] == (2 * i[b] + 1) * n[a] for a in first for b in first)
        assert max((2 * i[a] + 1) * n[b] for a in live for b in range(3)) < 1 << 25
        if len(first) > 1:
            for k in range(1, len(first)):
                for sub in itertools.combinations(first, k):            # every non-empty proper subset of the crossing axes
                    side = list(c)
                    for a in sub:
                        side[a] += s[a]
                    out.append(tuple(side))
        for a in first:
            c[a] += s[a]
            i[a] += 1
        if c != list(D):
            out.append(tuple(c))
    return out


def counting(views, depth):
    v = np.asarray(views, I64).reshape(-1, 3)
    return ((v >= 0) & (v < (1 << depth))).all(1)


def cells_in_range(origin, dims, v, radius):
    """int64 [m, 3]: the cells q of the region with |q - v|^2 <= radius^2"""
    spans = [np.arange(max(origin[a], v[a] - radius), min(origin[a] + dims[a], v[a] + radius + 1), dtype=I64) for a in range(3)]
    x, y, z = np.meshgrid(*spans, indexing="ij")
    q = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1)
    return q[((q - np.asarray(v, I64)) ** 2).sum(1) <= radius * radius]


def walk_pairs(occ, v, q):
    """bool [n]: for the pairs v[n, 3], q[n, 3] of cells of the root, whether no cell of S(v, q) is occupied -- the integer walk,
    all pairs at once.  Per axis the key (2 i_a + 1) * (the product of the other two |D|, a zero taken as 1) orders the next
    crossings as cross-multiplication does; an axis with D_a = 0 never crosses; an axis that has made all its crossings has a key
    above every live one.  Equal keys are a tie."""
    v, q = np.asarray(v, I64).reshape(-1, 3), np.asarray(q, I64).reshape(-1, 3)
    d = q - v
    n, s = np.abs(d), np.sign(d)
    m = np.maximum(n, 1)
    grow = 2 * np.stack([m[:, 1] * m[:, 2], m[:, 0] * m[:, 2], m[:, 0] * m[:, 1]], 1)
    key = np.where(n > 0, grow // 2, I64(1) << 62)
    c = v.copy()
    seen = np.ones(v.shape[0], bool)
    live = np.nonzero((d != 0).any(1))[0]
    subsets = [np.array([(k >> a) & 1 for a in range(3)], bool) for k in range(1, 7)]
    while live.size:
        k, cc, ss = key[live], c[live], s[live]
        first = k == k.min(1)[:, None]
        blocked = np.zeros(live.size, bool)
        tie = first.sum(1) > 1
        if tie.any():
            for sub in subsets:                                         # the proper subsets of the crossing axes
                at = np.nonzero(tie & ~(sub & ~first).any(1) & (sub != first).any(1))[0]
                if at.size:
                    p = cc[at] + ss[at] * sub
                    blocked[at] |= occ[p[:, 2], p[:, 1], p[:, 0]]
        cc = cc + ss * first
        key[live] = k + grow[live] * first
        c[live] = cc
        arrived = (cc == q[live]).all(1)
        blocked |= occ[cc[:, 2], cc[:, 1], cc[:, 0]] & ~arrived & ~blocked
        seen[live[blocked]] = False
        live = live[~(blocked | arrived)]
    return seen


def _field(depth, origin, dims, radius, views, sight):
    """the two outputs from `sight(v, q[m, 3]) -> bool [m]`: mask only for at most 32 viewpoints"""
    assert 0 <= radius <= MAX_RADIUS and all(n >= 0 for n in dims)
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) for a in range(3))
    views = np.asarray(views, I64).reshape(-1, 3)
    shape = (dims[2], dims[1], dims[0])
    mask, count = np.zeros(shape, np.uint32), np.zeros(shape, np.int32)
    done = {}
    for k in np.nonzero(counting(views, depth))[0]:
        v = tuple(int(a) for a in views[k])
        if v not in done:
            q = cells_in_range(origin, dims, v, radius)
            q = q[sight(v, q)] - np.asarray(origin, I64)
            done[v] = (q[:, 2], q[:, 1], q[:, 0])
        if k < MAX_VIEWS_MASK:
            mask[done[v]] |= np.uint32(1 << k)
        count[done[v]] += 1
    out = {"count": count}
    if views.shape[0] <= MAX_VIEWS_MASK:
        out["mask"] = mask
    return out


def visibility_field_brute(occ, depth, origin, dims, radius, views):
    """-> {"mask" uint32, "count" int32}, each [nz, ny, nx]: svoslam_pool_visibility_field by its definition"""
    def sight(v, q):
        out = np.zeros(q.shape[0], bool)
        for j in range(q.shape[0]):
            c = supercover_brute(tuple(int(a) for a in q[j] - np.asarray(v))) + np.asarray(v, I64)
            out[j] = not occ[c[:, 2], c[:, 1], c[:, 0]].any()
        return out
    return _field(depth, origin, dims, radius, views, sight)


def visibility_field_walk(occ, depth, origin, dims, radius, views):
    """the same outputs by the device's route: the integer walk from v towards q"""
    return _field(depth, origin, dims, radius, views, lambda v, q: walk_pairs(occ, np.broadcast_to(np.asarray(v, I64), q.shape), q))


def visibility_at(occ, depth, cells, radius, views):
    """(mask uint32 [m] or None above 32 viewpoints, count int32 [m]): the field's values at the cells[m, 3] alone, by the walk --
    for a region too large to walk all of it on the host"""
    cells, views = np.asarray(cells, I64).reshape(-1, 3), np.asarray(views, I64).reshape(-1, 3)
    mask, count = np.zeros(cells.shape[0], np.uint32), np.zeros(cells.shape[0], np.int32)
    done = {}
    for k in np.nonzero(counting(views, depth))[0]:
        v = tuple(int(a) for a in views[k])
        if v not in done:
            at = np.nonzero(((cells - views[k]) ** 2).sum(1) <= radius * radius)[0]
            done[v] = at[walk_pairs(occ, np.broadcast_to(views[k], (at.size, 3)), cells[at])]
        if k < MAX_VIEWS_MASK:
            mask[done[v]] |= np.uint32(1 << k)
        count[done[v]] += 1
    return (mask if views.shape[0] <= MAX_VIEWS_MASK else None), count


def same_outputs(got, want, names=None):
    for name in names or sorted(want):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape)
        bad = np.argwhere(got[name] != want[name])
        assert bad.shape[0] == 0, (name, bad.shape[0], bad[:5].tolist(), got[name][tuple(bad[:5].T)].tolist(),
                                   want[name][tuple(bad[:5].T)].tolist())


def seen_and_in_range(occ, depth, origin, dims, radius, views):
    """(pairs seen, pairs in range) over the counting viewpoints, by the walk"""
    views = np.asarray(views, I64).reshape(-1, 3)
    live = counting(views, depth)
    in_range = sum(cells_in_range(origin, dims, tuple(int(a) for a in v), radius).shape[0] for v in views[live])
    return int(visibility_field_walk(occ, depth, origin, dims, radius, views)["count"].sum()), in_range


def choose_views(occ, depth, origin, dims, radius, count, seed, where="mixed"):
    """`count` viewpoints [count, 3] for a region: cells a step or two off the occupied cells of the region inflated by the range
    (where a line of sight has something to decide), anywhere in that box if it holds none; "inside": in the region, "outside": in
    the root but not in the region, "mixed": either.  From 5 viewpoints on one in eight lies outside the root (it does not count),
    one in eight repeats viewpoint 0, and one lies in the root far from the region; they stand in the middle of the list, so
    that the bits after them show that nothing was renumbered."""
    rng = np.random.default_rng(seed)
    n_side = 1 << depth
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    lo, hi = np.maximum(o - max(radius, 2), 0), np.minimum(o + n + max(radius, 2), n_side)
    z, y, x = np.nonzero(occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
    near = np.stack([x, y, z], 1) + lo
    if near.shape[0]:
        cand = near[rng.integers(0, near.shape[0], 4000)] + rng.integers(-2, 3, (4000, 3))
    else:
        cand = rng.integers(lo, hi, (4000, 3))
    cand = np.concatenate([cand, rng.integers(lo, hi, (4000, 3)), rng.integers(o, o + n, (4000, 3))])
    cand = cand[rng.permutation(cand.shape[0])]
    cand = cand[((cand >= 0) & (cand < n_side)).all(1)]
    inside = ((cand >= o) & (cand < o + n)).all(1)
    if where == "inside" or (where == "outside" and inside.all()):
        cand = cand[inside]
    elif where == "outside":
        cand = cand[~inside]
    views = cand[:count].copy()
    assert views.shape[0] == count
    if count >= 5:
        extra = max(1, count // 8)
        for j in range(extra):
            views[1 + 3 * j] = [(-1, 5, 5), (n_side, 0, 0), (3, -7, 2), (4, 4, n_side + 9)][j % 4]
            views[2 + 3 * j] = views[0]
        views[3] = [0 if 2 * (o[a] + n[a] // 2) > n_side else n_side - 1 for a in range(3)]
    return views.astype(np.int32)


# ---- the two restatements of the supercover ----------------------------------------------------------------------------------
def test_the_walk_is_the_supercover_for_every_target_within_7():
    """all 3375 targets of [-7, 7]^3 from the origin: the walk's cells are the definition's, no cell is tested twice, and the set
    is symmetric in v and q"""
    ties = 0
    for D in itertools.product(range(-7, 8), repeat=3):
        cells = walk_cells(D)
        brute = {tuple(c) for c in supercover_brute(D).tolist()}
        assert len(set(cells)) == len(cells) and set(cells) == brute, (D, sorted(set(cells) ^ brute))
        back = {tuple(np.asarray(c) + np.asarray(D)) for c in supercover_brute(tuple(-d for d in D)).tolist()}
        assert back == brute, D
        ties += len(cells) > sum(abs(d) for d in D) - 1 > 0              # a tie of two axes: one step fewer, two side cells more
    assert ties > 500                                                   # many of the targets pass through an edge or a corner


def test_the_numpy_walk_is_the_scalar_walk():
    """every target of [-5, 5]^3 against every single blocker of its bounding box: the vectorised walk answers as the cell list"""
    for D in itertools.product(range(-5, 6, 1), repeat=3):
        if D[0] < 0 or (D[0] == 0 and D[1] < 0):                        # the mirrored half is the test above's symmetry
            continue
        v = np.array([5, 5, 5], I64)
        tested = set(walk_cells(D))
        box = [c for c in itertools.product(*[range(min(0, d), max(0, d) + 1) for d in D])]
        occs = np.zeros((len(box), 11, 11, 11), bool)
        for j, c in enumerate(box):
            occs[j, c[2] + 5, c[1] + 5, c[0] + 5] = True
        big = occs.reshape(-1, 11, 11)                                  # the scenes stacked along z: one walk for all of them
        vs = np.stack([np.array([5, 5, 5 + 11 * j]) for j in range(len(box))])
        got = walk_pairs(big, vs, vs + np.asarray(D))
        want = np.array([c not in tested for c in box])
        assert np.array_equal(got, want), D


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_occ(fused):
    return occupancy(fused[0], DEPTH)


# the (placement, region, range) cases in which no pair can be blocked, whatever the viewpoints -- written out, and each entry's
# reason is asserted in the test: at R = 0 and R = 1 only the viewpoint's cell and its face neighbours are in range, with nothing
# between; high_corner and offset_37 have no occupied cell within 8 cells of them; a viewpoint inside one_cell is the cell itself
NOTHING_TO_DECIDE = ({(w, r, radius) for w in ("inside", "outside") for r in fused_regions(DEPTH) for radius in (0, 1)} |
                     {(w, r, radius) for w in ("inside", "outside") for r in ("high_corner", "offset_37") for radius in (3, 8)} |
                     {("inside", "one_cell", radius) for radius in (3, 8)})


def deciding_views(occ, origin, dims, radius, where, seed):
    """5 viewpoints for the region, chosen until some in-range cell is seen and some is not (at most 40 seeded choices)"""
    for k in range(40):
        views = choose_views(occ, DEPTH, origin, dims, radius, 5, seed + 1000 * k, where)
        s, r = seen_and_in_range(occ, DEPTH, origin, dims, radius, views)
        if 0 < s < r:
            break
    return views, s, r


@pytest.mark.parametrize("radius", CPU_RANGES)
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
@pytest.mark.parametrize("where", ["inside", "outside"])
def test_the_walk_is_the_definition_on_the_fused_pool(fused_occ, where, region, radius):
    """per region of fused_regions(6) and range, with 5 viewpoints in the region or outside it, chosen so that the case decides
    something: some in-range cells of counting viewpoints are seen and some are not.  The cases where that cannot be are listed in
    NOTHING_TO_DECIDE; for those the reason is asserted instead"""
    origin, dims = fused_regions(DEPTH)[region]
    views, seen, in_range = deciding_views(fused_occ, origin, dims, radius, where, 100 + sorted(fused_regions(DEPTH)).index(region))
    want = visibility_field_brute(fused_occ, DEPTH, origin, dims, radius, views)
    same_outputs(visibility_field_walk(fused_occ, DEPTH, origin, dims, radius, views), want)
    assert np.array_equal(want["count"], popcount(want["mask"])) and seen == int(want["count"].sum())
    if (where, region, radius) not in NOTHING_TO_DECIDE:
        assert 0 < seen < in_range, (seen, in_range)
    elif radius >= 2 and region != "one_cell":                          # no occupied cell within the range of any cell of the region
        lo, hi = np.maximum(np.asarray(origin) - radius, 0), np.asarray(origin) + np.asarray(dims) + radius
        assert not fused_occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any()
    elif radius >= 2:                                                   # the one cell seen from itself
        assert dims == (1, 1, 1) and where == "inside" and seen == in_range
    else:                                                               # nothing lies between a cell and its face neighbour
        assert seen == in_range


def popcount(mask):
    return sum(((mask >> np.uint32(k)) & np.uint32(1)).astype(np.int32) for k in range(32))


def test_sight_is_symmetric_on_the_fused_pool(fused_occ):
    """the field from viewpoint a read at b equals the field from b read at a"""
    rng = np.random.default_rng(7)
    z, y, x = np.nonzero(fused_occ)
    near = np.stack([x, y, z], 1)
    a = np.clip(near[rng.integers(0, near.shape[0], 3000)] + rng.integers(-3, 4, (3000, 3)), 0, 63)
    b = np.clip(a + rng.integers(-9, 10, (3000, 3)), 0, 63)
    ab, ba = walk_pairs(fused_occ, a, b), walk_pairs(fused_occ, b, a)
    assert np.array_equal(ab, ba) and ab.sum() > 300 and (~ab).sum() > 300
    for j in range(40):                                                 # ... and through the field itself
        va, vb = [int(t) for t in a[j]], [int(t) for t in b[j]]
        fa = visibility_field_walk(fused_occ, DEPTH, vb, (1, 1, 1), 16, [va])["mask"][0, 0, 0]
        fb = visibility_field_walk(fused_occ, DEPTH, va, (1, 1, 1), 16, [vb])["mask"][0, 0, 0]
        assert fa == fb == int(ab[j])


# ---- hand-built pools: every value written out -----------------------------------------------------------------------------------
HAND_DEPTH = 4                                                          # a root of 16 cells a side
V0 = (0, 0, 0)


def hand_cases():
    """name -> (occupied cells, range, viewpoints, {cell: the mask expected there}); the field is taken over the whole root"""
    out = {}

    def one(name, occupied, q, seen, radius=6, v=V0):
        out[name] = (occupied, radius, [v], {q: int(seen)})
    # q = (1,1,0): the segment passes through the edge between (1,0,0) and (0,1,0): either blocks
    one("edge_x_side", [(1, 0, 0)], (1, 1, 0), False)
    one("edge_y_side", [(0, 1, 0)], (1, 1, 0), False)
    one("edge_both_sides", [(1, 0, 0), (0, 1, 0)], (1, 1, 0), False)
    one("edge_nothing", [(2, 2, 0), (1, 1, 1)], (1, 1, 0), True)
    # q = (2,1,0) has no tie: the cells are (1,0,0) and (1,1,0)
    one("no_tie_first", [(1, 0, 0)], (2, 1, 0), False)
    one("no_tie_second", [(1, 1, 0)], (2, 1, 0), False)
    one("no_tie_beside", [(0, 1, 0), (2, 0, 0)], (2, 1, 0), True)
    # q = (3,1,0) ties in the middle, between (1,0,0) (2,0,0) (1,1,0) (2,1,0)
    one("middle_tie_low", [(2, 0, 0)], (3, 1, 0), False)
    one("middle_tie_high", [(1, 1, 0)], (3, 1, 0), False)
    one("middle_tie_beside", [(0, 1, 0), (3, 0, 0), (1, 2, 0)], (3, 1, 0), True)
    # q = (1,1,1): through the corner; each of the six other cells of the 2^3 block alone blocks
    for c in itertools.product((0, 1), repeat=3):
        if c not in ((0, 0, 0), (1, 1, 1)):
            one("corner_%d%d%d" % c, [c], (1, 1, 1), False)
    # q = (3,3,1): a three-axis tie at the midpoint, the corner (2,2,1) of the cells (1..2, 1..2, 0..1)
    one("midpoint_corner", [(2, 2, 0)], (3, 3, 1), False)
    one("midpoint_corner_beside", [(0, 0, 1)], (3, 3, 1), True)
    one("occupied_target_is_seen", [(4, 2, 1)], (4, 2, 1), True)
    one("occupied_viewpoint_is_ignored", [(0, 0, 0)], (4, 2, 1), True)
    one("occupied_viewpoint_sees_itself", [(0, 0, 0)], (0, 0, 0), True)
    out["range_0_sees_only_the_viewpoint"] = ([], 0, [(3, 4, 5)], {(3, 4, 5): 1, (4, 4, 5): 0, (3, 3, 5): 0, (3, 4, 6): 0, (2, 4, 5): 0})
    one("range_5_reaches_3_4_0", [], (3, 4, 0), True, radius=5)
    one("range_4_does_not", [], (3, 4, 0), False, radius=4)
    # the wall x = 3 with the hole (3,8,8), seen from (1,8,8): behind it a cell is seen iff the segment stays strictly inside the
    # hole over the wall's thickness, x from 3 to 4: it leaves the wall 5/2 cells of x from the viewpoint's centre, |dy| 5 / (2 dx) <
    # 1/2 off the axis, so 5 |dy| < dx and 5 |dz| < dx, dx = x - 1; a touch of the hole's rim (5 |dy| == dx) is blocked.  In front of
    # the wall everything is seen
    wall = [(3, y, z) for y in range(16) for z in range(16) if (y, z) != (8, 8)]
    behind = {(x, y, z): int(5 * abs(y - 8) < x - 1 and 5 * abs(z - 8) < x - 1) for x in range(4, 16) for y in range(16) for z in range(16)}
    behind.update({(x, y, z): 1 for x in range(3) for y in range(16) for z in range(16)})
    behind[(3, 8, 8)] = 1
    assert sum(behind[c] for c in behind if c[0] > 3) == 3 * 1 + 5 * 9 + 4 * 25 and behind[(6, 9, 8)] == 0 and behind[(7, 9, 8)] == 1
    out["wall_with_a_hole"] = (wall, 16, [(1, 8, 8)], behind)
    # (5,3,1) from (8,8,8) under the 48 reflections and axis permutations.  Untransformed the walk goes (1,0,0) (1,1,0) (2,1,0),
    # then through the corner (3,2,1) of the cells (2..3, 1..2, 0..1), then (3,2,1) (4,2,1) (4,3,1).  (2,2,1) touches the segment only
    # in that corner and blocks; (2,0,0) and (4,1,1) lie beside it
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            def t(c):
                return tuple(8 + signs[a] * c[perm[a]] for a in range(3))
            tag = "".join("xyz"[perm[a]] + "+-"[signs[a] < 0] for a in range(3))
            out["531_blocked_" + tag] = ([t((2, 2, 1))], 6, [t(V0)], {t((5, 3, 1)): 0, t((2, 1, 0)): 1})
            out["531_beside_" + tag] = ([t((2, 0, 0)), t((4, 1, 1))], 6, [t(V0)], {t((5, 3, 1)): 1})
    return out


HAND_CASES = hand_cases()
ROOT_REGION = ((0, 0, 0), (1 << HAND_DEPTH,) * 3)


def check_hand_case(field, want):
    for (x, y, z), seen in want.items():
        assert field["mask"][z, y, x] == seen and field["count"][z, y, x] == seen, ((x, y, z), field["mask"][z, y, x], seen)


@pytest.mark.parametrize("name", sorted(n for n in HAND_CASES if not n.startswith("531_")) + ["531"])
def test_hand_built_pools(name):
    for case in [n for n in sorted(HAND_CASES) if n.startswith("531_")] if name == "531" else [name]:
        occupied, radius, views, want = HAND_CASES[case]
        words = cells_pool(occupied, HAND_DEPTH) if occupied else HandPool().words()
        occ = occupancy(words, HAND_DEPTH)
        assert int(occ.sum()) == len(set(occupied))
        walk = visibility_field_walk(occ, HAND_DEPTH, *ROOT_REGION, radius, views)
        check_hand_case(walk, want)
        if case == "wall_with_a_hole":                                  # the definition on the cells written out, not on all 4096
            for q, seen in list(want.items())[::23]:
                brute = visibility_field_brute(occ, HAND_DEPTH, q, (1, 1, 1), radius, views)
                assert brute["mask"][0, 0, 0] == seen
        else:
            same_outputs(visibility_field_brute(occ, HAND_DEPTH, *ROOT_REGION, radius, views), walk)


def test_the_hand_cases_cover_all_48_transforms():
    assert len([n for n in HAND_CASES if n.startswith("531_blocked_")]) == 48
    assert len({min(HAND_CASES[n][3]) for n in HAND_CASES if n.startswith("531_beside_")}) == 48   # 48 different targets


def test_viewpoints_that_do_not_count_duplicates_and_bit_positions():
    occ = occupancy(cells_pool([(5, 5, 5)], HAND_DEPTH), HAND_DEPTH)
    views = [(4, 5, 5), (-1, 5, 5), (4, 5, 5), (16, 0, 0), (6, 5, 5), (5, 5, -3)]
    for restatement in (visibility_field_brute, visibility_field_walk):
        got = restatement(occ, HAND_DEPTH, (3, 5, 5), (5, 1, 1), 3, views)
        #                                 x = 3      4      5      6      7: (5,5,5) is between the viewpoints at 4 and at 6
        assert got["mask"][0, 0].tolist() == [0b00101, 0b00101, 0b10101, 0b10000, 0b10000]
        assert got["count"][0, 0].tolist() == [2, 2, 3, 1, 1]
        none = restatement(occ, HAND_DEPTH, (3, 5, 5), (5, 1, 1), 3, np.zeros((0, 3), np.int32))
        assert not none["mask"].any() and not none["count"].any()
        many = restatement(occ, HAND_DEPTH, (3, 5, 5), (5, 1, 1), 3, [(4, 5, 5)] * 33)
        assert "mask" not in many and many["count"][0, 0].tolist() == [33, 33, 33, 0, 0]


def test_the_values_at_single_cells_are_the_fields(fused_occ):
    origin, dims = fused_regions(DEPTH)["low_corner"]
    views = choose_views(fused_occ, DEPTH, origin, dims, 8, 32, 3)
    field = visibility_field_walk(fused_occ, DEPTH, origin, dims, 8, views)
    cells = region_cells(origin, dims)[::3]
    mask, count = visibility_at(fused_occ, DEPTH, cells, 8, views)
    assert np.array_equal(mask, field["mask"].reshape(-1)[::3]) and np.array_equal(count, field["count"].reshape(-1)[::3])
    assert len(set(mask.tolist())) > 20
    assert visibility_at(fused_occ, DEPTH, cells, 8, np.concatenate([views, views[:1]]))[0] is None


def test_a_zero_dimension_is_an_empty_field():
    occ = occupancy(cells_pool([(5, 5, 5)], HAND_DEPTH), HAND_DEPTH)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        got = visibility_field_walk(occ, HAND_DEPTH, (0, 0, 0), dims, 2, [(1, 1, 1)])
        assert got["mask"].shape == got["count"].shape == (dims[2], dims[1], dims[0])


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_visibility_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_visibility_field", "svoslam_workspace_visibility_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "visibility_field") and hasattr(pkg.Workspace, "visibility_buffers")
    assert pkg.MAX_VIEWS_MASK == MAX_VIEWS_MASK
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_visibility_field(" in header and "int svoslam_workspace_visibility_buffers(" in header
    assert "#define SVOSLAM_MAX_VIEWS_MASK 32" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
    text = " ".join(header.split())
    assert "svoslam_pool_visibility_field: its two launches, one bracket per call" in text
    assert "only at an edge or a corner is blocked" in text and "sight is symmetric in v and q" in text
