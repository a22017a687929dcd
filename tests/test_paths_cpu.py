"""Straightening planned paths (svoslam_field_segment_clearance, svoslam_field_shorten_paths; include/svoslam.h, DESIGN.md section
22): the specification restated cell by cell -- segment_clearance_ref walks C(a, b) in walk order over the distance field,
shorten_path_ref tries every j of the window -- and a second time vectorised over the segments with numpy (the walk of
test_visibility_cpu.walk_pairs, carrying the minimum and the first cell that attains it).  The two are proven equal on hand-built
fields with every value written out, on the two worlds of tests/test_plan_cpu.py and on paths traced over a pool fused by the CPU
oracle.  No GPU.

segment_clearance_ref and shorten_path_ref are what the device calls must produce; tests/test_gpu_paths.py compares against them
value for value."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from test_field_cpu import fused_regions
from test_plan_cpu import WORLD_DEPTH, cost_field_words, trace_path, world
from test_surface_cpu import load_pkg
from test_visibility_cpu import walk_cells
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
INF = 1 << 40                                                           # g where the field says -1: above every squared distance


# ---- the specification, restated -------------------------------------------------------------------------------------------
def g_of(field, origin, c):
    """g(c): the field's value at the absolute cell c, INF where it is -1, 0 outside the region"""
    nz, ny, nx = field.shape
    x, y, z = (int(c[a]) - int(origin[a]) for a in range(3))
    if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
        return 0
    v = int(field[z, y, x])
    return INF if v < 0 else v


def walk_order(D):
    """test_visibility_cpu.walk_cells as a generator, in Python integers of any size, so that a caller can stop at the first cell
    it needs: the cells of S(0, D) in walk order (proven equal to walk_cells below)"""
    n = [abs(d) for d in D]
    s = [(d > 0) - (d < 0) for d in D]
    i, c, left = [0, 0, 0], [0, 0, 0], sum(n)
    while left:
        live = [a for a in range(3) if i[a] < n[a]]
        first = [a for a in live if all((2 * i[a] + 1) * n[b] <= (2 * i[b] + 1) * n[a] for b in live)]
        if len(first) > 1:
            for k in range(1, len(first)):
                for sub in itertools.combinations(first, k):
                    yield tuple(c[a] + (s[a] if a in sub else 0) for a in range(3))
        for a in first:
            c[a] += s[a]
            i[a] += 1
        left -= len(first)
        if left:
            yield tuple(c)


def cells_of(a, b):
    """C(a, b) in walk order: a, the supercover, b (a alone when a == b)"""
    a, b = tuple(int(v) for v in a), tuple(int(v) for v in b)
    yield a
    if a != b:
        for c in walk_order(tuple(b[k] - a[k] for k in range(3))):
            yield tuple(a[k] + c[k] for k in range(3))
        yield b


def segment_clearance_ref(field, origin, a, b):
    """-> (minimum, cell): svoslam_field_segment_clearance for one segment.  The minimum of g over C(a, b), -1 when infinite, and the
    first cell in walk order that attains it.  Leaving at 0 changes nothing: nothing is below it."""
    best, at = None, None
    for c in cells_of(a, b):
        v = g_of(field, origin, c)
        if best is None or v < best:
            best, at = v, c
        if best == 0:
            break
    return (-1 if best == INF else best), at


def admissible_ref(field, origin, r, cells, a, j):
    """the shortcut a -> j of the path `cells`"""
    if j == a + 1:
        return True
    m = min(g_of(field, origin, cells[i]) for i in range(a, j + 1))
    return all(g_of(field, origin, c) > r * r and g_of(field, origin, c) >= m for c in cells_of(cells[a], cells[j]))


def shorten_path_ref(field, origin, r, cells, lookahead=0, skipped=None):
    """-> the vertex indices: svoslam_field_shorten_paths for one path (cells: its L stored cells).  Every j of the window is tried.
    `skipped`: a list that receives (a, j, chosen) for every inadmissible j below the chosen one."""
    L = len(cells)
    if L == 0:
        return []
    out, a = [0], 0
    while a < L - 1:
        hi = L - 1 if lookahead == 0 else min(L - 1, a + lookahead)
        ok = [j for j in range(a + 1, hi + 1) if admissible_ref(field, origin, r, cells, a, j)]
        if skipped is not None:
            skipped += [(a, j, ok[-1]) for j in range(a + 1, ok[-1]) if j not in ok]
        a = ok[-1]
        out.append(a)
    return out


def shorten_first_failure(field, origin, r, cells, lookahead=0):
    """the WRONG implementation the specification warns of: scan up from a + 1 until the first inadmissible j"""
    L = len(cells)
    out, a = ([0], 0) if L else ([], 0)
    while a < L - 1:
        hi = L - 1 if lookahead == 0 else min(L - 1, a + lookahead)
        j = a + 1
        while j + 1 <= hi and admissible_ref(field, origin, r, cells, a, j + 1):
            j += 1
        a = j
        out.append(a)
    return out


# ---- the second restatement: all segments at once ----------------------------------------------------------------------------
def g_many(field, origin, c):
    nz, ny, nx = field.shape
    rel = np.asarray(c, I64).reshape(-1, 3) - np.asarray(origin, I64)
    inside = ((rel >= 0) & (rel < np.array([nx, ny, nz], I64))).all(1)
    v = np.zeros(rel.shape[0], I64)
    at = rel[inside]
    got = field[at[:, 2], at[:, 1], at[:, 0]].astype(I64)
    v[inside] = np.where(got < 0, INF, got)
    return v


def segment_clearance_vec(field, origin, a, b):
    """-> (minimum int64 [n], cells int64 [n, 3]) for the segments a[n, 3] .. b[n, 3]: the integer walk with keys, all segments at
    once; a lane leaves when it has reached 0.  |D| below 2^16 per axis (int64 keys)."""
    a, b = np.asarray(a, I64).reshape(-1, 3), np.asarray(b, I64).reshape(-1, 3)
    d = b - a
    n, s = np.abs(d), np.sign(d)
    assert n.max(initial=0) < 1 << 16
    m = np.maximum(n, 1)
    grow = 2 * np.stack([m[:, 1] * m[:, 2], m[:, 0] * m[:, 2], m[:, 0] * m[:, 1]], 1)
    key = np.where(n > 0, grow // 2, I64(1) << 62)
    c = a.copy()
    best, at = g_many(field, origin, a), a.copy()
    left = n.sum(1)

    def take(rows, cells):
        v = g_many(field, origin, cells)
        lower = v < best[rows]
        best[rows[lower]] = v[lower]
        at[rows[lower]] = cells[lower]
    subsets = [np.array(sub, bool) for sub in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))]
    live = np.nonzero((left > 0) & (best > 0))[0]
    while live.size:
        k = key[live]
        first = k == k.min(1)[:, None]
        tie = first.sum(1) > 1
        for sub in subsets:                                             # the proper subsets of the crossing axes, in walk order
            rows = live[tie & ~(sub & ~first).any(1) & (sub != first).any(1)]
            rows = rows[best[rows] > 0]
            if rows.size:
                take(rows, c[rows] + s[rows] * sub)
        c[live] += s[live] * first
        key[live] = k + grow[live] * first
        left[live] -= first.sum(1)
        rows = live[best[live] > 0]                                     # the entered cell: b itself when the walk has arrived
        take(rows, c[rows])
        live = live[(left[live] > 0) & (best[live] > 0)]
    return np.where(best >= INF, -1, best), at


def shorten_path_vec(field, origin, r, cells, lookahead=0):
    """shorten_path_ref by the vectorised walk: per anchor every j of the window at once, m(a, j) a running minimum"""
    cells = np.asarray(cells, I64).reshape(-1, 3)
    L = cells.shape[0]
    if L == 0:
        return []
    g = g_many(field, origin, cells)
    out, a = [0], 0
    while a < L - 1:
        hi = L - 1 if lookahead == 0 else min(L - 1, a + lookahead)
        j = np.arange(a + 1, hi + 1)
        m = np.minimum.accumulate(g[a:hi + 1])[1:]
        low, _ = segment_clearance_vec(field, origin, np.broadcast_to(cells[a], (j.size, 3)), cells[j])
        low = np.where(low < 0, INF, low)
        ok = (low > r * r) & (low >= m)
        ok[0] = True
        a = int(j[np.nonzero(ok)[0][-1]])
        out.append(a)
    return out


def both(field, origin, r, cells, lookahead=0):
    got = shorten_path_ref(field, origin, r, cells, lookahead)
    assert shorten_path_vec(field, origin, r, cells, lookahead) == got, (lookahead, got)
    return got


def polyline_length(cells, vertices):
    p = np.asarray(cells, np.float64)[vertices]
    return float(np.sqrt((np.diff(p, axis=0) ** 2).sum(1)).sum())


# ---- fields by hand ---------------------------------------------------------------------------------------------------------------
def field_about(occupied, origin, dims, radius):
    """the distance field of a few occupied cells, by the formula itself"""
    out = np.full((dims[2], dims[1], dims[0]), -1, np.int32)
    for z, y, x in itertools.product(range(dims[2]), range(dims[1]), range(dims[0])):
        d = min(((x + origin[0] - c[0]) ** 2 + (y + origin[1] - c[1]) ** 2 + (z + origin[2] - c[2]) ** 2 for c in occupied), default=INF)
        if d <= radius * radius:
            out[z, y, x] = d
    return out


def flat(dims, value, cells=()):
    """a field of one value with a few cells (relative (x, y, z) -> value) set"""
    out = np.full((dims[2], dims[1], dims[0]), value, np.int32)
    for (x, y, z), v in dict(cells).items():
        out[z, y, x] = v
    return out


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
WALKS = {                                                               # D -> the cells of S(0, D) in walk order, by hand
    (1, 1, 0): [(1, 0, 0), (0, 1, 0)],                                  # the edge tie: x's side cell, then y's
    (1, 1, 1): [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)],   # the corner: one axis x y z, two axes xy xz yz
    (2, 1, 0): [(1, 0, 0), (1, 1, 0)],                                  # x at 1/4, y at 1/2, x at 3/4: no tie
    (3, 1, 0): [(1, 0, 0), (2, 0, 0), (1, 1, 0), (2, 1, 0)],            # x at 1/6, x and y at 1/2 (sides x, y, then the diagonal), x at 5/6
    (0, 0, 0): [],
    (-1, 0, 1): [(-1, 0, 0), (0, 0, 1)],
    (0, -3, 0): [(0, -1, 0), (0, -2, 0)],
}


def test_the_walk_order_by_hand_and_against_walk_cells():
    for D, want in WALKS.items():
        assert list(walk_order(D)) == want and walk_cells(D) == want, D
    for D in itertools.product(range(-5, 6), repeat=3):
        assert list(walk_order(D)) == walk_cells(D), D
    # far beyond the keys of section 19, where walk_cells' own assertion stops it: the first cells of a line to the end of int32
    far = walk_order(((1 << 32) - 1, (1 << 32) - 1, 1))
    assert [next(far) for _ in range(5)] == [(1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 1, 0), (1, 2, 0)]


def segment_cases():
    """-> [(field, origin, a, b, minimum, first cell that attains it (absolute))], every value by hand"""
    o, dims = (10, 20, 30), (4, 3, 2)
    A = (10, 20, 30)
    out = []

    def add(field, D, low, rel, a=A):
        out.append((field, o, a, tuple(a[k] + D[k] for k in range(3)), low, tuple(rel[k] + o[k] for k in range(3))))
    # the edge tie: both side cells at 5 -> x's comes first; y's alone
    add(flat(dims, 9, {(1, 0, 0): 5, (0, 1, 0): 5}), (1, 1, 0), 5, (1, 0, 0))
    add(flat(dims, 9, {(0, 1, 0): 5}), (1, 1, 0), 5, (0, 1, 0))
    add(flat(dims, 9, {(1, 1, 0): 9}), (1, 1, 0), 9, (0, 0, 0))         # all equal: a
    add(flat(dims, 9, {(1, 1, 0): 8}), (1, 1, 0), 8, (1, 1, 0))         # b alone
    # the corner: each of the six side cells alone, all six, and pairs across the groups
    six = WALKS[(1, 1, 1)]
    for c in six:
        add(flat(dims, 9, {c: 4}), (1, 1, 1), 4, c)
    add(flat(dims, 9, {c: 4 for c in six}), (1, 1, 1), 4, (1, 0, 0))
    add(flat(dims, 9, {(1, 1, 0): 4, (0, 0, 1): 4}), (1, 1, 1), 4, (0, 0, 1))   # z's cell comes before xy's
    add(flat(dims, 9, {(0, 1, 1): 4, (1, 0, 1): 4}), (1, 1, 1), 4, (1, 0, 1))   # xz before yz
    add(flat(dims, 9, {(0, 1, 1): 4, (1, 1, 1): 4}), (1, 1, 1), 4, (0, 1, 1))   # yz before b
    # tie-free (2,1,0): (2,0,0) and (0,1,0) are not on the line
    add(flat(dims, 9, {(2, 0, 0): 1, (0, 1, 0): 1}), (2, 1, 0), 9, (0, 0, 0))
    add(flat(dims, 9, {(1, 1, 0): 3, (1, 0, 0): 3}), (2, 1, 0), 3, (1, 0, 0))
    # the middle tie of (3,1,0): all four cells between the ends
    for k, c in enumerate(WALKS[(3, 1, 0)]):
        add(flat(dims, 9, {d: 2 for d in WALKS[(3, 1, 0)][k:]}), (3, 1, 0), 2, c)
    add(flat(dims, 9, {(3, 0, 0): 1, (0, 1, 0): 1}), (3, 1, 0), 9, (0, 0, 0))
    # a == b
    add(flat(dims, 9, {(0, 0, 0): 7}), (0, 0, 0), 7, (0, 0, 0))
    # an all -1 field: -1 at a; one finite cell on the line: that cell
    add(flat(dims, -1), (3, 2, 1), -1, (0, 0, 0))
    add(flat(dims, -1, {(1, 1, 0): 6}), (2, 2, 0), 6, (1, 1, 0))
    # an occupied cell on the line: the first one
    add(flat(dims, 9, {(1, 0, 0): 0, (2, 0, 0): 0}), (3, 0, 0), 0, (1, 0, 0))
    # an end outside the region: 0 at that end -- b beyond the high x face, the cells before it inside
    add(flat(dims, 9), (4, 0, 0), 0, (4, 0, 0))
    add(flat(dims, 9), (6, 0, 0), 0, (4, 0, 0))                          # the first cell outside, not b
    add(flat(dims, 9, {(2, 0, 0): 0}), (6, 0, 0), 0, (2, 0, 0))          # an occupied cell before the face
    add(flat(dims, 9), (-1, -1, 0), 0, (-1, 0, 0))                       # a tie that ends outside: x's side cell first
    add(flat(dims, 9), (3, 1, 0), 0, (-1, 0, 0), a=(9, 20, 30))          # a outside: 0 at a, nothing walked
    # b at the ends of int32: the walk leaves the region long before.  x, y, x, y: (12,21) (12,22) (13,22), then row 23 is outside
    a = (11, 21, 30)
    add(flat(dims, 9), ((1 << 31) - 1 - a[0], (1 << 31) - 1 - a[1], 1), 0, (3, 3, 0), a=a)
    add(flat(dims, 9), (-(1 << 31) - a[0], 0, 0), 0, (-1, 1, 0), a=a)
    add(flat(dims, 9, {(2, 2, 0): 0}), ((1 << 31) - 1 - a[0], (1 << 31) - 1 - a[1], 1), 0, (2, 2, 0), a=a)
    low = -(1 << 31)                                                    # both ends outside, as far apart as int32 allows: 0 at a
    add(flat(dims, 9), ((1 << 32) - 1,) * 3, 0, (low - o[0], low - o[1], low - o[2]), a=(low, low, low))
    # a zero entry of dims: every cell is outside
    out.append((np.zeros((0, 3, 4), np.int32), o, A, (13, 20, 30), 0, A))
    return out


SEGMENT_CASES = segment_cases()


def test_the_first_cell_that_attains_the_minimum():
    assert len(SEGMENT_CASES) == 35
    for k, (field, o, a, b, low, at) in enumerate(SEGMENT_CASES):
        assert segment_clearance_ref(field, o, a, b) == (low, at), k
        if max(abs(b[i] - a[i]) for i in range(3)) < 1 << 16:
            lows, ats = segment_clearance_vec(field, o, [a], [b])
            assert (int(lows[0]), tuple(ats[0].tolist())) == (low, at), k


# ---- shortening by hand: every vertex written out ---------------------------------------------------------------------------------------
def staircase(start, moves):
    cells = [tuple(start)]
    for axis, step in moves:
        c = list(cells[-1])
        c[axis] += step
        cells.append(tuple(c))
    return cells


ROUND_THE_PILLAR = [(0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0), (3, 1, 0), (4, 1, 0), (5, 1, 0), (5, 2, 0), (6, 2, 0), (7, 2, 0), (8, 2, 0)]
PILLAR = (4, 2, 0)
DETOUR = [(0, 1, 0), (0, 2, 0), (1, 2, 0), (1, 3, 0), (2, 3, 0), (3, 3, 0), (4, 3, 0), (5, 3, 0), (5, 2, 0), (6, 2, 0), (6, 1, 0)]


def shorten_cases():
    """name -> (field, origin, clearance, cells, lookahead, expected vertices)"""
    out = {}
    o = (0, 0, 0)
    empty = flat((6, 5, 4), -1)
    stairs = staircase((0, 0, 0), [(0, 1), (1, 1), (0, 1), (2, 1), (1, 1), (0, 1), (2, 1), (0, 1), (1, 1), (2, 1), (0, 1), (1, 1)])
    # an empty map: nothing is nearer than infinity, every shortcut is admissible
    out["empty_map_staircase"] = (empty, o, 0, stairs, 0, [0, 12])
    out["empty_map_staircase_clearance_3"] = (empty, o, 3, stairs, 0, [0, 12])
    out["empty_map_lookahead_5"] = (empty, o, 0, stairs, 5, [0, 5, 10, 12])
    out["empty_map_lookahead_1"] = (empty, o, 0, stairs, 1, list(range(13)))
    out["no_cells"] = (empty, o, 0, [], 0, [])
    out["one_cell"] = (empty, o, 0, stairs[:1], 0, [0])
    out["two_cells"] = (empty, o, 0, stairs[:2], 0, [0, 1])
    out["three_cells"] = (empty, o, 0, stairs[:3], 0, [0, 2])
    # one pillar at (4,2,0) on a radius-0 field: plain line of sight.  From (0,2) the row is cut by the pillar; (5,1) is the last
    # cell in sight -- the line (0,2) .. (5,1) passes the corner between (2,2), (3,2), (2,1), (3,1) and then runs along y = 1
    near = field_about([PILLAR], o, (9, 4, 1), 0)
    out["round_the_pillar"] = (near, o, 0, ROUND_THE_PILLAR, 0, [0, 6, 10])
    out["round_the_pillar_lookahead_1"] = (near, o, 0, ROUND_THE_PILLAR, 1, list(range(11)))
    out["round_the_pillar_lookahead_2"] = (near, o, 0, ROUND_THE_PILLAR, 2, [0, 2, 4, 6, 8, 10])
    # W = 3: from (3,2) neither (5,1), whose line enters (4,2), nor (4,1), whose side cell it is, only the next cell
    out["round_the_pillar_lookahead_3"] = (near, o, 0, ROUND_THE_PILLAR, 3, [0, 3, 4, 6, 9, 10])
    # cells outside the region and a jump: an anchor or a target outside has g = 0, only its a + 1 step is admissible
    out["last_cell_outside"] = (empty, o, 0, [(0, 0, 0), (1, 0, 0), (7, 0, 0)], 0, [0, 1, 2])
    out["first_cell_outside"] = (empty, o, 0, [(-1, 0, 0), (3, 1, 0), (5, 2, 0), (0, 0, 0)], 0, [0, 1, 3])
    out["a_jump_of_two_cells"] = (empty, o, 0, [(0, 0, 0), (5, 4, 3)], 0, [0, 1])
    out["a_jump_inside_a_path"] = (empty, o, 0, [(0, 0, 0), (0, 1, 0), (5, 4, 3), (5, 4, 2), (5, 3, 2)], 0, [0, 4])
    # a cell outside between cells inside: m of the stretch is 0, the shortcut over it only has to keep the clearance
    out["a_cell_outside_is_skipped"] = (empty, o, 0, [(0, 0, 0), (1, 0, 0), (9, 0, 0), (2, 0, 0), (3, 0, 0)], 0, [0, 4])
    # every cell outside: a zero entry of dims
    out["no_region"] = (np.zeros((4, 0, 6), np.int32), o, 0, stairs[:5], 0, [0, 1, 2, 3, 4])
    # an occupied cell (3,0,0) with its rings up to 3: the detour keeps 8 or more from it (squared); the straight line (0,1) .. (6,1)
    # would pass (3,1), at 1 -- refused; from (0,1) the last admissible cell is (1,3): already (2,3)'s line passes (1,1), at 5
    rings = field_about([(3, 0, 0)], o, (7, 4, 1), 3)
    out["the_detour_keeps_its_rings"] = (rings, o, 0, DETOUR, 0, None)
    # ... the same path on the radius-0 field: one segment, past the occupied cell
    out["the_detour_on_a_radius_0_field"] = (field_about([(3, 0, 0)], o, (7, 4, 1), 0), o, 0, DETOUR, 0, [0, 10])
    # ... at clearance 1 on the radius-1 field the cells beside (3,0,0) are closed: (3,1) at 1 blocks the straight line again
    out["the_detour_on_a_radius_1_field"] = (field_about([(3, 0, 0)], o, (7, 4, 1), 1), o, 1, DETOUR, 0, None)
    return out


SHORTEN_CASES = shorten_cases()
PINNED = {                                                              # the cases whose vertices the restatement gave, checked by hand below
    "the_detour_keeps_its_rings": [0, 3, 7, 10],
    "the_detour_on_a_radius_1_field": [0, 7, 10],                       # (5,3): the first cell whose line from (0,1) passes above (3,1)
}


@pytest.mark.parametrize("name", sorted(SHORTEN_CASES))
def test_shortening_by_hand(name):
    field, origin, r, cells, lookahead, want = SHORTEN_CASES[name]
    want = PINNED[name] if want is None else want
    got = both(field, origin, r, cells, lookahead)
    assert got == want, got
    for a, j in zip(got, got[1:]):                                      # every segment is admissible, and no vertex could have been later
        assert admissible_ref(field, origin, r, cells, a, j)
        hi = len(cells) - 1 if lookahead == 0 else min(len(cells) - 1, a + lookahead)
        assert not any(admissible_ref(field, origin, r, cells, a, k) for k in range(j + 1, hi + 1))


def test_the_detour_by_hand():
    field, origin, r, cells, _, _ = SHORTEN_CASES["the_detour_keeps_its_rings"]
    g = [g_of(field, origin, c) for c in cells]
    assert g == [INF, INF, 8, INF, INF, 9, INF, INF, 8, INF, INF]
    assert segment_clearance_ref(field, origin, cells[0], cells[10]) == (1, (3, 1, 0))      # the straight line: through the nearest ring
    assert not admissible_ref(field, origin, 0, cells, 0, 10)
    assert segment_clearance_ref(field, origin, cells[0], cells[4]) == (5, (1, 1, 0)) and not admissible_ref(field, origin, 0, cells, 0, 4)
    assert segment_clearance_ref(field, origin, cells[0], cells[3]) == (8, (1, 2, 0)) and admissible_ref(field, origin, 0, cells, 0, 3)
    near = SHORTEN_CASES["the_detour_on_a_radius_0_field"][0]
    assert segment_clearance_ref(near, origin, cells[0], cells[10]) == (-1, cells[0])


# ---- the two worlds of tests/test_plan_cpu.py ------------------------------------------------------------------------------------------
LOOKAHEADS = (0, 1, 2, 7, 63, 64, 65, 130)
_PATHS = {}


def world_path(name, which):
    """the cells of a traced path of the world, as tuples: 'weighted' down the cost field, 'reach' down the reach field; from the
    world's start, or from the farthest cell where it has none"""
    if (name, which) not in _PATHS:
        w = world(name)
        values = w["cost"] if which == "weighted" else w["steps"]
        start = w["start"]
        if start is None:
            start = np.array(np.unravel_index(np.argmax(w["cost"]), w["cost"].shape)[::-1]) + np.asarray(w["origin"])
        cells, length = trace_path(values, w["origin"], start, values.size)
        assert length == cells.shape[0]
        _PATHS[name, which] = [tuple(c) for c in cells.tolist()]
    return _PATHS[name, which]


_SHORTENED = {}


def world_vertices(name, which, lookahead, radius=None):
    """shorten_path_ref on a world's path, computed once (radius: the field truncated to it; default the world's comfort field)"""
    key = (name, which, lookahead, radius)
    if key not in _SHORTENED:
        w = world(name)
        field = w["field"] if radius is None else np.where((w["field"] >= 0) & (w["field"] <= radius * radius), w["field"], -1).astype(np.int32)
        skipped = []
        _SHORTENED[key] = (shorten_path_ref(field, w["origin"], w["clearance"], world_path(name, which), lookahead, skipped), skipped, field)
    return _SHORTENED[key]


TWO_ROUTES_WAYPOINTS = [(10, 32, 3), (104, 26, 3), (104, 13, 3), (102, 10, 3), (98, 9, 3), (10, 4, 3)]


def test_two_routes_stays_in_the_gate():
    w = world("two_routes")
    cells = world_path("two_routes", "weighted")
    assert len(cells) == 217
    got, skipped, field = world_vertices("two_routes", "weighted", 0)
    assert [cells[v] for v in got] == TWO_ROUTES_WAYPOINTS, [cells[v] for v in got]
    assert shorten_path_vec(field, w["origin"], w["clearance"], cells, 0) == got
    # through the gate: no segment touches a cell of the tunnel's columns inside the wall
    for a, j in zip(got, got[1:]):
        assert not any(9 <= c[0] <= 11 and 14 <= c[1] <= 21 for c in cells_of(cells[a], cells[j]))
    assert any(100 <= c[0] <= 114 and 14 <= c[1] <= 21 for a, j in zip(got, got[1:]) for c in cells_of(cells[a], cells[j]))
    # admissibility is not monotone: an inadmissible j below the chosen one, and "scan until the first failure" gives another result
    assert skipped, "no anchor with an inadmissible j below the chosen one"
    assert shorten_first_failure(field, w["origin"], w["clearance"], cells, 0) != got
    assert len(world_vertices("two_routes", "weighted", 64)[0]) == 8 and len(world_vertices("two_routes", "weighted", 7)[0]) == 33
    assert polyline_length(cells, got) <= len(cells) - 1


def test_two_routes_the_reach_path_is_one_segment():
    cells = world_path("two_routes", "reach")
    assert len(cells) == 29
    assert world_vertices("two_routes", "reach", 0)[0] == [0, 28]


def test_two_routes_plain_line_of_sight_goes_through_the_tunnel():
    """the reason for the rule: against the field truncated to the clearance radius, where every cell beyond it is infinitely far,
    the weighted path through the gate collapses to the one segment through the tunnel"""
    w = world("two_routes")
    cells = world_path("two_routes", "weighted")
    got, _, near = world_vertices("two_routes", "weighted", 0, radius=w["clearance"])
    assert got == [0, 216]
    assert all(c[0] == 10 for c in cells_of(cells[0], cells[216]))
    assert segment_clearance_ref(near, w["origin"], cells[0], cells[216])[0] == -1
    assert segment_clearance_ref(w["field"], w["origin"], cells[0], cells[216])[0] == 4    # a tunnel three cells wide: its middle is 2 from a wall


@pytest.mark.parametrize("lookahead,count", [(0, 20), (64, 27)])
def test_the_serpentine(lookahead, count):
    w = world("serpentine")
    cells = world_path("serpentine", "weighted")
    assert len(cells) == 894
    got, _, field = world_vertices("serpentine", "weighted", lookahead)
    assert len(got) == count, got
    assert shorten_path_vec(field, w["origin"], w["clearance"], cells, lookahead) == got
    assert polyline_length(cells, got) <= len(cells) - 1


@pytest.mark.parametrize("name,which", [("two_routes", "weighted"), ("two_routes", "reach"), ("serpentine", "weighted")])
def test_every_segment_is_admissible_and_no_vertex_could_be_later(name, which):
    w = world(name)
    cells = world_path(name, which)
    r = w["clearance"]
    g = [g_of(w["field"], w["origin"], c) for c in cells]
    for lookahead in (0, 64, 7):
        got = world_vertices(name, which, lookahead)[0]
        assert got[0] == 0 and got[-1] == len(cells) - 1 and all(a < j for a, j in zip(got, got[1:]))
        for a, j in zip(got, got[1:]):
            low = segment_clearance_ref(w["field"], w["origin"], cells[a], cells[j])[0]
            low = INF if low < 0 else low
            assert j == a + 1 or (low > r * r and low >= min(g[a:j + 1])), (a, j)
            hi = len(cells) - 1 if lookahead == 0 else min(len(cells) - 1, a + lookahead)
            assert not any(admissible_ref(w["field"], w["origin"], r, cells, a, k) for k in range(j + 1, hi + 1)), (a, j)
        assert polyline_length(cells, got) <= len(cells) - 1


@pytest.mark.parametrize("name", ["two_routes", "serpentine"])
def test_the_two_restatements_agree_on_the_worlds(name):
    w = world(name)
    for which in ("weighted", "reach"):
        cells = world_path(name, which)
        for lookahead in LOOKAHEADS:
            assert shorten_path_vec(w["field"], w["origin"], w["clearance"], cells, lookahead) == world_vertices(name, which, lookahead)[0], (which, lookahead)
        assert world_vertices(name, which, 1)[0] == list(range(len(cells)))
    rng = np.random.default_rng(5)
    o, dims = np.asarray(w["origin"]), np.asarray(w["dims"])
    a = rng.integers(-1, dims + 1, (300, 3)) + o
    b = rng.integers(-1, dims + 1, (300, 3)) + o
    lows, ats = segment_clearance_vec(w["field"], w["origin"], a, b)
    for k in range(300):
        assert segment_clearance_ref(w["field"], w["origin"], a[k], b[k]) == (int(lows[k]), tuple(ats[k].tolist())), (a[k], b[k])


# ---- a pool fused by the oracle -----------------------------------------------------------------------------------------------------------
def fused_paths(words, depth, region, clearance, comfort, ring, count, seed):
    """-> (field with radius comfort, origin, dims, [cells of a traced path as tuples]): a cost field seeded at a seeded traversable
    cell of the region and paths traced from `count` seeded reached cells"""
    from test_field_cpu import distance_field_separable
    origin, dims = fused_regions(depth)[region]
    field = distance_field_separable(words, depth, origin, dims, comfort)
    rng = np.random.default_rng(seed)
    free = np.argwhere((field < 0) | (field > clearance * clearance))[:, ::-1]
    if free.shape[0] == 0:
        return field, origin, dims, []
    goal = free[rng.integers(free.shape[0])] + np.asarray(origin)
    cost = cost_field_words(words, depth, origin, dims, clearance, comfort, ring, [goal], field=field)
    reached = np.argwhere(cost >= 0)[:, ::-1]
    picks = reached[rng.choice(reached.shape[0], min(count, reached.shape[0]), replace=False)]
    far = np.array(np.unravel_index(np.argmax(cost), cost.shape)[::-1])
    paths = []
    for p in [far] + list(picks):
        cells, length = trace_path(cost, origin, p + np.asarray(origin), cost.size)
        assert length == cells.shape[0] >= 1
        paths.append([tuple(c) for c in cells.tolist()])
    return field, origin, dims, paths


FUSED_REGIONS = ("low_corner", "high_corner", "one_cell", "offset_37")


@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", FUSED_REGIONS)
def test_the_two_restatements_agree_on_the_fused_pool(fused, depth, region):
    words, _ = fused
    shortened = 0
    for clearance, comfort, ring in ((0, 2, [8, 3]), (1, 3, [9, 2])):
        field, origin, dims, paths = fused_paths(words, depth, region, clearance, comfort, ring, 6, 3)
        for cells in paths:
            for lookahead in (0, 1, 2, 7):
                got = both(field, origin, clearance, cells, lookahead)
                assert got[0] == 0 and got[-1] == len(cells) - 1
                shortened += len(got) < len(cells)
            assert both(field, origin, clearance, cells, 1) == list(range(len(cells)))
        rng = np.random.default_rng(7)
        o, n = np.asarray(origin), np.asarray(dims)
        a = rng.integers(-1, n + 1, (200, 3)) + o
        b = rng.integers(-1, n + 1, (200, 3)) + o
        lows, ats = segment_clearance_vec(field, origin, a, b)
        for k in range(200):
            assert segment_clearance_ref(field, origin, a[k], b[k]) == (int(lows[k]), tuple(ats[k].tolist()))
    if region in ("low_corner", "high_corner"):
        assert shortened > 4, shortened


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_path_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_field_segment_clearance", "svoslam_field_shorten_paths"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    for name in ("segment_clearance", "shorten_paths", "plan_paths"):
        assert callable(getattr(pkg, name, None)), name
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_field_segment_clearance(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3]," in header
    assert "int svoslam_field_shorten_paths(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells," in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
    assert "#define SVOSLAM_MAX_RADIUS_CELLS %d" % MAX_RADIUS in header
