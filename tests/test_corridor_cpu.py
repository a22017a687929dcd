"""Safe corridors along planned paths (svoslam_field_grow_boxes, svoslam_field_path_corridors; include/svoslam_corridor.h, DESIGN.md
section 27): the specification restated cell by cell in Python integers -- grow_box_ref tries the six directions round by round
and looks at every cell of every slab, path_corridors_ref chains the boxes along a path -- and a second time on a boolean mask of
the free cells with numpy slab slices.  The two are proven equal on hand-built fields with every value written out and on the
traced paths of the two worlds of tests/test_plan_cpu.py.  No GPU.

grow_boxes_ref and path_corridors_ref are what the device calls must produce; tests/test_gpu_corridor.py compares against them
value for value."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_paths_cpu import flat, g_of, world_path
from test_plan_cpu import world
from test_surface_cpu import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))          # (axis, 0 = the low face | 1 = the high face): -x +x -y +y -z +z


def wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


# ---- the specification, restated cell by cell --------------------------------------------------------------------------------
def free_ref(field, origin, r, c):
    """a cell is free iff g(c) > r^2; g is 0 outside the region (test_paths_cpu.g_of)"""
    return g_of(field, origin, c) > r * r


def in_region(field, origin, lo, hi):
    """the box lo .. hi lies inside the region: the O(1) test that comes before any cell is looked at"""
    nz, ny, nx = field.shape
    return all(int(origin[a]) <= int(lo[a]) and int(hi[a]) < int(origin[a]) + n for a, n in enumerate((nx, ny, nz)))


def box_cells(lo, hi):
    return ((x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1))


def grow_box_ref(field, origin, r, E, lo, hi):
    """grow(box) -> (lo, hi, layers) for a box of free cells: rounds of -x +x -y +y -z +z, each direction against the box as it is
    now, until a round grows nothing"""
    lo, hi, grown = [int(v) for v in lo], [int(v) for v in hi], [0] * 6
    while True:
        any_grew = False
        for d, (axis, high) in enumerate(DIRECTIONS):
            if grown[d] >= E:
                continue
            s_lo, s_hi = list(lo), list(hi)
            s_lo[axis] = s_hi[axis] = hi[axis] + 1 if high else lo[axis] - 1
            if in_region(field, origin, s_lo, s_hi) and all(free_ref(field, origin, r, c) for c in box_cells(s_lo, s_hi)):
                (hi if high else lo)[axis] = s_lo[axis]
                grown[d] += 1
                any_grew = True
        if not any_grew:
            return tuple(lo), tuple(hi), sum(grown)


def grow_boxes_ref(field, origin, r, E, seed):
    """-> (box as 6 ints, layers): svoslam_field_grow_boxes for one seed"""
    seed = [int(v) for v in seed]
    lo, hi = seed[:3], seed[3:]
    if not (all(lo[a] <= hi[a] for a in range(3)) and in_region(field, origin, lo, hi)
            and all(free_ref(field, origin, r, c) for c in box_cells(lo, hi))):
        return tuple(seed), -1
    lo, hi, layers = grow_box_ref(field, origin, r, E, lo, hi)
    return lo + hi, layers


def anchor_box_ref(field, origin, r, E, cells, a):
    """-> (box as 6 ints, e(a), empty) of the anchor index a of the path `cells`"""
    p = cells[a]
    if not free_ref(field, origin, r, p):
        return tuple(p) + tuple(wrap32(v - 1) for v in p), a, True
    lo, hi = list(p), list(p)
    if a + 1 < len(cells):
        q = cells[a + 1]
        if sum(abs(q[k] - p[k]) for k in range(3)) == 1 and free_ref(field, origin, r, q):
            lo, hi = [min(p[k], q[k]) for k in range(3)], [max(p[k], q[k]) for k in range(3)]
    lo, hi, _ = grow_box_ref(field, origin, r, E, lo, hi)
    e = a
    while e + 1 < len(cells) and all(lo[k] <= cells[e + 1][k] <= hi[k] for k in range(3)):
        e += 1
    return lo + hi, e, False


def path_corridors_ref(field, origin, r, E, cells):
    """-> (boxes, anchors, gaps): svoslam_field_path_corridors for one path (cells: its L stored cells, tuples of int)"""
    cells = [tuple(int(v) for v in c) for c in cells]
    boxes, anchors, gaps, a = [], [], 0, 0
    while cells:
        box, e, empty = anchor_box_ref(field, origin, r, E, cells, a)
        boxes.append(box)
        anchors.append(a)
        gaps += empty or (e == a and a < len(cells) - 1)
        if e == len(cells) - 1:
            break
        a = e if e > a else a + 1
    return boxes, anchors, gaps


# ---- the second restatement: a mask of the free cells, slabs as slices ----------------------------------------------------------
def free_mask(field, r):
    return (field < 0) | (field > r * r)


def grow_box_mask(mask, lo, hi, E):
    """grow over the mask, relative cells: a slab is one slice, free iff it is inside the mask and all of it is set"""
    lo, hi, grown = list(lo), list(hi), [0] * 6
    shape = mask.shape[::-1]
    grew = True
    while grew:
        grew = False
        for d, (axis, high) in enumerate(DIRECTIONS):
            at = hi[axis] + 1 if high else lo[axis] - 1
            if grown[d] >= E or not 0 <= at < shape[axis]:
                continue
            cut = [slice(lo[k], hi[k] + 1) for k in range(3)]
            cut[axis] = slice(at, at + 1)
            if mask[cut[2], cut[1], cut[0]].all():
                (hi if high else lo)[axis] = at
                grown[d] += 1
                grew = True
    return lo, hi, sum(grown)


def grow_boxes_mask(field, origin, r, E, seed):
    mask, o = free_mask(field, r), [int(v) for v in origin]
    seed = [int(v) for v in seed]
    lo, hi = [seed[k] - o[k] for k in range(3)], [seed[k + 3] - o[k] for k in range(3)]
    shape = mask.shape[::-1]
    if not all(0 <= lo[k] <= hi[k] < shape[k] for k in range(3)) or not mask[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].all():
        return tuple(seed), -1
    lo, hi, layers = grow_box_mask(mask, lo, hi, E)
    return tuple(lo[k] + o[k] for k in range(3)) + tuple(hi[k] + o[k] for k in range(3)), layers


def path_corridors_mask(field, origin, r, E, cells):
    mask, o = free_mask(field, r), np.asarray(origin, np.int64)
    shape = np.array(mask.shape[::-1], np.int64)
    p = np.asarray(cells, np.int64).reshape(-1, 3) - o
    L = p.shape[0]
    inside = ((p >= 0) & (p < shape)).all(1)
    free = np.zeros(L, bool)
    free[inside] = mask[p[inside, 2], p[inside, 1], p[inside, 0]]
    pair = np.zeros(L, bool)
    pair[:-1] = (np.abs(np.diff(p, axis=0)).sum(1) == 1) & free[1:]
    boxes, anchors, gaps, a = [], [], 0, 0
    while L:
        anchors.append(a)
        if not free[a]:
            at = p[a] + o
            boxes.append(tuple(at.tolist()) + tuple(wrap32(v - 1) for v in at.tolist()))
            e = a
            gaps += 1
        else:
            lo, hi = (np.minimum(p[a], p[a + 1]), np.maximum(p[a], p[a + 1])) if pair[a] else (p[a], p[a])
            lo, hi, _ = grow_box_mask(mask, lo.tolist(), hi.tolist(), E)
            out = ~((p[a:] >= lo) & (p[a:] <= hi)).all(1)
            e = a + (int(np.argmax(out)) if out.any() else L - a) - 1
            boxes.append(tuple((np.array(lo) + o).tolist()) + tuple((np.array(hi) + o).tolist()))
            gaps += e == a and a < L - 1
        if e == L - 1:
            break
        a = e if e > a else a + 1
    return boxes, anchors, int(gaps)


def both_boxes(field, origin, r, E, seed):
    got = grow_boxes_ref(field, origin, r, E, seed)
    assert grow_boxes_mask(field, origin, r, E, seed) == got, (seed, got)
    return got


def both_paths(field, origin, r, E, cells):
    got = path_corridors_ref(field, origin, r, E, cells)
    assert path_corridors_mask(field, origin, r, E, cells) == got, (r, E)
    return got


def check_chain(field, origin, r, cells, boxes, anchors):
    """what an unbroken chain (gaps == 0) promises: consecutive boxes share the next anchor's cell, every path cell lies in a box,
    every cell of every box is free"""
    mask, o = free_mask(field, r), np.asarray(origin)

    def holds(box, c):
        return all(box[k] <= c[k] <= box[k + 3] for k in range(3))
    assert anchors[0] == 0 and all(a < b for a, b in zip(anchors, anchors[1:]))
    for k in range(1, len(anchors)):
        assert holds(boxes[k - 1], cells[anchors[k]]) and holds(boxes[k], cells[anchors[k]]), k
    for k, a in enumerate(anchors):
        last = anchors[k + 1] if k + 1 < len(anchors) else len(cells) - 1
        assert all(holds(boxes[k], cells[j]) for j in range(a, last + 1)), k
    for box in boxes:
        lo, hi = np.array(box[:3]) - o, np.array(box[3:]) - o
        assert (lo >= 0).all() and (lo <= hi).all() and (hi < np.array(mask.shape[::-1])).all(), box
        assert mask[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].all(), box


# ---- fields by hand ---------------------------------------------------------------------------------------------------------------
def grow_cases():
    """name -> (field, origin, r, E, seed, the box and the layers worked out by hand)"""
    cases = {}
    # a free cell walled in on all sides: the 26 cells around it are occupied
    f = flat((3, 3, 3), 0, {(1, 1, 1): 9})
    cases["walled_in"] = (f, (5, -3, 7), 1, 4, (6, -2, 8, 6, -2, 8), (6, -2, 8, 6, -2, 8), 0)
    # E = 0: nothing may grow, in a field with nothing near
    f = flat((4, 4, 4), -1)
    cases["extent_0"] = (f, (0, 0, 0), 2, 0, (1, 1, 1, 2, 2, 2), (1, 1, 1, 2, 2, 2), 0)
    # nothing near, a large E: the region's border stops each of the six sides: 2 + 2, 1 + 2, 1 + 1 layers from the cell (2, 1, 1)
    f = flat((5, 4, 3), -1)
    cases["the_border_on_six_sides"] = (f, (10, 20, 30), 3, 64, (12, 21, 31, 12, 21, 31), (10, 20, 30, 14, 23, 32), 9)
    # E layers a direction and no more: 6 E in all
    f = flat((9, 9, 9), 50)
    cases["extent_2"] = (f, (-4, -4, -4), 7, 2, (0, 0, 0, 0, 0, 0), (-2, -2, -2, 2, 2, 2), 12)
    # the order of the round, a plane of 3 x 3 at r = 1 (free: 5, not free: 0)
    #   y 2:  5 5 5
    #   y 1:  0 5 5
    #   y 0:  5 5 0         the seed is (1, 0)
    # -x grows first, to (0, 0); +x meets the 0 at (2, 0); the +y slab is then (0, 1) (1, 1), and (0, 1) is not free: the box of
    # the cell alone is (0, 0) .. (1, 0) and does not hold the free cell (1, 1) above the seed
    f = flat((3, 3, 1), 5, {(2, 0, 0): 0, (0, 1, 0): 0})
    cases["the_order_of_the_round"] = (f, (0, 0, 0), 1, 4, (1, 0, 0, 1, 0, 0), (0, 0, 0, 1, 0, 0), 1)
    # from the pair (1, 0) (1, 1): -x meets (0, 1), +x meets (2, 0), +y grows to (1, 2), then nothing
    cases["the_pair_of_that_plane"] = (f, (0, 0, 0), 1, 4, (1, 0, 0, 1, 1, 0), (1, 0, 0, 1, 2, 0), 1)
    # a 3 x 3 plate at z 1 of 5 x 5 x 3, E = 1: -x +x -y +y -z grow, the +z slab is by then the whole plane z 2
    free = (0, 0, 0, 4, 4, 2)
    cases["a_plate"] = (flat((5, 5, 3), 8), (0, 0, 0), 2, 1, (1, 1, 1, 3, 3, 1), free, 6)
    for name, corner in (("low_low", (0, 0, 2)), ("high_low", (4, 0, 2)), ("low_high", (0, 4, 2)), ("high_high", (4, 4, 2))):
        cases["a_plate_and_a_slab_corner_" + name] = (flat((5, 5, 3), 8, {corner: 4}), (0, 0, 0), 2, 1, (1, 1, 1, 3, 3, 1), (0, 0, 0, 4, 4, 1), 5)
    # g exactly r^2 is not free, r^2 + 1 is
    cases["r2_and_r2_plus_1"] = (flat((3, 1, 1), 9, {(0, 0, 0): 4, (2, 0, 0): 5}), (0, 0, 0), 2, 9, (1, 0, 0, 1, 0, 0), (1, 0, 0, 2, 0, 0), 1)
    # -1 is farther than every radius
    cases["minus_1_is_free"] = (flat((3, 1, 1), -1, {(2, 0, 0): 0}), (7, 7, 7), 3, 9, (7, 7, 7, 7, 7, 7), (7, 7, 7, 8, 7, 7), 1)
    # seeds that are not valid come back as they were, with -1
    f = flat((4, 4, 4), -1, {(2, 2, 2): 0})
    top = (1 << 31) - 1
    for name, seed in (("lo_above_hi", (2, 1, 1, 1, 1, 1)), ("partly_outside", (3, 3, 3, 4, 3, 3)), ("below_the_region", (-1, 0, 0, 0, 0, 0)),
                       ("holds_a_cell_that_is_not_free", (1, 1, 1, 2, 2, 2)), ("far_outside", (top - 1, top - 1, top - 1, top, top, top)),
                       ("all_of_int32", (-top - 1, 0, 0, top, 0, 0)), ("far_below", (-top - 1, -top - 1, -top - 1, -top - 1, -top - 1, -top - 1))):
        cases["invalid_" + name] = (f, (0, 0, 0), 0, 3, seed, seed, -1)
    # the same field, a valid seed beside the occupied cell (2, 2, 2): +x meets it in every round, the other five reach the border:
    # 1 layer -x, 2 -y, 1 +y, 2 -z, 1 +z
    cases["beside_the_occupied_cell"] = (f, (0, 0, 0), 0, 3, (1, 2, 2, 1, 2, 2), (0, 0, 0, 1, 3, 3), 7)
    return cases


GROW_CASES = grow_cases()


@pytest.mark.parametrize("name", sorted(GROW_CASES))
def test_growing_by_hand(name):
    field, origin, r, E, seed, box, layers = GROW_CASES[name]
    assert both_boxes(field, origin, r, E, seed) == (tuple(box), layers)
    if layers >= 0:
        check_chain(field, origin, r, [seed[:3]], [box], [0])


def test_the_order_dependence_and_the_pair_seed():
    """the box grown from p_a alone can miss the free face neighbour p_(a+1) that a box grown in another order would hold; the pair
    seed holds it by construction: e(a) >= a + 1"""
    field, origin, r, E, seed, box, _ = GROW_CASES["the_order_of_the_round"]
    cells = [(1, 0, 0), (1, 1, 0), (1, 2, 0)]
    assert free_ref(field, origin, r, cells[1]) and not all(box[k] <= cells[1][k] <= box[k + 3] for k in range(3))
    got, e, empty = anchor_box_ref(field, origin, r, E, cells, 0)
    assert got == GROW_CASES["the_pair_of_that_plane"][5] and e == 2 and not empty
    assert both_paths(field, origin, r, E, cells) == ([got], [0], 0)


LINE = flat((8, 1, 1), -1)                                              # eight free cells in a row
STEP = flat((4, 2, 1), -1, {(0, 1, 0): 0, (1, 1, 0): 0, (3, 0, 0): 0})  # free: x 0 .. 2 of row 0, x 2 .. 3 of row 1
PATH_CASES = {                                                          # name -> (field, origin, r, E, cells, boxes, anchors, gaps), by hand
    "no_cells": (LINE, (0, 0, 0), 0, 4, [], [], [], 0),
    "one_free_cell": (LINE, (0, 0, 0), 0, 2, [(3, 0, 0)], [(1, 0, 0, 5, 0, 0)], [0], 0),
    "one_cell_that_is_not_free": (STEP, (0, 0, 0), 0, 2, [(3, 0, 0)], [(3, 0, 0, 2, -1, -1)], [0], 1),
    "one_cell_outside_the_region": (LINE, (0, 0, 0), 0, 2, [(-(1 << 31), 9, 0)], [(-(1 << 31), 9, 0, (1 << 31) - 1, 8, -1)], [0], 1),
    # E = 0: every box is the pair, and the last cell closes the chain
    "pairs": (LINE, (0, 0, 0), 0, 0, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], [(0, 0, 0, 1, 0, 0), (1, 0, 0, 2, 0, 0), (2, 0, 0, 3, 0, 0)], [0, 1, 2], 0),
    # round the step: the first box is row 0, the second the column x 2, the third row 1
    "round_the_step": (STEP, (0, 0, 0), 0, 8, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0), (3, 1, 0)],
                       [(0, 0, 0, 2, 0, 0), (2, 0, 0, 2, 1, 0), (2, 1, 0, 3, 1, 0)], [0, 2, 3], 0),
    # a jump: the box of (1) alone ends the stretch at once (a gap), the chain goes on behind it
    "a_jump": (LINE, (0, 0, 0), 0, 0, [(0, 0, 0), (1, 0, 0), (5, 0, 0), (6, 0, 0)], [(0, 0, 0, 1, 0, 0), (1, 0, 0, 1, 0, 0), (5, 0, 0, 6, 0, 0)], [0, 1, 2], 1),
    "a_jump_inside_one_box": (LINE, (0, 0, 0), 0, 8, [(0, 0, 0), (1, 0, 0), (5, 0, 0), (6, 0, 0)], [(0, 0, 0, 7, 0, 0)], [0], 0),
    # through a cell that is not free: its box is empty, the anchor moves on by one
    "through_a_blocked_cell": (STEP, (0, 0, 0), 0, 8, [(2, 0, 0), (3, 0, 0), (3, 1, 0)],
                               [(0, 0, 0, 2, 0, 0), (3, 0, 0, 2, -1, -1), (2, 1, 0, 3, 1, 0)], [0, 1, 2], 2),
}


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_corridors_by_hand(name):
    field, origin, r, E, cells, boxes, anchors, gaps = PATH_CASES[name]
    assert both_paths(field, origin, r, E, cells) == (boxes, anchors, gaps)
    if gaps == 0 and cells:
        check_chain(field, origin, r, cells, boxes, anchors)


def stored_prefix(cells, length, max_cells):
    """the cells a call uses of a path stored with `length`: the first min(|length|, max_cells)"""
    return cells[:min(abs(length), max_cells)]


def test_a_negative_length_a_truncated_path_and_max_boxes():
    field, origin, r, E, cells, boxes, anchors, gaps = PATH_CASES["round_the_step"]
    assert both_paths(field, origin, r, E, stored_prefix(cells, -5, 5)) == (boxes, anchors, gaps)     # a stopped walk: its stored cells
    # truncated to three cells: the first box alone, and its last cell closes the chain
    assert both_paths(field, origin, r, E, stored_prefix(cells, 5, 3)) == (boxes[:1], [0], 0)
    assert both_paths(field, origin, r, E, stored_prefix(cells, -5, 4)) == (boxes[:2], [0, 2], 0)
    # max_boxes below the count: the device stores boxes[:max_boxes] and anchors[:max_boxes], the count stays 3
    assert len(boxes) == 3 and boxes[:2] == [(0, 0, 0, 2, 0, 0), (2, 0, 0, 2, 1, 0)]


# ---- the two worlds of tests/test_plan_cpu.py ------------------------------------------------------------------------------------------
WORLD_PATHS = [("two_routes", "weighted"), ("two_routes", "reach"), ("serpentine", "weighted"), ("serpentine", "reach")]
RADII, EXTENTS = (0, 1), (0, 1, 4, 64)
_CORRIDORS = {}


def world_corridors(name, which, r, E):
    """path_corridors_ref on a world's path against the world's comfort field, computed once"""
    key = (name, which, r, E)
    if key not in _CORRIDORS:
        w = world(name)
        _CORRIDORS[key] = path_corridors_ref(w["field"], w["origin"], r, E, world_path(name, which))
    return _CORRIDORS[key]


@pytest.mark.parametrize("name,which", WORLD_PATHS)
def test_the_worlds(name, which):
    w = world(name)
    cells = world_path(name, which)
    unbroken = 0
    for r in RADII:
        assert r <= w["comfort"]
        for E in EXTENTS:
            boxes, anchors, gaps = world_corridors(name, which, r, E)
            assert path_corridors_mask(w["field"], w["origin"], r, E, cells) == (boxes, anchors, gaps), (r, E)
            if gaps == 0:
                check_chain(w["field"], w["origin"], r, cells, boxes, anchors)
                unbroken += 1
            if E == 0 and gaps == 0:
                assert anchors == list(range(len(cells) - 1))           # every box a pair
    # a path traced at the world's clearance is a chain of free face neighbours at every r up to it
    assert unbroken >= 4 * (1 + w["clearance"])


def test_two_routes_box_counts():
    cells = world_path("two_routes", "weighted")
    assert len(cells) == 217
    counts = [len(world_corridors("two_routes", "weighted", 1, E)[0]) for E in EXTENTS]
    assert counts == [216, 106, 43, 5], counts
    assert all(world_corridors("two_routes", "weighted", 1, E)[2] == 0 for E in EXTENTS)


def test_the_serpentine_reach_path_at_a_larger_clearance_is_mostly_gaps():
    """the reach path was traced at clearance 0 and hugs the walls: at r = 1 most of its cells are not free"""
    w = world("serpentine")
    cells = world_path("serpentine", "reach")
    for E in EXTENTS:
        boxes, anchors, gaps = world_corridors("serpentine", "reach", 1, E)
        empty = sum(b[3] < b[0] for b in boxes)
        assert empty == 835 and len(boxes) >= 858 and gaps >= empty, (E, empty, len(boxes), gaps)
        assert empty == sum(not free_ref(w["field"], w["origin"], 1, cells[a]) for a in anchors)


def test_the_two_restatements_agree_on_seeds_all_over_a_world():
    w = world("two_routes")
    o, dims = np.asarray(w["origin"]), np.asarray(w["dims"])
    rng = np.random.default_rng(11)
    lo = rng.integers(-1, dims + 1, (150, 3)) + o
    hi = lo + rng.integers(-1, 3, (150, 3))
    valid = 0
    for k in range(150):
        for r, E in ((0, 3), (1, 64)):
            valid += both_boxes(w["field"], w["origin"], r, E, lo[k].tolist() + hi[k].tolist())[1] >= 0
    assert 20 < valid < 280, valid                                      # both kinds, many times


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_the_header_the_signatures_and_the_library():
    pkg = load_pkg()
    assert isinstance(pkg.corridors.SIGNATURES, dict) and pkg.corridors.MAX_EXTENT == 65536
    header = open(os.path.join(ROOT, "include", "svoslam_corridor.h")).read()
    declared = sorted(set(re.findall(r"\b(svoslam_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(pkg.corridors.SIGNATURES) == ["svoslam_field_grow_boxes", "svoslam_field_path_corridors"]
    assert "#define SVOSLAM_MAX_CORRIDOR_EXTENT 65536" in header and '#include "svoslam.h"' in header
    assert not set(pkg.corridors.SIGNATURES) & set(pkg.SIGNATURES)
    assert "svoslam_field_grow_boxes" not in open(pkg.HEADER_PATH).read()
    L = C.CDLL(pkg.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), "%s is not exported" % name
    for name in ("grow_boxes", "path_corridors", "plan_corridors"):
        assert callable(getattr(pkg.corridors, name, None)), name
    assert not hasattr(pkg, "grow_boxes") and not hasattr(pkg, "path_corridors")


def test_no_gpu_means_loud_failure():
    import torch
    pkg = load_pkg()
    if torch.cuda.is_available():
        return
    L = pkg.corridors.lib()
    i3 = (C.c_int32 * 3)(0, 0, 0)
    assert L.svoslam_field_grow_boxes(None, i3, i3, 0, 0, None, 0, None, None, None) == -2       # SVOSLAM_ERR_NO_DEVICE
    assert L.svoslam_field_path_corridors(None, i3, i3, 0, 0, None, None, 0, 0, 0, None, None, None, None, None) == -2
    assert b"no CPU fallback" in L.svoslam_last_error()


def test_importing_the_package_still_loads_neither_torch_nor_the_library():
    code = ("import sys; sys.path.insert(0, %r); import svoslam_pkg; pkg = svoslam_pkg.load(); abi = sys.modules['octree_slam_amd._abi'];"
            "assert 'torch' not in sys.modules, 'torch was imported'; assert abi._lib is None and pkg.corridors._bound is None;"
            "assert sorted(pkg.corridors.SIGNATURES) == ['svoslam_field_grow_boxes', 'svoslam_field_path_corridors']; print('lazy')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "lazy", out.stderr


def test_the_argument_checks_come_before_any_device():
    pkg = load_pkg()
    for origin, dims in (((0, 0), (2, 2, 2)), ((0, 0, 0), (2, 2))):
        with pytest.raises(ValueError):
            pkg.corridors.grow_boxes([], origin, dims, 0, 0, [])
        with pytest.raises(ValueError):
            pkg.corridors.path_corridors([], origin, dims, 0, 0, [], [])
