"""The owner field of a map region (svoslam_pool_owner_field; include/svoslam.h): which seed is nearest by
path.  The definition restated by brute force -- one reach field per label, the minimum, the smallest label that attains it
(owner_field_words) -- and a second restatement as ONE breadth-first pass in which a cell of level k takes the smallest owner among
its neighbours of level k - 1 (owner_field_levels); the two proven equal on a pool fused by the CPU oracle, on random occupancy
(where the file asserts that ties are common enough to exercise the tie rule) and on hand-built pools with every value written
out.  Then `segment_rooms` restated in numpy on a hand scene with written-out figures.  No GPU.

owner_field_words is what the device call must produce; tests/test_gpu_owner.py compares against it value for value."""
import ctypes as C
import os

import numpy as np
import pytest

from test_components_cpu import component_labels_words, component_sizes, random_pool, RANDOM_DEPTH
from test_field_cpu import distance_field_separable, distance_field_words, fields, fused_regions  # noqa: F401
from test_reach_cpu import REACH_CASES, cells_pool, counted_seeds, reach_field_words, seeds_for
from test_surface_cpu import HandPool, load_pkg
from test_volume_cpu import DEPTH, fused  # noqa: F401

I64 = np.int64
NO_OWNER = (1 << 31) - 1                                                # above every label: 0 .. 2^31 - 2
TILE = (64, 8, 8)                                                       # map_relax.hpp: the cells of a tile, x y z


# ---- the specification, restated -------------------------------------------------------------------------------------------
def seed_labels(free, origin, dims, seeds=None, seed_field=None):
    """-> (cells [m, 3] int64 region-relative x y z, labels [m] int64, seeds_used): the counted seeds.  List form: every entry in the
    region and in T, its label its index, duplicates each their own row.  Field form: the cells of T with 0 <= v < 2^31 - 1."""
    assert (seeds is None) != (seed_field is None)
    if seed_field is None:
        s = np.asarray(seeds, I64).reshape(-1, 3) - np.asarray(origin, I64)
        k = np.arange(s.shape[0], dtype=I64)
        keep = ((s >= 0) & (s < np.asarray(dims, I64))).all(1)
        s, k = s[keep], k[keep]
        keep = free[s[:, 2], s[:, 1], s[:, 0]]
        return s[keep], k[keep], int(keep.sum())
    v = np.asarray(seed_field).astype(I64)
    assert v.shape == free.shape
    at = np.argwhere(free & (v >= 0) & (v < NO_OWNER))
    return at[:, ::-1], v[at[:, 0], at[:, 1], at[:, 2]], at.shape[0]


def owner_field_words(words, depth, origin, dims, clearance, seeds=None, seed_field=None, field=None, ties=None):
    """-> (steps, owner, seeds_used), int32 [nz, ny, nx] each: svoslam_pool_owner_field by its definition, by brute force.  One
    reach_field_words per label (from all the counted seeds that carry it); the steps are the minimum over the labels; the owner is
    the smallest label that attains the minimum; elsewhere the owner is the steps' -1 or -2.  `ties`: a list that receives the
    number of reached cells at which more than one label attains the minimum."""
    if field is None:
        field = distance_field_words(words, depth, origin, dims, clearance)
    free = field == -1
    cells, labels, used = seed_labels(free, origin, dims, seeds, seed_field)
    steps = np.where(free, -1, -2).astype(np.int32)
    owner = steps.astype(I64)
    best = np.full(free.shape, np.iinfo(I64).max, I64)
    attained = np.zeros(free.shape, I64)
    for label in np.unique(labels)[::-1]:                               # descending: the smallest label is written last
        mine = cells[labels == label] + np.asarray(origin, I64)
        one = reach_field_words(words, depth, origin, dims, clearance, mine, field=field).astype(I64)
        reached = one >= 0
        attained = np.where(reached & (one == best), attained + 1, np.where(reached & (one < best), 1, attained))
        owner = np.where(reached & (one <= best), label, owner)
        best = np.where(reached & (one < best), one, best)
    steps = np.where(best < np.iinfo(I64).max, best, steps).astype(np.int32)
    if ties is not None:
        ties.append(int((attained > 1).sum()))
    return steps, owner.astype(np.int32), used


def owner_field_levels(words, depth, origin, dims, clearance, seeds=None, seed_field=None):
    """the same by another route: the traversable set from the separable distance field, then ONE breadth-first pass.  Level 0 is
    the seed cells, each with the smallest label it carries; the cells of level k are the unreached traversable face neighbours
    inside the region of level k - 1, and each takes the minimum owner over its neighbours of level k - 1."""
    free = distance_field_separable(words, depth, origin, dims, clearance) == -1
    cells, labels, used = seed_labels(free, origin, dims, seeds, seed_field)
    steps = np.where(free, -1, -2).astype(np.int32)
    owner = np.full(free.shape, NO_OWNER, I64)
    np.minimum.at(owner, (cells[:, 2], cells[:, 1], cells[:, 0]), labels)
    front = owner < NO_OWNER
    level = 0
    while front.any():
        steps[front] = level
        carried = np.where(front, owner, NO_OWNER)
        offered = np.full(free.shape, NO_OWNER, I64)
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            offered[tuple(hi)] = np.minimum(offered[tuple(hi)], carried[tuple(lo)])
            offered[tuple(lo)] = np.minimum(offered[tuple(lo)], carried[tuple(hi)])
        front = (offered < NO_OWNER) & (steps == -1)
        owner = np.where(front, offered, owner)
        level += 1
    return steps, np.where(steps >= 0, owner, steps).astype(np.int32), used


def field_of_list(origin, dims, seeds):
    """the seed field that says what a seed list says: at every region cell that carries entries the smallest index, else -1"""
    out = np.full((dims[2], dims[1], dims[0]), -1, np.int32)
    s = np.asarray(seeds, I64).reshape(-1, 3) - np.asarray(origin, I64)
    for k in range(s.shape[0] - 1, -1, -1):
        if ((s[k] >= 0) & (s[k] < np.asarray(dims, I64))).all():
            out[s[k, 2], s[k, 1], s[k, 0]] = k
    return out


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_level_pass_is_the_brute_force(fused, fields, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    rng = np.random.default_rng(11)
    for clearance in (0, 1):
        field = fields(depth, region, clearance)
        for count in ((7,) if (region, depth) == ("whole_root", DEPTH) else (2, 7)):     # 262144 cells: once is enough
            seeds = seeds_for(field == -1, origin, dims, depth, count, rng)[::-1]     # the ignored entries first: labels are not 0 .. m - 1
            steps, owner, used = owner_field_words(words, depth, origin, dims, clearance, seeds, field=field)
            assert steps.dtype == owner.dtype == np.int32 and steps.shape == owner.shape == (dims[2], dims[1], dims[0])
            assert np.array_equal(steps, reach_field_words(words, depth, origin, dims, clearance, seeds, field=field)), (clearance, count)
            again = owner_field_levels(words, depth, origin, dims, clearance, seeds)
            assert np.array_equal(again[0], steps) and np.array_equal(again[1], owner) and again[2] == used, (clearance, count)
            assert used == counted_seeds(field == -1, origin, dims, seeds).shape[0] == min(count, int((field == -1).sum()))
            assert np.array_equal(owner[steps < 0], steps[steps < 0]) and (owner[steps >= 0] >= 0).all()
            # the field form of the same seeds gives the same owners
            as_field = field_of_list(origin, dims, seeds)
            for restatement in (owner_field_words, owner_field_levels):
                got = restatement(words, depth, origin, dims, clearance, seed_field=as_field)
                assert np.array_equal(got[0], steps) and np.array_equal(got[1], owner), (restatement.__name__, clearance, count)


# ---- random occupancy: where ties are common -----------------------------------------------------------------------------------
# (pool: p of test_components_cpu.random_pool at depth 7, or "wide" = its wide_random_pool at depth 8; origin; dims; clearance;
# seeds from T).  nx 1, 63, 64, 65, 130: the edges of a row word, a wavefront and a tile; ny, nz 1, 7, 8, 9, 17: one row, one less
# than, equal to, one more than and more than twice the tile's side; origin x 0, 37, N - nx; 1, 2, 12 and 300 seeds.
RANDOM_CASES = [
    (0.2, (0, 5, 52), (64, 17, 8), 0, 12), (0.31, (0, 5, 52), (64, 17, 8), 1, 2), (0.2, (37, 3, 50), (65, 9, 7), 1, 300),
    (0.31, (37, 3, 50), (65, 9, 7), 0, 12), (0.31, (65, 10, 60), (63, 7, 17), 0, 300), (0.2, (65, 10, 60), (63, 7, 17), 1, 1),
    (0.31, (37, 8, 55), (1, 8, 9), 0, 300), (0.2, (127, 8, 55), (1, 17, 1), 0, 2), ("wide", (37, 3, 50), (130, 17, 9), 0, 12),
    ("wide", (126, 4, 51), (130, 1, 17), 0, 300), ("wide", (0, 5, 52), (130, 9, 1), 1, 2), (0.31, (0, 5, 52), (65, 17, 1), 0, 12),
    (0.2, (0, 20, 60), (64, 1, 1), 0, 300), ("wide", (37, 3, 50), (130, 8, 8), 1, 12),
]
TIE_CASES = [(0.2, (37, 5, 52), (65, 17, 17), 0, 12), (0.31, (37, 5, 52), (65, 17, 17), 0, 12)]
_random = {}


def random_case(case):
    """-> (words, depth, origin, dims, clearance, seeds, steps, owner, seeds_used, ties), by the brute force, computed once"""
    if case not in _random:
        from test_components_cpu import WIDE_DEPTH, wide_random_pool
        p, origin, dims, clearance, count = case
        words, depth = (wide_random_pool()[0], WIDE_DEPTH) if p == "wide" else (random_pool(p)[0], RANDOM_DEPTH)
        field = distance_field_separable(words, depth, origin, dims, clearance)
        seeds = seeds_for(field == -1, origin, dims, depth, count, np.random.default_rng(len(_random) + 20))
        if count == 300:                                                # duplicates too: the first forty again, in reverse
            seeds = np.concatenate([seeds, seeds[:40][::-1]])
        ties = []
        steps, owner, used = owner_field_words(words, depth, origin, dims, clearance, seeds, field=field, ties=ties)
        for a in (steps, owner):
            a.setflags(write=False)
        _random[case] = (words, depth, origin, dims, clearance, seeds, steps, owner, used, ties[0])
    return _random[case]


@pytest.mark.parametrize("case", TIE_CASES, ids=lambda c: "p%s" % c[0])
def test_random_occupancy_has_ties(case):
    """12 seeds in 65 x 17 x 17 cells of random occupancy: at least 3 % of the reached cells have more than one nearest seed, or the
    tie rule is not exercised (found for this draw: about 8 %)"""
    words, depth, origin, dims, clearance, seeds, steps, owner, used, ties = random_case(case)
    reached = int((steps >= 0).sum())
    assert used == 12 and reached > 5000, (used, reached)
    assert ties >= 0.03 * reached, (ties, reached)
    again = owner_field_levels(words, depth, origin, dims, clearance, seeds)
    assert np.array_equal(again[0], steps) and np.array_equal(again[1], owner) and again[2] == used


def test_an_empty_tile_with_four_seeds_has_ties():
    origin, dims = (0, 0, 0), (64, 8, 8)
    seeds = [(5, 1, 2), (40, 6, 1), (58, 2, 7), (22, 5, 5)]
    ties = []
    steps, owner, used = owner_field_words(HandPool().words(), 6, origin, dims, 0, seeds, ties=ties)
    assert used == 4 and (steps >= 0).all() and ties[0] >= 0.03 * 4096, ties
    again = owner_field_levels(HandPool().words(), 6, origin, dims, 0, seeds)
    assert np.array_equal(again[0], steps) and np.array_equal(again[1], owner)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "p%s-%dx%dx%d-r%d-seeds%d" % (c[0], *c[2], c[3], c[4]))
def test_random_occupancy_both_restatements(case):
    words, depth, origin, dims, clearance, seeds, steps, owner, used, ties = random_case(case)
    again = owner_field_levels(words, depth, origin, dims, clearance, seeds)
    assert np.array_equal(again[0], steps) and np.array_equal(again[1], owner) and again[2] == used
    assert np.array_equal(steps, reach_field_words(words, depth, origin, dims, clearance, seeds))


def test_the_random_cases_cover_the_shapes():
    nx, nyz, ox, radii, counts = set(), set(), set(), set(), set()
    reached = tied = 0
    for case in RANDOM_CASES:
        p, origin, dims, clearance, count = case
        n_side = 256 if p == "wide" else 128
        nx.add(dims[0]); nyz.update(dims[1:]); radii.add(clearance); counts.add(count)
        ox.add("lo" if origin[0] == 0 else "hi" if origin[0] + dims[0] == n_side else origin[0])
        got = random_case(case)
        reached, tied = reached + int((got[6] >= 0).sum()), tied + got[9]
    assert nx == {1, 63, 64, 65, 130} and nyz == {1, 7, 8, 9, 17} and ox == {"lo", "hi", 37} and radii == {0, 1}
    assert counts == {1, 2, 12, 300} and reached > 20000 and tied > 1000, (reached, tied)


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def owner_cases():
    """name -> (words, depth, origin, dims, clearance, seeds or None, seed_field or None, expected steps, expected owner, expected
    seeds_used).  n: not traversable, u: unreachable, M: the largest label"""
    out = {}
    n, u, M = -2, -1, (1 << 31) - 2
    empty = HandPool().words()
    i32 = lambda rows: np.array(rows, np.int32)                         # noqa: E731
    # two seeds at the ends of a corridor: of odd length the middle cell is as near to both and goes to the smaller index
    out["corridor_odd"] = (empty, 3, (1, 4, 2), (7, 1, 1), 0, [(7, 4, 2), (1, 4, 2)], None, i32([[[0, 1, 2, 3, 2, 1, 0]]]),
                           i32([[[1, 1, 1, 0, 0, 0, 0]]]), 2)
    out["corridor_odd_swapped"] = (empty, 3, (1, 4, 2), (7, 1, 1), 0, [(1, 4, 2), (7, 4, 2)], None, i32([[[0, 1, 2, 3, 2, 1, 0]]]),
                                   i32([[[0, 0, 0, 0, 1, 1, 1]]]), 2)
    out["corridor_even"] = (empty, 3, (1, 4, 2), (6, 1, 1), 0, [(6, 4, 2), (1, 4, 2)], None, i32([[[0, 1, 2, 2, 1, 0]]]),
                            i32([[[1, 1, 1, 0, 0, 0]]]), 2)
    # a diamond: the cell in the middle has four predecessors; those first in index order (-x, -y) carry 1, the others 0
    out["diamond"] = (empty, 3, (2, 2, 5), (3, 3, 1), 0, [(4, 4, 5), (2, 2, 5)], None, i32([[[0, 1, 2], [1, 2, 1], [2, 1, 0]]]),
                      i32([[[1, 1, 0], [1, 0, 0], [0, 0, 0]]]), 2)
    # three entries on one cell: the cell takes the smallest index, every entry counts
    out["duplicates_on_a_cell"] = (empty, 3, (1, 4, 2), (5, 1, 1), 0, [(5, 4, 2), (1, 4, 2), (1, 4, 2), (1, 4, 2)], None,
                                   i32([[[0, 1, 2, 1, 0]]]), i32([[[1, 1, 0, 0, 0]]]), 4)
    # a seed on a blocked cell, outside the region, outside the root: ignored; the labels of the two that count are 4 and 5
    one = REACH_CASES["one_cell_in_the_way"][0]                         # (2,3,3) is occupied
    out["ignored_seeds_keep_their_index"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(2, 3, 3), (5, 3, 3), (-1, 3, 3), (8, 3, 3), (1, 3, 3), (4, 4, 3)],
                                             None, i32([[[2, 1, 2, 3, 2], [1, 0, n, 2, 1], [2, 1, 2, 1, 0]]]),
                                             i32([[[4, 4, 4, 4, 5], [4, 4, n, 5, 5], [4, 4, 4, 5, 5]]]), 2)
    out["no_seed_counts"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [(2, 3, 3), (7, 7, 7), (-(1 << 31), 3, 3)], None,
                             i32([[[u, u, u, u, u], [u, u, n, u, u], [u, u, u, u, u]]]), i32([[[u, u, u, u, u], [u, u, n, u, u], [u, u, u, u, u]]]), 0)
    out["no_seeds"] = (one, 3, (0, 2, 3), (5, 3, 1), 0, [], None, out["no_seed_counts"][7], out["no_seed_counts"][8], 0)
    # a wall at x = 3 whose only gap, y = 6, lies outside the region y = 0..3: it splits the region, and what no seed reaches is -1
    gap = REACH_CASES["the_gap_is_outside_the_region"][0]
    out["a_wall_splits_the_region"] = (gap, 3, (0, 0, 3), (8, 4, 1), 0, [(0, 0, 3)], None, REACH_CASES["the_gap_is_outside_the_region"][6],
                                       i32([[[0, 0, 0, n, u, u, u, u]] * 4]), 1)
    out["a_seed_on_each_side_of_the_wall"] = (gap, 3, (0, 0, 3), (8, 4, 1), 0, [(7, 3, 3), (0, 0, 3)], None,
                                              i32([[[0, 1, 2, n, 6, 5, 4, 3], [1, 2, 3, n, 5, 4, 3, 2], [2, 3, 4, n, 4, 3, 2, 1], [3, 4, 5, n, 3, 2, 1, 0]]]),
                                              i32([[[1, 1, 1, n, 0, 0, 0, 0]] * 4]), 2)
    # ... a region that holds the gap: the far side is 13 steps and more from (0,0,3), and nearer to (7,0,3) except by the gap
    out["the_gap_is_inside_the_region"] = (gap, 3, (0, 0, 3), (8, 7, 1), 0, [(7, 0, 3), (0, 0, 3)], None,
                                           i32([[[0, 1, 2, n, 3, 2, 1, 0], [1, 2, 3, n, 4, 3, 2, 1], [2, 3, 4, n, 5, 4, 3, 2], [3, 4, 5, n, 6, 5, 4, 3],
                                                 [4, 5, 6, n, 7, 6, 5, 4], [5, 6, 7, n, 8, 7, 6, 5], [6, 7, 8, 9, 9, 8, 7, 6]]]),
                                           i32([[[1, 1, 1, n, 0, 0, 0, 0]] * 6 + [[1, 1, 1, 1, 0, 0, 0, 0]]]), 2)
    # clearance 1 about the cell (2,3,3) in the plane z = 3: the cell and its four face neighbours are blocked
    out["clearance_1"] = (one, 3, (0, 2, 3), (5, 5, 1), 1, [(0, 6, 3), (4, 2, 3)], None,
                          i32([[[4, 5, n, 1, 0], [3, n, n, n, 1], [2, 3, n, 3, 2], [1, 2, 3, 4, 3], [0, 1, 2, 3, 4]]]),
                          i32([[[0, 0, n, 1, 1], [0, n, n, n, 1], [0, 0, n, 1, 1], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0]]]), 2)
    # the field form: the labels 0, 7 and 2^31 - 2; -1 and 2^31 - 1 are no seeds
    out["field_form_labels"] = (empty, 3, (0, 4, 2), (8, 1, 1), 0, None, i32([[[7, -1, M + 1, -1, M, -1, -1, 0]]]),
                                i32([[[0, 1, 2, 1, 0, 1, 1, 0]]]), i32([[[7, 7, 7, M, M, M, 0, 0]]]), 3)
    out["field_form_seed_on_a_blocked_cell"] = (one, 3, (0, 3, 3), (5, 1, 1), 0, None, i32([[[3, -1, 5, -1, -(1 << 31)]]]),
                                                i32([[[0, 1, n, u, u]]]), i32([[[3, 3, n, u, u]]]), 1)
    # one label on several cells: the nearest cell of the label counts
    out["field_form_a_label_on_two_cells"] = (empty, 3, (0, 4, 2), (8, 1, 1), 0, None, i32([[[9, -1, -1, 4, -1, -1, -1, 9]]]),
                                              i32([[[0, 1, 1, 0, 1, 2, 1, 0]]]), i32([[[9, 9, 4, 4, 4, 4, 9, 9]]]), 3)
    return out


OWNER_CASES = owner_cases()


@pytest.mark.parametrize("name", sorted(OWNER_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, clearance, seeds, seed_field, want_steps, want_owner, used = OWNER_CASES[name]
    assert want_steps.dtype == want_owner.dtype == np.int32 and want_steps.shape == want_owner.shape == (dims[2], dims[1], dims[0])
    for restatement in (owner_field_words, owner_field_levels):
        steps, owner, counted = restatement(words, depth, origin, dims, clearance, seeds, seed_field)
        assert steps.dtype == owner.dtype == np.int32
        assert np.array_equal(steps, want_steps), (restatement.__name__, steps.tolist())
        assert np.array_equal(owner, want_owner), (restatement.__name__, owner.tolist())
        assert counted == used
    if seeds is not None:                                               # the same seeds as a field: the same owners
        steps, owner, _ = owner_field_words(words, depth, origin, dims, clearance, seed_field=field_of_list(origin, dims, seeds))
        assert np.array_equal(steps, want_steps) and np.array_equal(owner, want_owner)


def test_a_zero_dimension_is_an_empty_field():
    words = REACH_CASES["one_cell_in_the_way"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        for restatement in (owner_field_words, owner_field_levels):
            steps, owner, used = restatement(words, 3, (0, 0, 0), dims, 1, [(0, 0, 0)])
            assert steps.shape == owner.shape == (dims[2], dims[1], dims[0]) and steps.dtype == owner.dtype == np.int32 and used == 0


# ---- ties across tile faces, and the owner that arrives late ---------------------------------------------------------------------
FACE_DEPTH, FACE_ORIGIN, FACE_DIMS = 8, (37, 20, 100), (130, 17, 9)
# region-relative seed pairs in an empty region: the cells as near to both lie on the named plane, a face of a tile
FACE_PAIRS = {"x_lane_0": ((60, 8, 4), (68, 8, 4), 0, 64), "x_lane_63": ((59, 8, 4), (67, 8, 4), 0, 63), "y_first_row": ((70, 4, 4), (70, 12, 4), 1, 8),
              "y_last_row": ((70, 3, 4), (70, 11, 4), 1, 7), "z_last_layer": ((70, 8, 6), (70, 8, 8), 2, 7), "z_first_layer": ((70, 8, 7), (70, 9, 8), 2, 8),
              "all_axes": ((20, 2, 1), (100, 14, 7), 0, 64)}


def face_seeds(name, swapped):
    a, b, axis, plane = FACE_PAIRS[name]
    pair = [tuple(FACE_ORIGIN[k] + v[k] for k in range(3)) for v in ((b, a) if swapped else (a, b))]
    return pair, axis, plane


@pytest.mark.parametrize("name", sorted(FACE_PAIRS))
def test_the_face_pairs_tie_on_tile_faces(name):
    words = HandPool().words()
    for swapped in (False, True):
        seeds, axis, plane = face_seeds(name, swapped)
        ties = []
        steps, owner, used = owner_field_words(words, FACE_DEPTH, FACE_ORIGIN, FACE_DIMS, 0, seeds, ties=ties)
        one = [reach_field_words(words, FACE_DEPTH, FACE_ORIGIN, FACE_DIMS, 0, [s]) for s in seeds]
        tied = one[0] == one[1]
        on_plane = np.take(tied, plane, axis=2 - axis)
        assert used == 2 and ties[0] == tied.sum() and on_plane.sum() >= 9, (ties, int(on_plane.sum()))
        assert plane % TILE[axis] in (0, TILE[axis] - 1)
        assert (owner[tied] == 0).all() and (owner == 1).sum() > 1000


LATE_DEPTH, LATE_ORIGIN, LATE_DIMS = 8, (0, 40, 9), (256, 8, 1)
LATE_SEEDS = [(252, 46, 9), (0, 40, 9)]                                # label 0: at the end of the coil; label 1: the corridor's far end


def late_pool(low_label_far):
    """-> (words, seeds).  A corridor, row 0 of the region, through four tiles of x; in the last tile (x 192 .. 255) a coil of three
    more rows (2, 4, 6; the rows between are walls with one gap each, at x 192, 255, 192) that joins the corridor at x = 192, 192
    moves from the seed at its end.  The other seed is at x = 0: 192 moves from the junction too.  Everything downstream of the
    junction, x 192 .. 255 of row 0, is as near to both.  The coil's seed reaches it inside the last tile, in the first round; the
    far seed's owner arrives three tile faces later.  `low_label_far`: the far seed is entry 0, so the late arrival wins."""
    blocked = [(x, 40 + y, 9) for y in range(1, 8) for x in range(192)]
    blocked += [(x, 40 + 7, 9) for x in range(192, 256)]
    for y, gap in ((1, 192), (3, 255), (5, 192)):
        blocked += [(x, 40 + y, 9) for x in range(192, 256) if x != gap]
    return cells_pool(blocked, LATE_DEPTH), (LATE_SEEDS[::-1] if low_label_far else LATE_SEEDS)


@pytest.mark.parametrize("low_label_far", [True, False])
def test_the_late_owner_geometry(low_label_far):
    words, seeds = late_pool(low_label_far)
    steps, owner, used = owner_field_words(words, LATE_DEPTH, LATE_ORIGIN, LATE_DIMS, 0, seeds)
    one = [reach_field_words(words, LATE_DEPTH, LATE_ORIGIN, LATE_DIMS, 0, [s]) for s in seeds]
    far = (slice(0, 1), slice(0, 1), slice(192, 256))                   # row 0 of the last tile
    assert used == 2 and LATE_DIMS[0] >= 4 * TILE[0]
    assert np.array_equal(one[0][far], one[1][far]) and np.array_equal(steps[far][0, 0], np.arange(192, 256))   # both are nearest seeds
    assert (owner[far] == 0).all()
    coil = 1 if low_label_far else 0
    assert seeds[coil][0] // TILE[0] == 3 and seeds[1 - coil][0] // TILE[0] == 0     # three tile faces apart
    assert (owner[0, 0, :192] == 1 - coil).all() and owner[0, 6, 252] == coil
    again = owner_field_levels(words, LATE_DEPTH, LATE_ORIGIN, LATE_DIMS, 0, seeds)
    assert np.array_equal(again[0], steps) and np.array_equal(again[1], owner)


# ---- segment_rooms, restated -------------------------------------------------------------------------------------------------------
def segment_rooms_words(words, depth, origin, dims, clearance, door, min_core=1):
    """-> the dict of segment_rooms by its steps: the components of the cells `door` clear are the cores, those under min_core
    cells are dropped, the owner field at `clearance` grows the cores back; sizes by counting, doors by visiting every cell face"""
    assert door >= clearance
    cores = component_labels_words(words, depth, origin, dims, door, False).copy()
    cores[component_sizes(cores) < max(min_core, 1)] = -1
    steps, rooms, _ = owner_field_words(words, depth, origin, dims, clearance, seed_field=cores)
    labels = sorted(set(rooms[rooms >= 0].tolist()))
    faces = {}
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        for a, b in zip(rooms[tuple(lo)].reshape(-1).tolist(), rooms[tuple(hi)].reshape(-1).tolist()):
            if a >= 0 and b >= 0 and a != b:
                faces[(min(a, b), max(a, b))] = faces.get((min(a, b), max(a, b)), 0) + 1
    doors = np.array([(a, b, faces[(a, b)]) for a, b in sorted(faces)], I64).reshape(-1, 3)
    return dict(rooms=rooms, steps=steps, cores=cores, labels=np.array(labels, np.int32),
                core_sizes=np.array([(cores == k).sum() for k in labels], I64), room_sizes=np.array([(rooms == k).sum() for k in labels], I64),
                doors=doors)


ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS = 4, (1, 2, 6), (13, 7, 1)
# the plane z = 6, rows y = 2 .. 8 of the region, x = 1 .. 13: '#' occupied.  Two rooms of 5 x 5 and 5 x 5 less a column, joined by
# a door one cell wide in the wall x = 7; behind the wall x = 12 a closet one cell wide, sealed: it is narrower than the door
# clearance, so it has no core, and no path leads to it
ROOMS_PLAN = ["#############",
              "#.....#.....#",
              "#.....#....#.",
              "#..........#.",
              "#.....#....#.",
              "#.....#....#.",
              "#############"]


def rooms_pool():
    return cells_pool([(ROOMS_ORIGIN[0] + x, ROOMS_ORIGIN[1] + y, ROOMS_ORIGIN[2]) for y, row in enumerate(ROOMS_PLAN)
                       for x, c in enumerate(row) if c == "#"], ROOMS_DEPTH)


def rooms_scene_expected():
    """-> (a, b, rooms at door_cells = 1 and clearance 0), every value written out.  The cores are the cells with no occupied face
    neighbour: x 2 .. 4, y 2 .. 4 and the cell (5,3) in front of the door, 10 cells from index 2 * 13 + 2; x 8 .. 9, y 2 .. 4 and
    the cell (7,3), 7 cells from index 2 * 13 + 8.  The door cell (6,3) is one move from both cores: the smaller label."""
    n, u, a, b = -2, -1, 2 * 13 + 2, 2 * 13 + 8
    rooms = np.array([[[n] * 13,
                       [n, a, a, a, a, a, n, b, b, b, b, b, n],
                       [n, a, a, a, a, a, n, b, b, b, b, n, u],
                       [n, a, a, a, a, a, a, b, b, b, b, n, u],
                       [n, a, a, a, a, a, n, b, b, b, b, n, u],
                       [n, a, a, a, a, a, n, b, b, b, b, n, u],
                       [n] * 13]], np.int32)
    return a, b, rooms


def test_segment_rooms_on_the_hand_scene():
    words = rooms_pool()
    a, b, want = rooms_scene_expected()
    got = segment_rooms_words(words, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, 1)
    assert got["labels"].tolist() == [a, b] and got["core_sizes"].tolist() == [10, 7]
    assert np.array_equal(got["rooms"], want), got["rooms"].tolist()
    assert got["room_sizes"].tolist() == [26, 21] and got["doors"].tolist() == [[a, b, 1]]    # one cell face, between (6,3) and (7,3)
    assert got["steps"][0, 3, 6] == 1 and got["steps"][0, 3, 5] == 0 and got["steps"][0, 3, 7] == 0 and got["steps"][0, 1, 1] == 2
    assert (got["rooms"][0, 2:6, 12] == -1).all() and (got["steps"][0, 2:6, 12] == -1).all()   # the closet: free, reached by no core
    # door_cells = 0: the cores are the components of free space themselves: the two rooms are one, from the first free cell
    # (1,1); the sealed closet is its own component of 4 cells, so with min_core = 5 it is no core and stays at -1
    first, closet = 1 * 13 + 1, 2 * 13 + 12
    whole = segment_rooms_words(words, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, 0, min_core=5)
    assert whole["labels"].tolist() == [first] and whole["room_sizes"].tolist() == [47] and whole["core_sizes"].tolist() == [47]
    assert whole["doors"].shape == (0, 3) and np.array_equal(whole["rooms"] == first, want >= 0) and np.array_equal(whole["rooms"] < 0, want < 0)
    assert (whole["steps"][whole["rooms"] >= 0] == 0).all() and np.array_equal(whole["rooms"] == -1, want == -1)
    both = segment_rooms_words(words, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, 0)
    assert both["labels"].tolist() == [first, closet] and both["room_sizes"].tolist() == [47, 4] and both["doors"].shape == (0, 3)
    # min_core above the smaller core: one room that takes everything it reaches
    big = segment_rooms_words(words, ROOMS_DEPTH, ROOMS_ORIGIN, ROOMS_DIMS, 0, 1, min_core=8)
    assert big["labels"].tolist() == [a] and big["core_sizes"].tolist() == [10] and big["room_sizes"].tolist() == [47]
    assert big["doors"].shape == (0, 3) and np.array_equal(big["rooms"] == a, want >= 0) and (big["cores"] == b).sum() == 0
    assert big["steps"][0, 1, 11] == 6 + 2                              # from the core's cell (5,3) through the door, 6 along x and 2 along y


def test_library_exports_the_owner_call():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "svoslam_pool_owner_field"), "svoslam_pool_owner_field is not exported"
    assert "svoslam_pool_owner_field" in pkg.SIGNATURES and len(pkg.SIGNATURES["svoslam_pool_owner_field"][1]) == 13
    assert hasattr(pkg, "owner_field") and hasattr(pkg, "segment_rooms")
    assert [f[0] for f in pkg._OwnerStats._fields_] == ["rounds", "tile_runs", "seeds_used", "owner_rounds", "owner_tile_runs"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_owner_field(" in header
    assert "typedef struct { int32_t rounds, tile_runs, seeds_used, owner_rounds, owner_tile_runs; } svoslam_owner_stats;" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
