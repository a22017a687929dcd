"""The component labels of a map region (svoslam_pool_label_components; include/svoslam.h): the definition
restated as a flood, level by level, from the smallest unlabelled cell of the set; a second restatement that relaxes "the minimum
over myself and my six neighbours" to a fixed point on the set of the separable distance field; the two proven equal on a pool
fused by the CPU oracle, on random occupancy and on hand-built pools with every output value written out; the first also checked
against the reach field's restatement seeded at a component's smallest cell, and against scipy.ndimage.label where scipy imports.
No GPU.

component_labels_words (the definition) is what the device call must produce; tests/test_gpu_components.py compares against it
value for value."""
import ctypes as C
import os

import numpy as np
import pytest

from test_field_cpu import distance_field_separable, distance_field_words, fields, fused_regions  # noqa: F401
from test_reach_cpu import cells_pool, reach_field_words
from test_surface_cpu import HAND, HandPool, OPAQUE, load_pkg, occupied_cells, path_of, rgba
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
TILE = (64, 8, 8)                                                       # map_components.hip: the cells of a tile, x y z


# ---- the specification, restated -------------------------------------------------------------------------------------------
def the_set(field, solid):
    """S: the cells where the distance field with radius = clearance is -1 (FREE), or the region's other cells (SOLID)"""
    return (field == -1) != bool(solid)


def flood_labels(in_set, tile=None):
    """-> int32 like in_set: -1 outside the set, else the smallest flat index of the cell's 6-connected component.  The cells are
    visited in index order; an unlabelled one starts a flood that grows level by level: the cells of level k + 1 are the unlabelled
    face neighbours in the set of the cells of level k, found with boolean array shifts, which cannot leave the array (each level
    works on the box about the last one, one cell wider).  `tile` (x, y, z): moves across the faces of that tiling are not made --
    the labels of the parts a component has inside each tile."""
    labels = np.full(in_set.shape, -1, np.int32)
    todo = in_set.copy()
    front = np.zeros(in_set.shape, bool)
    flat_todo, shape = todo.reshape(-1), in_set.shape
    for q in np.flatnonzero(in_set.reshape(-1)):
        if not flat_todo[q]:
            continue
        at = np.unravel_index(q, shape)
        lo, hi = [int(v) for v in at], [int(v) + 1 for v in at]
        front[at], todo[at], labels[at] = True, False, q
        while True:
            box = tuple(slice(max(lo[a] - 1, 0), min(hi[a] + 1, shape[a])) for a in range(3))
            f, grown = front[box], np.zeros(front[box].shape, bool)
            for axis in range(3):
                if f.shape[axis] < 2:
                    continue
                below, above = [slice(None)] * 3, [slice(None)] * 3
                below[axis], above[axis] = slice(None, -1), slice(1, None)
                ok = True
                if tile is not None:                                    # the move from i to i + 1 stays inside a tile
                    ok = (np.arange(box[axis].start + 1, box[axis].stop) % tile[2 - axis] != 0).reshape([-1 if a == axis else 1 for a in range(3)])
                grown[tuple(above)] |= f[tuple(below)] & ok
                grown[tuple(below)] |= f[tuple(above)] & ok
            new = grown & todo[box]
            front[box] = new
            if not new.any():
                break
            todo[box] &= ~new
            labels[box][new] = q
            for a in range(3):
                hit = np.flatnonzero(new.any(axis=tuple(b for b in range(3) if b != a)))
                lo[a], hi[a] = box[a].start + int(hit[0]), box[a].start + int(hit[-1]) + 1
    return labels


def component_labels_words(words, depth, origin, dims, clearance, solid, field=None):
    """-> int32 [nz, ny, nx]: svoslam_pool_label_components by its definition.  The set is taken from the distance field with radius
    = clearance (`field`: that field when the caller has it already), then flooded from the smallest unlabelled index."""
    assert 0 <= clearance <= MAX_RADIUS
    if field is None:
        field = distance_field_words(words, depth, origin, dims, clearance)
    assert field.shape == (dims[2], dims[1], dims[0])
    return flood_labels(the_set(field, solid))


def component_labels_relaxed(words, depth, origin, dims, clearance, solid):
    """the same labels by another route: the set from the separable distance field, then every cell of it takes the minimum over
    itself and its six neighbours in the set, all cells at once, repeated until nothing changes"""
    in_set = the_set(distance_field_separable(words, depth, origin, dims, clearance), solid)
    none = np.iinfo(I64).max
    s = np.where(in_set, np.arange(in_set.size, dtype=I64).reshape(in_set.shape), none)
    while True:
        t = s.copy()
        for axis in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(None, -1), slice(1, None)
            t[tuple(hi)] = np.minimum(t[tuple(hi)], s[tuple(lo)])
            t[tuple(lo)] = np.minimum(t[tuple(lo)], s[tuple(hi)])
        t = np.where(in_set, t, none)
        if np.array_equal(t, s):
            break
        s = t
    return np.where(in_set, s, -1).astype(np.int32)


def component_sizes(labels):
    """-> int32 like labels: the cells of the component at every cell of the set, 0 elsewhere"""
    flat = labels.reshape(-1)
    count = np.bincount(flat[flat >= 0], minlength=max(flat.size, 1))
    return np.where(flat >= 0, count[np.maximum(flat, 0)], 0).astype(np.int32).reshape(labels.shape)


def component_stats(labels):
    """-> (components, largest): what stats must hold when sizes are asked for"""
    flat = labels.reshape(-1)
    roots = np.flatnonzero(flat == np.arange(flat.size))
    return int(roots.size), int(component_sizes(labels).max()) if flat.size else 0


def check_contract(labels):
    """the labels are canonical: fixed points, and never above their own index"""
    flat = labels.reshape(-1)
    at = np.flatnonzero(flat >= 0)
    assert labels.dtype == np.int32 and (flat[at] <= at).all() and np.array_equal(flat[flat[at]], flat[at]) and (flat >= -1).all()


def tile_facts(labels):
    """of a labelling and the tiling of 64 x 8 x 8 cells: (components, components with cells in more than one tile, the most
    tile-local parts any component has in one tile) -- the parts are the components of the set when no move crosses a tile face"""
    parts = flood_labels(labels >= 0, tile=TILE)
    z, y, x = np.nonzero(labels >= 0)
    tiles_y, tiles_x = -(-labels.shape[1] // TILE[1]), -(-labels.shape[2] // TILE[0])
    tile = ((z // TILE[2]) * tiles_y + y // TILE[1]) * tiles_x + x // TILE[0]
    per_tile = np.unique(np.stack([labels[z, y, x].astype(I64), tile], 1), axis=0)
    per_part = np.unique(np.stack([labels[z, y, x].astype(I64), tile, parts[z, y, x].astype(I64)], 1), axis=0)
    spanning = int((np.unique(per_tile[:, 0], return_counts=True)[1] > 1).sum()) if per_tile.size else 0
    most = int(np.unique(per_part[:, :2], axis=0, return_counts=True)[1].max()) if per_part.size else 0
    return component_stats(labels)[0], spanning, most


def scipy_labels(in_set):
    """scipy.ndimage.label (6-connectivity is its default structure) mapped to the smallest index of each component"""
    ndi = pytest.importorskip("scipy.ndimage")
    lab, count = ndi.label(in_set)
    flat = lab.reshape(-1)
    first = np.full(count + 1, -1, I64)
    at = np.flatnonzero(flat)[::-1]
    first[flat[at]] = at                                                # the last write per label is its smallest index
    return first[flat].astype(np.int32).reshape(in_set.shape), count


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [DEPTH, DEPTH - 2])
@pytest.mark.parametrize("region", sorted(fused_regions(DEPTH)))
def test_the_relaxation_is_the_flood(fused, fields, depth, region):
    words, _ = fused
    origin, dims = fused_regions(depth)[region]
    in_set = outside = 0
    for clearance in (1,) if (region, depth) == ("whole_root", DEPTH) else (0, 1, 3):
        field = fields(depth, region, clearance)
        for solid in (False, True):
            want = component_labels_words(words, depth, origin, dims, clearance, solid, field=field)
            assert want.shape == (dims[2], dims[1], dims[0])
            check_contract(want)
            if depth < DEPTH or region != "whole_root":                 # 64^3 cells relax for seconds: that region at depth 4 only
                assert np.array_equal(component_labels_relaxed(words, depth, origin, dims, clearance, solid), want), (clearance, solid)
            assert np.array_equal(want >= 0, (field == -1) != solid)
            in_set, outside = in_set + int((want >= 0).sum()), outside + int((want < 0).sum())
    if depth == DEPTH and region in ("whole_root", "low_corner"):
        assert in_set > 1000 and outside > 1000, (in_set, outside)


@pytest.mark.parametrize("region", ["whole_root", "low_corner", "offset_37"])
def test_a_component_is_the_support_of_the_reach_field_from_its_smallest_cell(fused, fields, region):
    words, _ = fused
    depth = DEPTH - 1
    origin, dims = fused_regions(depth)[region]
    for clearance in (0, 1):
        field = fields(depth, region, clearance)
        want = component_labels_words(words, depth, origin, dims, clearance, False, field=field)
        roots = np.flatnonzero(want.reshape(-1) == np.arange(want.size))
        assert roots.size >= 1
        for q in roots[:3].tolist() + roots[-1:].tolist():
            z, y, x = np.unravel_index(q, want.shape)
            seed = (origin[0] + int(x), origin[1] + int(y), origin[2] + int(z))
            steps = reach_field_words(words, depth, origin, dims, clearance, [seed], field=field)
            assert np.array_equal(steps >= 0, want == q) and np.array_equal(steps == -2, want == -1)


@pytest.mark.parametrize("region", ["whole_root", "low_corner"])
def test_the_flood_is_scipy_label_at_minimum_indices(fused, fields, region):
    words, _ = fused
    origin, dims = fused_regions(DEPTH)[region]
    for clearance in (0, 1):
        field = fields(DEPTH, region, clearance)
        for solid in (False, True):
            got, count = scipy_labels(the_set(field, solid))
            want = component_labels_words(words, DEPTH, origin, dims, clearance, solid, field=field)
            assert np.array_equal(got, want) and count == component_stats(want)[0]
            if region == "whole_root":                                  # the fused cloud is a closed surface: it proves little
                assert count <= (1 if solid else 2)                     # about merging, which is why the random pools exist


# ---- random occupancy: the pools that can break a union-find ---------------------------------------------------------------------
RANDOM_DEPTH = 7
RANDOM_P = (0.2, 0.31, 0.45)
RANDOM_REGIONS = {"A": ((0, 5, 52), (128, 17, 17)), "B": ((37, 3, 50), (65, 9, 7)), "C": ((0, 3, 50), (128, 40, 40))}
# at p = 0.31, clearance 0, SOLID: region -> at least (components, components in more than one tile, tile-local parts of one
# component in one tile).  Found for this draw: A (2391, 318, 10), C (11635, 1136, 25); same p at clearance 1, FREE: 1558 and 8735
RANDOM_FACTS = {"A": (1000, 100, 4), "C": (5000, 500, 8)}
_random = {}


def random_pool(p):
    """-> (words, occ [z, y, x]): one generator, seeded 7, drawn for p = 0.2, 0.31, 0.45 in that order; the cell of occ[z, y, x] is
    (x, y + 3, z + 50) at depth 7"""
    if not _random:
        rng = np.random.default_rng(7)
        for each in RANDOM_P:
            occ = rng.random((40, 40, 128)) < each
            z, y, x = np.nonzero(occ)
            _random[each] = (cells_pool(zip(x.tolist(), (y + 3).tolist(), (z + 50).tolist()), RANDOM_DEPTH), occ)
    return _random[p]


WIDE_DEPTH = 8
_wide = []


def wide_random_pool():
    """-> (words, occ [z, y, x]): a draw of the same kind on a lattice wide enough for rows of 130 cells at any offset:
    default_rng(8), occ = random((20, 20, 256)) < 0.31, the cell of occ[z, y, x] is (x, y + 3, z + 50) at depth 8"""
    if not _wide:
        occ = np.random.default_rng(8).random((20, 20, 256)) < 0.31
        z, y, x = np.nonzero(occ)
        _wide.append((cells_pool(zip(x.tolist(), (y + 3).tolist(), (z + 50).tolist()), WIDE_DEPTH), occ))
    return _wide[0]


_expected = {}


def random_expected(p, region, clearance, solid):
    """-> (origin, dims, labels by the definition on the separable field), computed once and left unchanged"""
    key = (p, region, clearance, solid)
    if key not in _expected:
        origin, dims = RANDOM_REGIONS[region]
        field_key = (p, region, clearance)
        if field_key not in _expected:
            _expected[field_key] = distance_field_separable(random_pool(p)[0], RANDOM_DEPTH, origin, dims, clearance)
        _expected[key] = (origin, dims, component_labels_words(random_pool(p)[0], RANDOM_DEPTH, origin, dims, clearance, solid,
                                                               field=_expected[field_key]))
        _expected[key][2].setflags(write=False)
    return _expected[key]


def test_the_random_pool_is_its_recipe():
    """the pool's occupied set is the draw, so S at clearance 0 is the draw cut to the region"""
    for p in RANDOM_P:
        words, occ = random_pool(p)
        xyz = occupied_cells(words, RANDOM_DEPTH)[0]
        back = np.zeros(occ.shape, bool)
        back[xyz[:, 2] - 50, xyz[:, 1] - 3, xyz[:, 0]] = True
        assert xyz.shape[0] == occ.sum() and np.array_equal(back, occ)
        origin, dims, want = random_expected(p, "A", 0, True)
        assert np.array_equal(want >= 0, occ[2:19, 2:19, :])


_facts = {}


def random_facts(region):
    if region not in _facts:
        _facts[region] = tile_facts(random_expected(0.31, region, 0, True)[2])
    return _facts[region]


@pytest.mark.parametrize("region", sorted(RANDOM_FACTS))
def test_the_random_pool_has_components_that_span_tiles(region):
    """the facts that make these the cases they are meant to be: a condition on the restatement's result"""
    facts = random_facts(region)
    assert all(got >= need for got, need in zip(facts, RANDOM_FACTS[region])), facts
    if region == "A":
        assert facts == (2391, 318, 10)
        assert component_stats(random_expected(0.31, "A", 1, False)[2])[0] == 1558


@pytest.mark.parametrize("p", RANDOM_P)
def test_random_occupancy_both_restatements(p):
    words = random_pool(p)[0]
    for clearance in (0, 1):
        for solid in (False, True):
            origin, dims, want = random_expected(p, "B", clearance, solid)
            check_contract(want)
            assert np.array_equal(component_labels_relaxed(words, RANDOM_DEPTH, origin, dims, clearance, solid), want)
    origin, dims, want = random_expected(p, "A", 0, True)
    assert np.array_equal(component_labels_relaxed(words, RANDOM_DEPTH, origin, dims, 0, True), want)


def test_random_occupancy_is_scipy_label():
    for region in ("A", "B"):
        for clearance, solid in ((0, True), (1, False)):
            want = random_expected(0.31, region, clearance, solid)[2]
            got, count = scipy_labels(want >= 0)
            assert np.array_equal(got, want) and count == component_stats(want)[0]


def test_the_wide_random_pool_is_its_recipe():
    words, occ = wide_random_pool()
    xyz = occupied_cells(words, WIDE_DEPTH)[0]
    back = np.zeros(occ.shape, bool)
    back[xyz[:, 2] - 50, xyz[:, 1] - 3, xyz[:, 0]] = True
    assert xyz.shape[0] == occ.sum() and np.array_equal(back, occ)
    origin, dims = (126, 5, 52), (130, 9, 7)                            # a row of three words whose last holds two cells
    want = component_labels_words(words, WIDE_DEPTH, origin, dims, 0, True, field=distance_field_separable(words, WIDE_DEPTH, origin, dims, 0))
    assert np.array_equal(want >= 0, occ[2:9, 2:11, 126:256])
    assert np.array_equal(component_labels_relaxed(words, WIDE_DEPTH, origin, dims, 0, True), want)
    assert tile_facts(want)[1] >= 20 and (want[:, :, 127] >= 0).any() and (want[:, :, 128:] >= 0).any()


# ---- the serpentine maze with walls every fourth row: no placement of a region gives a tile three parts of the corridor ---------
def test_the_maze_with_walls_every_fourth_row_has_two_parts_per_tile_wherever_the_region_lies():
    """tests/test_gpu_components.py asserts three tile-local parts of one component in one tile for the maze with walls every
    second row, and two for this one.  Eight rows meet at most three of its corridors, with two consecutive walls between them; one
    of the two has its gap at the low end of x, the other at the high end.  For the three pieces to be ONE component the region
    must hold both gaps, so it is at least 122 cells wide from x <= 3: two tiles in x, the first holding the low gap and the
    second the high one, and in each the gap joins two of the three pieces inside the tile.  At clearance 1 a corridor is one
    free row, and eight rows hold two.  Counted here for every row offset of the region modulo the walls' pitch (tiles further down meet the others) and x origins 0 and 32."""
    from test_gpu_reach import MAZE_DEPTH, maze
    words, origin, dims, seed = maze(4, 8)
    for clearance in (0, 1):
        most = []
        for dy in range(4):
            for ox in (0, 32):
                o, d = (ox, origin[1] + dy, origin[2]), (dims[0] - ox, dims[1] - dy, dims[2])
                most.append(tile_facts(flood_labels(distance_field_separable(words, MAZE_DEPTH, o, d, clearance) == -1))[2])
        assert max(most) == 2, most


# ---- staircases: one-cell-thick paths that make long union chains ---------------------------------------------------------------
STAIR_DEPTH, STAIR_START, STAIR_CYCLES = 9, (150, 200, 201), 88


def staircase(mirrored):
    """-> (cells in path order, origin, dims, index in the path of the cell with the smallest output index).  From STAIR_START the
    path steps +x, +y, +z in turn, STAIR_CYCLES times: every cell has a larger output index than the one before, so the
    component's minimum is the first cell and the tile-local roots increase along the path.  `mirrored`: a second arm leaves the
    start stepping +z, -x, -y in turn, so the minimum is in the middle of the path and both arms climb away from it."""
    arm, at = [], list(STAIR_START)
    for k in range(3 * STAIR_CYCLES):
        at[k % 3] += 1
        arm.append(tuple(at))
    other, at = [], list(STAIR_START)
    for k in range(3 * STAIR_CYCLES if mirrored else 0):
        at[(2, 0, 1)[k % 3]] += (1, -1, -1)[k % 3]
        other.append(tuple(at))
    cells = other[::-1] + [STAIR_START] + arm
    lo = [min(c[a] for c in cells) - 1 for a in range(3)]
    hi = [max(c[a] for c in cells) + 1 for a in range(3)]
    return cells, tuple(lo), tuple(hi[a] - lo[a] + 1 for a in range(3)), len(other)


@pytest.mark.parametrize("mirrored", [False, True])
def test_the_staircase_is_one_component_through_many_tiles(mirrored):
    cells, origin, dims, first = staircase(mirrored)
    rel = np.asarray(cells, I64) - np.asarray(origin, I64)
    index = (rel[:, 2] * dims[1] + rel[:, 1]) * dims[0] + rel[:, 0]
    assert np.argmin(index) == first and (np.diff(index[first:]) > 0).all()
    assert (np.diff(index[:first + 1][::-3]) > 0).all()                 # the other arm climbs cycle by cycle (its -x and -y steps do not)
    assert len(set(map(tuple, (rel // np.asarray(TILE)).tolist()))) >= 20
    want = component_labels_words(cells_pool(cells, STAIR_DEPTH), STAIR_DEPTH, origin, dims, 0, True,
                                  field=distance_field_separable(cells_pool(cells, STAIR_DEPTH), STAIR_DEPTH, origin, dims, 0))
    assert component_stats(want) == (1, len(cells)) and want.max() == index[first]
    assert tile_facts(want)[:2] == (1, 1)


# ---- hand-built pools: every output value written out ----------------------------------------------------------------------------
def component_cases():
    """name -> (words, depth, origin, dims, clearance, solid, expected int32 labels [nz, ny, nx], expected components, largest)"""
    out = {}
    n = -1
    empty = HandPool().words()
    # an empty pool: FREE is one component with label 0, SOLID is nothing
    out["empty_pool_free"] = (empty, 2, (1, 0, 1), (3, 4, 2), 0, False, np.zeros((2, 4, 3), np.int32), 1, 24)
    out["empty_pool_free_clearance_2"] = (empty, 2, (1, 0, 1), (3, 4, 2), 2, False, np.zeros((2, 4, 3), np.int32), 1, 24)
    out["empty_pool_solid"] = (empty, 2, (1, 0, 1), (3, 4, 2), 0, True, np.full((2, 4, 3), n, np.int32), 0, 0)
    # a closed box: the shell of the 3 x 3 x 3 block about (3,3,3), seen in the plane z = 3 with a margin of one cell
    shell = cells_pool([(x, y, z) for z in (2, 3, 4) for y in (2, 3, 4) for x in (2, 3, 4) if (x, y, z) != (3, 3, 3)], 3)
    out["closed_box_plane_free"] = (shell, 3, (1, 1, 3), (5, 5, 1), 0, False,
                                    np.array([[[0, 0, 0, 0, 0], [0, n, n, n, 0], [0, n, 12, n, 0], [0, n, n, n, 0], [0, 0, 0, 0, 0]]], np.int32), 2, 16)
    out["closed_box_plane_solid"] = (shell, 3, (1, 1, 3), (5, 5, 1), 0, True,
                                     np.array([[[n, n, n, n, n], [n, 6, 6, 6, n], [n, 6, n, 6, n], [n, 6, 6, 6, n],
                                                [n, n, n, n, n]]], np.int32), 1, 8)
    # ... and with a margin of one cell all round: the outside (98 cells, label 0), the inside (cell (2,2,2) of the region, index
    # 62), and the shell as one SOLID component from its first cell (1,1,1), index 31
    box_free = np.zeros((5, 5, 5), np.int32)
    box_free[1:4, 1:4, 1:4] = n
    box_free[2, 2, 2] = 62
    out["closed_box_free"] = (shell, 3, (1, 1, 1), (5, 5, 5), 0, False, box_free, 2, 98)
    box_solid = np.full((5, 5, 5), n, np.int32)
    box_solid[1:4, 1:4, 1:4] = 31
    box_solid[2, 2, 2] = n
    out["closed_box_solid"] = (shell, 3, (1, 1, 1), (5, 5, 5), 0, True, box_solid, 1, 26)
    # two cells that touch only by an edge, (2,2,3) and (3,3,3): separate; the free cells round them are one component
    edge = cells_pool([(2, 2, 3), (3, 3, 3)], 3)
    out["edge_contact_solid"] = (edge, 3, (1, 1, 3), (4, 4, 1), 0, True,
                                 np.array([[[n, n, n, n], [n, 5, n, n], [n, n, 10, n], [n, n, n, n]]], np.int32), 2, 1)
    out["edge_contact_free"] = (edge, 3, (1, 1, 3), (4, 4, 1), 0, False,
                                np.array([[[0, 0, 0, 0], [0, n, 0, 0], [0, 0, n, 0], [0, 0, 0, 0]]], np.int32), 1, 14)
    # ... in the region of the four cells alone the two free cells touch by an edge only as well
    out["edge_contact_free_2x2"] = (edge, 3, (2, 2, 3), (2, 2, 1), 0, False, np.array([[[n, 1], [2, n]]], np.int32), 2, 1)
    # two cells that touch only by a corner, (2,2,2) and (3,3,3): separate; the other six cells of the block are a ring
    corner = cells_pool([(2, 2, 2), (3, 3, 3)], 3)
    out["corner_contact_solid"] = (corner, 3, (2, 2, 2), (2, 2, 2), 0, True, np.array([[[0, n], [n, n]], [[n, n], [n, 7]]], np.int32), 2, 1)
    out["corner_contact_free"] = (corner, 3, (2, 2, 2), (2, 2, 2), 0, False, np.array([[[n, 1], [1, 1]], [[1, 1], [1, n]]], np.int32), 1, 6)
    # a U of five cells, (1,3,3) (1,2,3) (2,2,3) (3,2,3) (3,3,3): in the row y = 3 alone its two ends are joined only through
    # cells outside the region -- separate; so are the three free cells between and beside them
    u = cells_pool([(1, 3, 3), (1, 2, 3), (2, 2, 3), (3, 2, 3), (3, 3, 3)], 3)
    out["joined_outside_the_region_solid"] = (u, 3, (0, 3, 3), (5, 1, 1), 0, True, np.array([[[n, 1, n, 3, n]]], np.int32), 2, 1)
    out["joined_outside_the_region_free"] = (u, 3, (0, 3, 3), (5, 1, 1), 0, False, np.array([[[0, n, 2, n, 4]]], np.int32), 3, 1)
    # ... a region that holds the U's bottom joins them, and cuts the free cell inside the U off
    out["joined_inside_the_region_solid"] = (u, 3, (0, 2, 3), (5, 2, 1), 0, True, np.array([[[n, 1, 1, 1, n], [n, 1, n, 1, n]]], np.int32), 1, 5)
    out["joined_inside_the_region_free"] = (u, 3, (0, 2, 3), (5, 2, 1), 0, False, np.array([[[0, n, n, n, 4], [0, n, 7, n, 4]]], np.int32), 3, 2)
    # a wall at x = 3 whose only gap, y = 6, lies outside the region y = 0..3: the two sides are separate components
    gap = cells_pool([(3, y, 3) for y in range(8) if y != 6], 3)
    out["the_gap_is_outside_the_region"] = (gap, 3, (0, 0, 3), (8, 4, 1), 0, False, np.array([[[0, 0, 0, n, 4, 4, 4, 4]] * 4], np.int32), 2, 16)
    out["the_wall_is_one_component"] = (gap, 3, (0, 0, 3), (8, 4, 1), 0, True, np.array([[[n, n, n, 3, n, n, n, n]] * 4], np.int32), 1, 4)
    # ... a region that holds the gap is one free component
    through = np.zeros((1, 7, 8), np.int32)
    through[0, :6, 3] = n
    out["the_gap_is_inside_the_region"] = (gap, 3, (0, 0, 3), (8, 7, 1), 0, False, through, 1, 50)
    # a wall at y = 1, just outside the region y = 2..3: with clearance 1 it makes the region's border row solid
    wall = cells_pool([(x, 1, 3) for x in range(8)], 3)
    out["wall_outside_clearance_1_solid"] = (wall, 3, (0, 2, 3), (8, 2, 1), 1, True, np.array([[[0] * 8, [n] * 8]], np.int32), 1, 8)
    out["wall_outside_clearance_1_free"] = (wall, 3, (0, 2, 3), (8, 2, 1), 1, False, np.array([[[n] * 8, [8] * 8]], np.int32), 1, 8)
    out["wall_outside_clearance_0_solid"] = (wall, 3, (0, 2, 3), (8, 2, 1), 0, True, np.full((1, 2, 8), n, np.int32), 0, 0)
    # alpha 127 beside 128 at depth 2: (2,2,2) is occupied, (3,2,2) is not
    out["alpha_127_128_free"] = (HAND["alpha_127_128"][0], 2, (0, 2, 2), (4, 1, 1), 0, False, np.array([[[0, 0, n, 3]]], np.int32), 2, 2)
    out["alpha_127_128_solid"] = (HAND["alpha_127_128"][0], 2, (0, 2, 2), (4, 1, 1), 0, True, np.array([[[n, n, 2, n]]], np.int32), 1, 1)
    # d one below the leaf depth: the leaf (5,2,6) of depth 3 is cell (2,1,3) at depth 2
    leaf = HandPool()
    leaf.put(path_of(5, 2, 6, 3), [OPAQUE, OPAQUE, rgba(43, 2, 3, 255)])
    out["one_level_above_the_leaf_solid"] = (leaf.words(), 2, (0, 1, 3), (4, 2, 1), 0, True, np.array([[[n, n, 2, n], [n, n, n, n]]], np.int32), 1, 1)
    out["one_level_above_the_leaf_free"] = (leaf.words(), 2, (0, 1, 3), (4, 2, 1), 0, False, np.array([[[0, 0, n, 0], [0, 0, 0, 0]]], np.int32), 1, 7)
    # two cells two apart, (2,3,3) and (4,3,3): separate at clearance 0, one SOLID component when dilated by 1
    two = cells_pool([(2, 3, 3), (4, 3, 3)], 3)
    out["two_apart_clearance_0"] = (two, 3, (0, 2, 3), (7, 3, 1), 0, True,
                                    np.array([[[n] * 7, [n, n, 9, n, 11, n, n], [n] * 7]], np.int32), 2, 1)
    out["two_apart_clearance_1_solid"] = (two, 3, (0, 2, 3), (7, 3, 1), 1, True,
                                          np.array([[[n, n, 2, n, 2, n, n], [n, 2, 2, 2, 2, 2, n], [n, n, 2, n, 2, n, n]]], np.int32), 1, 9)
    out["two_apart_clearance_1_free"] = (two, 3, (0, 2, 3), (7, 3, 1), 1, False,
                                         np.array([[[0, 0, n, 3, n, 5, 5], [0, n, n, n, n, n, 5], [0, 0, n, 17, n, 5, 5]]], np.int32), 4, 5)
    return out


COMPONENT_CASES = component_cases()


@pytest.mark.parametrize("name", sorted(COMPONENT_CASES))
def test_hand_built_pools(name):
    words, depth, origin, dims, clearance, solid, want, components, largest = COMPONENT_CASES[name]
    assert want.dtype == np.int32 and want.shape == (dims[2], dims[1], dims[0])
    for restatement in (component_labels_words, component_labels_relaxed):
        got = restatement(words, depth, origin, dims, clearance, solid)
        assert got.dtype == np.int32 and np.array_equal(got, want), (restatement.__name__, got.tolist())
    check_contract(want)
    assert component_stats(want) == (components, largest)
    sizes = component_sizes(want)
    assert sizes.reshape(-1)[np.flatnonzero(want.reshape(-1) == np.arange(want.size))].sum() == (want >= 0).sum()


def test_a_zero_dimension_is_an_empty_result():
    words = COMPONENT_CASES["edge_contact_solid"][0]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        for restatement in (component_labels_words, component_labels_relaxed):
            got = restatement(words, 3, (0, 0, 0), dims, 1, True)
            assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32
            assert component_sizes(got).shape == got.shape and component_stats(got) == (0, 0)


def test_library_exports_the_component_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_label_components", "svoslam_workspace_component_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "label_components") and hasattr(pkg.Workspace, "component_buffers")
    assert (pkg.COMPONENTS_FREE, pkg.COMPONENTS_SOLID) == (0, 1)
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_label_components(" in header and "} svoslam_component_stats;" in header
    assert "#define SVOSLAM_COMPONENTS_FREE  0" in header and "#define SVOSLAM_COMPONENTS_SOLID 1" in header
    assert "int svoslam_workspace_component_buffers(const svoslam_workspace *ws, void *d_ptrs[2], uint64_t bytes[2]);" in header
    assert "#define SVOSLAM_STAGE_QUERY 12" in header and "#define SVOSLAM_STAGE_COUNT 13" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header and "#define SVOSLAM_MAX_RADIUS_CELLS %d" % MAX_RADIUS in header
