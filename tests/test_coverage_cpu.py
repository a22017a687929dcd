"""Viewpoints that cover a map region (svoslam_pool_cover_views; include/svoslam.h): the specification
restated in numpy -- the target rule, the candidate-by-target sight matrix by the visibility field's integer walk, and the greedy
set cover with its tie rule -- checked against the visibility field's mask (an independent route to the same sight rule), against a
brute-force cover that recomputes every gain from sets of cell tuples, on hand-built pools with every value written out and on a
pool fused by the CPU oracle.  No GPU.

cover_views_host below is what the device call must produce; tests/test_gpu_coverage.py compares against it bit for bit."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest

from test_field_cpu import fused_regions, region_cells
from test_reach_cpu import cells_pool
from test_surface_cpu import HandPool, load_pkg
from test_visibility_cpu import counting, occupancy, visibility_field_walk, walk_pairs
from test_volume_cpu import DEPTH, MAX_RADIUS, fused  # noqa: F401

I64 = np.int64
SURFACE, FREE, ALL = 0, 1, 2                                            # include/svoslam.h SVOSLAM_COVER_*
MODES = {"surface": SURFACE, "free": FREE, "all": ALL}
MAX_COVER_VIEWS = 1024                                                  # include/svoslam.h SVOSLAM_MAX_COVER_VIEWS
OUTPUTS = ("seen", "chosen", "gain", "round", "summary")
CPU_RANGES = (0, 1, 3, 8)


# ---- the specification, restated -------------------------------------------------------------------------------------------
def targets_host(occ, depth, origin, dims, mode, select=None):
    """bool [nz, ny, nx]: the targets of the region.  Surface: occupied, and a face neighbour that lies in the root is not"""
    n_side = 1 << depth
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    box = (slice(o[2], o[2] + n[2]), slice(o[1], o[1] + n[1]), slice(o[0], o[0] + n[0]))
    if mode == ALL:
        out = np.ones((dims[2], dims[1], dims[0]), bool)
    elif mode == FREE:
        out = ~occ[box]
    else:
        assert mode == SURFACE
        solid = np.ones((n_side + 2,) * 3, bool)                        # what lies outside the root is no free neighbour
        solid[1:-1, 1:-1, 1:-1] = occ
        open_side = np.zeros_like(occ)
        for axis in range(3):
            for step in (0, 2):
                cut = [slice(1, -1)] * 3
                cut[axis] = slice(step, n_side + step)
                open_side |= ~solid[tuple(cut)]
        out = (occ & open_side)[box]
    if select is not None:
        out = out & (np.asarray(select).reshape(out.shape) != 0)
    return out


def sight_matrix_host(occ, depth, radius, cands, cells):
    """(bool [n_cands, T]: candidate c sees target t; the (candidate, target) pairs in range): the range test, then the walk"""
    cands, cells = np.asarray(cands, I64).reshape(-1, 3), np.asarray(cells, I64).reshape(-1, 3)
    if cands.shape[0] == 0:
        return np.zeros((0, cells.shape[0]), bool), 0
    places, entry = np.unique(cands, axis=0, return_inverse=True)       # a duplicate is walked once: it has its twin's row
    rows = np.zeros((places.shape[0], cells.shape[0]), bool)
    near = np.zeros(places.shape[0], I64)
    for c in np.nonzero(counting(places, depth))[0]:
        at = np.nonzero(((cells - places[c]) ** 2).sum(1) <= radius * radius)[0]
        near[c] = at.size
        rows[c, at[walk_pairs(occ, np.broadcast_to(places[c], (at.size, 3)), cells[at])]] = True
    entry = entry.reshape(-1)
    return rows[entry], int(near[entry].sum())


def cover_views_host(occ, depth, origin, dims, radius, mode, select, cands, k_max, min_gain=1):
    """svoslam_pool_cover_views in numpy -> {"seen" [n], "chosen" [k_max], "gain" [k_max], "round" [nz, ny, nx], "summary" [4]}, all
    int32, and for the tests "_matrix", "_cells" (the targets' absolute cells in target order), "_in_range" (pairs) and "_ties" (the
    rounds in which more than one candidate had the largest gain)"""
    assert 0 <= radius <= MAX_RADIUS and 0 <= k_max <= MAX_COVER_VIEWS and min_gain >= 1
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) and dims[a] >= 0 for a in range(3))
    cands = np.asarray(cands, I64).reshape(-1, 3)
    flags = targets_host(occ, depth, origin, dims, mode, select).reshape(-1)
    at = np.nonzero(flags)[0]                                           # region order: the targets' numbering
    cells = region_cells(origin, dims)[at]
    matrix, in_range = sight_matrix_host(occ, depth, radius, cands, cells)
    chosen, gain = np.full(k_max, -1, np.int32), np.zeros(k_max, np.int32)
    coverable = np.nonzero(matrix.any(0))[0]                            # the other targets take no part in any gain
    sees = matrix[:, coverable]
    first = np.full(coverable.size, -2, np.int32)
    covered = np.zeros(coverable.size, bool)
    ties = 0
    for j in range(k_max):
        gains = (sees & ~covered).sum(1)
        if gains.size == 0 or gains.max() < min_gain:
            break
        c = int(np.argmax(gains))                                       # the first of the largest: the lowest index
        ties += int((gains == gains[c]).sum() > 1)
        chosen[j], gain[j] = c, gains[c]
        first[sees[c] & ~covered] = j
        covered |= sees[c]
    rounds = np.full(flags.size, -1, np.int32)
    rounds[at] = -2
    rounds[at[coverable]] = first
    summary = np.array([at.size, (chosen >= 0).sum(), covered.sum(), coverable.size], np.int32)
    return {"seen": matrix.sum(1).astype(np.int32), "chosen": chosen, "gain": gain, "round": rounds.reshape(dims[2], dims[1], dims[0]),
            "summary": summary, "_matrix": matrix, "_cells": cells, "_in_range": in_range, "_ties": ties}


def cover_brute(occ, depth, origin, dims, radius, mode, select, cands, k_max, min_gain=1):
    """(chosen, gain, covered cells) by sets of cell tuples: what each candidate sees comes from the visibility field of that
    candidate alone, and every gain of every round is counted anew"""
    flags = targets_host(occ, depth, origin, dims, mode, select)
    targets = {tuple(c) for c in region_cells(origin, dims)[flags.reshape(-1)].tolist()}
    sees = []
    for v in np.asarray(cands, I64).reshape(-1, 3):
        count = visibility_field_walk(occ, depth, origin, dims, radius, [v])["count"]
        sees.append({tuple(c) for c in region_cells(origin, dims)[count.reshape(-1) > 0].tolist()} & targets)
    covered, chosen, gain = set(), [], []
    for _ in range(k_max):
        best, best_gain = -1, min_gain - 1
        for c, s in enumerate(sees):
            if len(s - covered) > best_gain:                            # strictly more: an equal gain later in the list loses
                best, best_gain = c, len(s - covered)
        if best < 0:
            break
        chosen.append(best)
        gain.append(best_gain)
        covered |= sees[best]
    return chosen, gain, covered


def same_cover(got, want, names=OUTPUTS):
    for name in names:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (name, got[name].dtype, got[name].shape)
        bad = np.argwhere(got[name] != want[name])
        assert bad.shape[0] == 0, (name, bad.shape[0], bad[:5].tolist(), got[name][tuple(bad[:5].T)].tolist(),
                                   want[name][tuple(bad[:5].T)].tolist())


def draw_candidates(occ, depth, origin, dims, radius, mode, count, seed):
    """`count` free cells of the root, each within max(radius, 1) cells per axis of a target (of a region cell where there is no
    target), seeded"""
    rng = np.random.default_rng(seed)
    cells = region_cells(origin, dims)
    flags = targets_host(occ, depth, origin, dims, mode).reshape(-1)
    base = cells[flags] if flags.any() else cells
    reach = max(radius, 1)
    out = np.zeros((0, 3), I64)
    while out.shape[0] < count:
        c = base[rng.integers(0, base.shape[0], 4 * count)] + rng.integers(-reach, reach + 1, (4 * count, 3))
        c = c[counting(c, depth)]
        out = np.concatenate([out, c[~occ[c[:, 2], c[:, 1], c[:, 0]]]])
    return out[:count].astype(np.int32)


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_occ(fused):
    return occupancy(fused[0], DEPTH)


# the (mode, region, range) cases of the fused pool that decide something: at least two rounds, an in-range pair that is blocked,
# and targets left after round 0.  The others are written out with their reason, which the test asserts instead
DECIDING = {("surface", "whole_root", 3), ("surface", "whole_root", 8), ("surface", "low_corner", 3), ("surface", "low_corner", 8),
            ("free", "low_corner", 8)}
# per deciding case: (T, in-range pairs that are blocked, rounds, the first three gains, rounds decided by the tie rule) of the
# restatement with draw_candidates' 64 candidates -- recorded figures of this draw (the counts of blocked pairs and rounds depend on
# the candidates drawn; T does not)
FIGURES = {("surface", "whole_root", 3): (554, 997, 49, [16, 13, 11], 39), ("surface", "whole_root", 8): (554, 8429, 31, [76, 69, 66], 16),
           ("surface", "low_corner", 3): (77, 582, 18, [21, 8, 6], 12), ("surface", "low_corner", 8): (77, 2271, 11, [23, 14, 13], 4),
           ("free", "low_corner", 8): (2393, 2269, 10, [942, 695, 321], 3)}
NO_SURFACE = ("high_corner", "one_cell", "offset_37")                   # T = 0 in surface mode
NO_BLOCKER = ("high_corner", "offset_37")                               # free mode: no occupied cell within 8 cells
FUSED_CASES = [(m, r, radius) for m in ("surface", "free") for r in sorted(fused_regions(DEPTH)) for radius in CPU_RANGES
               if (m, r, radius) in DECIDING or radius <= 1 or (m == "surface" and r in NO_SURFACE) or (m == "free" and r in NO_BLOCKER)]


@lru_cache(maxsize=None)
def _fused_case(words_key, mode, region, radius, k_max=64, count=64):
    occ = _fused_case.occ[words_key]
    origin, dims = fused_regions(DEPTH)[region]
    cands = draw_candidates(occ, DEPTH, origin, dims, radius, MODES[mode], count, 7 + 31 * radius + sorted(fused_regions(DEPTH)).index(region))
    return cands, cover_views_host(occ, DEPTH, origin, dims, radius, MODES[mode], None, cands, k_max)


_fused_case.occ = {}


def fused_case(occ, mode, region, radius):
    """(candidates, cover_views_host's result) of a fused case: 64 candidates, k_max = 64; computed once and left unchanged"""
    key = hash(occ.tobytes())
    _fused_case.occ.setdefault(key, occ)
    return _fused_case(key, mode, region, radius)


@pytest.mark.parametrize("mode,region,radius", FUSED_CASES)
def test_fused_pool_cases_decide_something_or_say_why_not(fused_occ, mode, region, radius):
    origin, dims = fused_regions(DEPTH)[region]
    cands, want = fused_case(fused_occ, mode, region, radius)
    T, n_chosen, covered, coverable = want["summary"].tolist()
    blocked = want["_in_range"] - int(want["_matrix"].sum())
    assert want["seen"].sum() == want["_matrix"].sum() and covered == want["gain"].sum() and (want["round"] >= 0).sum() == covered
    if (mode, region, radius) in DECIDING:
        assert n_chosen >= 2 and blocked >= 1 and want["gain"][0] < T, (T, n_chosen, blocked, want["gain"][:3])
        assert want["_ties"] >= 1                                       # a round in which the lowest index decided
        assert (T, blocked, n_chosen, want["gain"][:3].tolist(), want["_ties"]) == FIGURES[mode, region, radius]
        assert (np.diff(want["gain"][:n_chosen]) <= 0).all() and covered == coverable   # 64 rounds for 64 candidates: all of it
    elif mode == "surface" and region in NO_SURFACE:
        assert T == 0 and n_chosen == 0 and not want["seen"].any() and (want["round"] == -1).all()
    elif radius <= 1:                                                   # nothing lies between a cell and its face neighbour
        assert blocked == 0
    else:
        lo, hi = np.maximum(np.asarray(origin) - 8, 0), np.asarray(origin) + np.asarray(dims) + 8
        assert not fused_occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any() and blocked == 0


def test_the_deciding_cases_are_the_ones_written_out(fused_occ):
    T = {(m, r): int(targets_host(fused_occ, DEPTH, *fused_regions(DEPTH)[r], MODES[m]).sum()) for m in MODES for r in fused_regions(DEPTH)}
    assert T["surface", "whole_root"] == 554 and T["surface", "low_corner"] == 77 and T["free", "low_corner"] == 2393
    assert all(T["surface", r] == 0 for r in NO_SURFACE) and int(fused_occ.sum()) == 575


@pytest.mark.parametrize("mode,region,radius", [("surface", "low_corner", 3), ("surface", "low_corner", 8), ("free", "low_corner", 8),
                                                ("all", "offset_37", 3), ("surface", "whole_root", 3)])
def test_the_matrix_is_the_visibility_fields_mask(fused_occ, mode, region, radius):
    """at most 32 candidates: column c of the matrix is bit c of the visibility field's mask at the targets"""
    origin, dims = fused_regions(DEPTH)[region]
    cands = draw_candidates(fused_occ, DEPTH, origin, dims, radius, MODES[mode], 32, 5)
    cands[3], cands[9] = (-1, 4, 4), cands[2]                           # one that does not count, one duplicate
    want = cover_views_host(fused_occ, DEPTH, origin, dims, radius, MODES[mode], None, cands, 0)
    mask = visibility_field_walk(fused_occ, DEPTH, origin, dims, radius, cands)["mask"]
    at = want["_cells"] - np.asarray(origin)
    bits = mask[at[:, 2], at[:, 1], at[:, 0]]
    for c in range(32):
        assert np.array_equal(want["_matrix"][c], ((bits >> np.uint32(c)) & 1).astype(bool)), c
    assert want["_matrix"].any() and not want["_matrix"][3].any() and np.array_equal(want["_matrix"][9], want["_matrix"][2])


@pytest.mark.parametrize("mode,region,radius,min_gain", [("surface", "low_corner", 3, 1), ("surface", "low_corner", 8, 1),
                                                         ("surface", "low_corner", 8, 4), ("free", "offset_37", 3, 1)])
def test_the_greedy_choice_is_the_brute_force_cover(fused_occ, mode, region, radius, min_gain):
    origin, dims = fused_regions(DEPTH)[region]
    cands = draw_candidates(fused_occ, DEPTH, origin, dims, radius, MODES[mode], 24, 11)
    cands[5] = cands[1]
    want = cover_views_host(fused_occ, DEPTH, origin, dims, radius, MODES[mode], None, cands, 24, min_gain)
    chosen, gain, covered = cover_brute(fused_occ, DEPTH, origin, dims, radius, MODES[mode], None, cands, 24, min_gain)
    n = int(want["summary"][1])
    assert n == len(chosen) >= 2 and want["chosen"][:n].tolist() == chosen and want["gain"][:n].tolist() == gain
    assert (want["chosen"][n:] == -1).all() and (want["gain"][n:] == 0).all() and want["summary"][2] == len(covered)
    o = np.asarray(origin)
    assert {tuple(c) for c in (np.argwhere(want["round"] >= 0)[:, ::-1] + o).tolist()} == covered


# ---- hand-built pools: every value written out -----------------------------------------------------------------------------------
HAND_DEPTH = 4                                                          # a root of 16 cells a side
ROOT_REGION = ((0, 0, 0), (16, 16, 16))
WALL = [(8, y, z) for y in range(16) for z in range(16)]
GROUP_A, GROUP_B = [(5, 7, 8), (5, 8, 8), (5, 9, 8)], [(11, 8, 8), (11, 8, 9)]
TWO = [(4, 4, 4), (10, 4, 4)]


def select_cells(cells, origin=(0, 0, 0), dims=(16, 16, 16)):
    out = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    for x, y, z in cells:
        out[z - origin[2], y - origin[1], x - origin[0]] = 1
    return out


def hand_cases():
    """name -> dict(occupied, origin, dims, radius, mode, select, cands, k_max, min_gain; then what is expected: seen, chosen, gain,
    summary, and rounds = {cell: its d_round value} for the cells written out; every other cell of the region is -1)"""
    out = {}

    def case(name, occupied, cands, k_max, seen, chosen, gain, summary, rounds, radius=10, mode=SURFACE, select=None, min_gain=1,
             region=ROOT_REGION):
        out[name] = dict(occupied=occupied, origin=region[0], dims=region[1], radius=radius, mode=mode, select=select, cands=cands,
                         k_max=k_max, min_gain=min_gain, seen=seen, chosen=chosen, gain=gain, summary=summary, rounds=rounds)
    both = WALL + GROUP_A + GROUP_B
    sides = [(3, 8, 8), (13, 8, 8)]                                     # one candidate on each side of the wall x = 8
    groups = select_cells(GROUP_A + GROUP_B)
    rounds_ab = {**{c: 0 for c in GROUP_A}, **{c: 1 for c in GROUP_B}}
    # each side sees its own group and not the other: two rounds, the larger group first; two more rounds asked for than needed
    case("wall_between_two_groups", both, sides, 4, [3, 2], [0, 1, -1, -1], [3, 2, 0, 0], [5, 2, 5, 5], rounds_ab, select=groups)
    case("wall_candidates_swapped", both, sides[::-1], 2, [2, 3], [1, 0], [3, 2], [5, 2, 5, 5], rounds_ab, select=groups)
    case("min_gain_stops_early", both, sides, 4, [3, 2], [0, -1, -1, -1], [3, 0, 0, 0], [5, 1, 3, 5],
         {**{c: 0 for c in GROUP_A}, **{c: -2 for c in GROUP_B}}, select=groups, min_gain=3)
    case("k_max_stops_early", both, sides, 1, [3, 2], [0], [3], [5, 1, 3, 5],
         {**{c: 0 for c in GROUP_A}, **{c: -2 for c in GROUP_B}}, select=groups)
    # without group A the candidate that was best sees nothing
    case("select_removes_the_best_candidates_targets", both, sides, 4, [0, 2], [1, -1, -1, -1], [2, 0, 0, 0], [2, 1, 2, 2],
         {c: 0 for c in GROUP_B}, select=select_cells(GROUP_B))
    # two surface cells 6 apart, each candidate 2 cells from one of them at range 3
    case("equal_gains_lower_index_wins", TWO, [(10, 6, 4), (4, 6, 4)], 2, [1, 1], [0, 1], [1, 1], [2, 2, 2, 2],
         {(10, 4, 4): 0, (4, 4, 4): 1}, radius=3)
    case("duplicate_gains_nothing_after_its_twin", TWO, [(4, 6, 4), (4, 6, 4), (10, 6, 4)], 3, [1, 1, 1], [0, 2, -1], [1, 1, 0],
         [2, 2, 2, 2], {(4, 4, 4): 0, (10, 4, 4): 1}, radius=3)
    case("candidates_outside_the_root", TWO, [(-1, 6, 4), (4, 6, 4), (16, 4, 4), (10, 4, 16)], 2, [0, 1, 0, 0], [1, -1], [1, 0],
         [2, 1, 1, 1], {(4, 4, 4): 0, (10, 4, 4): -2}, radius=3)
    case("range_0_standing_on_a_target", TWO, [(10, 5, 4), (4, 4, 4)], 2, [0, 1], [1, -1], [1, 0], [2, 1, 1, 1],
         {(4, 4, 4): 0, (10, 4, 4): -2}, radius=0)
    case("no_targets", [], [(4, 6, 4), (10, 6, 4)], 2, [0, 0], [-1, -1], [0, 0], [0, 0, 0, 0], {}, radius=3)
    case("no_candidates", TWO, [], 2, [], [-1, -1], [0, 0], [2, 0, 0, 0], {(4, 4, 4): -2, (10, 4, 4): -2}, radius=3)
    case("k_max_0", TWO, [(4, 6, 4), (4, 5, 4)], 0, [1, 1], [], [], [2, 0, 0, 1], {(4, 4, 4): -2, (10, 4, 4): -2}, radius=3)
    # the surface rule: the centre of a solid 3 x 3 x 3 block is no target, its 26 other cells are
    block = [(x, y, z) for x in (5, 6, 7) for y in (5, 6, 7) for z in (5, 6, 7)]
    case("enclosed_cell_is_no_target", block, [], 0, [], [], [], [26, 0, 0, 0], {c: -2 for c in block if c != (6, 6, 6)}, radius=3)
    # (0, 5, 5) on the root's face x = 0: its five neighbours in the root are occupied, the sixth is no cell
    five = [(1, 5, 5), (0, 4, 5), (0, 6, 5), (0, 5, 4), (0, 5, 6)]
    case("root_face_is_no_free_neighbour", five + [(0, 5, 5)], [], 0, [], [], [], [5, 0, 0, 0], {c: -2 for c in five}, radius=3)
    # ... and in the root's far corner, at R = 0 (the inflation by 1 is clipped there)
    far = [(14, 15, 15), (15, 14, 15), (15, 15, 14)]
    case("root_corner_is_no_free_neighbour", far + [(15, 15, 15)], [(15, 15, 15)], 1, [0], [-1], [0], [2, 0, 0, 0],
         {(14, 15, 15): -2, (15, 14, 15): -2}, radius=0, region=((14, 14, 15), (2, 2, 1)))
    # a region of one cell: all six neighbours lie outside the region and are free
    case("free_neighbour_outside_the_region", [(5, 5, 5)], [(5, 7, 5)], 1, [1], [0], [1], [1, 1, 1, 1], {(5, 5, 5): 0}, radius=2,
         region=((5, 5, 5), (1, 1, 1)))
    return out


HAND_CASES = hand_cases()


def hand_words(case):
    return cells_pool(case["occupied"], HAND_DEPTH) if case["occupied"] else HandPool().words()


def hand_call(case):
    """the arguments of cover_views_host behind (occ, depth)"""
    return (case["origin"], case["dims"], case["radius"], case["mode"], case["select"], np.asarray(case["cands"], np.int32).reshape(-1, 3),
            case["k_max"], case["min_gain"])


def check_hand_case(got, case):
    for name in ("seen", "chosen", "gain", "summary"):
        assert got[name].tolist() == case[name], (name, got[name].tolist(), case[name])
    want = np.full(got["round"].shape, -1, np.int32)
    for (x, y, z), r in case["rounds"].items():
        want[z - case["origin"][2], y - case["origin"][1], x - case["origin"][0]] = r
    assert np.array_equal(got["round"], want), np.argwhere(got["round"] != want)[:5].tolist()


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_built_pools(name):
    case = HAND_CASES[name]
    occ = occupancy(hand_words(case), HAND_DEPTH)
    assert int(occ.sum()) == len(set(case["occupied"]))
    got = cover_views_host(occ, HAND_DEPTH, *hand_call(case))
    check_hand_case(got, case)
    chosen, gain, covered = cover_brute(occ, HAND_DEPTH, *hand_call(case))
    n = int(got["summary"][1])
    assert got["chosen"][:n].tolist() == chosen and got["gain"][:n].tolist() == gain and got["summary"][2] == len(covered)


def test_a_zero_dimension_is_an_empty_cover():
    occ = occupancy(cells_pool(TWO, HAND_DEPTH), HAND_DEPTH)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got = cover_views_host(occ, HAND_DEPTH, (2, 2, 2), dims, 3, ALL, None, [(4, 6, 4)], 3)
        assert got["round"].shape == (dims[2], dims[1], dims[0]) and got["summary"].tolist() == [0, 0, 0, 0]
        assert got["chosen"].tolist() == [-1] * 3 and got["gain"].tolist() == [0] * 3 and got["seen"].tolist() == [0]


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_cover_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_cover_views", "svoslam_workspace_cover_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "cover_views") and hasattr(pkg.Workspace, "cover_buffers")
    assert (pkg.COVER_SURFACE, pkg.COVER_FREE, pkg.COVER_ALL) == (SURFACE, FREE, ALL) and pkg.MAX_COVER_VIEWS == MAX_COVER_VIEWS
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_pool_cover_views(" in header and "int svoslam_workspace_cover_buffers(" in header
    for line in ("#define SVOSLAM_COVER_SURFACE 0", "#define SVOSLAM_COVER_FREE    1", "#define SVOSLAM_COVER_ALL     2",
                 "#define SVOSLAM_MAX_COVER_VIEWS 1024", "#define SVOSLAM_STAGE_QUERY 12", "#define SVOSLAM_STAGE_COUNT 13",
                 "#define SVOSLAM_ABI_VERSION 1"):
        assert line in header, line
    text = " ".join(header.split())
    assert "svoslam_pool_cover_views: its launches, the readback of T and all k_max rounds, one bracket per call" in text
    assert "the call reads T back once" in text and "among equal gains the LOWEST INDEX" in text
