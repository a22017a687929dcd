"""The observed space of a map region (svoslam_field_observe_rays and svoslam_pool_frontier_field; include/svoslam.h, DESIGN.md
section 25): the specification restated in numpy -- every sensor ray classified (void, outside, far, marked), the cells a marked ray
passes through and ends in by the visibility field's integer walk, the accumulate rule, and the six states of the observation held
against the map -- checked on a hand scene with every figure written out, against the supercover's definition, against the
visibility field (what a viewpoint sees is never vacated) and on a pool fused by the CPU oracle.  No GPU.

observe_rays_host and frontier_field_host below are what the device calls must produce; tests/test_gpu_observe.py compares against
them byte for byte."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

from test_coverage_cpu import cover_views_host
from test_field_cpu import fused_regions, midpoints, region_cells
from test_reach_cpu import cells_pool
from test_score_cpu import move
from test_surface_cpu import load_pkg
from test_visibility_cpu import occupancy, supercover_brute, visibility_field_walk, walk_cells
from test_volume_cpu import DEPTH, ROOT_CENTER, ROOT_EDGE, F, cell_in_block, fused, plane  # noqa: F401

I64 = np.int64
THROUGH, END = 1, 2                                                     # include/svoslam.h SVOSLAM_OBS_*
UNKNOWN, FREE, FRONTIER, OCCUPIED, VACATED, UNMAPPED = range(6)         # include/svoslam.h SVOSLAM_STATE_*
VOID, OUTSIDE, FAR, MARKED = range(4)                                   # the order of the summary's ray counts
MAX_DEPTH = 16
IDENTITY = np.eye(4, dtype=F).reshape(16)


# ---- the specification, restated -------------------------------------------------------------------------------------------
def in_root(depth, center, edge, v):
    """bool [...]: every component of v[..., 3] is finite and P_a(0) <= v_a <= P_a(N)"""
    n_side = 1 << depth
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    with np.errstate(all="ignore"):
        p0, pn = plane(c, np.zeros(3, I64), n_side, h), plane(c, np.full(3, n_side), n_side, h)
        return np.isfinite(v).all(-1) & ((p0 <= v) & (v <= pn)).all(-1)


def cells_of(depth, center, edge, v):
    """int64 [..., 3]: c_a(v_a), the non-strict count (meaningful where in_root)"""
    n_side = 1 << depth
    h, c = F(edge) / F(n_side), np.asarray(center, F)
    zero, full = np.zeros(v.shape[:-1], I64), np.full(v.shape[:-1], n_side, I64)
    with np.errstate(all="ignore"):
        return np.stack([cell_in_block(c[a], n_side, h, v[..., a], zero, full, False) for a in range(3)], -1)


def frames_of(points, poses):
    """(points [n_frames, n, 3], poses [n_frames, 16]) binary32: frame f's points are block f"""
    poses = np.asarray(poses, F).reshape(-1, 16)
    points = np.asarray(points, F).reshape(poses.shape[0], -1, 3) if poses.shape[0] else np.zeros((0, 0, 3), F)
    return points, poses


def classify_rays(depth, center, edge, points, poses, range_cells=0):
    """-> (class [n_frames, n] uint8, s [n_frames, n, 3], e [n_frames, n, 3]): steps 1 to 6 of one ray, for every ray"""
    assert 1 <= depth <= MAX_DEPTH and 0 <= range_cells <= 1 << MAX_DEPTH
    points, poses = frames_of(points, poses)
    n_frames, n = points.shape[:2]
    cls = np.zeros((n_frames, n), np.uint8)
    s, e = np.zeros((n_frames, n, 3), I64), np.zeros((n_frames, n, 3), I64)
    for f in range(n_frames):
        void = ~np.isfinite(points[f]).all(1)
        w = move(poses[f], points[f])[0]
        assert w.dtype == F
        o = np.broadcast_to(poses[f, 12:15], w.shape)
        inside = in_root(depth, center, edge, o) & in_root(depth, center, edge, w)
        s[f], e[f] = cells_of(depth, center, edge, o), cells_of(depth, center, edge, w)
        d2 = ((e[f] - s[f]) ** 2).sum(1)                                # below 2^33 in a root of depth 16
        far = (d2 > range_cells * range_cells) if range_cells > 0 else np.zeros(n, bool)
        cls[f] = np.where(void, VOID, np.where(~inside, OUTSIDE, np.where(far, FAR, MARKED)))
    return cls, s, e


def mark_cells(obs, origin, dims, cells, bit):
    c = np.asarray(cells, I64).reshape(-1, 3) - np.asarray(origin, I64)
    c = c[((c >= 0) & (c < np.asarray(dims, I64))).all(1)]
    obs[c[:, 2], c[:, 1], c[:, 0]] |= np.uint8(bit)


def observe_rays_host(depth, center, edge, origin, dims, points, poses, range_cells=0, accumulate=False, obs=None, through=None):
    """svoslam_field_observe_rays in numpy -> (obs uint8 [nz, ny, nx], summary int64 [6]).  `through(D)`: the cells of S(0, D)
    (default: the integer walk of the visibility field, walk_cells)"""
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) and dims[a] >= 0 for a in range(3))
    through = through or walk_cells
    cls, s, e = classify_rays(depth, center, edge, points, poses, range_cells)
    marks = np.zeros((dims[2], dims[1], dims[0]), np.uint8)
    done = set()
    for f, j in np.argwhere(cls == MARKED):
        a, b = tuple(int(v) for v in s[f, j]), tuple(int(v) for v in e[f, j])
        if (a, b) in done:                                              # the result is a set
            continue
        done.add((a, b))
        mark_cells(marks, origin, dims, [b], END)
        if a != b:
            between = np.asarray(through(tuple(y - x for x, y in zip(a, b))), I64).reshape(-1, 3) + np.asarray(a, I64)
            mark_cells(marks, origin, dims, np.concatenate([[a], between]), THROUGH)
    if accumulate:
        assert obs is not None
        out = np.asarray(obs, np.uint8).reshape(marks.shape) | marks    # bits 2..7 stay as found
    else:
        out = marks
    summary = np.array([(cls == k).sum() for k in (VOID, OUTSIDE, FAR, MARKED)] + [((out & THROUGH) != 0).sum(), ((out & END) != 0).sum()], I64)
    return out, summary


def frontier_field_host(occ, depth, origin, dims, obs):
    """svoslam_pool_frontier_field in numpy -> {"state" uint8, "frontier" uint8 [nz, ny, nx], "summary" int32 [6]}"""
    assert all(0 <= origin[a] and origin[a] + dims[a] <= (1 << depth) and dims[a] >= 0 for a in range(3))
    o, n = np.asarray(origin, I64), np.asarray(dims, I64)
    solid = occ[o[2]:o[2] + n[2], o[1]:o[1] + n[1], o[0]:o[0] + n[0]]
    obs = np.asarray(obs, np.uint8).reshape(solid.shape)
    t, e = (obs & THROUGH) != 0, (obs & END) != 0
    unknown = ~solid & ~t & ~e
    free = ~solid & t & ~e
    beside = np.zeros(solid.shape, bool)                                # a face neighbour IN THE REGION is unknown
    padded = np.zeros(tuple(v + 2 for v in solid.shape), bool)
    padded[1:-1, 1:-1, 1:-1] = unknown
    for axis in range(3):
        for step in (0, 2):
            cut = [slice(1, -1)] * 3
            cut[axis] = slice(step, step + solid.shape[axis])
            beside |= padded[tuple(cut)]
    state = np.full(solid.shape, UNKNOWN, np.uint8)
    state[free] = FREE
    state[free & beside] = FRONTIER
    state[solid] = OCCUPIED
    state[solid & t & ~e] = VACATED
    state[~solid & e] = UNMAPPED
    return {"state": state, "frontier": (state == FRONTIER).astype(np.uint8),
            "summary": np.bincount(state.reshape(-1), minlength=6).astype(np.int32)}


def explore_views_host(occ, depth, origin, dims, obs, cands, range_cells, k_max, min_gain=1):
    """explore_views: the frontier field, then the cover of the free cells selected by its frontier bytes"""
    field = frontier_field_host(occ, depth, origin, dims, obs)
    return field, cover_views_host(occ, depth, origin, dims, range_cells, 1, field["frontier"], cands, k_max, min_gain)


def slab_cells(a, b, cells):
    """bool [m]: which of cells[m, 3], other than a and b, have a closed cube that meets the closed segment between the centres of
    the cells a and b -- the definition of S(a, b) (supercover_brute's test, in Fractions) applied to the listed cells only"""
    D = [int(y - x) for x, y in zip(a, b)]
    out = np.zeros(len(cells), bool)
    for k, cell in enumerate(np.asarray(cells, I64).tolist()):
        c = [int(cell[i] - a[i]) for i in range(3)]
        if c == [0, 0, 0] or c == D:
            continue
        lo, hi = Fraction(0), Fraction(1)
        for i in range(3):
            if D[i] == 0:
                if c[i] != 0:                                           # the coordinate stays at the centre of a's layer
                    lo, hi = Fraction(1), Fraction(0)
                continue
            t0, t1 = Fraction(2 * c[i] - 1, 2 * D[i]), Fraction(2 * c[i] + 1, 2 * D[i])
            lo, hi = max(lo, min(t0, t1)), min(hi, max(t0, t1))
        out[k] = lo <= hi                                               # closed against closed: a touch counts
    return out


def same_bytes(got, want, what="obs"):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), want[tuple(bad[:5].T)].tolist())


# ---- the hand scene: every figure written out ---------------------------------------------------------------------------------------
HAND_DEPTH = 4                                                          # a root of 16 cells a side
HAND_CENTER, HAND_EDGE = (8.0, 8.0, 8.0), 8.0                           # plane k of every axis is the number k: cell centres are k + 1/2
ROOT_REGION = ((0, 0, 0), (16, 16, 16))
HAND_REGION = ((1, 4, 4), (9, 9, 9))
HOLE, FLOATER, SENSOR, BEYOND = (8, 8, 8), (5, 8, 8), (2, 8, 8), (15, 8, 8)
WALL = [(8, y, z) for y in range(16) for z in range(16) if (8, y, z) != HOLE]
HAND_ENDS = [(8, y, z) for y in range(4, 13) for z in range(4, 13) if (8, y, z) != HOLE] + [BEYOND]


def centres(cells, depth=HAND_DEPTH, center=HAND_CENTER, edge=HAND_EDGE):
    """float32 [m, 3]: the centres of cells[m, 3]"""
    return np.concatenate([midpoints(depth, center, edge, c, (1, 1, 1)) for c in np.asarray(cells, I64).reshape(-1, 3).tolist()] or
                          [np.zeros((0, 3), F)])


def pose_at(cell, depth=HAND_DEPTH, center=HAND_CENTER, edge=HAND_EDGE):
    """the identity moved to the centre of `cell`: float32 [16], column-major"""
    pose = IDENTITY.copy()
    pose[12:15] = centres([cell], depth, center, edge)[0]
    return pose


def frame_to(sensor, ends, depth=HAND_DEPTH, center=HAND_CENTER, edge=HAND_EDGE):
    """(points [m, 3] in the sensor frame, pose [16]) of the rays from the centre of `sensor` to the centres of `ends`"""
    pose = pose_at(sensor, depth, center, edge)
    return (centres(ends, depth, center, edge) - pose[12:15]).astype(F), pose


def hand_occ(floater=True):
    return occupancy(cells_pool(WALL + ([FLOATER] if floater else []), HAND_DEPTH), HAND_DEPTH)


def hand_obs(region=ROOT_REGION):
    points, pose = frame_to(SENSOR, HAND_ENDS)
    return observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *region, points, pose)


def test_the_hand_scene_over_the_whole_root():
    points, pose = frame_to(SENSOR, HAND_ENDS)
    cls, s, e = classify_rays(HAND_DEPTH, HAND_CENTER, HAND_EDGE, points, pose)
    assert (cls == MARKED).all() and (s == SENSOR).all() and e[0].tolist() == [list(c) for c in HAND_ENDS] and len(HAND_ENDS) == 81
    obs, summary = hand_obs()
    assert summary.tolist() == [0, 0, 0, 81, 197, 81]
    got = frontier_field_host(hand_occ(), HAND_DEPTH, *ROOT_REGION, obs)
    assert got["summary"].tolist() == [3643, 93, 103, 255, 1, 1]
    assert np.argwhere(got["state"] == VACATED)[:, ::-1].tolist() == [list(FLOATER)]        # rays passed through it, none ended in it
    assert np.argwhere(got["state"] == UNMAPPED)[:, ::-1].tolist() == [list(BEYOND)]        # a ray ended where the map has nothing
    assert np.array_equal(got["frontier"], got["state"] == FRONTIER) and got["frontier"].dtype == np.uint8
    bare = frontier_field_host(hand_occ(floater=False), HAND_DEPTH, *ROOT_REGION, obs)
    assert bare["summary"].tolist() == [3643, 94, 103, 255, 0, 1]


def test_the_hand_scene_over_a_region_the_border_makes_no_frontier():
    origin, dims = HAND_REGION
    obs, summary = hand_obs(HAND_REGION)
    whole, _ = hand_obs()
    same_bytes(obs, whole[4:13, 4:13, 1:10])                            # only cells of the region are stored, and all of those
    got = frontier_field_host(hand_occ(), HAND_DEPTH, origin, dims, obs)
    assert got["summary"].tolist() == [457, 93, 98, 80, 1, 0]
    full = frontier_field_host(hand_occ(), HAND_DEPTH, *ROOT_REGION, whole)["state"]
    outside = full.copy()
    outside[4:13, 4:13, 1:10] = UNKNOWN
    # the five frontier cells the region loses are the ray through the hole beyond the region's last x ...
    assert np.argwhere(outside == FRONTIER)[:, ::-1].tolist() == [[x, 8, 8] for x in range(10, 15)]
    same_bytes(got["state"], full[4:13, 4:13, 1:10], "state")           # ... and here no frontier cell depends on a neighbour outside


def test_a_neighbour_outside_the_region_makes_no_frontier():
    obs, _ = hand_obs()
    full = frontier_field_host(hand_occ(), HAND_DEPTH, *ROOT_REGION, obs)["state"]
    assert full[8, 8, 2:8].tolist() == [FRONTIER, FREE, FREE, VACATED, FREE, FREE] and full[8, 7, 2] == UNKNOWN
    origin, dims = (2, 8, 8), (6, 1, 1)                                 # the sensor's row alone: its unknown neighbours are cut off
    got = frontier_field_host(hand_occ(), HAND_DEPTH, origin, dims, obs[8:9, 8:9, 2:8])
    assert got["state"].reshape(-1).tolist() == [FREE, FREE, FREE, VACATED, FREE, FREE] and got["summary"].tolist() == [0, 5, 0, 0, 1, 0]
    origin, dims = (2, 7, 8), (6, 2, 1)                                 # with the row below it the sensor's cell is a frontier again
    got = frontier_field_host(hand_occ(), HAND_DEPTH, origin, dims, obs[8:9, 7:9, 2:8])
    assert got["state"][0, 1].tolist() == [FRONTIER, FREE, FREE, VACATED, FREE, FREE] and got["frontier"][0, 1, 0] == 1


def test_a_ray_whose_cells_all_lie_outside_the_region_still_counts():
    points, pose = frame_to(SENSOR, HAND_ENDS)
    obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, (12, 0, 0), (3, 3, 3), points, pose)
    assert summary.tolist() == [0, 0, 0, 81, 0, 0] and not obs.any()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, (1, 4, 4), dims, points, pose)
        assert obs.shape == (dims[2], dims[1], dims[0]) and summary.tolist() == [0, 0, 0, 81, 0, 0]
    obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *HAND_REGION, points[:0], pose)
    assert summary.tolist() == [0] * 6 and not obs.any() and obs.shape == (9, 9, 9)


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def random_frames(rng, n_frames, n, depth=HAND_DEPTH, center=HAND_CENTER, edge=HAND_EDGE):
    """frames whose sensors stand in different cells, rays to cells anywhere in the root"""
    n_side = 1 << depth
    points, poses = np.zeros((n_frames, n, 3), F), np.zeros((n_frames, 16), F)
    for f in range(n_frames):
        points[f], poses[f] = frame_to(rng.integers(0, n_side, 3), rng.integers(0, n_side, (n, 3)), depth, center, edge)
    return points, poses


def test_the_walk_marks_the_supercover_of_the_definition():
    rng = np.random.default_rng(3)
    for D in [(3, 0, 0), (0, -4, 0), (2, 2, 0), (3, -3, 3), (5, 3, 1), (-7, 2, 6), (1, 1, 1), (6, 4, 2), (0, 0, 0)] + rng.integers(-7, 8, (12, 3)).tolist():
        D = tuple(int(v) for v in D)
        a = (8, 8, 8)
        b = tuple(x + d for x, d in zip(a, D))
        points, pose = frame_to(a, [b])
        obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, points, pose)
        want = np.zeros((16, 16, 16), np.uint8)
        mark_cells(want, *ROOT_REGION, [b], END)
        if a != b:
            mark_cells(want, *ROOT_REGION, np.concatenate([[a], supercover_brute(D) + np.asarray(a)]), THROUGH)
        same_bytes(obs, want)
        cells = region_cells(*ROOT_REGION)
        inside = slab_cells(a, b, cells).reshape(16, 16, 16)            # the definition once more, cell by cell
        want_through = inside.copy()
        if a != b:
            want_through[a[2], a[1], a[0]] = True
        assert np.array_equal((obs & THROUGH) != 0, want_through), D
        assert summary.tolist() == [0, 0, 0, 1, int(want_through.sum()), 1]
    obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, *frame_to((8, 8, 8), [(8, 8, 8)]))
    assert summary.tolist() == [0, 0, 0, 1, 0, 1] and obs[8, 8, 8] == END   # s = e: the end alone


def test_marking_in_parts_with_accumulate_is_marking_at_once_in_any_order():
    rng = np.random.default_rng(11)
    points, poses = random_frames(rng, 3, 40)
    origin, dims = (2, 1, 3), (11, 13, 9)
    args = (HAND_DEPTH, HAND_CENTER, HAND_EDGE, origin, dims)
    whole, summary = observe_rays_host(*args, points, poses)
    assert summary[3] == 120 and summary[4] > 100 and summary[5] > 20
    first, _ = observe_rays_host(*args, points[:1], poses[:1])
    both, part = observe_rays_host(*args, points[1:], poses[1:], accumulate=True, obs=first)
    same_bytes(both, whole)
    assert part.tolist() == [0, 0, 0, 80] + summary[4:].tolist()        # the cell counts are those of d_obs after the call
    order = rng.permutation(3)
    lanes = rng.permutation(40)
    mixed, again = observe_rays_host(*args, points[order][:, lanes], poses[order])
    same_bytes(mixed, whole)
    assert again.tolist() == summary.tolist()
    twice, _ = observe_rays_host(*args, np.concatenate([points, points], 1), poses)   # a set: a ray marked twice marks once
    same_bytes(twice, whole)


def test_bits_2_to_7_survive_accumulate_and_are_cleared_without_it():
    rng = np.random.default_rng(12)
    points, poses = random_frames(rng, 1, 25)
    args = (HAND_DEPTH, HAND_CENTER, HAND_EDGE, (0, 0, 0), (16, 16, 16))
    before = rng.integers(0, 256, (16, 16, 16)).astype(np.uint8)
    marks, _ = observe_rays_host(*args, points, poses)
    kept, summary = observe_rays_host(*args, points, poses, accumulate=True, obs=before)
    assert np.array_equal(kept & 0xFC, before & 0xFC) and np.array_equal(kept & 3, (before | marks) & 3)
    assert summary[4] == ((kept & THROUGH) != 0).sum() and summary[5] == ((kept & END) != 0).sum()
    fresh, _ = observe_rays_host(*args, points, poses, accumulate=False, obs=before)
    same_bytes(fresh, marks)
    assert not (fresh & 0xFC).any()
    none, counts = observe_rays_host(*args, points[:, :0], poses, accumulate=True, obs=before)   # no rays: left unchanged
    same_bytes(none, before)
    assert counts[:4].tolist() == [0, 0, 0, 0] and counts[4] == ((before & THROUGH) != 0).sum()


def seen_ends(occ, depth, sensor, radius):
    """the occupied cells the visibility field says `sensor` sees within `radius`, in region order"""
    n_side = 1 << depth
    mask = visibility_field_walk(occ, depth, (0, 0, 0), (n_side,) * 3, radius, [sensor])["count"] > 0
    return region_cells((0, 0, 0), (n_side,) * 3)[(mask & occ).reshape(-1)]


def test_what_the_visibility_field_sees_is_never_vacated_and_a_hidden_end_is_given_away():
    occ = hand_occ()
    ends = seen_ends(occ, HAND_DEPTH, SENSOR, 12)
    assert ends.shape[0] > 60 and list(FLOATER) in ends.tolist()
    obs, summary = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, *frame_to(SENSOR, ends))
    got = frontier_field_host(occ, HAND_DEPTH, *ROOT_REGION, obs)
    assert got["summary"][VACATED] == 0 and got["summary"][UNMAPPED] == 0 and got["summary"][OCCUPIED] == occ.sum()
    assert got["summary"][FRONTIER] > 0 and summary[5] == ends.shape[0]
    hidden = [(12, 8, 8), (9, 3, 12), (8, 0, 0)]                        # behind the floater and the hole, behind the wall, a wall cell the sensor cannot see
    seen = visibility_field_walk(occ, HAND_DEPTH, *ROOT_REGION, 16, [SENSOR])["count"]
    for end in hidden:
        assert seen[end[2], end[1], end[0]] == 0
        obs, _ = observe_rays_host(HAND_DEPTH, HAND_CENTER, HAND_EDGE, *ROOT_REGION, *frame_to(SENSOR, [end]))
        assert (((obs & THROUGH) != 0) & occ).any(), end               # the ray puts THROUGH on at least one occupied cell


# ---- classification edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,center,edge", [(4, HAND_CENTER, HAND_EDGE), (6, ROOT_CENTER, ROOT_EDGE), (12, (0.3, -7.1, 2.0), 3.3)])
def test_points_on_the_root_planes_and_one_ulp_beside_them(depth, center, edge):
    n_side = 1 << depth
    h = F(edge) / F(n_side)
    pose = pose_at((2, 2, 2), depth, center, edge)
    for a in range(3):
        for k, on, below, above in ((0, 0, -1, 0), (1, 1, 0, 1), (n_side - 1, n_side - 1, n_side - 2, n_side - 1), (n_side, n_side - 1, n_side - 1, -1)):
            pl = plane(center[a], k, n_side, h)
            for value, cell in ((pl, on), (np.nextafter(pl, F(-np.inf)), below), (np.nextafter(pl, F(np.inf)), above)):
                w = centres([(2, 2, 2)], depth, center, edge)[0]
                w[a] = value
                at_w = IDENTITY.copy()                                  # the sensor at the value itself, the point (0, 0, 0): o = w
                at_w[12:15] = w
                cls, s, e = classify_rays(depth, center, edge, [[0, 0, 0]], at_w)
                assert np.array_equal(move(at_w, [[0, 0, 0]])[0, 0].view(np.uint32), w.view(np.uint32))
                if cell < 0:
                    assert cls[0, 0] == OUTSIDE
                else:
                    assert cls[0, 0] == MARKED and s[0, 0, a] == e[0, 0, a] == cell and s[0, 0, (a + 1) % 3] == 2
                # and as the end alone, the sensor standing in cell (2, 2, 2)
                cls, s, e = classify_rays(depth, center, edge, [(w - pose[12:15]).astype(F)], pose)
                moved = move(pose, [(w - pose[12:15]).astype(F)])[0, 0]
                if moved[a] == value:                                   # the difference and the sum gave the value back
                    assert (cls[0, 0] == OUTSIDE) == (cell < 0) and (cell < 0 or e[0, 0, a] == cell)


def test_nan_inf_outside_far_and_a_ray_within_one_cell():
    depth, center, edge = HAND_DEPTH, HAND_CENTER, HAND_EDGE
    pose = pose_at(SENSOR)
    points = np.array([[1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0], [20, 0, 0], [0.25, 0.25, -0.25]], F)
    cls, s, e = classify_rays(depth, center, edge, points, pose)
    assert cls[0].tolist() == [MARKED, VOID, VOID, VOID, OUTSIDE, OUTSIDE, MARKED]   # 3e38 is finite: the ray is not void, its end lies outside
    assert s[0, 6].tolist() == e[0, 6].tolist() == list(SENSOR)
    poses = np.tile(pose, (6, 1))
    poses[1, 12] = F(np.nan)                                            # o is not finite
    poses[2, 5] = F(np.nan)                                             # w is not finite
    poses[3, 13] = F(np.inf)
    poses[4, 12] = F(-0.5)                                              # o outside the root, w = p + o inside for p = (1, 0, 0)
    poses[5, [3, 7, 11, 15]] = F(np.nan)                                # the bottom row is never read
    cls, s, e = classify_rays(depth, center, edge, np.tile(points, (6, 1, 1)), poses)
    for f in (1, 2, 3, 4):
        assert cls[f].tolist() == [OUTSIDE, VOID, VOID, VOID, OUTSIDE, OUTSIDE, OUTSIDE], f
    assert in_root(depth, center, edge, move(poses[4], points[:1])[0])[0]
    assert np.array_equal(cls[5], cls[0])
    obs, summary = observe_rays_host(depth, center, edge, *ROOT_REGION, np.tile(points, (6, 1, 1)), poses)
    assert summary[:4].tolist() == [18, 20, 0, 4] and summary[:4].sum() == 42
    # FAR at |D|^2 = R^2 and at R^2 + 1: D = (3, 4, 0) has |D|^2 = 25, D = (3, 4, 1) has 26
    ends = [(5, 12, 8), (5, 12, 9)]
    for radius, want in ((5, [MARKED, FAR]), (6, [MARKED, MARKED]), (4, [FAR, FAR]), (0, [MARKED, MARKED]), (1 << 16, [MARKED, MARKED])):
        cls, s, e = classify_rays(depth, center, edge, *frame_to(SENSOR, ends), radius)
        assert cls[0].tolist() == want, radius
    obs, summary = observe_rays_host(depth, center, edge, *ROOT_REGION, *frame_to(SENSOR, ends), 5)
    assert summary.tolist() == [0, 0, 1, 1, len(walk_cells((3, 4, 0))) + 1, 1]   # the far ray is skipped whole, not truncated


# ---- a pool fused by the oracle ------------------------------------------------------------------------------------------------
FUSED_SENSOR = (20, 9, 3)                                               # a free cell beside the cloud, inside low_corner
FUSED_RANGE = 24
# the regions that cannot hold all of UNKNOWN, FREE, FRONTIER and OCCUPIED, with the reason
NOT_ALL_STATES = {"high_corner": "no occupied cell in the region, and no ray of the frame reaches it",
                  "offset_37": "no occupied cell in the region, and no ray of the frame reaches it",
                  "one_cell": "one cell has one state"}
FUSED_CASES = sorted(fused_regions(DEPTH))


@pytest.fixture(scope="module")
def fused_occ(fused):
    return occupancy(fused[0], DEPTH)


def fused_frame(occ):
    """(points [1, m, 3], poses [1, 16]): a synthetic frame of the fused pool -- the sensor in FUSED_SENSOR, turned a quarter about z,
    one ray to every occupied cell it sees within FUSED_RANGE cells, and three voids as a depth image has them"""
    ends = seen_ends(occ, DEPTH, FUSED_SENSOR, FUSED_RANGE)
    world, pose = frame_to(FUSED_SENSOR, ends, DEPTH, ROOT_CENTER, ROOT_EDGE)
    pose[[0, 1, 4, 5]] = (0, 1, -1, 0)                                  # sensor x is world y, sensor y is world -x
    points = np.stack([world[:, 1], -world[:, 0], world[:, 2]], 1).astype(F)
    points = np.concatenate([points, [[np.inf, 0, 0], [0, np.nan, 0], [np.inf] * 3]]).astype(F)
    return points[None], pose[None], ends


def test_the_fused_frame_ends_where_it_was_aimed(fused_occ):
    assert not fused_occ[FUSED_SENSOR[2], FUSED_SENSOR[1], FUSED_SENSOR[0]]
    points, poses, ends = fused_frame(fused_occ)
    cls, s, e = classify_rays(DEPTH, ROOT_CENTER, ROOT_EDGE, points, poses, FUSED_RANGE)
    assert ends.shape[0] >= 50 and cls[0, :-3].tolist() == [MARKED] * ends.shape[0] and cls[0, -3:].tolist() == [VOID] * 3
    assert np.array_equal(e[0, :-3], ends) and (s[0] == FUSED_SENSOR).all()


@pytest.mark.parametrize("region", FUSED_CASES)
def test_fused_pool_cases_hold_every_state_or_say_why_not(fused_occ, region):
    origin, dims = fused_regions(DEPTH)[region]
    points, poses, ends = fused_frame(fused_occ)
    obs, summary = observe_rays_host(DEPTH, ROOT_CENTER, ROOT_EDGE, origin, dims, points, poses, FUSED_RANGE)
    got = frontier_field_host(fused_occ, DEPTH, origin, dims, obs)
    assert summary[:4].tolist() == [3, 0, 0, ends.shape[0]] and got["summary"].sum() == dims[0] * dims[1] * dims[2]
    assert got["summary"][VACATED] == 0                                # the ends are what the sensor sees
    if region in NOT_ALL_STATES:
        assert not all(got["summary"][k] > 0 for k in (UNKNOWN, FREE, FRONTIER, OCCUPIED))
        if region != "one_cell":
            lo, hi = np.asarray(origin), np.asarray(origin) + np.asarray(dims)
            assert not fused_occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any() and not obs.any()
    else:
        assert all(got["summary"][k] > 0 for k in (UNKNOWN, FREE, FRONTIER, OCCUPIED)), got["summary"].tolist()


def test_the_cases_without_every_state_are_the_ones_written_out(fused_occ):
    points, poses, _ = fused_frame(fused_occ)
    short = set()
    for region, (origin, dims) in fused_regions(DEPTH).items():
        obs, _ = observe_rays_host(DEPTH, ROOT_CENTER, ROOT_EDGE, origin, dims, points, poses, FUSED_RANGE)
        counts = frontier_field_host(fused_occ, DEPTH, origin, dims, obs)["summary"]
        if not all(counts[k] > 0 for k in (UNKNOWN, FREE, FRONTIER, OCCUPIED)):
            short.add(region)
    assert short == set(NOT_ALL_STATES)


# ---- explore_views -------------------------------------------------------------------------------------------------------------------
def test_explore_views_is_the_cover_of_the_frontier_cells():
    occ = hand_occ()
    obs, _ = hand_obs()
    cands = np.array([(3, 8, 8), (4, 3, 8), (4, 13, 8), (12, 8, 8), (4, 8, 13), (-1, 0, 0), (3, 8, 8)], np.int32)
    field, cover = explore_views_host(occ, HAND_DEPTH, *ROOT_REGION, obs, cands, 6, 4)
    want = cover_views_host(occ, HAND_DEPTH, *ROOT_REGION, 6, 1, field["frontier"], cands, 4)
    for name in ("seen", "chosen", "gain", "round", "summary"):
        assert np.array_equal(cover[name], want[name])
    assert cover["summary"][0] == field["summary"][FRONTIER] == 103 and cover["summary"][1] >= 2
    assert ((cover["round"] != -1) == (field["state"] == FRONTIER)).all()      # the targets are the frontier cells, all of them free
    assert cover["seen"][5] == 0 and cover["seen"][6] == cover["seen"][0] > 0   # outside the root; a duplicate


# ---- the header and the library ------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_calls_and_keeps_its_pins():
    pkg = load_pkg()
    raw = open(pkg.HEADER_PATH).read()
    header = " ".join(raw.split())
    assert ("int svoslam_field_observe_rays(svoslam_workspace *ws, uint8_t *d_obs, int32_t max_depth, const float center[3], float edge_length, "
            "const int32_t origin_cell[3], const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, int32_t n_frames, "
            "int32_t range_cells, int32_t accumulate, int64_t *d_summary /* 6, may be NULL */, void *stream);") in header
    assert ("int svoslam_pool_frontier_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3], "
            "const int32_t dims[3], const uint8_t *d_obs, uint8_t *d_state /* may be NULL */, uint8_t *d_frontier /* may be NULL */, "
            "int32_t *d_summary /* 6, may be NULL */, void *stream);") in header
    assert "int svoslam_workspace_observe_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);" in header
    assert "int svoslam_workspace_frontier_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);" in header
    for line in ("#define SVOSLAM_OBS_THROUGH 1", "#define SVOSLAM_OBS_END     2", "#define SVOSLAM_STATE_UNKNOWN  0", "#define SVOSLAM_STATE_FREE     1",
                 "#define SVOSLAM_STATE_FRONTIER 2", "#define SVOSLAM_STATE_OCCUPIED 3", "#define SVOSLAM_STATE_VACATED  4", "#define SVOSLAM_STATE_UNMAPPED 5",
                 "#define SVOSLAM_ABI_VERSION 1", "#define SVOSLAM_STAGE_QUERY 12", "#define SVOSLAM_STAGE_COUNT 13"):
        assert line in raw, line
    between = raw[raw.index("#define SVOSLAM_STAGE_QUERY 12"):raw.index("#define SVOSLAM_STAGE_COUNT 13")]
    assert "svoslam_field_observe_rays" in between and "svoslam_pool_frontier_field" in between


def test_library_exports_the_observe_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_field_observe_rays", "svoslam_pool_frontier_field", "svoslam_workspace_observe_buffers", "svoslam_workspace_frontier_buffers"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert len(pkg.SIGNATURES["svoslam_field_observe_rays"][1]) == 15 and len(pkg.SIGNATURES["svoslam_pool_frontier_field"][1]) == 10
    for name in ("observe_rays", "frontier_field", "explore_views"):
        assert hasattr(pkg, name)
    assert hasattr(pkg.Workspace, "observe_buffers") and hasattr(pkg.Workspace, "frontier_buffers")
    assert (pkg.OBS_THROUGH, pkg.OBS_END) == (THROUGH, END)
    assert (pkg.STATE_UNKNOWN, pkg.STATE_FREE, pkg.STATE_FRONTIER, pkg.STATE_OCCUPIED, pkg.STATE_VACATED, pkg.STATE_UNMAPPED) == tuple(range(6))
    assert pkg.STAGE_QUERY == 12 and len(pkg.STAGE_NAMES) == 13
    tools = os.path.join(os.path.dirname(pkg.HEADER_PATH), "..", "tools")
    assert os.path.exists(os.path.join(tools, "map_frontier.py")) and os.path.exists(os.path.join(tools, "map_frontier_bench.py"))
