"""svoslam_field_grow_boxes and svoslam_field_path_corridors on the device: every value equals the host restatements of the
specification (tests/test_corridor_cpu.py: grow_boxes_ref, every cell of every slab, and path_corridors_ref) -- on the hand-built
fields, on fields the device's own distance_field produced and on paths its own trace_paths produced, each first proven equal to
its own restatement.  Exact integers, no tolerance anywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_corridor_cpu import (EXTENTS, GROW_CASES, PATH_CASES, RADII, check_chain, grow_boxes_ref, path_corridors_ref, world_corridors)
from test_field_cpu import distance_field_separable
from test_gpu_field import case_region, same_field
from test_gpu_paths import stored_cells, world_on_the_device
from test_gpu_query import fused_pool
from test_paths_cpu import flat, world_path
from test_plan_cpu import ramp, world
from test_surface_cpu import CENTER, EDGE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -6


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """(pool, its words, the fused points, workspace) at depth 6: fused on the device, twice, shared by the tests below and left
    unchanged"""
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 6, 15000, 41)
    return pool, pool.words(), pts, ws


def same_boxes(pkg, field, origin, r, E, seeds):
    """the device's box and layers of every seed equal grow_boxes_ref's"""
    seeds = np.asarray(seeds, np.int64).reshape(-1, 6)
    boxes, layers = pkg.corridors.grow_boxes(field, origin, field.shape[::-1], r, E, seeds.astype(np.int32))
    assert boxes.dtype == np.int32 and layers.dtype == np.int32 and boxes.shape == (seeds.shape[0], 6) and layers.shape == (seeds.shape[0],)
    for k, s in enumerate(seeds.tolist()):
        want = grow_boxes_ref(field, origin, r, E, s)
        assert (tuple(boxes[k].tolist()), int(layers[k])) == want, (k, s, boxes[k].tolist(), int(layers[k]), want)
    return boxes, layers


def same_corridors(pkg, field, origin, r, E, paths, lengths, want=None):
    """the device's boxes, anchors, counts and gaps of every path equal path_corridors_ref's (or `want`, its results computed
    before), and nothing behind a path's boxes was written"""
    boxes, anchors, counts, gaps = pkg.corridors.path_corridors(field, origin, field.shape[::-1], r, E, paths, lengths)
    n = paths.shape[0]
    assert all(a.dtype == np.int32 for a in (boxes, anchors, counts, gaps)) and counts.shape == (n,) and gaps.shape == (n,)
    room = int(counts.max()) if n else 0
    assert boxes.shape == (n, room, 6) and anchors.shape == (n, room)
    for k in range(n):
        w_boxes, w_anchors, w_gaps = want[k] if want is not None else path_corridors_ref(field, origin, r, E, stored_cells(paths, lengths, k))
        assert int(counts[k]) == len(w_boxes) and int(gaps[k]) == w_gaps, (k, r, E, int(counts[k]), len(w_boxes), int(gaps[k]), w_gaps)
        assert anchors[k, :len(w_boxes)].tolist() == w_anchors, (k, r, E)
        assert [tuple(b) for b in boxes[k, :len(w_boxes)].tolist()] == w_boxes, (k, r, E)
        assert (boxes[k, len(w_boxes):] == -1).all() and (anchors[k, len(w_boxes):] == -1).all()
    return boxes, anchors, counts, gaps


# ---- the hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GROW_CASES))
def test_growing_by_hand(env, name):
    pkg, torch = env
    field, origin, r, E, seed, box, layers = GROW_CASES[name]
    got, added = same_boxes(pkg, field, origin, r, E, [seed])
    assert tuple(got[0].tolist()) == tuple(box) and added.tolist() == [layers]


def test_all_seeds_of_one_field_in_one_call(env):
    pkg, torch = env
    same = [c for c in GROW_CASES.values() if c[0] is GROW_CASES["invalid_lo_above_hi"][0]]
    assert len(same) >= 8
    boxes, layers = same_boxes(pkg, same[0][0], same[0][1], same[0][2], same[0][3], [c[4] for c in same])
    assert [tuple(b) for b in boxes.tolist()] == [tuple(c[5]) for c in same] and layers.tolist() == [c[6] for c in same]
    assert (layers == -1).sum() >= 7 and (layers >= 0).any()


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_corridors_by_hand(env, name):
    pkg, torch = env
    field, origin, r, E, cells, boxes, anchors, gaps = PATH_CASES[name]
    paths = np.asarray(cells, np.int64).astype(np.int32).reshape(1, -1, 3)
    got = same_corridors(pkg, field, origin, r, E, paths, np.array([len(cells)], np.int32))
    assert [tuple(b) for b in got[0][0].tolist()] == boxes and got[1][0].tolist() == anchors and got[2].tolist() == [len(boxes)]
    assert got[3].tolist() == [gaps]


# ---- grow_boxes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 5, 257])
def test_seed_counts(env, count):
    """a partial block of four wavefronts, a whole one, one more, and many blocks with a ragged tail: seeds all over a world, some
    of them not valid"""
    pkg, torch = env
    w = world("two_routes")
    o, dims = np.asarray(w["origin"]), np.asarray(w["dims"])
    rng = np.random.default_rng(count)
    lo = rng.integers(-1, dims + 1, (count, 3)) + o
    hi = lo + rng.integers(-1, 3, (count, 3))
    boxes, layers = same_boxes(pkg, w["field"], w["origin"], 1, 5, np.concatenate([lo, hi], 1))
    if count == 257:
        assert (layers == -1).sum() > 20 and (layers > 0).sum() > 20 and len(set(layers.tolist())) > 5


SLABS = {63: (9, 7), 64: (8, 8), 65: (13, 5), 129: (43, 3)}              # cells -> the slab's extent on its two axes, the lower axis first


@pytest.mark.parametrize("cells", sorted(SLABS))
@pytest.mark.parametrize("facing", [0, 1, 2])
def test_one_blocked_cell_in_a_slab(env, cells, facing):
    """the seed is a plate one cell thick against the low border of a region two cells thick along `facing`: the only slab inside
    the region is the plate's copy beside it, `cells` cells.  One cell of it at r^2 at the slab index 0, 63, 64 or the last (x
    fastest, as the lanes stride over it) stops the layer; with none it grows"""
    pkg, torch = env
    u, v = SLABS[cells]
    others = [a for a in range(3) if a != facing]
    dims = [0, 0, 0]
    dims[facing], dims[others[0]], dims[others[1]] = 2, u, v
    hi = [n - 1 for n in dims]
    hi[facing] = 0
    seed = [0, 0, 0] + hi
    blocked_at = sorted({0, 63, 64, cells - 1} & set(range(cells)))
    assert len(blocked_at) == {63: 2, 64: 2, 65: 3, 129: 4}[cells]       # 63 cells: 0 and the last; 64: 0 and 63, the last
    for index in [None] + blocked_at:
        at = [0, 0, 0]
        if index is not None:
            at[facing], at[others[0]], at[others[1]] = 1, index % u, index // u
        field = flat(dims, 10, {} if index is None else {tuple(at): 9})
        boxes, layers = same_boxes(pkg, field, (3, -5, 7), 3, 1, [[s + o for s, o in zip(seed, (3, -5, 7) * 2)]])
        assert layers.tolist() == [1 if index is None else 0], (index, layers)


@pytest.mark.parametrize("E", [0, 1, 3])
def test_every_cell_of_a_small_region(env, fused, E):
    pkg, torch = env
    pool, words, pts, ws = fused
    origin, dims = case_region(words, 6, (6, 5, 4), "pt", 3)
    field = pkg.distance_field(ws, pool, 6, origin, dims, 3)
    same_field(field, distance_field_separable(words, 6, origin, dims, 3))
    assert (field == 0).sum() > 0 and (field > 0).sum() > 10            # decided on the restatement's equal
    cells = [(origin[0] + x, origin[1] + y, origin[2] + z) for z in range(dims[2]) for y in range(dims[1]) for x in range(dims[0])]
    for r in (0, 1):
        boxes, layers = same_boxes(pkg, field, origin, r, E, [c + c for c in cells])
        assert (layers == -1).any() and (layers >= 0).any()
        assert E == 0 or len(set(layers.tolist())) > 2


# ---- path_corridors --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(env):
    """name -> (the device's comfort field, paths, lengths) of the two worlds: test_gpu_paths.world_on_the_device, once"""
    pkg, torch = env
    return {name: world_on_the_device(pkg, name) for name in ("two_routes", "serpentine")}


@pytest.mark.parametrize("name", ["two_routes", "serpentine"])
def test_the_worlds(env, worlds, name):
    """trace_paths' own output in, at every (r, E): the weighted and the reach path in one call"""
    pkg, torch = env
    w = world(name)
    field, paths, lengths = worlds[name]
    cells = [world_path(name, "weighted"), world_path(name, "reach")]
    for r in RADII:
        for E in EXTENTS:
            want = [world_corridors(name, which, r, E) for which in ("weighted", "reach")]
            boxes, anchors, counts, gaps = same_corridors(pkg, field, w["origin"], r, E, paths, lengths, want)
            for k in range(2):
                if gaps[k] == 0:
                    check_chain(field, w["origin"], r, cells[k], [tuple(b) for b in boxes[k, :counts[k]].tolist()], anchors[k, :counts[k]].tolist())
            if name == "two_routes" and r == 1:
                assert int(counts[0]) == {0: 216, 1: 106, 4: 43, 64: 5}[E] and gaps.tolist() == [0, 0]
            if name == "serpentine" and r == 1:
                assert (boxes[1, :counts[1], 3] < boxes[1, :counts[1], 0]).sum() == 835 and gaps[1] >= 835
            if r <= w["clearance"]:
                assert gaps.tolist() == [0, 0]


@pytest.fixture(scope="module")
def many_paths(env, fused):
    """257 traced paths on a region of the depth-6 pool, some of length 0, some lengths negated as a stopped walk's are, some cut by
    max_cells: (field, origin, dims, clearance, extent, paths, lengths, the restatement's result per path)"""
    pkg, torch = env
    pool, words, pts, ws = fused
    r, R, E = 1, 3, 2
    origin, dims = case_region(words, 6, (40, 24, 8), "pt", R)
    field = pkg.distance_field(ws, pool, 6, origin, dims, R)
    same_field(field, distance_field_separable(words, 6, origin, dims, R))
    free = np.argwhere((field < 0) | (field > r * r))[:, ::-1] + np.asarray(origin)
    rng = np.random.default_rng(9)
    cost = pkg.cost_field(ws, pool, 6, origin, dims, r, R, [6, 2], [free[rng.integers(free.shape[0])].tolist()])
    reached, blocked = np.argwhere(cost >= 0)[:, ::-1] + np.asarray(origin), np.argwhere(cost == -2)[:, ::-1] + np.asarray(origin)
    assert reached.shape[0] >= 237 and blocked.shape[0] >= 10
    starts = np.concatenate([reached[rng.choice(reached.shape[0], 237, replace=False)], blocked[:10], np.array([[origin[0] + 40, origin[1], origin[2]]] * 10)])
    starts = starts[rng.permutation(257)]
    lengths = pkg.trace_paths(cost, origin, dims, starts, 0)[1]
    paths, lengths = pkg.trace_paths(cost, origin, dims, starts, int(np.sort(lengths)[200]))      # the longest fifth is cut by max_cells
    lengths = lengths.copy()
    lengths[::5] = -lengths[::5]
    assert (lengths == 0).sum() == 20 and (lengths < 0).sum() > 30 and (np.abs(lengths) > paths.shape[1]).sum() > 20
    want = [path_corridors_ref(field, origin, r, E, stored_cells(paths, lengths, k)) for k in range(257)]
    return field, origin, dims, r, E, paths, lengths, want


def test_many_paths_in_one_call_and_the_argument_forms(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, E, paths, lengths, want = many_paths
    boxes, anchors, counts, gaps = same_corridors(pkg, field, origin, r, E, paths, lengths, want)
    assert sum(len(w[0]) == 0 for w in want) == 20 and sum(len(w[0]) > 3 for w in want) > 50 and gaps.tolist() == [0] * 257
    for k in range(257):
        if want[k][0]:
            check_chain(field, origin, r, stored_cells(paths, lengths, k), want[k][0], want[k][1])
    for k in (3, 255):                                                  # one path in a call
        one = pkg.corridors.path_corridors(field, origin, dims, r, E, paths[k:k + 1], lengths[k:k + 1])
        assert one[2].tolist() == [len(want[k][0])] and [tuple(b) for b in one[0][0].tolist()] == want[k][0] and one[1][0].tolist() == want[k][1]
    # a second identical call gives identical bytes
    again = pkg.corridors.path_corridors(field, origin, dims, r, E, paths, lengths)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (boxes, anchors, counts, gaps)))
    # tensors in, tensors out
    t = [torch.from_numpy(a).cuda() for a in (field, paths, lengths)]
    got = pkg.corridors.path_corridors(t[0], origin, dims, r, E, t[1], t[2], as_tensor=True)
    assert all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.int32 for a in got)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, (boxes, anchors, counts, gaps)))
    seeds = np.concatenate([paths[:, 0], paths[:, 0]], 1)               # every start cell as a seed; the -1 rows of length 0 as they are
    b_arr, l_arr = pkg.corridors.grow_boxes(field, origin, dims, r, E, seeds)
    b_t, l_t = pkg.corridors.grow_boxes(t[0], origin, dims, r, E, torch.from_numpy(seeds).cuda(), as_tensor=True)
    assert isinstance(b_t, torch.Tensor) and b_t.is_cuda and l_t.dtype == torch.int32
    assert np.array_equal(b_t.cpu().numpy(), b_arr) and np.array_equal(l_t.cpu().numpy(), l_arr)
    assert pkg.corridors.grow_boxes(field, origin, dims, r, E, seeds)[0].tobytes() == b_arr.tobytes()
    for k in range(0, 257, 8):
        assert (tuple(b_arr[k].tolist()), int(l_arr[k])) == grow_boxes_ref(field, origin, r, E, seeds[k].tolist())
    with pytest.raises(ValueError):
        pkg.corridors.path_corridors(field, origin, dims, r, E, paths[:, :, :2], lengths)
    with pytest.raises(ValueError):
        pkg.corridors.path_corridors(field, origin, dims, r, E, t[1].to(torch.int64), t[2])
    with pytest.raises(ValueError):
        pkg.corridors.grow_boxes(field, origin, (dims[0], dims[1], dims[2] - 1), r, E, seeds)
    with pytest.raises(ValueError):
        pkg.corridors.grow_boxes(field, origin, dims, r, E, torch.from_numpy(seeds))


def test_max_boxes_and_the_optional_pointers(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, E, paths, lengths, want = many_paths
    L = pkg.corridors.lib()
    t_field, t_paths, t_lengths = (torch.from_numpy(a).cuda() for a in (field, paths, lengths))
    o3, n3 = (C.c_int32 * 3)(*origin), (C.c_int32 * 3)(*dims)
    counts = torch.full((257,), -77, dtype=torch.int32, device="cuda")
    gaps = torch.full((257,), -77, dtype=torch.int32, device="cuda")

    def call(room, boxes, anchors, d_gaps):
        return L.svoslam_field_path_corridors(pkg._ptr(t_field), o3, n3, r, E, pkg._ptr(t_paths), pkg._ptr(t_lengths), 257, paths.shape[1], room,
                                              pkg._ptr(boxes), pkg._ptr(anchors), pkg._ptr(counts), pkg._ptr(d_gaps), pkg._stream())
    # 0 with NULL buffers and a NULL d_gaps: the counts alone
    assert call(0, None, None, None) == 0
    assert counts.tolist() == [len(w[0]) for w in want] and (gaps == -77).all()
    assert call(0, None, None, gaps) == 0 and gaps.tolist() == [w[2] for w in want]
    # shorter than the counts: the first three, the whole count, the rest of a sentinel-filled buffer untouched
    boxes = torch.full((257, 5, 6), -77, dtype=torch.int32, device="cuda")
    anchors = torch.full((257, 5), -77, dtype=torch.int32, device="cuda")
    counts.fill_(-77)
    assert call(3, boxes, anchors, None) == 0
    assert counts.tolist() == [len(w[0]) for w in want] and sum(len(w[0]) > 3 for w in want) > 20
    flat_boxes, flat_anchors = boxes.cpu().numpy().reshape(-1, 6), anchors.cpu().numpy().reshape(-1)    # rows of 3 in buffers of 257 * 5
    for k in range(257):
        kept = min(len(want[k][0]), 3)
        assert [tuple(b) for b in flat_boxes[3 * k:3 * k + kept].tolist()] == want[k][0][:kept] and (flat_boxes[3 * k + kept:3 * k + 3] == -77).all(), k
        assert flat_anchors[3 * k:3 * k + kept].tolist() == want[k][1][:kept] and (flat_anchors[3 * k + kept:3 * k + 3] == -77).all(), k
    assert (flat_boxes[257 * 3:] == -77).all() and (flat_anchors[257 * 3:] == -77).all()
    short = pkg.corridors.path_corridors(field, origin, dims, r, E, paths, lengths, max_boxes=2)
    assert short[0].shape == (257, 2, 6) and short[1].shape == (257, 2) and short[2].tolist() == [len(w[0]) for w in want]
    assert all(short[1][k, :min(len(want[k][1]), 2)].tolist() == want[k][1][:2] for k in range(257))
    # cut by max_cells: the same paths with room for seven cells
    cut = np.ascontiguousarray(paths[:, :7])
    same_corridors(pkg, field, origin, r, E, cut, lengths)


# ---- around the calls ------------------------------------------------------------------------------------------------------------
def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    L = pkg.corridors.lib()
    field = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    seeds = torch.tensor([[1, 1, 1, 2, 2, 2], [3, 3, 3, 4, 3, 3]], dtype=torch.int32, device="cuda")
    boxes = torch.full((2, 6), -77, dtype=torch.int32, device="cuda")
    layers = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    paths = torch.tensor([[[0, 0, 0], [1, 0, 0], [1, 1, 0], [2, 1, 0]], [[3, 3, 3], [3, 3, 2], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32, device="cuda")
    lengths = torch.tensor([4, 2], dtype=torch.int32, device="cuda")
    chain = torch.full((2, 4, 6), -77, dtype=torch.int32, device="cuda")
    anchors = torch.full((2, 4), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    gaps = torch.full((2,), -77, dtype=torch.int32, device="cuda")
    null = C.c_void_p(0)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def grow(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), r=1, E=1, s=pkg._ptr(seeds), n=2, out=pkg._ptr(boxes), added=pkg._ptr(layers)):
        return L.svoslam_field_grow_boxes(f, i3(origin), i3(dims), r, E, s, n, out, added, pkg._stream())

    def chains(f=pkg._ptr(field), origin=(0, 0, 0), dims=(4, 4, 4), r=1, E=1, p=pkg._ptr(paths), ln=pkg._ptr(lengths), n=2, cap=4, room=4,
               b=pkg._ptr(chain), a=pkg._ptr(anchors), out=pkg._ptr(counts), g=pkg._ptr(gaps)):
        return L.svoslam_field_path_corridors(f, i3(origin), i3(dims), r, E, p, ln, n, cap, room, b, a, out, g, pkg._stream())
    # every error first: nothing is written
    for call in (grow, chains):
        assert call(origin=None) == INVALID and call(dims=None) == INVALID and call(dims=(-1, 4, 4)) == INVALID and call(dims=(4, 4, -1)) == INVALID
        assert call(n=-1) == INVALID and call(f=null) == INVALID and call(r=-1) == INVALID and call(r=4097) == INVALID and call(r=-1, n=0) == INVALID
        assert call(E=-1) == INVALID and call(E=65537) == INVALID and call(E=65537, n=0) == INVALID
        assert call(dims=(65536, 65536, 1)) == LIMIT and call(dims=(2048, 1024, 1024)) == LIMIT and call(dims=(65537, 1, 1)) == LIMIT
        assert call(dims=(1, 65537, 1)) == LIMIT and call(dims=(1, 1, 65537)) == LIMIT and call(dims=(65536, 65536, 65536)) == LIMIT
    assert grow(s=null) == INVALID and grow(out=null) == INVALID and grow(added=null) == INVALID
    assert chains(cap=-1) == INVALID and chains(room=-1) == INVALID and chains(p=null) == INVALID and chains(ln=null) == INVALID
    assert chains(b=null) == INVALID and chains(a=null) == INVALID and chains(out=null) == INVALID
    assert chains(n=1 << 20, cap=1 << 10) == LIMIT and chains(n=(1 << 31) - 1, cap=(1 << 31) - 1) == LIMIT
    assert chains(n=1 << 20, cap=4, room=1 << 9) == LIMIT and chains(n=(1 << 31) - 1, cap=0, room=1) == LIMIT
    for t in (boxes, layers, chain, anchors, counts, gaps):
        assert (t == -77).all()
    # nothing to do
    assert grow(n=0, f=null, s=null, out=null, added=null) == 0 and chains(n=0, f=null, p=null, ln=null, b=null, a=null, out=null, g=null) == 0
    assert (layers == -77).all() and (counts == -77).all()
    # the calls themselves: an all -1 field of 4 x 4 x 4
    assert grow() == 0 and boxes.tolist() == [[0, 0, 0, 3, 3, 3], [3, 3, 3, 4, 3, 3]] and layers.tolist() == [6, -1]
    assert grow(E=0) == 0 and boxes.tolist() == [[1, 1, 1, 2, 2, 2], [3, 3, 3, 4, 3, 3]] and layers.tolist() == [0, -1]
    assert grow(E=65536, r=4096) == 0 and layers.tolist() == [6, -1]
    assert grow(dims=(65536, 1, 1), f=pkg._ptr(torch.zeros(65536, dtype=torch.int32, device="cuda"))) == 0 and layers.tolist() == [-1, -1]
    assert chains(E=0) == 0 and counts.tolist() == [3, 1] and gaps.tolist() == [0, 0]
    assert anchors.tolist() == [[0, 1, 2, -77], [0, -77, -77, -77]]
    assert chain[0, :3].tolist() == [[0, 0, 0, 1, 0, 0], [1, 0, 0, 1, 1, 0], [1, 1, 0, 2, 1, 0]] and chain[1, 0].tolist() == [3, 3, 2, 3, 3, 3]
    assert (chain[0, 3] == -77).all() and (chain[1, 1:] == -77).all()
    assert chains(E=65536, g=null) == 0 and counts.tolist() == [1, 1] and chain[0, 0].tolist() == [0, 0, 0, 3, 3, 3]
    chain.fill_(-77)
    anchors.fill_(-77)
    assert chains(cap=0, p=null) == 0 and counts.tolist() == [0, 0] and gaps.tolist() == [0, 0]
    assert chains(room=0, b=null, a=null) == 0 and counts.tolist() == [1, 1]
    assert (chain == -77).all() and (anchors == -77).all()
    # a zero entry of dims: no cell is free, every seed comes back with -1 and every box of a path is empty
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        layers.fill_(-77)
        assert grow(dims=dims, f=null) == 0 and layers.tolist() == [-1, -1] and boxes.tolist() == seeds.tolist()
        assert chains(dims=dims, f=null) == 0 and counts.tolist() == [4, 2] and gaps.tolist() == [4, 2]
        assert chain[0].tolist() == [[0, 0, 0, -1, -1, -1], [1, 0, 0, 0, -1, -1], [1, 1, 0, 0, 0, -1], [2, 1, 0, 1, 0, -1]]
        assert anchors.tolist() == [[0, 1, 2, 3], [0, 1, -77, -77]]
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, many_paths):
    pkg, torch = env
    field, origin, dims, r, E, paths, lengths, want = many_paths
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.corridors.grow_boxes(field, origin, dims, r, E, [[origin[0], origin[1], origin[2]] * 2])
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
        pkg.corridors.path_corridors(field, origin, dims, r, E, paths, lengths, max_boxes=4)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 1 and ms > 0.0
        pkg.corridors.path_corridors(field, origin, dims, r, E, paths, lengths)        # two passes: two calls
        assert pkg.stage_timing_read(pkg.STAGE_QUERY)[1] == 2
        pkg.corridors.grow_boxes(field, origin, dims, r, E, np.zeros((0, 6), np.int32))    # nothing is launched, nothing is bracketed
        with pytest.raises(Exception):
            pkg.corridors.path_corridors(field, origin, dims, r, 65537, paths, lengths, max_boxes=4)   # refused: not bracketed either
        assert pkg.stage_timing_read(pkg.STAGE_QUERY)[1] == 0
    finally:
        pkg.stage_timing([])


# ---- plan_corridors and the tool -----------------------------------------------------------------------------------------------------
def test_plan_corridors_then_the_map_plan_tool(env, fused, tmp_path):
    pkg, torch = env
    pool, words, pts, ws = fused
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    clearance, comfort, penalty, extent = 1, 3, 5, 3
    ring = ramp(clearance, comfort, penalty)
    field = distance_field_separable(words, 6, lo.tolist(), dims.tolist(), comfort)
    cell = 2.0 * EDGE / 64
    corner = np.asarray(CENTER, np.float64) - EDGE

    def centre(c):
        return (corner + (np.asarray(c, np.float64) + 0.5) * cell).tolist()
    free = np.argwhere((field < 0) | (field > clearance * clearance))[:, ::-1] + lo
    goal_cell = free[0].tolist()
    old = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), [centre(goal_cell)], clearance, comfort, ring)
    reached = np.argwhere(old["cost"] > 0)[:, ::-1] + lo
    blocked = (np.argwhere(old["cost"] == -2)[0][::-1] + lo).tolist()
    far = (np.array(np.unravel_index(np.argmax(old["cost"]), old["cost"].shape)[::-1]) + lo).tolist()
    starts_m = [centre(c) for c in (far, reached[reached.shape[0] // 2].tolist(), goal_cell, blocked)] + [[100.0, 0.0, 0.0]]
    old = pkg.plan_paths(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m, clearance, comfort, ring, straighten=True, max_lookahead=5)
    new = pkg.corridors.plan_corridors(ws, pool, 6, CENTER, EDGE, box, centre(goal_cell), starts_m, clearance, comfort, ring, extent,
                                       straighten=True, max_lookahead=5)
    assert set(new) == set(old) and np.array_equal(new["cost"], old["cost"])
    chained = 0
    for p, q in zip(new["paths"], old["paths"]):
        assert set(p) == set(q) | {"boxes", "boxes_m", "anchors", "gaps"}
        if q["cells"] is None:
            assert all(p[k] is None for k in p if k != "cell")
            continue
        assert all(np.array_equal(p[k], q[k]) for k in q)
        cells = [tuple(c) for c in p["cells"].tolist()]
        boxes, anchors, gaps = path_corridors_ref(field, lo.tolist(), clearance, extent, cells)
        assert p["boxes"].dtype == np.int32 and [tuple(b) for b in p["boxes"].tolist()] == boxes
        assert p["anchors"].dtype == np.int32 and p["anchors"].tolist() == anchors and p["gaps"] == gaps == 0
        check_chain(field, lo.tolist(), clearance, cells, boxes, anchors)
        assert p["boxes_m"].dtype == np.float64 and p["boxes_m"].shape == (len(boxes), 6)
        assert np.array_equal(p["boxes_m"][:, :3], corner + p["boxes"][:, :3].astype(np.float64) * cell)
        assert np.array_equal(p["boxes_m"][:, 3:], corner + (p["boxes"][:, 3:].astype(np.float64) + 1.0) * cell)
        # every centre of the path lies strictly inside a box in metres
        inside = (p["polyline"][:, None, :] > p["boxes_m"][None, :, :3]) & (p["polyline"][:, None, :] < p["boxes_m"][None, :, 3:])
        assert inside.all(2).any(1).all()
        chained += len(boxes) > 1
    assert chained >= 2 and new["paths"][2]["anchors"].tolist() == [0]
    # the tool, in a child process
    ckpt = tmp_path / "map.svopool"
    pool.save(ckpt, CENTER, EDGE, 6)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "map_plan.py"), str(ckpt), str(tmp_path / "corridor.npz"), "--clearance", str(clearance),
           "--comfort", str(comfort), "--penalty", str(penalty), "--box"] + [repr(float(v)) for v in box] + ["--goal"] + [repr(float(v)) for v in centre(goal_cell)]
    for s in starts_m:
        cmd += ["--start"] + [repr(float(v)) for v in s]
    run = subprocess.run(cmd + ["--corridor", str(extent)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(cmd[3])
    same_field(z["cost"], old["cost"])
    assert int(z["corridor_extent"]) == extent and z["corridor_gaps"].dtype == np.int32 and z["corridor_gaps"].tolist() == [0] * 5
    assert "vertices_0" not in z.files
    stored = np.asarray(CENTER, np.float32).astype(np.float64) - EDGE   # the checkpoint keeps the centre in binary32
    for k, p in enumerate(new["paths"]):
        if p["cells"] is None:
            assert z["boxes_%d" % k].shape == (0, 6) and z["boxes_m_%d" % k].shape == (0, 6) and z["anchors_%d" % k].shape == (0,)
            continue
        assert np.array_equal(z["cells_%d" % k], p["cells"]) and np.array_equal(z["boxes_%d" % k], p["boxes"])
        assert np.array_equal(z["anchors_%d" % k], p["anchors"])
        faces = p["boxes"].astype(np.float64) + np.array([0, 0, 0, 1, 1, 1], np.float64)
        assert np.array_equal(z["boxes_m_%d" % k], np.tile(stored, 2) + faces * cell)
    run = subprocess.run(cmd[:3] + [str(tmp_path / "bad.npz")] + cmd[4:] + ["--corridor", "65537"], capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "--corridor" in run.stderr
