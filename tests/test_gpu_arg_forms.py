"""The forms a cell list may take, through every wrapper that takes one -- reach_field, owner_field and cost_field (seeds),
visibility_field (views), cover_views (candidates), trace_paths (starts) and segment_clearance (segments): a Python list, an int64
array, a flat array, a contiguous int32 cuda tensor and a non-contiguous int32 cuda view of the same cells give identical outputs;
an empty list gives what it always gave (recorded below from the one-file package that preceded the split into submodules); a
float cuda tensor is refused by name.  Nothing here says what a field's values should be: the per-feature tests own that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CENTER, EDGE, DEPTH = (0.0, 0.0, 0.0), 1.0, 5                  # 32^3 cells of 1/16
# a dozen occupied cells: a wall of six and three single cells inside the region, three cells outside it
OCCUPIED = [(15, y, 16) for y in range(12, 18)] + [(13, 13, 13), (18, 18, 18), (12, 19, 12), (5, 5, 5), (25, 20, 7), (16, 16, 25)]
ORIGIN, REGIONS = (12, 12, 12), ((8, 8, 8), (8, 0, 8))
CELLS = [(13, 14, 15), (17, 15, 14), (18, 13, 18), (2, 2, 2)]   # three free cells of the region and one outside it
SEGMENTS = [(13, 14, 15, 17, 15, 14), (18, 13, 18, 13, 14, 15), (17, 15, 14, 2, 2, 2), (14, 12, 16, 16, 17, 16)]   # the last crosses the wall


class World:
    pass


@pytest.fixture(scope="module")
def world():
    """the map, and per region the two fields the path calls read; built once and left unchanged"""
    import torch
    import svoslam_pkg
    w = World()
    w.pkg, w.torch = svoslam_pkg.load(), torch
    points = ((np.asarray(OCCUPIED, np.float64) + 0.5) / 16.0 - 1.0).astype(np.float32)      # the cells' centres
    colors = np.full((len(OCCUPIED), 3), 200, np.uint8)
    w.ws, w.pool = w.pkg.Workspace(), w.pkg.Pool()
    w.pkg.svo_from_point_cloud(w.ws, torch.from_numpy(points).cuda(), torch.from_numpy(colors).cuda(), DEPTH, w.pool, CENTER, EDGE)
    w.steps = {n: w.pkg.reach_field(w.ws, w.pool, DEPTH, ORIGIN, n, 0, [CELLS[0]], as_tensor=True) for n in REGIONS}
    w.dist = {n: w.pkg.distance_field(w.ws, w.pool, DEPTH, ORIGIN, n, 3, as_tensor=True) for n in REGIONS}
    return w


# name -> (the word for the list in a refusal, its rows, call(world, dims, list) -> the outputs as a list of numpy arrays)
CALLS = {
    "reach_field": ("seeds", CELLS, lambda w, n, c: [w.pkg.reach_field(w.ws, w.pool, DEPTH, ORIGIN, n, 0, c)]),
    "owner_field": ("seeds", CELLS, lambda w, n, c: list(w.pkg.owner_field(w.ws, w.pool, DEPTH, ORIGIN, n, 0, seeds=c))),
    "cost_field": ("seeds", CELLS, lambda w, n, c: [w.pkg.cost_field(w.ws, w.pool, DEPTH, ORIGIN, n, 0, 1, [3], c)]),
    "visibility_field": ("views", CELLS, lambda w, n, c: list(w.pkg.visibility_field(w.ws, w.pool, DEPTH, ORIGIN, n, 6, c,
                                                                                      want=("mask", "count")).values())),
    "cover_views": ("candidates", CELLS, lambda w, n, c: list(w.pkg.cover_views(w.ws, w.pool, DEPTH, ORIGIN, n, 6, c, 2).values())),
    "trace_paths": ("starts", CELLS, lambda w, n, c: list(w.pkg.trace_paths(w.steps[n], ORIGIN, n, c, 4))),
    "segment_clearance": ("segments", SEGMENTS, lambda w, n, c: list(w.pkg.segment_clearance(w.dist[n], ORIGIN, n, c, want_cell=True))),
}


def forms(torch, rows):
    """the same rows in every form a wrapper takes; "tensor", the contiguous int32 cuda tensor, is the one the others are held to"""
    a = np.asarray(rows, np.int64)
    t = torch.from_numpy(a.astype(np.int32)).cuda()
    wide = torch.full((a.shape[0], 2 * a.shape[1]), 7, dtype=torch.int32, device="cuda")
    wide[:, :a.shape[1]] = t
    view = wide[:, :a.shape[1]]
    assert t.is_contiguous() and not view.is_contiguous()
    return {"tensor": t, "list": a.tolist(), "int64": a, "flat": a.reshape(-1), "view": view}


def same(got, want):
    assert len(got) == len(want)
    for g, x in zip(got, want):
        assert g.dtype == x.dtype and g.shape == x.shape and np.array_equal(g, x)


@pytest.mark.parametrize("dims", REGIONS)
@pytest.mark.parametrize("name", sorted(CALLS))
def test_every_form_of_a_cell_list_gives_the_same_outputs(world, name, dims):
    _, rows, call = CALLS[name]
    given = forms(world.torch, rows)
    want = call(world, dims, given.pop("tensor"))
    for form, cells in given.items():
        same(call(world, dims, cells), want)


def empty_outputs(dims):
    """what each call gave for an empty list before the split: nothing reached, seen or chosen, no path and no segment"""
    shape = (dims[2], dims[1], dims[0])
    inside = [q for q in OCCUPIED if all(ORIGIN[a] <= q[a] < ORIGIN[a] + dims[a] for a in range(3))]
    blocked = np.full(shape, -1, np.int32)                         # -1: no path leads here; -2: an occupied cell
    for x, y, z in inside:
        blocked[z - ORIGIN[2], y - ORIGIN[1], x - ORIGIN[0]] = -2
    assert len(inside) == (9 if min(dims) > 0 else 0)
    none = np.zeros(0, np.int32)
    return {
        "reach_field": [blocked], "owner_field": [blocked, blocked], "cost_field": [blocked],
        "visibility_field": [np.zeros(shape, np.uint32), np.zeros(shape, np.int32)],
        # seen, chosen, gain, round (-2: a target no chosen candidate sees), summary (targets, chosen, covered, coverable)
        "cover_views": [none, np.array([-1, -1], np.int32), np.array([0, 0], np.int32), blocked, np.array([len(inside), 0, 0, 0], np.int32)],
        "trace_paths": [np.zeros((0, 4, 3), np.int32), none],
        "segment_clearance": [none, np.zeros((0, 3), np.int32)],
    }


@pytest.mark.parametrize("dims", REGIONS)
def test_an_empty_list_gives_what_it_always_gave(world, dims):
    want = empty_outputs(dims)
    empties = ([], np.zeros((0, 3), np.int64), world.torch.zeros((0, 3), dtype=world.torch.int32, device="cuda"))
    for name, (_, _, call) in CALLS.items():
        for cells in empties if name != "segment_clearance" else ([], np.zeros((0, 6), np.int32)):
            same(call(world, dims, cells), want[name])
    rounds = 1 if min(dims) > 0 else 0                               # one round finds nothing to do; no cells, no round
    stats = {}
    world.pkg.reach_field(world.ws, world.pool, DEPTH, ORIGIN, dims, 0, [], stats=stats)
    assert stats == {"rounds": rounds, "tile_runs": 0, "seeds_used": 0}
    stats = {}
    world.pkg.owner_field(world.ws, world.pool, DEPTH, ORIGIN, dims, 0, seeds=[], stats=stats)
    assert stats == {"rounds": rounds, "tile_runs": 0, "seeds_used": 0, "owner_rounds": rounds, "owner_tile_runs": 0}
    stats = {}
    world.pkg.cost_field(world.ws, world.pool, DEPTH, ORIGIN, dims, 0, 1, [3], [], stats=stats)
    assert stats == {"rounds": rounds, "tile_runs": 0, "seeds_used": 0, "max_weight": 4}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_float_tensor_is_refused_by_name(world, name):
    what, rows, call = CALLS[name]
    wrong = world.torch.zeros((2, len(rows[0])), dtype=world.torch.float32, device="cuda")
    with pytest.raises(ValueError) as e:
        call(world, REGIONS[0], wrong)
    assert str(e.value) == "a %s tensor is int32 on the device" % what
