"""svoslam_pool_distance_field on the device: every value equals the host restatement of the specification
(tests/test_field_cpu.py: distance_field_words, the definition, for the small cases; distance_field_separable, proven equal to it
there, for the larger ones) applied to the pool's own words -- never a second device result alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_field_cpu import FIELD_CASES, distance_field_separable, distance_field_words, midpoints
from test_gpu_query import fused_pool
from test_surface_cpu import CENTER, EDGE, HandPool, OPAQUE, occupied_cells

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_MAX_RADIUS = 64            # map_field.hip: a larger radius reads the intermediate from global memory
SEGMENT = 64                   # ... and a column is cut into segments of this many outputs


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def fused(env):
    """depth -> (pool, its words, the fused points, workspace): fused on the device, twice, shared by the tests below and left
    unchanged"""
    pkg, torch = env
    out = {}
    for depth in (6, 9):
        ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 41)
        out[depth] = (pool, pool.words(), pts, ws)
    return out


def same_field(got, want):
    assert got.dtype == np.int32 and want.dtype == np.int32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (bad.shape[0], bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), want[tuple(bad[:5].T)].tolist())


# ---- hand-built pools ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth, origin, dims, radius, want = FIELD_CASES[name]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    got = pkg.distance_field(ws, pool, depth, origin, dims, radius)
    same_field(got, want)
    same_field(got, distance_field_words(words, depth, origin, dims, radius))
    if depth > 1:                                                  # the level above, from the same words
        o = [v // 2 for v in origin]
        n = [(origin[a] + dims[a] + 1) // 2 - o[a] for a in range(3)]
        same_field(pkg.distance_field(ws, pool, depth - 1, o, n, radius), distance_field_words(words, depth - 1, o, n, radius))


# ---- fused pools -------------------------------------------------------------------------------------------------------------
# (fused depth, d, (nx, ny, nz), origin x: "lo" 0 | "in" 37 | "hi" N - nx | "pt" about the cloud, R).  nx 1, 63, 64, 65, 130: the edges
# of a row word and of a wavefront; ny, nz 1, 2, 70 (70: longer than one column segment); origin x 37: a row that starts inside a
# word; R 64: larger than most of these regions, so the halo dominates and is clipped by the root.  y and z are placed about an
# occupied cell.  Sizes that do not fit the lattice of d are cut to it (N = 16 at d = 4, 64 at 6, 128 at 7).
FUSED_CASES = [
    (9, 9, (1, 1, 1), "pt", 0), (9, 9, (63, 2, 70), "in", 1), (9, 9, (64, 70, 2), "lo", 5), (9, 9, (65, 2, 2), "hi", 5),
    (9, 9, (130, 70, 1), "in", 64), (9, 9, (130, 1, 70), "hi", 64), (9, 9, (65, 70, 70), "pt", 5), (9, 9, (130, 2, 2), "pt", 1),
    (9, 7, (64, 2, 70), "in", 5), (9, 7, (130, 1, 2), "lo", 64), (9, 7, (63, 70, 1), "hi", 1), (9, 7, (1, 2, 2), "pt", 0),
    (6, 6, (63, 2, 70), "lo", 64), (6, 6, (64, 70, 1), "lo", 5), (6, 6, (1, 1, 2), "hi", 1), (6, 6, (20, 7, 3), "in", 5),
    (6, 6, (65, 70, 70), "pt", 0), (6, 4, (65, 70, 70), "lo", 64), (6, 4, (1, 2, 1), "hi", 0), (6, 4, (5, 1, 2), "in", 1),
    # an R above what the LDS-staged path takes: the other path
    (9, 9, (4, 4, 4), "pt", LDS_MAX_RADIUS + 36),
]


def case_region(words, d, shape, ox, radius):
    """-> (origin, dims) of a case on the lattice of d"""
    n_side = 1 << d
    dims = [min(v, n_side) for v in shape]
    xyz = occupied_cells(words, d)[0]
    anchor = xyz[xyz.shape[0] // 2]
    origin = [int(np.clip(anchor[a] - dims[a] // 2, 0, n_side - dims[a])) for a in range(3)]
    origin[0] = {"lo": 0, "in": min(37, n_side - dims[0]), "hi": n_side - dims[0], "pt": origin[0]}[ox]
    return origin, dims


@pytest.fixture(scope="module")
def reference(fused):
    """case -> (origin, dims, the restatement's field), computed once"""
    cache = {}

    def get(case):
        if case not in cache:
            depth, d, shape, ox, radius = case
            words = fused[depth][1]
            origin, dims = case_region(words, d, shape, ox, radius)
            cache[case] = (origin, dims, distance_field_separable(words, d, origin, dims, radius))
        return cache[case]
    return get


def check_the_cases_are_not_empty(words_of, reference):
    """on the restatement's results, never the device's: over the fused cases with R >= 3 there are cells on occupied ones, cells
    near them, cells with nothing within R, and cells whose value comes from an occupied cell outside the region"""
    zero = positive = none = from_outside = 0
    nx, nyz, ox, radii, paths = set(), set(), set(), set(), set()
    for case in FUSED_CASES:
        depth, d, shape, kind, radius = case
        origin, dims, want = reference(case)
        nx.add(dims[0]); nyz.update(dims[1:]); ox.add(kind); radii.add(radius); paths.add(radius <= LDS_MAX_RADIUS)
        if radius < 3:
            continue
        zero, positive, none = zero + int((want == 0).sum()), positive + int((want > 0).sum()), none + int((want == -1).sum())
        if want.size <= 20000:
            xyz = occupied_cells(words_of(depth), d)[0]
            inside = ((xyz >= np.asarray(origin)) & (xyz < np.asarray(origin) + np.asarray(dims))).all(1)
            from_outside += int((want != distance_field_words(None, d, origin, dims, radius, cells=xyz[inside])).sum())
    assert zero > 100 and positive > 100 and none > 20 and from_outside >= 1, (zero, positive, none, from_outside)
    assert nx >= {1, 63, 64, 65, 130} and nyz >= {1, 2, 70} and ox == {"lo", "in", "hi", "pt"} and radii >= {0, 1, 5, 64}
    assert paths == {True, False} and max(max(reference(c)[1][1:]) for c in FUSED_CASES) > SEGMENT


def test_the_fused_cases_are_not_empty(fused, reference):
    check_the_cases_are_not_empty(lambda depth: fused[depth][1], reference)


@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: "fused%d-d%d-%dx%dx%d-%s-R%d" % (c[0], c[1], *c[2], c[3], c[4]))
def test_fused_cloud(env, fused, reference, case):
    pkg, torch = env
    pool, words, pts, ws = fused[case[0]]
    origin, dims, want = reference(case)
    same_field(pkg.distance_field(ws, pool, case[1], origin, dims, case[4]), want)


def test_the_field_is_the_device_nearest_occupied_at_the_midpoints(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[9]
    origin, dims = case_region(words, 9, (65, 3, 2), "pt", 5)
    want = distance_field_words(words, 9, origin, dims, 5)
    assert (want == 0).sum() > 0 and (want > 0).sum() > 20
    got = pkg.distance_field(ws, pool, 9, origin, dims, 5)
    same_field(got, want)
    near = pkg.nearest_occupied(pool, 9, CENTER, EDGE, midpoints(9, CENTER, EDGE, origin, dims), 5, outputs=("dist2",))["dist2"]
    same_field(got, near.reshape(got.shape))


def test_depth_16_cells_beyond_15_bits(env):
    pkg, torch = env
    ws, pool, pts = fused_pool(pkg, torch, 16, 2000, 43)
    words = pool.words()
    xyz = occupied_cells(words, 16)[0]
    anchor = xyz[np.argmax(xyz.max(1))]
    dims = [65, 2, 2]
    origin = [int(np.clip(anchor[a] - dims[a] // 2, 0, (1 << 16) - dims[a])) for a in range(3)]
    want = distance_field_words(words, 16, origin, dims, 5)
    assert max(origin) >= 1 << 15 and (want == 0).sum() > 0 and (want > 0).sum() > 20
    same_field(pkg.distance_field(ws, pool, 16, origin, dims, 5), want)


def test_depth_1_pool(env):
    pkg, torch = env
    hp = HandPool()
    hp.put([3], [OPAQUE])
    hp.put([4], [OPAQUE])
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(hp.words())
    for radius, want in ((0, [[[-1, -1], [-1, 0]], [[0, -1], [-1, -1]]]), (1, [[[1, 1], [1, 0]], [[0, 1], [1, 1]]])):
        got = pkg.distance_field(ws, pool, 1, (0, 0, 0), (2, 2, 2), radius)
        same_field(got, np.array(want, np.int32))                  # (1,1,0) and (0,0,1) are occupied
        same_field(got, distance_field_words(hp.words(), 1, (0, 0, 0), (2, 2, 2), radius))


def test_pending_fusions_are_drained(env):
    pkg, torch = env
    depth = 8
    ws, pool, pts = fused_pool(pkg, torch, depth, 15000, 47)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    dims = (130, 70, 9)
    cell = np.floor((pts[0] - (np.asarray(CENTER) - EDGE)) / (2.0 * EDGE / (1 << depth))).astype(int)   # about a fused point
    origin = [int(np.clip(cell[a] - dims[a] // 2, 0, (1 << depth) - dims[a])) for a in range(3)]
    unsynced = pkg.distance_field(ws, pool, depth, origin, dims, 9)
    assert pool._p.pending > 0                                     # the call drains the stream and leaves the pool's record alone
    assert pool.size > 8 and pool._p.pending == 0                  # svoslam_pool_sync
    words = pool.words()
    want = distance_field_separable(words, depth, origin, dims, 9)
    assert (want == 0).sum() > 100 and (want > 0).sum() > 100 and (want == -1).sum() > 20
    same_field(pkg.distance_field(ws, pool, depth, origin, dims, 9), unsynced)
    same_field(unsynced, want)


def test_workspace_slots_are_reused(env, fused):
    pkg, torch = env
    pool, words, pts, _ = fused[6]
    ws = pkg.Workspace()
    assert ws.field_buffers() == [(0, 0)] * 3
    large, small = ((0, 0, 0), (64, 64, 40)), ((5, 3, 7), (33, 20, 9))
    first = pkg.distance_field(ws, pool, 6, *large, 5)
    slots = ws.field_buffers()
    assert all(p != 0 and b > 0 for p, b in slots)
    again = pkg.distance_field(ws, pool, 6, *large, 5)
    assert ws.field_buffers() == slots                             # a second call of the same size allocates nothing
    want = distance_field_separable(words, 6, *large, 5)
    same_field(first, want)
    same_field(again, want)
    got = pkg.distance_field(ws, pool, 6, *small, 5)               # a smaller call in the larger call's slots
    assert ws.field_buffers() == slots
    same_field(got, distance_field_separable(words, 6, *small, 5))
    same_field(got, want[7:16, 3:23, 5:38])


def test_as_tensor(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    origin, dims = (3, 0, 9), (61, 30, 5)
    got = pkg.distance_field(ws, pool, 6, origin, dims, 5, as_tensor=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (5, 30, 61)
    same_field(got.cpu().numpy(), distance_field_separable(words, 6, origin, dims, 5))


def test_box_to_cells_then_the_field_and_the_map_esdf_tool(env, fused, tmp_path):
    """the field of the box one would hand to count_boxes: the cells count_boxes counts are the field's zeros; and
    tools/map_esdf.py writes that field for a saved map"""
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    box = np.concatenate([pts[0] - 0.3, pts[0] + 0.25]).astype(np.float32)
    lo, hi = pkg.box_to_cells(6, CENTER, EDGE, box)
    dims = hi - lo + 1
    want = distance_field_separable(words, 6, lo.tolist(), dims.tolist(), 7)
    got = pkg.distance_field(ws, pool, 6, lo, dims, 7)
    same_field(got, want)
    count = int(pkg.count_boxes(pool, 6, CENTER, EDGE, box[None, :], outputs=("count",))["count"][0])
    assert count == int((want == 0).sum()) and count > 20 and (want > 0).sum() > 100
    ckpt, out = tmp_path / "map.svopool", tmp_path / "esdf.npz"
    pool.save(ckpt, CENTER, EDGE, 6)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_esdf.py"), str(ckpt), str(out), "--radius", "7", "--box"] +
                       [repr(float(v)) for v in box], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    same_field(z["dist2"], want)
    assert z["origin"].tolist() == lo.tolist() and z["dims"].tolist() == dims.tolist() and int(z["depth"]) == 6
    cell = 2.0 * EDGE / 64
    assert float(z["cell_size"]) == cell and z["metres"].dtype == np.float32 and z["metres"].shape == want.shape
    assert np.array_equal(z["metres"], np.where(want >= 0, np.sqrt(np.maximum(want, 0).astype(np.float64)) * cell, np.inf).astype(np.float32))
    assert "%d of %d cells occupied" % (count, want.size) in r.stdout


def test_nothing_to_do_and_argument_errors(env):
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    L = pkg.lib()
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        got = pkg.distance_field(ws, pool, 5, (1, 2, 3), dims, 4)
        assert got.shape == (dims[2], dims[1], dims[0]) and got.dtype == np.int32
    assert ws.field_buffers() == [(0, 0)] * 3                      # nothing was launched, nothing allocated
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    null, ptr = C.c_void_p(0), pkg._ptr(buf)

    def i3(v):
        return None if v is None else (C.c_int32 * 3)(*v)

    def field(ws_ref=ws._h, pool_ref=C.byref(pool._p), depth=5, origin=(1, 2, 3), dims=(4, 2, 2), radius=3, out=ptr):
        return L.svoslam_pool_distance_field(ws_ref, pool_ref, depth, i3(origin), i3(dims), radius, out, pkg._stream())
    assert field() == 0 and field(dims=(0, 2, 2)) == 0 and field(pool_ref=None, dims=(4, 0, 2)) == 0
    assert field(dims=(4, 2, 0), out=null) == 0 and field(pool_ref=None, dims=(0, 0, 0), out=null) == 0
    assert field(ws_ref=None) == -1 and field(origin=None) == -1 and field(dims=None) == -1
    assert field(ws_ref=None, dims=(0, 2, 2)) == -1 and field(depth=0, dims=(0, 2, 2)) == -1
    assert field(depth=0) == -1 and field(depth=17) == -1
    assert field(dims=(-1, 2, 2)) == -1 and field(dims=(4, 2, -1)) == -1 and field(dims=(0, -1, 2)) == -1
    for a in range(3):                                             # one cell outside the root on each side
        origin, dims = [1, 2, 3], [4, 2, 2]
        origin[a] = -1
        assert field(origin=origin) == -1
        origin[a] = 32 - dims[a] + 1
        assert field(origin=origin) == -1
        origin[a] = 32 - dims[a]
        assert field(origin=origin) == 0
        origin[a], dims[a] = 0, 33
        assert field(origin=origin, dims=dims) == -1
    assert field(radius=0) == 0 and field(radius=64) == 0
    assert field(radius=-1) == -1 and field(radius=4097) == -1 and field(radius=4097, dims=(0, 2, 2)) == -1
    assert field(pool_ref=None) == -1 and field(out=null) == -1
    blank = pkg._PoolStruct(None, 0, 0, None, 0, 0)                # an uninitialised pool
    assert field(pool_ref=C.byref(blank)) == -1 and field(pool_ref=C.byref(blank), dims=(0, 2, 2)) == 0
    # more than 2^31 - 1 output cells, and an intermediate of more than 2^31 - 1 elements: refused before anything is allocated
    slots = ws.field_buffers()
    assert field(depth=16, origin=(0, 0, 0), dims=(2048, 1024, 1024)) == -6
    assert field(depth=16, origin=(0, 4096, 4096), dims=(65536, 1, 1), radius=4096) == -6
    assert ws.field_buffers() == slots
    with pytest.raises(Exception):
        pkg.distance_field(ws, pool, 5, (0, 0, 0), (4, 4, 4), 4097)
    with pytest.raises(Exception):
        pkg.distance_field(ws, pool, 5, (30, 0, 0), (4, 4, 4), 3)
    assert L.svoslam_abi_version() == 1


def test_stage_timing_records_one_pair_per_call(env, fused):
    pkg, torch = env
    pool, words, pts, ws = fused[6]
    pkg.stage_timing([pkg.STAGE_QUERY])
    try:
        pkg.distance_field(ws, pool, 6, (0, 0, 0), (64, 20, 3), 5)
        pkg.distance_field(ws, pool, 4, (1, 2, 3), (9, 3, 3), LDS_MAX_RADIUS + 1)
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 2 and ms > 0.0
        pkg.distance_field(ws, pool, 6, (0, 0, 0), (64, 0, 3), 5)  # nothing is launched, nothing is bracketed
        ms, pairs = pkg.stage_timing_read(pkg.STAGE_QUERY)
        assert pairs == 0
    finally:
        pkg.stage_timing([])
