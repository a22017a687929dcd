"""GPU parity where the reference's march reads NODE 0's colour word (tests/node0_scenes.py): samples with an LOD <= 0, and
samples in octant 0 whose walk stops on level 1.  Every render is compared with the CPU oracle byte for byte, the step and
level counters included; tests/test_node0_scenes_cpu.py proves on the CPU that each scene reaches the case it is named for.

 * LOD <= 0 over a level-8 cell WITH children: the brick march must not take the grid's word of the level-8 node there
   (cone_trace.hip decode()), nor add a negative level to its counter;
 * node 0's word is rewritten by every commit (the root pass Q6) without any level-5 block being marked: the grid and
   pyramid entries that hold it -- level-1 cell 0 always, everything under octant 0 while node 0 is childless -- must follow
   (pool_grid.hip pool_grid_node0)."""
import numpy as np
import pytest

import node0_scenes as S
from util import describe_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


_REF = {}


def reference(oracle, key, words, view, mode=0):
    """the oracle's render of `words` from the named view: computed once per (key, view, mode), shared by the tests"""
    k = (key, view, mode)
    if k not in _REF:
        vm, w, h = S.view_matrix(oracle, view)
        ref, steps, levels = oracle.cone_trace(words, w, h, S.FOV, vm, S.CENTER, S.EDGE, mode)
        assert steps <= S.MAX_ORACLE_STEPS
        ref.setflags(write=False)
        _REF[k] = (ref, steps, levels)
    return _REF[k]


def check(env, oracle, ptr, key, words, view, mode=0):
    pkg, torch = env
    vm, w, h = S.view_matrix(oracle, view)
    ref, steps, levels = reference(oracle, key, words, view, mode)
    img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    pkg.cone_trace_svo(img, S.FOV, vm, ptr, S.CENTER, S.EDGE, mode, counters=cnt)
    got, counters = img.cpu().numpy(), cnt.cpu().tolist()
    print("%s %s mode %d: [steps, levels] %s, oracle %s; %s" % (key, view, mode, counters, [steps, levels], describe_mismatch(got, ref)))
    assert counters == [steps, levels], (key, view, counters, [steps, levels])
    assert np.array_equal(got, ref), (key, view, describe_mismatch(got, ref))


@pytest.fixture(scope="module")
def lod0_words(oracle):
    opool = oracle.Pool()
    S.fuse_all(opool, S.lod0_clouds())
    return opool.words()


@pytest.fixture(scope="module")
def polarity_words(lod0_words):
    return {rc: S.opposite_polarity_words(lod0_words, rc) for rc in (True, False)}


@pytest.mark.parametrize("mode", [0, 1])
def test_lod_le0_reads_node0_saturated_over_unsaturated_boundary_cells(env, oracle, lod0_words, mode):
    """scene LOD0, a pool fused by the library (grid built, then updated block-wise by the last commit): node 0's word is
    saturated, the deep boundary cells the samples clamp into are not -- the reference retires every ray on its first sample
    with LOD 0"""
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    (p0, c0, times), (p1, c1, _) = S.lod0_clouds()
    t0, k0 = torch.from_numpy(p0).cuda(), torch.from_numpy(c0).cuda()
    for _ in range(times):
        pkg.svo_from_point_cloud_async(ws, t0, k0, S.DEPTH, pool, S.CENTER, S.EDGE)
    img = torch.zeros((30, 40, 4), dtype=torch.uint8, device="cuda")
    pkg.cone_trace_svo(img, S.FOV, S.view_matrix(oracle, "lod0_plus")[0], pool.data_ptr, S.CENTER, S.EDGE, mode)   # the grid exists from here on
    pkg.svo_from_point_cloud_async(ws, torch.from_numpy(p1).cuda(), torch.from_numpy(c1).cuda(), S.DEPTH, pool, S.CENTER, S.EDGE)
    assert np.array_equal(pool.words(), lod0_words)
    check(env, oracle, pool.data_ptr, "lod0", lod0_words, "lod0_plus", mode)
    check(env, oracle, pool.data_ptr, "lod0", lod0_words, "lod0_minus", mode)


@pytest.mark.parametrize("raise_corner", [True, False])
def test_lod_le0_node0_unsaturated_runs_on_to_negative_lods(env, oracle, polarity_words, raise_corner):
    """the same tree through set_words with node 0 below saturation: the reference never retires on node 0 and runs on to LODs
    -1 and -2.  raise_corner: the + corner's deep path saturated (a march that takes the level-8 word retires early);
    otherwise nothing is saturated (a march that adds negative levels miscounts)"""
    pkg, torch = env
    words = polarity_words[raise_corner]
    pool = pkg.Pool()
    pool.set_words(words)
    for mode in (0, 1):
        check(env, oracle, pool.data_ptr, ("polarity", raise_corner), words, "lod0_minus", mode)
    check(env, oracle, pool.data_ptr, ("polarity", raise_corner), words, "lod0_plus", 0)


@pytest.mark.parametrize("raise_corner", [True, False])
def test_lod_le0_in_memory_the_library_does_not_know(env, oracle, polarity_words, lod0_words, raise_corner):
    """the same words as a plain device tensor: cone_trace_kernel with a grid built for the render"""
    pkg, torch = env
    for key, words in ((("polarity", raise_corner), polarity_words[raise_corner]), ("lod0", lod0_words)):
        foreign = torch.from_numpy(words.view(np.int32).copy()).cuda()
        for view in ("lod0_minus", "lod0_plus"):
            check(env, oracle, foreign.data_ptr(), key, words, view, 0)


@pytest.mark.parametrize("raise_corner", [True, False])
def test_lod_le0_with_bursts_off(env, oracle, polarity_words, lod0_words, raise_corner):
    """svoslam_config.march_ahead < 0: one sample per iteration throughout (the plain loop's decode alone)"""
    pkg, torch = env
    before = pkg.configure(march_ahead=-1)
    try:
        for key, words in ((("polarity", raise_corner), polarity_words[raise_corner]), ("lod0", lod0_words)):
            pool = pkg.Pool()
            pool.set_words(words)
            for view in ("lod0_minus", "lod0_plus"):
                check(env, oracle, pool.data_ptr, key, words, view, 0)
    finally:
        pkg.configure(march_ahead=before["march_ahead"])


# ---- node 0's word changes without a marked block -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stale_states(oracle):
    return {False: S.stale_sequence(oracle), True: S.stale_sequence(oracle, S.stale_first_frame_with_octant0())}


def fuse_blocking(pkg, torch, ctx, pts, col, between):
    pkg.svo_from_point_cloud(ctx["ws"], pts, col, S.DEPTH, ctx["pool"], S.CENTER, S.EDGE)


def fuse_async(pkg, torch, ctx, pts, col, between):
    pkg.svo_from_point_cloud_async(ctx["ws"], pts, col, S.DEPTH, ctx["pool"], S.CENTER, S.EDGE)


def fuse_deferred(pkg, torch, ctx, pts, col, between):
    ws, pool = ctx["ws"], ctx["pool"]
    if not ctx.get("created"):      # the first fusion creates the pool (as in tests/test_gpu_fusion.py): every later frame is deferred
        ctx["created"] = True
        return fuse_async(pkg, torch, ctx, pts, col, between)
    pkg.svo_fuse_sort(ws, pts, S.DEPTH, S.CENTER, S.EDGE)
    pkg.svo_fuse_plan(ws, len(pts), S.DEPTH, pool)
    pkg.svo_fuse_commit_deferred(ws, col, S.DEPTH, pool)
    if between:
        between()        # a render between commit and apply still shows the old map
    pkg.svo_fuse_apply(ws, pool)


def fuse_keyrange(pkg, torch, ctx, pts, col, between):
    """the frame cut by key range over two replicas of the pool (tests/test_gpu_keyrange.py); replica 0 is the one rendered"""
    n, world = len(pts), 2
    if "reps" not in ctx:
        ctx["reps"] = [ctx["pool"], pkg.Pool(1 << 22)]
        ctx["wss"] = [pkg.Workspace() for _ in range(world)]
        ctx["deltas"] = [torch.zeros(pkg.KEYRANGE_FIXED_WORDS + 48 * 6400, dtype=torch.int32, device="cuda") for _ in range(world)]
        ctx["keys"] = torch.empty(6400, dtype=torch.int64, device="cuda")
        ctx["idx"] = torch.empty(6400, dtype=torch.int32, device="cuda")
    keys, idx = ctx["keys"][:n], ctx["idx"][:n]
    pkg.svo_fuse_sort(ctx["ws"], pts, S.DEPTH, S.CENTER, S.EDGE)
    pkg.svo_fuse_export_sorted(ctx["ws"], n, keys, idx)
    for r in range(world):
        pkg.svo_fuse_keyrange_commit(ctx["wss"][r], keys, idx, col, S.DEPTH, ctx["reps"][r], r, world, ctx["deltas"][r])
    for r in range(world):
        pkg.svo_fuse_keyrange_apply(ctx["wss"][r], keys, S.DEPTH, ctx["reps"][r], ctx["deltas"])
        assert pkg.svo_fuse_keyrange_status(ctx["wss"][r]) == 0


PATHS = {"blocking": fuse_blocking, "async": fuse_async, "deferred": fuse_deferred, "keyrange": fuse_keyrange}


def run_stale_sequence(env, oracle, states, first, views, path, key):
    pkg, torch = env
    frames, words = states
    ctx = dict(ws=pkg.Workspace(), pool=pkg.Pool(1 << 22) if path == "keyrange" else pkg.Pool())   # (replicas: as tests/test_gpu_keyrange.py sizes them)
    pool, fuse = ctx["pool"], PATHS[path]
    pts, col = S.stale_cloud()
    tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
    fp, fc = (torch.from_numpy(first[0]).cuda(), torch.from_numpy(first[1]).cuda()) if first is not None else (tp, tc)
    fuse(pkg, torch, ctx, fp, fc, None)
    assert np.array_equal(pool.words(), words[0])
    for view in views:      # the grid is built and valid from here on
        check(env, oracle, pool.data_ptr, (key, 1), words[0], view)
    for k in range(2, frames + 1):   # node 0's alpha crosses saturation in the last frame
        last = k == frames
        fuse(pkg, torch, ctx, tp, tc, (lambda: check(env, oracle, pool.data_ptr, (key, frames - 1), words[frames - 2], views[0])) if last else None)
    assert S.alpha_of(words[-2], 0) < S.SATURATED <= S.alpha_of(words[-1], 0)
    assert np.array_equal(pool.words(), words[-1])
    for view in views:
        check(env, oracle, pool.data_ptr, (key, frames), words[-1], view)


@pytest.mark.parametrize("path", ["blocking", "async", "deferred", "keyrange"])
def test_node0_word_follows_commits_outside_octant0_node0_childless(env, oracle, stale_states, path):
    """scene "stale": every frame fuses octant 7 only, node 0 stays childless and every grid / pyramid entry under octant 0 holds
    (1, node 0's word).  Rendered after frame 1 and after the frame in which node 0's alpha crosses saturation: the fresh word
    retires every ray on its first sample, the previous one marches on (the counters tell even where the image cannot)"""
    assert not (int(stale_states[False][1][-1][0]) & S.FLAG)
    run_stale_sequence(env, oracle, stale_states[False], None, ("stale_coarse", "stale_fine"), path, "stale")


@pytest.mark.parametrize("path", ["async", "deferred"])
def test_node0_word_follows_commits_outside_octant0_node0_with_children(env, oracle, stale_states, path):
    """frame 1 also puts a few hundred points into octant 0, later frames fuse octant 7 only: node 0's word lives in the
    pyramid's level-1 cell 0, which samples with LOD 1 in octant 0 (ray length 0.75 .. 1.5 m) read"""
    assert int(stale_states[True][1][-1][0]) & S.FLAG
    run_stale_sequence(env, oracle, stale_states[True], S.stale_first_frame_with_octant0(), ("stale_coarse",), path, "stale6")
