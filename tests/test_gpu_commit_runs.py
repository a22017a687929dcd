"""The fusion commit (csrc/svo_build.hip) on clouds designed by their runs of equal keys (tests/commit_runs.py; test_commit_runs_cpu.py
holds the designs to what they claim): every case in every FORM of the commit -- the blocking insert (fill_kernel + one
mip_level_kernel per level), the asynchronous direct commit (fill_mip_local_kernel + the two-tier mip_straddle2_kernel), split_early +
commit (links from leaf_rec0), commit_deferred + apply (shadow words, apply lists, the single-workgroup mip_straddle_kernel) and the
structure chain (plan_structure ahead of the commits) -- over three frames: the cloud into a fresh pool, the same cloud again, the cloud
with its run lengths rotated by one place.  After every frame the pool is the oracle's, bit for bit.

What the cases put where (T = 512 keys: a workgroup of the plan and of the leaf kernel; G = 16 T: a tier-1 group):
  one_leaf, invalid_front, invalid_only_tail   whole groups without a head: mc == 99 for every tile, the search for the next head over
                                               more than 16 tiles, a super straddler through a group that adds nothing
  on_the_cuts, siblings                        runs that end on T, 2T, G-T, G, G+T, 2G and one key beside them; the parent straddles, the leaves do not
  staircase                                    run i is tile i, and every common-prefix length 0 ... depth-1 stands at a tile's and at a group's edge
  ragged_end                                   a last tile of one key, with and without a head; a last group of one tile
  random_runs                                  all of it at once
  huge                                         8194 fill tiles (> kSlots x kStradThreads = 8192: the plain loop of mip_straddle_kernel, deferred form) in
                                               513 groups (> kStrad2Threads = 256: the second pass of tier 2, asynchronous form)
and test_marks_and_tables_with_few_heads holds the marks for the ray march, which heads alone make, to the entry-by-entry checker."""
import functools
import time

import numpy as np
import pytest

import commit_runs as cr
from accel_check import Rig, check_marks
from util import describe_mismatch

pytestmark = pytest.mark.gpu
CENTER, EDGE = cr.CENTER, cr.EDGE


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    assert torch.cuda.is_available()
    assert pkg.device_arch().startswith("gfx950")
    return pkg, torch


@functools.lru_cache(maxsize=2)
def record(case_id):
    """the frames of a case and the oracle's pool after each of them (size, words), computed once for all forms; read-only"""
    from oracle import oracle as ora
    case = cr.BY_ID[case_id]
    clouds = cr.frames(case)
    opool, after = ora.Pool(), []
    t0 = time.perf_counter()
    for pts, col in clouds:
        opool.insert_cloud(pts, col, case["depth"], CENTER, EDGE)
        words = opool.words()
        words.setflags(write=False)
        after.append((opool.size, words))
    for pts, col in clouds:
        pts.setflags(write=False)
        col.setflags(write=False)
    print("%s: %d points a frame, oracle %.2f s for %d frames, %d nodes" % (case_id, len(clouds[0][0]), time.perf_counter() - t0, len(clouds), after[-1][0]))
    return clouds, after


def commits(env, form, clouds, depth):
    """commits the frames in order in one form of the commit (the call sequences of test_gpu_fusion.py) and yields the pool after each"""
    pkg, torch = env
    dev = [(torch.from_numpy(np.array(p)).cuda(), torch.from_numpy(np.array(c)).cuda()) for p, c in clouds]      # (copies: the record is read-only)
    if form == "structure":     # every frame planned ahead on one stream, the commits in frame order on another
        pool = pkg.Pool(1 << 23)
        wss = [pkg.Workspace() for _ in dev]
        s_struct, s_col = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        evs = []
        with torch.cuda.stream(s_struct):
            pkg.pool_structure_begin(pool)
            for ws, (tp, _) in zip(wss, dev):
                pkg.svo_fuse_sort(ws, tp, depth, CENTER, EDGE)
                pkg.svo_fuse_plan_structure(ws, len(tp), depth, pool)
                e = torch.cuda.Event()
                e.record()
                evs.append(e)
        for ws, (_, tc), e in zip(wss, dev, evs):
            with torch.cuda.stream(s_col):
                s_col.wait_event(e)
                pkg.svo_fuse_commit(ws, tc, depth, pool)
            torch.cuda.synchronize()
            yield pool
        return
    ws, pool = pkg.Workspace(), (pkg.Pool(1 << 22) if form == "early" else pkg.Pool())
    for f, (tp, tc) in enumerate(dev):
        n = len(tp)
        if form == "blocking":
            pkg.svo_from_point_cloud(ws, tp, tc, depth, pool, CENTER, EDGE)
        elif form == "async" or (form == "deferred" and f == 0):       # (the first fusion creates the pool)
            pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, CENTER, EDGE)
        elif form == "early":
            pkg.svo_fuse_sort(ws, tp, depth, CENTER, EDGE)
            pkg.svo_fuse_plan(ws, n, depth, pool)
            pkg.svo_fuse_split_early(ws, n, depth, pool)
            pkg.svo_fuse_commit(ws, tc, depth, pool)
        else:
            assert form == "deferred"
            pkg.svo_fuse_sort(ws, tp, depth, CENTER, EDGE)
            pkg.svo_fuse_plan(ws, n, depth, pool)
            pkg.svo_fuse_commit_deferred(ws, tc, depth, pool)
            pkg.svo_fuse_apply(ws, pool)
        yield pool


def assert_pool_is(pool, size, words, what, links_of=None):
    """links_of: the oracle's words after a LATER frame whose splits are in the pool already (the structure chain: plan_structure
    writes its splits with their links ahead of every commit; a link once there never changes, and the new tiles lie behind `size`).
    The colour words are this frame's, the structure words those of the later frame, both exactly"""
    assert pool.size == size, "%s: %d nodes, the oracle has %d" % (what, pool.size, size)
    got = pool.words()
    if links_of is not None:
        words = words.copy()
        words[0::2] = links_of[0:2 * size:2]
    assert np.array_equal(got, words), "%s: %s" % (what, describe_mismatch(got, words))


@pytest.mark.parametrize("case_id,form", [(c["id"], form) for c in cr.CASES for form in cr.FORMS])
def test_commit_of_designed_runs_matches_oracle(env, oracle, case_id, form):
    clouds, after = record(case_id)
    case = cr.BY_ID[case_id]
    for f, pool in enumerate(commits(env, form, clouds, case["depth"])):
        assert_pool_is(pool, *after[f], "%s, %s, frame %d" % (case_id, form, f + 1), links_of=after[-1][1] if form == "structure" else None)


@pytest.mark.parametrize("form", ["async", "deferred"])
def test_huge_commit_matches_oracle(env, oracle, form):
    """more than 8192 fill tiles and more than 256 straddle groups: two frames of 4 194 817 uniformly random points at depth 3 (runs of
    about G equal keys).  Its time is the oracle's two inserts (1.5 to 2.4 s) and building the clouds; the commits themselves take milliseconds"""
    clouds, after = record(cr.HUGE["id"])
    tiles = -(-len(clouds[0][0]) // cr.T)
    assert tiles > 8 * 1024 and -(-tiles // 16) > 256
    for f, pool in enumerate(commits(env, form, clouds, cr.HUGE["depth"])):
        assert_pool_is(pool, *after[f], "huge, %s, frame %d" % (form, f + 1))


@pytest.mark.parametrize("depth", [10, 13])
def test_marks_and_tables_with_few_heads(env, oracle, depth):
    """the marks of the level grid, the brick ring and the sibling ring are made by heads only (pool_grid_mark, brick_mark_test in
    fill_mip_local_kernel): clouds with a handful of heads in a wavefront and whole workgroups without one, at depth 10 and at depth
    13 (brick shift 1), once by a direct commit and once by commit_deferred + apply, each held to the whole-field check"""
    pkg, torch = env
    # (brick shift 1: the brick field's window is the middle half of the cube; octants 3 then 4 lie in it, and so do the first two runs)
    first, second = cr.on_the_cuts(depth, 0, first=[3, 4] + [1] * (depth - 2)), cr.random_runs(depth, 1)
    if depth == 13:
        first, second = second, first
    rig = Rig(env, oracle, CENTER, EDGE)
    rig.render()

    def finite(pts):
        return pts[np.isfinite(pts).all(1)]

    # a direct commit
    pts, col = cr.build(first, cr.rng_of(first))
    rig.fuse(pts, col, depth)
    rig.recent = [finite(pts)]
    rig.marks("%s, direct commit" % first["id"])
    rig.render()
    seen = rig.check("%s, direct commit" % first["id"])
    assert seen["bricks"] and seen["view"]["brick_shift"] == (0 if depth <= 12 else 1) and seen["lines"] > 0 and seen["missing"] == 0
    # a deferred commit and its apply
    pts, col = cr.build(second, cr.rng_of(second))
    tp, tc = rig.dev(pts, col)
    pkg.svo_fuse_sort(rig.ws, tp, depth, CENTER, EDGE)
    pkg.svo_fuse_plan(rig.ws, len(pts), depth, rig.pool)
    pkg.svo_fuse_commit_deferred(rig.ws, tc, depth, rig.pool)
    torch.cuda.synchronize()
    v = rig.pool.accel_view()
    assert v["deferred_pending"]
    check_marks(env, rig.pool, v["epoch"] & 1, finite(pts), "%s, deferred commit" % second["id"], CENTER, EDGE)
    pkg.svo_fuse_apply(rig.ws, rig.pool)
    rig.opool.insert_cloud(pts, col, depth, CENTER, EDGE)
    rig.recent = [finite(pts)]
    rig.render()
    seen = rig.check("%s, deferred commit and apply" % second["id"])
    assert seen["bricks"] and not seen["view"]["deferred_pending"] and seen["lines"] > 0 and seen["missing"] == 0 and seen["recent"] > 0
