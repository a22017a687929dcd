"""Key-range sharded fusion on the GPU (csrc/svo_keyrange.hip; the protocol is pinned on the CPU by
tests/test_keyrange_gloo.py): `world` replicas of one pool in ONE process stand for the ranks -- every frame each of them plans and commits
its slice of the frame's sorted keys (svoslam_svo_fuse_keyrange_commit), the deltas are "all-gathered" (the tensors are simply shared), and
every replica applies all of them (svoslam_svo_fuse_keyrange_apply).  After every frame every replica must equal, byte for byte, the pool
that fused the frame in one piece (which in turn equals the CPU oracle's), and render the same image with the same step / level counters
through the level grid and the occupancy bricks -- replica 0 renders after every frame, the last replica only at the end (ranks of a
frame-sharded session render different frames: their dirty states differ)."""
import numpy as np
import pytest

from util import describe_mismatch, surface_cloud

pytestmark = pytest.mark.gpu

VIEWS = (((0.1, 0.2, -2.6), (0, 0, 0), (96, 72)), ((0.1, 0.2, -1.2), (0, 0, 0), (24, 480)), ((0.3, 0.1, 0.62), (0.28, 0.05, 0.2), (32, 480)))


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def render(pkg, torch, pool, view, w, h, center, edge):
    img = torch.full((h, w, 4), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    pkg.cone_trace_svo(img, 45.0, view, pool.data_ptr, center, edge, 0, counters=cnt)
    return img.cpu().numpy(), cnt.cpu().tolist()


@pytest.mark.parametrize("world,depth", [(2, 12), (3, 12), (8, 12), (4, 14), (8, 9)])
def test_keyrange_replicas_equal_the_one_piece_fusion(env, oracle, world, depth):
    pkg, torch = env
    rng = np.random.default_rng(40 + world + depth)
    center, edge = (0.0, 0.0, 0.0), 1.0
    n = 12000
    ref, opool = pkg.Pool(1 << 22), oracle.Pool()
    reps = [pkg.Pool(1 << 22) for _ in range(world)]
    ws_sort, ws_ref = pkg.Workspace(), pkg.Workspace()
    wss = [pkg.Workspace() for _ in range(world)]
    cap_words = pkg.KEYRANGE_FIXED_WORDS + 48 * n
    deltas = [torch.zeros(cap_words, dtype=torch.int32, device="cuda") for _ in range(world)]
    keys = torch.empty(n, dtype=torch.int64, device="cuda"); idx = torch.empty(n, dtype=torch.int32, device="cuda")
    base, bcol = surface_cloud(rng, n)
    sharded_frames, shared_records, used = 0, [], []
    for f in range(7):
        if f == 0:
            pts, col = base, bcol
        else:   # the surface again, a little displaced and with new colours; frame 4 brings points with NaNs and duplicates
            pts = (base + rng.normal(0, 0.002, base.shape).astype(np.float32) + np.float32(0.003 * f)).astype(np.float32)
            col = rng.integers(0, 256, bcol.shape, dtype=np.uint8)
            if f == 4:
                pts[::37] = np.nan
                pts[1::50] = pts[0]
        tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
        pkg.svo_fuse_sort(ws_sort, tp, depth, center, edge)
        pkg.svo_fuse_export_sorted(ws_sort, n, keys, idx)

        def replicated(pool, ws):
            pkg.svo_fuse_adopt_sorted(ws, keys, idx, depth)
            pkg.svo_fuse_plan(ws, n, depth, pool)
            pkg.svo_fuse_commit(ws, tc, depth, pool)

        replicated(ref, ws_ref)
        opool.insert_cloud(pts, col, depth, center, edge)
        # every frame cut by key range -- the first one into EMPTY replicas: all its splits start above the splitter level, every rank plans
        # the same top records and the apply ranks them in the ranks' union
        for r in range(world):
            pkg.svo_fuse_keyrange_commit(wss[r], keys, idx, tc, depth, reps[r], r, world, deltas[r])
        for r in range(world):
            pkg.svo_fuse_keyrange_apply(wss[r], keys, depth, reps[r], deltas)
            assert pkg.svo_fuse_keyrange_status(wss[r]) == 0
        sharded_frames += 1
        shared_records.append(max(int(d[13].item()) for d in deltas))
        used.append([int(d[pkg.KEYRANGE_USED_WORD].item()) * 4 for d in deltas])
        want = ref.words()
        assert np.array_equal(want, opool.words())
        for r in range(world):
            assert reps[r].size == ref.size, (f, r, reps[r].size, ref.size)
            got = reps[r].words()
            assert np.array_equal(got, want), (f, r, np.nonzero(got != want)[0][:10], shared_records)
        for eye, tgt, (w, h) in VIEWS[: 3 if f % 2 == 0 else 1]:
            view = oracle.look_at(eye, tgt, (0, 1, 0))
            a, ca = render(pkg, torch, ref, view, w, h, center, edge)
            b, cb = render(pkg, torch, reps[0], view, w, h, center, edge)
            assert np.array_equal(a, b) and ca == cb, (f, eye, describe_mismatch(b, a), ca, cb)
    assert sharded_frames == 7 and shared_records[0] > 0, shared_records     # (the first frame had records above the splitter level)
    for eye, tgt, (w, h) in VIEWS:   # the last replica has rendered nothing so far: six frames of marks at once
        view = oracle.look_at(eye, tgt, (0, 1, 0))
        a, ca = render(pkg, torch, ref, view, w, h, center, edge)
        b, cb = render(pkg, torch, reps[-1], view, w, h, center, edge)
        assert np.array_equal(a, b) and ca == cb, (eye, describe_mismatch(b, a), ca, cb)
        if depth <= 12:
            words = opool.words()
            o, steps, levels = oracle.cone_trace(words, w, h, 45.0, view, center, edge, 0)
            assert np.array_equal(a, o) and ca == [steps, levels]
    total = np.array(used).sum(1)
    print("world %d depth %d: %d key-range frames, records above the splitter level per frame (max over ranks) %s, delta bytes per frame all ranks: %s; per rank of the last frame: %s"
          % (world, depth, sharded_frames, shared_records, total.tolist(), used[-1]))
    assert total.max() < 64 * depth * n   # 8 bytes per touched node + 64 per new tile (these jittered clouds give nearly every key its own chain of new tiles) + 43 KB fixed per rank


@pytest.mark.parametrize("world", [2, 5, 16])
def test_keyrange_new_territory_above_the_splitter_level(env, oracle, world):
    """frames that split nodes ABOVE the splitter level -- an empty pool, then points in octants the map has never touched, then a cloud
    spread over the whole root -- are planned in part by several ranks at once (the same records, the same tiles); the union numbering
    puts them where the one-piece fusion does"""
    pkg, torch = env
    rng = np.random.default_rng(5)
    center, edge, depth, n = (0.0, 0.0, 0.0), 1.0, 10, 4000
    reps, wss, ws_sort = [pkg.Pool(1 << 20) for _ in range(world)], [pkg.Workspace() for _ in range(world)], pkg.Workspace()
    opool = oracle.Pool()
    corner = (rng.random((n, 3), dtype=np.float32) * np.float32(0.2) + np.float32(0.1)).astype(np.float32)      # one corner of one octant
    spread = (rng.random((n, 3), dtype=np.float32) * np.float32(1.9) - np.float32(0.95)).astype(np.float32)     # every octant of the root
    keys = torch.empty(n, dtype=torch.int64, device="cuda"); idx = torch.empty(n, dtype=torch.int32, device="cuda")
    deltas = [torch.zeros(pkg.KEYRANGE_FIXED_WORDS + 48 * n, dtype=torch.int32, device="cuda") for _ in range(world)]
    tops = []
    for f, pts in enumerate((corner, (-corner).astype(np.float32), spread, (spread * np.float32(0.5)).astype(np.float32))):
        col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
        pkg.svo_fuse_sort(ws_sort, tp, depth, center, edge)
        pkg.svo_fuse_export_sorted(ws_sort, n, keys, idx)
        for r in range(world):
            pkg.svo_fuse_keyrange_commit(wss[r], keys, idx, tc, depth, reps[r], r, world, deltas[r])
        tops.append(sorted(int(d[13].item()) for d in deltas))
        for r in range(world):
            pkg.svo_fuse_keyrange_apply(wss[r], keys, depth, reps[r], deltas)
            assert pkg.svo_fuse_keyrange_status(wss[r]) == 0
        opool.insert_cloud(pts, col, depth, center, edge)
        want = opool.words()
        for r in range(world):
            assert reps[r].size == opool.size, (f, r, reps[r].size, opool.size)
            got = reps[r].words()
            assert np.array_equal(got, want), (f, r, np.nonzero(got != want)[0][:10])
    print("world %d: records above the splitter level per rank and frame: %s" % (world, tops))
    assert tops[0][-1] > 0 and tops[1][-1] > 0 and tops[2][-1] >= 8      # every one of these frames exercised the union


@pytest.mark.parametrize("world,per_rank,w,h,depth", [(2, 2, 320, 240, 10), (4, 1, 320, 240, 10), (8, 1, 160, 120, 9)])
def test_keyrange_session_equals_single_gpu_session(world, per_rank, w, h, depth):
    """every rank of a frame-sharded session whose FUSION is cut by key range (pipeline "keyrange" exchange; an emulated rank takes the
    other ranks' pose records, sorted arrays and deltas from tables): poses and map replica equal the one-GPU session's after every call,
    the frames it ray-marches equal the one-GPU images.  Every frame, the first of the map included, is cut by key range."""
    import importlib
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    from test_gpu_sharded import _cam_state, _stream
    center, edge = (0.0, 1.5, 0.0), 4.096
    n1, n2, first = 7, 6, 0
    n = n1 + n2
    dstack, cstack = _stream(synth, torch, n, w, h)
    views = [pl.ground_truth_view(k, synth) for k in range(n)]
    A = pl.SlamPipeline(w, h, depth, center, edge)
    ref_img, ref_state = [], []
    for k in range(n):
        ref_img.append(A.frame(dstack[k], cstack[k], k, views[k]).cpu().numpy().copy())
        if k in (n1 - 1, n - 1):
            ref_state.append((A.pool.size, A.pool.words().copy(), _cam_state(A.cam, torch, pkg)))
    f = synth.focal_length(w)
    D = pkg.Camera(w, h, f, f)
    table = torch.zeros((n, pkg.DELTA_FLOATS), dtype=torch.float32, device="cuda")
    for k in range(1, n):
        D.pair_delta(dstack[k - 1], cstack[k - 1], dstack[k], cstack[k], table[k])
    tab_k = torch.empty((n, w * h), dtype=torch.int64, device="cuda")
    tab_i = torch.empty((n, w * h), dtype=torch.int32, device="cuda")
    scam, sws = pkg.Camera(w, h, f, f), pkg.Workspace()
    for k in range(n):
        scam.apply_delta(table[k], k)
        pkg.svo_fuse_sort_frame(sws, dstack[k], scam.fusion_transform_ptr(), f, f, depth, center, edge)
        pkg.svo_fuse_export_sorted(sws, w * h, tab_k[k], tab_i[k])
    torch.cuda.synchronize()
    for rank in range(world):
        deltas, shared, nbytes = pl.keyrange_delta_table(tab_k, tab_i, cstack, first, rank, world, depth, 1 << 22)
        B = pl.SlamPipeline(w, h, depth, center, edge, dist=pl.EmulatedRank(rank, world, exchange="keyrange"), pool_capacity_nodes=1 << 22)
        assert B.keyrange and B.shard_sort
        B.dist.expect_keyrange(deltas)
        for part, (lo, hi) in enumerate(((0, n1), (n1, n))):
            B.dist.expect(table[lo:hi], lo, per_rank, tab_k[lo:hi], tab_i[lo:hi])
            imgs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(lo, hi)]
            B.run_stream_sharded(list(dstack[lo:hi]), list(cstack[lo:hi]), list(range(lo, hi)), views[lo:hi], images=imgs, per_rank=per_rank)
            torch.cuda.synchronize()
            B.keyrange_check()
            size, words, state = ref_state[part]
            assert B.pool.size == size and np.array_equal(B.pool.words(), words), (rank, part)
            got = _cam_state(B.cam, torch, pkg)
            assert np.array_equal(got.view(np.uint32), state.view(np.uint32)), (rank, part)
            for k in range(lo, hi):
                if k % world == rank:
                    assert np.array_equal(imgs[k - lo].cpu().numpy(), ref_img[k]), (rank, k, describe_mismatch(imgs[k - lo].cpu().numpy(), ref_img[k]))
        assert B._kr["frames"] == n and B._kr["whole"] == 0
        if rank == 0:
            print("world %d %dx%d: %d frames cut by key range, records above the splitter level per frame %s; delta bytes of all ranks per frame: %s"
                  % (world, w, h, n, shared, [sum(b) for b in nbytes]))
        B.close()
    assert shared[0] > 0
