"""Frame-sharded sessions (exchange "deltas") on the GPU: a frame's ICP is a function of two depth
images, so svoslam_camera_pair_delta may run anywhere and svoslam_camera_apply_delta composes the poses.  Checked
against the ordinary tracker, the CPU oracle, and -- for whole sessions -- the one-GPU frame loop, with the ranks of a
2- and a 3-rank session run one after the other on the one GPU there is (each with its own pool, cameras and runner;
pipeline.EmulatedRank stands in for the all-gather: the other ranks' records come from a table)."""
import importlib
import os

import numpy as np
import pytest

from util import describe_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    return pkg, torch, synth, pl


def _stream(synth, torch, n, w, h):
    depth, rgb = synth.render_stream(n, w, h, device="cuda")
    return depth, rgb


def _cam_state(cam, torch, pkg):
    p, o = cam.pose()
    m = pkg.copy_from_device(cam.fusion_transform_ptr(), (16,), np.float32)
    return np.concatenate([p, o, m, [cam.tracking_lost_count()]]).astype(np.float32)


@pytest.mark.parametrize("w,h", [(320, 240), (640, 480)])
def test_pair_delta_then_apply_equals_update_and_oracle(env, oracle, w, h):
    """apply_delta(pair_delta(k-1, k)) == update(k): pose, fusion transform, lost count, bit for bit, through a frame
    that abandons every pyramid level; and == the oracle's update_trans per frame"""
    pkg, torch, synth, pl = env
    n = 7
    depth, rgb = _stream(synth, torch, n, w, h)
    depth[4] = 0            # no measurement: frames 4 and 5 abandon every level
    f = synth.focal_length(w)
    A, D, P = pkg.Camera(w, h, f, f), pkg.Camera(w, h, f, f), pkg.Camera(w, h, f, f)
    ocam = oracle.Camera(w, h, f, f)
    rec = torch.zeros((n, pkg.DELTA_FLOATS), dtype=torch.float32, device="cuda")
    for k in range(n):
        assert A.update(depth[k], rgb[k], k) == 1
        if k > 0:
            D.pair_delta(depth[k - 1], rgb[k - 1], depth[k], rgb[k], rec[k])
        assert P.apply_delta(rec[k] if k > 0 else None, k) == 1
        a, p = _cam_state(A, torch, pkg), _cam_state(P, torch, pkg)
        assert np.array_equal(a.view(np.uint32), p.view(np.uint32)), (k, a, p)
        ocam.update(depth[k].cpu().numpy().view(np.uint16), rgb[k].cpu().numpy(), k)
        if k > 0:
            r = rec[k].cpu().numpy()
            assert np.array_equal(r[:16].view(np.uint32), ocam.last_update().view(np.uint32)), k
        op, oo = ocam.pose()
        assert np.array_equal(p[3:12].view(np.uint32), oo.view(np.uint32)) and int(p[-1]) == ocam.tracking_lost_count()
    assert int(_cam_state(P, torch, pkg)[-1]) == 6
    # records do not depend on the order they are produced in, nor on what the scratch camera did before
    again = torch.zeros_like(rec)
    for k in (5, 2, 6, 1, 3, 4):
        D.pair_delta(depth[k - 1], rgb[k - 1], depth[k], rgb[k], again[k])
    assert torch.equal(rec.view(torch.int32)[1:], again.view(torch.int32)[1:])
    # stale timestamps are skipped like update() skips them; update() and apply_delta() do not mix on one camera
    assert P.apply_delta(rec[1], 3) == 0
    with pytest.raises(pkg.SvoslamError):
        A.apply_delta(rec[1], 100)
    with pytest.raises(pkg.SvoslamError):
        P.update(depth[0], rgb[0], 100)
    with pytest.raises(pkg.SvoslamError):
        P.pair_delta(depth[0], rgb[0], depth[1], rgb[1], again[0])


@pytest.mark.parametrize("sort_sharded", [True, False])
@pytest.mark.parametrize("world,per_rank,w,h,depth", [(2, 2, 320, 240, 10), (3, 1, 160, 120, 8), (4, 2, 320, 240, 10), (8, 1, 160, 120, 9)])
def test_sharded_session_equals_single_gpu_session(env, world, per_rank, w, h, depth, sort_sharded, monkeypatch):
    """every rank of a frame-sharded session: poses and map replica equal the one-GPU session's after every call, the
    frames it ray-marches equal the one-GPU images; across ranks every frame is marched exactly once.  Two calls (the
    second starts mid-stream: its first frame is tracked against the last frame of the first call)."""
    pkg, torch, synth, pl = env
    center, edge = (0.0, 1.5, 0.0), 4.096
    n1, n2 = 7, 6
    n = n1 + n2
    dstack, cstack = _stream(synth, torch, n, w, h)
    views = [pl.ground_truth_view(k, synth) for k in range(n)]
    # one-GPU session: images of all frames, pool and pose after each part
    A = pl.SlamPipeline(w, h, depth, center, edge)
    ref_img, ref_state = [], []
    for k in range(n):
        ref_img.append(A.frame(dstack[k], cstack[k], k, views[k]).cpu().numpy().copy())
        if k in (n1 - 1, n - 1):
            ref_state.append((A.pool.size, A.pool.words().copy(), _cam_state(A.cam, torch, pkg)))
    # the records a session would exchange
    f = synth.focal_length(w)
    D = pkg.Camera(w, h, f, f)
    table = torch.zeros((n, pkg.DELTA_FLOATS), dtype=torch.float32, device="cuda")
    for k in range(1, n):
        D.pair_delta(dstack[k - 1], cstack[k - 1], dstack[k], cstack[k], table[k])
    torch.cuda.synchronize()
    # sort_sharded (round 3): the owner of a frame also back-projects and SORTS it, the sorted keys / point indices are
    # all-gathered and every other rank adopts them (svoslam_runner_run_sharded_presorted); the table holds what the owners
    # would deliver -- sorted with the pose their own chain of apply_delta gives
    tab_k = tab_i = None
    if sort_sharded:
        tab_k = torch.empty((n, w * h), dtype=torch.int64, device="cuda")
        tab_i = torch.empty((n, w * h), dtype=torch.int32, device="cuda")
        scam, sws = pkg.Camera(w, h, f, f), pkg.Workspace()
        for k in range(n):
            scam.apply_delta(table[k], k)
            pkg.svo_fuse_sort_frame(sws, dstack[k], scam.fusion_transform_ptr(), f, f, depth, center, edge)
            pkg.svo_fuse_export_sorted(sws, w * h, tab_k[k], tab_i[k])
        torch.cuda.synchronize()
    marched = np.zeros(n, np.int32)
    monkeypatch.setenv("SVOSLAM_SHARD_SORT", "1" if sort_sharded else "0")   # (the default follows the image size)
    for rank in range(world):
        B = pl.SlamPipeline(w, h, depth, center, edge, dist=pl.EmulatedRank(rank, world))
        assert B.shard_sort == sort_sharded
        for part, (lo, hi) in enumerate(((0, n1), (n1, n))):
            B.dist.expect(table[lo:hi], lo, per_rank, tab_k[lo:hi] if sort_sharded else None, tab_i[lo:hi] if sort_sharded else None)
            imgs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(lo, hi)]
            B.run_stream_sharded(list(dstack[lo:hi]), list(cstack[lo:hi]), list(range(lo, hi)), views[lo:hi], images=imgs,
                                 per_rank=per_rank)
            torch.cuda.synchronize()
            size, words, state = ref_state[part]
            assert B.pool.size == size and np.array_equal(B.pool.words(), words), (rank, part)
            got = _cam_state(B.cam, torch, pkg)
            assert np.array_equal(got.view(np.uint32), state.view(np.uint32)), (rank, part, got, state)
            for k in range(lo, hi):
                if k % world == rank:
                    marched[k] += 1
                    assert np.array_equal(imgs[k - lo].cpu().numpy(), ref_img[k]), (rank, k, describe_mismatch(imgs[k - lo].cpu().numpy(), ref_img[k]))
                else:
                    assert int(imgs[k - lo].max()) == 0      # not this rank's frame: untouched
    assert (marched == 1).all()


def test_sharded_path_over_rccl_one_rank(env):
    """exchange "deltas" through torch.distributed (RCCL, one rank): run_stream == the single-GPU run_stream"""
    pkg, torch, synth, pl = env
    import torch.distributed as dist
    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29543")
        dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        w, h, depth, center, edge = 320, 240, 10, (0.0, 1.5, 0.0), 4.096
        n = 9
        dstack, cstack = _stream(synth, torch, n, w, h)
        views = [pl.ground_truth_view(k, synth) for k in range(n)]
        A = pl.SlamPipeline(w, h, depth, center, edge, count_steps=True)
        B = pl.SlamPipeline(w, h, depth, center, edge, count_steps=True, dist=pl.DistContext(0, 1, force=True, exchange="deltas"))
        for P in (A, B):
            P.run_stream(list(dstack[:5]), list(cstack[:5]), list(range(5)), views[:5])
            P.run_stream(list(dstack[5:]), list(cstack[5:]), list(range(5, n)), views[5:])
            torch.cuda.synchronize()
        assert np.array_equal(A.image.cpu().numpy(), B.image.cpu().numpy())
        assert A.pool.size == B.pool.size and np.array_equal(A.pool.words(), B.pool.words())
        assert np.array_equal(_cam_state(A.cam, torch, pkg).view(np.uint32), _cam_state(B.cam, torch, pkg).view(np.uint32))
        assert torch.equal(A.counters, B.counters) and int(A.counters[0]) > 0
        B.reset(); A.reset()
        for P in (A, B):
            P.run_stream(list(dstack[:4]), list(cstack[:4]), list(range(4)), views[:4])
            torch.cuda.synchronize()
        assert np.array_equal(A.image.cpu().numpy(), B.image.cpu().numpy()) and np.array_equal(A.pool.words(), B.pool.words())
    finally:
        if created:
            dist.destroy_process_group()


def _two_process_worker(rank, world, port, out_dir, n, w, h, depth, exchange="deltas"):
    """one rank of a REAL two-process frame-sharded session (both processes on the one GPU there is, so the process group
    is gloo -- RCCL refuses two ranks on one device; the schedule, the collectives' order and the library calls are those
    of the RCCL path)"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    os.environ["SVOSLAM_MAILBOX"] = "1"     # (opt-in since round 4)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    torch.cuda.set_device(0)
    center, edge = (0.0, 1.5, 0.0), 4.096
    dstack, cstack = synth.render_stream(n, w, h, device="cuda")
    views = [pl.ground_truth_view(k, synth) for k in range(n)]
    P = pl.SlamPipeline(w, h, depth, center, edge, dist=pl.DistContext(rank, world, exchange=exchange), pool_capacity_nodes=1 << 21)
    if P.dist.mailbox is not None:   # two processes time-sliced on one shared device: a wait may take seconds, not the default ~1 s
        P.dist.mailbox.set_wait_limit(1 << 28)
    imgs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
    half = n // 2 + 1
    P.run_stream_sharded(list(dstack[:half]), list(cstack[:half]), list(range(half)), views[:half], images=imgs[:half], per_rank=2)
    P.run_stream_sharded(list(dstack[half:]), list(cstack[half:]), list(range(half, n)), views[half:], images=imgs[half:], per_rank=2)
    torch.cuda.synchronize()
    kr = getattr(P, "_kr", None)
    if exchange == "keyrange":
        P.keyrange_check()
    p, o = P.cam.pose()
    mb = P.dist.mailbox      # the pose records travelled through the peer-to-peer mailbox (hipIpc between the two processes)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), words=P.pool.words(), size=P.pool.size, pos=p, ori=o,
             lost=P.cam.tracking_lost_count(), images=np.stack([i.cpu().numpy() for i in imgs]),
             mailbox=np.array([mb is not None, bool(mb.failed()) if mb is not None else False]),
             keyrange=np.array([kr["frames"], kr["whole"]] if kr else [0, 0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["deltas", "keyrange"])
def test_two_process_sharded_session_on_one_gpu(env, tmp_path, exchange):
    """two processes, one process group, frames tracked and marched alternately: each rank's replica and poses equal the
    one-GPU session's, rank r holds the images of the frames k % 2 == r.  exchange "keyrange": the fusion is cut by key range as well --
    a REAL all-gather of the two ranks' deltas per frame, from the first frame of the map on."""
    pkg, torch, synth, pl = env
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    n, w, h, depth = 11, 160, 120, 8
    mp.get_context("spawn")
    mp.spawn(_two_process_worker, args=(2, port, str(tmp_path), n, w, h, depth, exchange), nprocs=2, join=True)
    center, edge = (0.0, 1.5, 0.0), 4.096
    dstack, cstack = synth.render_stream(n, w, h, device="cuda")
    A = pl.SlamPipeline(w, h, depth, center, edge)
    ref = [A.frame(dstack[k], cstack[k], k, pl.ground_truth_view(k, synth)).cpu().numpy().copy() for k in range(n)]
    pa, oa = A.cam.pose()
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert bool(z["mailbox"][0]) and not bool(z["mailbox"][1]), (r, z["mailbox"])     # used, and no wait gave up
        assert int(z["size"]) == A.pool.size and np.array_equal(z["words"], A.pool.words()), r
        assert np.array_equal(z["pos"], pa) and np.array_equal(z["ori"], oa) and int(z["lost"]) == A.cam.tracking_lost_count()
        for k in range(n):
            if k % 2 == r:
                assert np.array_equal(z["images"][k], ref[k]), (r, k)
            else:
                assert int(z["images"][k].max()) == 0
        if exchange == "keyrange":
            assert int(z["keyrange"][0]) == n and int(z["keyrange"][1]) == 0, z["keyrange"]   # every frame cut by key range


def test_bench_multi_rank_code_path_on_one_gpu(env):
    """bench.py launched as the driver launches it for N = 2 and N = 4 (torch.distributed.run, one process per rank), all
    ranks on the one GPU there is over gloo (SVOSLAM_BENCH_ONE_DEVICE=1: RCCL refuses two ranks on a device): the default
    frame-sharded exchange runs end to end -- per-rank march counts, the max-over-ranks timing, one JSON line on rank 0.
    Not a measurement."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for nproc in (2, 4):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        envv = dict(os.environ, SVOSLAM_BENCH_ONE_DEVICE="1")
        out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                              "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                              "--gpus", str(nproc), "--steps", "12", "--warmup", "3", "--map-frames", "0", "--full", "--no-cpu-baseline"],
                             env=envv, capture_output=True, text=True, timeout=600)
        lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
        assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-800:], out.stderr[-1500:])
        j = json.loads(lines[0])
        assert j["n_gpus"] == nproc and j["steps"] == 12 and j["value"] > 0 and j["scaling"] == "strong"
        assert "update_trans" in j["config"]["parallelism"] and j["roofline"]["kernel_ms"] > 0
