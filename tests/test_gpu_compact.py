"""svoslam_pool_compact / svoslam_pool_graft_subtree on the device, bit for bit against the host restatement of their
specification (tests/test_compact_cpu.py: compact_words / graft_words), oracle/formats.py and the CPU oracle -- never
against a second HIP pool alone."""
import importlib

import numpy as np
import pytest

from test_compact_cpu import FLAG, MASK, compact_words, graft_words
from util import surface_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    return pkg, torch, synth, pl


CENTER, EDGE = (0.05, -0.02, 0.01), 1.0
# the status in SvoslamError's text: the refusals below are pinned to the status the specification names
ERR_FORMAT, ERR_INVALID_ARG = r"status -9 \(file format", r"status -1 \(invalid argument"


def fuse_clouds(pkg, torch, pool, ws, seed, n, depth, center=CENTER, edge=EDGE, opool=None, points=12000):
    rng = np.random.default_rng(seed)
    for k in range(n):
        pts, col = surface_cloud(rng, points)
        pts = pts + np.float32(0.01 * k)
        pkg.svo_from_point_cloud_async(ws, torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda(), depth, pool, center, edge)
        if opool is not None:
            opool.insert_cloud(pts, col, depth, center, edge)


def tile_levels(words):
    """tile levels below (and including) the root tile"""
    levels, level = 0, [0]
    while level:
        levels += 1
        level = [int(words[2 * (t + j)]) & MASK for t in level for j in range(8) if int(words[2 * (t + j)]) & FLAG]
    return levels


def render(pkg, torch, pool, center, edge, mode, w=64, h=48, eye=(0.1, 0.2, -2.5)):
    from oracle import oracle as ora
    view = ora.look_at(eye, (0, 0, 0), (0, 1, 0))
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    pkg.cone_trace_svo(img, 45.0, view, pool.data_ptr, center, edge, mode, counters=cnt)
    return img.cpu().numpy(), cnt.cpu().tolist()


@pytest.mark.parametrize("shrink", [False, True])
@pytest.mark.parametrize("case", ["fresh", "fused", "expanded", "evicted"])
def test_compact_equals_the_restatement(env, oracle, tmp_path, case, shrink):
    from oracle import formats as fm
    pkg, torch = env[0], env[1]
    ws, pool = pkg.Workspace(), pkg.Pool()
    if case != "fresh":
        fuse_clouds(pkg, torch, pool, ws, 7, 3, 9)
    if case == "expanded":
        pool.expand(CENTER, EDGE, toward=(-3.0, 4.0, 0.5))
    if case == "evicted":
        tree = fm.pull_to_cpu(pool.words())
        tops = [k for k in range(8) if tree[k][1] is not None]
        inner = next(k for k in range(8) if tree[tops[1]][1][k][1] is not None)
        pool.evict_subtree([tops[0]], tmp_path / "a.svosub")                 # a one-level and a two-level path
        pool.evict_subtree([tops[1], inner], tmp_path / "b.svosub")
    before = pool.words().copy()
    cap_before = pool.capacity
    want, want_map = compact_words(before, want_map=True)
    stats, old_tile = pool.compact(1 if shrink else 0, want_map=True)
    after = pool.words()
    assert np.array_equal(after, want)
    size_after = want.size // 2
    assert stats == {"size_before": before.size // 2, "size_after": size_after, "capacity_before": cap_before,
                     "capacity_after": size_after if shrink else cap_before, "levels": tile_levels(before),
                     "tiles_dropped": (before.size - want.size) // 16}
    assert pool.size == size_after and pool.capacity == stats["capacity_after"]
    if case == "fresh":
        assert size_after == 8 and stats["levels"] == 1
    if case == "evicted":
        dropped = sum(fm.read_subtree_file(tmp_path / f)["tiles"].size for f in ("a.svosub", "b.svosub"))
        assert stats["tiles_dropped"] == dropped > 0
    # the old-tile map: new tile k == old tile map[k] up to re-pointed word0
    m = old_tile.cpu().numpy().astype(np.uint32)
    assert np.array_equal(m, want_map)
    new_t = after.reshape(-1, 8, 2)
    old_t = before.reshape(-1, 8, 2)[m // 8]
    assert np.array_equal(new_t[:, :, 1], old_t[:, :, 1])
    flagged = (old_t[:, :, 0] & FLAG) != 0
    assert np.array_equal((new_t[:, :, 0] & FLAG) != 0, flagged)
    assert np.array_equal(new_t[:, :, 0][~flagged], old_t[:, :, 0][~flagged])
    assert np.array_equal(m[(new_t[:, :, 0][flagged] & MASK) // 8], old_t[:, :, 0][flagged] & MASK)


def test_a_compacted_map_is_the_same_map(env, oracle):
    pkg, torch = env[0], env[1]
    center, edge, depth = CENTER, EDGE, 9
    ws, pool = pkg.Workspace(), pkg.Pool()
    fuse_clouds(pkg, torch, pool, ws, 23, 3, depth)
    rng = np.random.default_rng(5)
    pts, col = surface_cloud(rng, 12000, jitter=0.001)
    tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
    for _ in range(66):                                   # saturated leaves: the model-depth raycast has something to answer
        pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, center, edge)
    f = 570.3 * 160 / 640.0
    cam = np.zeros(16, np.float32)
    cam[0], cam[5], cam[10], cam[15] = 1.0, 1.0, 1.0, 1.0
    cam[12:15] = (0.1, 0.2, -2.6)

    def observe():
        out = {}
        for bricks in (1, 0):
            prev = pkg.configure(march_bricks=bricks)
            try:
                for mode in (pkg.RENDER_REFERENCE, pkg.RENDER_CARRY):
                    out[(bricks, mode)] = render(pkg, torch, pool, center, edge, mode, 96, 72)
            finally:
                pkg.configure(march_bricks=prev["march_bricks"])
        render(pkg, torch, pool, center, edge, pkg.RENDER_REFERENCE, 96, 72)
        assert pool.march_accel()["bricks"] == 1          # the brick march is in use (again)
        md = torch.zeros((120, 160), dtype=torch.int16, device="cuda")
        pkg.raycast_model_depth(md, f, f, pool.data_ptr, center, edge, cam_to_world=cam)
        out["model"] = md.cpu().numpy()
        out["grid"] = pkg.extract_voxel_grid(ws, pool, depth, center, edge)
        return out

    a = observe()
    before = pool.words().copy()
    stats = pool.compact()
    assert stats["size_after"] == stats["size_before"]    # nothing was unreachable: the numbering is all that changed
    assert np.array_equal(pool.words(), compact_words(before))
    b = observe()
    for key in [(br, mode) for br in (1, 0) for mode in (pkg.RENDER_REFERENCE, pkg.RENDER_CARRY)]:
        assert a[key][0].any() and np.array_equal(a[key][0], b[key][0]) and a[key][1] == b[key][1], key
    assert (a["model"] != 0).any() and np.array_equal(a["model"], b["model"])
    assert a["grid"][0].shape[0] > 0
    assert np.array_equal(a["grid"][0], b["grid"][0]) and np.array_equal(a["grid"][1], b["grid"][1])
    for mode, omode in ((pkg.RENDER_REFERENCE, oracle.RENDER_REFERENCE), (pkg.RENDER_CARRY, oracle.RENDER_CARRY)):
        view = oracle.look_at((0.1, 0.2, -2.5), (0, 0, 0), (0, 1, 0))
        ref, steps, levels = oracle.cone_trace(compact_words(before), 96, 72, 45.0, view, center, edge, omode)
        assert np.array_equal(b[(1, mode)][0], ref) and b[(1, mode)][1] == [steps, levels]


def test_the_session_goes_on(env, oracle):
    from oracle import formats as fm
    pkg, torch = env[0], env[1]
    center, edge, depth = CENTER, EDGE, 9
    A, B = pkg.Pool(), pkg.Pool()
    wsa, wsb = pkg.Workspace(), pkg.Workspace()
    fuse_clouds(pkg, torch, A, wsa, 41, 2, depth)
    fuse_clouds(pkg, torch, B, wsb, 41, 2, depth)
    before = A.words().copy()
    assert np.array_equal(before, B.words())
    stats = A.compact(1)
    assert stats["capacity_after"] == stats["size_after"] == A.capacity
    O = oracle.Pool()
    O.load_words(compact_words(before))
    rng = np.random.default_rng(43)
    for how in ("async", "phased", "deferred"):
        pts, col = surface_cloud(rng, 12000)
        pts = pts + np.float32(0.03)
        tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
        for ws, pool in ((wsa, A), (wsb, B)):
            if how == "async":
                pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, center, edge)
                continue
            pkg.svo_fuse_sort(ws, tp, depth, center, edge)
            pkg.svo_fuse_plan(ws, len(pts), depth, pool)
            if how == "phased":
                pkg.svo_fuse_commit(ws, tc, depth, pool)
            else:
                pkg.svo_fuse_commit_deferred(ws, tc, depth, pool)
                pkg.svo_fuse_apply(ws, pool)
        O.insert_cloud(pts, col, depth, center, edge)
    wa, wb = A.words(), B.words()
    assert A.size == O.size and np.array_equal(wa, O.words())      # the compacted map fused on == the oracle doing the same
    assert fm.pull_to_cpu(wa) == fm.pull_to_cpu(wb)
    for mode in (pkg.RENDER_REFERENCE, pkg.RENDER_CARRY):
        ia, ca = render(pkg, torch, A, center, edge, mode)
        ib, cb = render(pkg, torch, B, center, edge, mode)
        assert ia.any() and np.array_equal(ia, ib) and ca == cb
    A.compact()
    B.compact()
    assert np.array_equal(A.words(), B.words())                   # the canonical form: the same tree is the same bytes
    assert np.array_equal(A.words(), compact_words(wb))


def test_a_plan_does_not_survive_a_compaction(env, oracle):
    """svo_fuse_plan leaves node indices of the numbering it read in the workspace: its commit is refused after a compaction
    (not written at stale indices, which may lie beyond a shrunk allocation), and a fresh plan goes through -- as a
    deferred commit, whose shadow words were sized for the capacity before the shrink."""
    pkg, torch = env[0], env[1]
    center, edge, depth = CENTER, EDGE, 9
    A, ws = pkg.Pool(), pkg.Workspace()
    fuse_clouds(pkg, torch, A, ws, 51, 2, depth)
    rng = np.random.default_rng(53)
    clouds = []
    for k in range(2):
        pts, col = surface_cloud(rng, 12000)
        clouds.append((pts + np.float32(0.02 * (k + 1)), col))
    tp, tc = torch.from_numpy(clouds[0][0]).cuda(), torch.from_numpy(clouds[0][1]).cuda()
    pkg.svo_fuse_sort(ws, tp, depth, center, edge)
    pkg.svo_fuse_plan(ws, len(tp), depth, A)
    pkg.svo_fuse_commit_deferred(ws, tc, depth, A)                 # allocates the shadow words for the present capacity
    pkg.svo_fuse_apply(ws, A)
    before = A.words().copy()
    tp, tc = torch.from_numpy(clouds[1][0]).cuda(), torch.from_numpy(clouds[1][1]).cuda()
    pkg.svo_fuse_sort(ws, tp, depth, center, edge)
    pkg.svo_fuse_plan(ws, len(tp), depth, A)
    stats = A.compact(1)
    assert stats["capacity_after"] == stats["size_after"] < stats["capacity_before"]
    expected = compact_words(before)
    with pytest.raises(pkg.SvoslamError, match=ERR_INVALID_ARG):
        pkg.svo_fuse_commit(ws, tc, depth, A)
    assert np.array_equal(A.words(), expected)
    O = oracle.Pool()
    O.load_words(expected)
    O.insert_cloud(clouds[1][0], clouds[1][1], depth, center, edge)
    pkg.svo_fuse_sort(ws, tp, depth, center, edge)
    pkg.svo_fuse_plan(ws, len(tp), depth, A)
    pkg.svo_fuse_commit_deferred(ws, tc, depth, A)
    pkg.svo_fuse_apply(ws, A)
    assert A.size == O.size and np.array_equal(A.words(), O.words())


def test_paging_gives_memory_back(env, oracle, tmp_path):
    from oracle import formats as fm
    pkg, torch = env[0], env[1]
    rng = np.random.default_rng(31)
    depth, center, edge = 8, (0, 0, 0), 1.0

    def cloud(lo, hi, n):
        p = (rng.random((n, 3)) * (np.array(hi) - np.array(lo)) + np.array(lo)).astype(np.float32)
        return torch.from_numpy(p).cuda(), torch.from_numpy(rng.integers(0, 256, (n, 3), dtype=np.uint8)).cuda()

    left = [cloud((-0.9, -0.9, -0.9), (-0.1, 0.9, 0.9), 30000) for _ in range(8)]      # x < 0: octants with bit 0 clear
    right = [cloud((0.1, -0.9, -0.9), (0.9, 0.9, 0.9), 30000) for _ in range(2)]       # x > 0

    def fuse(pools, c):
        for ws, p in pools:
            pkg.svo_from_point_cloud_async(ws, c[0], c[1], depth, p, center, edge)

    A, B, N, D = [(pkg.Workspace(), pkg.Pool()) for _ in range(4)]     # B: never paged; N: paged, never compacted; D: fused into
    everyone = [A, B, N, D]
    fuse(everyone, left[0]); fuse(everyone, right[0])
    path, f = [1], tmp_path / "sub.svosub"                             # root child 1 = (x > 0, y < 0, z < 0)
    A[1].evict_subtree(path, f)
    sub = fm.read_subtree_file(f)
    N[1].evict_subtree(path, tmp_path / "n.svosub")
    D[1].evict_subtree(path, tmp_path / "d.svosub")
    fuse([A, B, N], left[1])                                           # fuse elsewhere
    size_paged = A[1].size
    stats = A[1].compact(1)
    assert stats["size_before"] == size_paged and size_paged - stats["size_after"] == 8 * sub["tiles"].size
    assert stats["capacity_after"] == stats["size_after"] == A[1].capacity == A[1].size
    k = 2
    while A[1].size < sub["pool_size"] + 8 * sub["tiles"].size:       # until the pool has outgrown the file's pool_size
        assert k < len(left), "the map stopped growing"
        fuse([A, B], left[k])
        k += 1
    assert A[1].size >= sub["pool_size"]
    held = A[1].words().copy()
    with pytest.raises(pkg.SvoslamError, match=ERR_FORMAT):            # the slots the file names belong to other nodes now
        A[1].restore_subtree(f)
    assert np.array_equal(A[1].words(), held)
    A[1].graft_subtree(f)
    assert np.array_equal(A[1].words(), graft_words(held, sub))
    assert fm.pull_to_cpu(A[1].words()) == fm.pull_to_cpu(B[1].words())
    for mode in (pkg.RENDER_REFERENCE, pkg.RENDER_CARRY):
        ia, ca = render(pkg, torch, A[1], center, edge, mode)
        ib, cb = render(pkg, torch, B[1], center, edge, mode)
        assert ia.any() and np.array_equal(ia, ib) and ca == cb
    fuse([A, B], right[1])                                             # and the map goes on, into the grafted cube
    assert fm.pull_to_cpu(A[1].words()) == fm.pull_to_cpu(B[1].words())
    # a never-compacted pool: the same call, the same rule
    held = N[1].words().copy()
    N[1].graft_subtree(tmp_path / "n.svosub")
    assert np.array_equal(N[1].words(), graft_words(held, fm.read_subtree_file(tmp_path / "n.svosub")))
    fuse([D], left[1])
    N_tree = fm.pull_to_cpu(N[1].words())
    D[1].restore_subtree(tmp_path / "d.svosub")                        # (the old way back still works where nothing was compacted)
    assert N_tree == fm.pull_to_cpu(D[1].words())
    # fused into while it was out: refused, pool untouched
    D[1].evict_subtree(path, tmp_path / "d2.svosub")
    fuse([D], right[1])
    held = D[1].words().copy()
    with pytest.raises(pkg.SvoslamError, match=ERR_INVALID_ARG):
        D[1].graft_subtree(tmp_path / "d2.svosub")
    assert np.array_equal(D[1].words(), held)


def test_frame_loop_over_a_compaction(env):
    from oracle import formats as fm
    pkg, torch, synth, pl = env
    w, h, depth, center, edge, k = 160, 120, 8, (0.0, 1.5, 0.0), 4.096, 4
    frames = [synth.render_frame(i, w, h, device="cuda") for i in range(2 * k)]
    views = [pl.ground_truth_view(i, synth) for i in range(2 * k)]
    ds, cs = [f[0] for f in frames], [f[1] for f in frames]
    A = pl.SlamPipeline(w, h, depth, center, edge)
    B = pl.SlamPipeline(w, h, depth, center, edge)
    for P in (A, B):
        P.run_stream(ds[:k], cs[:k], list(range(k)), views[:k])
    torch.cuda.synchronize()
    before = A.pool.words().copy()
    A.pool.compact(1)
    assert np.array_equal(A.pool.words(), compact_words(before))
    for P in (A, B):
        P.run_stream(ds[k:], cs[k:], list(range(k, 2 * k)), views[k:])      # the same runner goes on
    torch.cuda.synchronize()
    assert A.image.any() and torch.equal(A.image, B.image)
    pa, oa = A.cam.pose(); pb, ob = B.cam.pose()
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(oa.view(np.uint32), ob.view(np.uint32))
    assert A.pool.size == B.pool.size
    assert fm.pull_to_cpu(A.pool.words()) == fm.pull_to_cpu(B.pool.words())


def test_malformed_foreign_pool_is_refused(env):
    """an error RETURN: the host-side cap on the tiles visited ends the walk of a cyclic pool after size / 8 tiles"""
    pkg = env[0]
    w = np.zeros(32, dtype=np.uint32)
    w[0] = FLAG | 8
    w[1] = w[17] = 0x7F102030
    w[16] = FLAG | 0                                       # node 8 points back at tile 0
    pool = pkg.Pool()
    pool.set_words(w)
    with pytest.raises(pkg.SvoslamError, match=ERR_FORMAT):
        pool.compact()
    assert pool.size == 16 and np.array_equal(pool.words(), w)
    with pytest.raises(ValueError):
        compact_words(w)
