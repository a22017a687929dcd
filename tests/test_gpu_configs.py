"""GPU parity at the exact sizes and geometries BASELINE.json's configs name (VERDICT r01 'configs_untested'):

  cfg4  1920x1080 RGB-D stream, depth-14 SVO, half-edge 8.192 m: every sensor kernel at 1080p, the ICP system with
        load_size = 20*1920/640 = 60 and its Q15 tail (localization_kernels.cu:303-326), the tracker, the fusion of
        a back-projected frame and whole frames incl. the raycast -- all bit-equal to the CPU oracle;
  cfg3  640x480, depth 12, centre (0,1.5,0), half-edge 4.096 m: whole frames at the exact geometry, and a long
        small-image run in which alpha saturates (>= 64 observations, Q10) so that reference-mode rays retire on
        real colour (Q9) instead of running to the range limit;
  cfg2  the reference's own objs/bunny_tex.obj + textures/texture1.bmp (committed as DATA fixtures under
        tests/data/): voxel list, node pool and three 640x480 cone-traced views against digests generated from the
        oracle by tests/golden/make_cfg2_golden.py, and against the live oracle.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

from util import cfg4_icp_maps, describe_mismatch, q15_bands, same_bits_or_nan

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CENTER = (0.0, 1.5, 0.0)


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    pl = importlib.import_module("octree_slam_amd.pipeline")
    return pkg, torch, synth, pl


def u16(t):
    return t.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ cfg4
W4, H4, D4, E4 = 1920, 1080, 14, 8.192


def test_cfg4_sensor_kernels_1080p(env, oracle):
    """bilateral, vertex / normal maps, the three-level pyramid and the bounding box at 1920x1080"""
    pkg, torch, synth, pl = env
    d, c = synth.render_frame(5, W4, H4)
    dn = d.numpy().view(np.uint16)
    f = synth.focal_length(W4)
    dd = d.cuda()
    out = torch.zeros((H4, W4), dtype=torch.int16, device="cuda")
    pkg.bilateral_filter(dd, out)
    ref = oracle.bilateral(dn)
    assert np.array_equal(u16(out), ref), describe_mismatch(u16(out), ref)
    # pyramid of the filtered depth (rgbd_camera.cpp:70-84): each level from the one above, maps at each level
    level, lw, lh = ref, W4, H4
    buf = out.clone()
    for lvl in range(3):
        v = torch.zeros((lh, lw, 3), dtype=torch.float32, device="cuda")
        n = torch.zeros((lh, lw, 3), dtype=torch.float32, device="cuda")
        pkg.generate_vertex_map(buf.view(-1)[: lw * lh].view(lh, lw), v, f, f, W4, H4)
        pkg.generate_normal_map(v, n)
        rv = oracle.vertex_map(level, f, f, W4, H4)
        rn = oracle.normal_map(rv)
        assert same_bits_or_nan(v.cpu().numpy(), rv), lvl
        assert same_bits_or_nan(n.cpu().numpy(), rn), lvl
        if lvl == 0:
            b0, b1 = pkg.point_cloud_bbox(v)
            r0, r1 = oracle.point_cloud_bbox(rv.reshape(-1, 3))
            assert np.array_equal(b0, r0) and np.array_equal(b1, r1)
        if lvl < 2:
            tmp = torch.zeros((lh // 2 * (lw // 2),), dtype=torch.int16, device="cuda")
            pkg.subsample_depth(buf, tmp, lw, lh)
            level = oracle.subsample_depth(level)
            lw, lh = lw // 2, lh // 2
            got = u16(buf).reshape(-1)[: lw * lh].reshape(lh, lw)
            assert np.array_equal(got, level), lvl


@pytest.mark.parametrize("w,h", [(1920, 1080), (960, 540), (480, 270), (1919, 1079)])
def test_cfg4_icp_cost2_load_size_60(env, oracle, w, h):
    """computeICPCost2 at the cfg4 pyramid sizes: load_size = 20*w/640 (60 at 1920, 30, 15; 59 for the ragged one),
    Q15: the d_A array has floor(n/load) entries while ceil(n/load) threads run -- the tail is excluded"""
    pkg, torch, synth, pl = env
    v1, n1, v2, n2 = cfg4_icp_maps(oracle, synth, w, h)   # (normals with a live last row: the tail of 1919x1079 could count)
    tens = [torch.from_numpy(x).cuda() for x in (v1, n1, v2, n2)]
    A, b = pkg.icp_cost2(*tens)
    rA, rb = oracle.icp_cost2(v1, n1, v2, n2)
    assert np.array_equal(A, rA) and np.array_equal(b, rb), (A - rA, b - rb)
    assert np.abs(A).max() > 0 and np.abs(b).max() > 0
    # 8 row bands (135 rows at 1080p) accumulate to the same exact sums
    acc = torch.zeros(27, dtype=torch.float64, device="cuda")
    for r in range(8):
        first, rows = pl.band_rows(h, r, 8)
        pkg.icp_accumulate(*tens, first * w, rows * w, acc)
    raw = oracle.icp_cost2_raw(v1, n1, v2, n2)
    assert np.array_equal(acc.cpu().numpy(), raw.astype(np.float64))
    # pixel bands, one ending inside the Q15 tail (1919x1079: 55 pixels of load 59) and one starting there
    for first, num in q15_bands(h, w):
        part = torch.zeros(27, dtype=torch.float64, device="cuda")
        pkg.icp_accumulate(*tens, first, num, part)
        assert np.array_equal(part.cpu().numpy(), oracle.icp_cost2_raw(v1, n1, v2, n2, first, num).astype(np.float64)), (first, num)


def test_cfg4_tracker_1080p(env, oracle):
    """RGBDCamera::update over 4 frames at 1920x1080: pose, last A / b / x and the fusion transform, bit for bit"""
    pkg, torch, synth, pl = env
    f = synth.focal_length(W4)
    cam, ocam = pkg.Camera(W4, H4, f, f), oracle.Camera(W4, H4, f, f)
    for k in range(4):
        d, c = synth.render_frame(k, W4, H4)
        assert cam.update(d.cuda(), c.cuda(), k) == ocam.update(d.numpy().view(np.uint16), c.numpy(), k) == 1
        p, o = cam.pose(); rp, ro = ocam.pose()
        assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)), (k, p, rp)
        assert np.array_equal(o.view(np.uint32), ro.view(np.uint32)), (k, o, ro)
        if k >= 1:
            A, b, x = cam.last_system(); rA, rb, rx = ocam.last_system()
            assert np.array_equal(A, rA) and np.array_equal(b, rb) and np.array_equal(x.view(np.uint32), rx.view(np.uint32)), k
        fus = pkg.copy_from_device(cam.fusion_transform_ptr(), (16,), np.float32)
        assert np.array_equal(fus.view(np.uint32), ocam.fusion_transform().view(np.uint32))
    assert cam.tracking_lost_count() == ocam.tracking_lost_count()


def _oracle_frame(oracle, ocam, opool, dn, cn, k, view, w, h, depth, center, edge, mode):
    f = 570.3 * w / 640.0
    ocam.update(dn, cn, k)
    v = oracle.vertex_map(dn, f, f, w, h)
    v = oracle.transform_vertex_map(v, ocam.fusion_transform())
    opool.insert_cloud(v.reshape(-1, 3), cn.reshape(-1, 3), depth, center, edge)
    img, steps, levels = oracle.cone_trace(opool, w, h, 45.0, view, center, edge, mode)
    return img, steps, levels


def _whole_frames(env, oracle, w, h, depth, edge, frames, mode, stride=1):
    """frame() on the device vs the oracle frame, every frame: pool words, image, pose, step / level counters; then the
    same frames through the four-stream native runner must reproduce the final state"""
    pkg, torch, synth, pl = env
    P = pl.SlamPipeline(w, h, depth, CENTER, edge, render_mode=mode, count_steps=True)
    ocam, opool = oracle.Camera(w, h, P.focal, P.focal), oracle.Pool()
    ds, cs, views = [], [], []
    tot_steps = tot_levels = 0
    for k in range(frames):
        d, c = synth.render_frame(stride * k, w, h)
        view = pl.ground_truth_view(stride * k, synth)
        dd, cc = d.cuda(), c.cuda()
        ds.append(dd); cs.append(cc); views.append(view)
        img = P.frame(dd, cc, k, view).cpu().numpy()
        rimg, steps, levels = _oracle_frame(oracle, ocam, opool, d.numpy().view(np.uint16), c.numpy(), k, view, w, h, depth,
                                            CENTER, edge, mode)
        tot_steps += steps; tot_levels += levels
        gw, cw = P.pool.words(), opool.words()
        assert P.pool.size == opool.size and np.array_equal(gw, cw), (k, describe_mismatch(gw, cw))
        assert np.array_equal(img, rimg), (k, describe_mismatch(img, rimg))
        p, o = P.cam.pose(); rp, ro = ocam.pose()
        assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)) and np.array_equal(o.view(np.uint32), ro.view(np.uint32)), k
        assert P.counters.tolist() == [tot_steps, tot_levels], (k, P.counters.tolist(), tot_steps, tot_levels)
    last = img
    final_words = gw
    Q = pl.SlamPipeline(w, h, depth, CENTER, edge, render_mode=mode, count_steps=True)
    Q.run_stream(ds, cs, list(range(frames)), views)
    torch.cuda.synchronize()
    assert hasattr(Q, "_runner")
    assert np.array_equal(Q.image.cpu().numpy(), last)
    assert Q.pool.size == opool.size and np.array_equal(Q.pool.words(), final_words)
    assert Q.counters.tolist() == [tot_steps, tot_levels]
    return P, opool


@pytest.mark.parametrize("mode", [1, 0])
def test_cfg4_whole_frames_1080p_depth14(env, oracle, mode):
    """BASELINE config 4 on one GPU: 1920x1080, depth 14, centre (0,1.5,0), half-edge 8.192 m"""
    _whole_frames(env, oracle, W4, H4, D4, E4, 3 if mode == 1 else 2, mode)


def test_cfg4_fusion_properties_full_size(env, oracle):
    """fusion of a back-projected 1080p frame at depth 14: the asynchronous, the blocking and the phased entry points
    give the same pool; inserting the same cloud twice only changes leaf colours / alpha and the Q4 splits"""
    pkg, torch, synth, pl = env
    f = synth.focal_length(W4)
    d, c = synth.render_frame(7, W4, H4, device="cuda")
    pts = torch.zeros((H4, W4, 3), dtype=torch.float32, device="cuda")
    pkg.generate_vertex_map(d, pts, f, f, W4, H4)
    pts, col = pts.view(-1, 3), c.view(-1, 3)
    pools = []
    for variant in range(3):
        ws, pool = pkg.Workspace(), pkg.Pool(1 << 20)
        for rep in range(2):
            if variant == 0:
                pkg.svo_from_point_cloud(ws, pts, col, D4, pool, CENTER, E4)
            elif variant == 1:
                pkg.svo_from_point_cloud_async(ws, pts, col, D4, pool, CENTER, E4)
            else:
                pkg.svo_fuse_sort(ws, pts, D4, CENTER, E4)
                pkg.svo_fuse_plan(ws, pts.shape[0], D4, pool)
                pkg.svo_fuse_commit(ws, col, D4, pool)
        pools.append(pool.words())
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])
    opool = oracle.Pool()
    pn, cn = pts.cpu().numpy(), col.cpu().numpy()
    for rep in range(2):
        opool.insert_cloud(pn, cn, D4, CENTER, E4)
    assert np.array_equal(pools[0], opool.words())


# ------------------------------------------------------------------------------------------------ cfg3
def test_cfg3_whole_frames_exact_geometry(env, oracle):
    """BASELINE config 3: 640x480, depth 12, centre (0,1.5,0), half-edge 4.096 m (leaf half-edge 1 mm)"""
    _whole_frames(env, oracle, 640, 480, 12, 4.096, 4, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_cfg3_alpha_saturation_long_run(env, oracle, mode):
    """72 frames of the config-3 stream at 96x72 into a depth-6 tree (12.8 cm leaves: every leaf in view is observed on
    every frame), so alpha reaches 255 (127 + 2 x 64, svo.cu:332) and reference-mode rays start to retire on a
    saturated node (cone_tracing_kernels.cu:108-121, Q9 / Q10) -- the regime the 300-frame config lives in.  Image,
    pool, pose and counters bit-equal on every frame."""
    pkg, torch, synth, pl = env
    w, h, depth, edge, frames = 96, 72, 6, 4.096, 72
    P = pl.SlamPipeline(w, h, depth, CENTER, edge, render_mode=mode)
    ocam, opool = oracle.Camera(w, h, P.focal, P.focal), oracle.Pool()
    saturated_seen = False
    coloured = 0
    for k in range(frames):
        d, c = synth.render_frame(k, w, h)
        view = pl.ground_truth_view(k, synth)
        img = P.frame(d.cuda(), c.cuda(), k, view).cpu().numpy()
        rimg, _, _ = _oracle_frame(oracle, ocam, opool, d.numpy().view(np.uint16), c.numpy(), k, view, w, h, depth, CENTER, edge, mode)
        assert np.array_equal(img, rimg), (k, describe_mismatch(img, rimg))
        if k % 8 == 7 or k == frames - 1:
            gw, cw = P.pool.words(), opool.words()
            assert np.array_equal(gw, cw), (k, describe_mismatch(gw, cw))
            saturated_seen = saturated_seen or bool(((cw[1::2] >> 24) >= 254).any())
        coloured = int((rimg[..., :3].max(-1) > 0).sum())
    assert saturated_seen                      # alpha did saturate
    assert coloured > w * h // 4               # and the last image is not degenerate
    o, ro = P.cam.pose()[1], ocam.pose()[1]
    assert np.array_equal(o.view(np.uint32), ro.view(np.uint32))


# ------------------------------------------------------------------------------------------------ cfg1
def test_cfg1_cube_obj(env, oracle):
    """BASELINE config 1 on the reference's own objs/cube.obj (tests/data/cube.obj): Scene::loadObjFile ->
    voxelizeMeshes at 2^5 -> depth-5 SVO -> one 256x256 render from the view of SURVEY 8d.1, both render modes, against the
    digests of the oracle's host walk (tests/golden/cfg1_cube.json, tests/golden/make_cfg1_golden.py)."""
    pkg, torch, synth, pl = env
    gold = json.load(open(os.path.join(HERE, "golden", "cfg1_cube.json")))
    obj = os.path.join(HERE, "data", "cube.obj")
    scene = pkg.Scene()
    scene.load_obj(obj)
    scene.voxelize_meshes(octree=True, log_n=5)
    mesh = pkg.Mesh(obj)
    ce, co, idx, scale = pkg.mesh_to_voxel_grid(pkg.Workspace(), mesh, None, 5)
    assert mesh.n_tris == gold["n_tris"] == 12 and len(idx) == gold["n_voxels"]
    assert _sha(idx.astype(np.int64)) == gold["voxel_index_sha256"]
    assert _sha(ce.cpu().numpy()) == gold["voxel_centers_sha256"] and _sha(co.cpu().numpy()) == gold["voxel_colors_sha256"]
    svo = scene.svo()
    assert svo["num_nodes"] == gold["num_nodes"] and svo["max_depth"] == 5
    assert [float(v) for v in svo["center"]] == gold["center"] and svo["size"] == gold["size"]
    assert _sha(scene.pool_words()) == gold["pool_sha256"]
    view = oracle.look_at((0.0, 0.1, -0.6), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0))
    for mode in (0, 1):
        img = torch.zeros((256, 256, 4), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        pkg.cone_trace_svo(img, 45.0, view, svo["data_ptr"], svo["center"], svo["size"], mode, cnt)
        assert cnt.tolist() == gold["image_steps_levels"][mode], mode
        assert _sha(img.cpu().numpy()) == gold["images_sha256"][mode], mode


# ------------------------------------------------------------------------------------------------ cfg2
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cfg2_views(center):
    c = np.asarray(center, np.float64)
    return [tuple(c + np.array(o)) for o in ((0.2, 0.3, -2.0), (1.7, 0.0, 0.2), (0.0, 0.02, -0.35))]


def test_cfg2_bunny_tex(env, oracle):
    """BASELINE config 2: bunny_tex.obj + texture1.bmp -> 2^10 voxel grid -> depth-10 SVO -> 640x480 cone trace from
    three views.  The bunny's AABB is not a cube (anisotropic voxels, voxel centres outside the root cube clamp into
    boundary leaves, several voxels per leaf: R1 / R12 under load)."""
    pkg, torch, synth, pl = env
    obj = os.path.join(HERE, "data", "bunny_tex.obj")
    bmp = os.path.join(HERE, "data", "texture1.bmp")
    gold = json.load(open(os.path.join(HERE, "golden", "cfg2_bunny.json")))
    log_n = 10
    scene = pkg.Scene()
    scene.load_obj(obj)
    scene.load_bmp(bmp)
    scene.voxelize_meshes(octree=True, log_n=log_n)
    # the voxel list itself (index order, centres, colours) through the kernel entry point
    mesh, tex = pkg.Mesh(obj), pkg.Texture(bmp)
    ce, co, idx, scale = pkg.mesh_to_voxel_grid(pkg.Workspace(), mesh, tex, log_n)
    assert mesh.n_tris == gold["n_tris"] == 4968
    assert len(idx) == gold["n_voxels"]
    assert _sha(idx.astype(np.int64)) == gold["voxel_index_sha256"]
    assert _sha(ce.cpu().numpy()) == gold["voxel_centers_sha256"]
    assert _sha(co.cpu().numpy()) == gold["voxel_colors_sha256"]
    svo = scene.svo()
    assert svo["num_nodes"] == gold["num_nodes"] and svo["max_depth"] == log_n
    assert [float(v) for v in svo["center"]] == gold["center"] and svo["size"] == gold["size"]
    words = scene.pool_words()
    assert _sha(words) == gold["pool_sha256"]
    center, size = svo["center"], svo["size"]
    imgs = []
    for vi, eye in enumerate(cfg2_views(center)):
        view = oracle.look_at(eye, tuple(np.asarray(center, np.float64)), (0, 1, 0))
        for mode in (0, 1):
            img = torch.zeros((480, 640, 4), dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
            pkg.cone_trace_svo(img, 45.0, view, svo["data_ptr"], center, size, mode, cnt)
            got = img.cpu().numpy()
            assert cnt.tolist() == gold["image_steps_levels"][vi][mode], (vi, mode)   # the whole traversal, sample by sample
            assert _sha(got) == gold["images_sha256"][vi][mode], (vi, mode)
            imgs.append(got)
    # a once-voxelized mesh has A = 129 everywhere (alpha 2 per sample, Q10): outside views are nearly black in the
    # reference too; the close-up (third view, carry mode) accumulates colour
    assert (imgs[5][..., :3].max(-1) > 0).sum() > 100000
    # and against the live oracle (same digests by construction of the golden file; this localises a mismatch)
    omesh, otex = oracle.mesh_load_obj(obj), oracle.load_bmp(bmp)
    rce, rco, ridx = oracle.mesh_to_voxel_grid(omesh, otex, log_n)
    assert np.array_equal(idx.astype(np.int64), ridx)
    opool = oracle.Pool()
    opool.insert_voxel_grid(rce, rco, log_n, center, float(size))
    assert np.array_equal(words, opool.words()), describe_mismatch(words, opool.words())
