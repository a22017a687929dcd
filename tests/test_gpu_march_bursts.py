"""The brick march's bursts (csrc/cone_trace.hip cone_trace_brick_kernel, phase 2: place / request / answer / burst) from the FIRST
step on, at every burst alignment, and the general LOD form of both march kernels.

At the default svoslam_config.march_ahead = 60 the burst code begins sixty steps from the eye, where cones are coarse: it answers
almost only pyramid samples (tests/test_march_bursts_cpu.py holds the numbers).  Here every scene of tests/march_scenes.py is
rendered with march_ahead in {-1, 0, 2, 3, 7, 60}: bursts off, bursts from step 2 on (0), and four alignments of the bursts
against the rays' ends.  Every render is compared with the CPU oracle byte for byte, its [steps, levels] counters with the
oracle's, and its per-pixel step counts (mode bit 0x100) with the lengths of the reference's rays (march_scenes.trace): a burst
that double-counts or drops a discarded sample shows per ray where the totals can cancel.  The maps: the surface cloud of
tests/test_gpu_bricks.py at depth 12 and 14 (both brick shapes), young, saturated by fusion and saturated by hand at every
level from 4 down; a dense patch on which walks END on the bricks' deepest levels (the surface cloud is too sparse for that);
and the node-0 scenes, whose rays run through LODs <= 0.

Fields of view: no other test renders with anything but 45 degrees.  20 and 70 are ordinary.  0, 180, -45 (a zero or negative
pixel scale), 1e-30, 1e-33, 1e-37 (pixel sizes tens of binades below the root cube's size) make the host clear `lod_always`, so
the four LOD_ALWAYS = false instantiations of the brick kernel run, every sample on the rare path with step_lod; the same
renders through cone_trace_kernel (foreign memory, carry mode, a depth-16 pool) take its fallback.  The three tiny positive
values go through three branches of step_lod -- ordinary operands, a subnormal pixel size, a zero or infinite quotient -- but
every LOD they produce is deeper than the tree: they prove that those branches agree with the oracle's walk and do nothing
worse, they do not pin the LOD's value.

Not tested: the `full_form` branches of the brick kernel (a level below -60).  The host sends that kernel only root cubes of
2^-20 .. 2^20 metres, whose LODs over ray lengths up to the 10 m range stay far above -60."""
import numpy as np
import pytest

import march_scenes as M
import node0_scenes as S
from util import configured, describe_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def render(env, ptr, fov, vm, w, h, center, edge, mode=0):
    """(image, [steps, levels]) of one render; mode bit 0x100: the pixel is the ray's step count -> (steps [h, w], None)"""
    pkg, torch = env
    img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
    if mode & 0x100:
        pkg.cone_trace_svo(img, fov, vm, ptr, center, edge, mode)
        return img.cpu().numpy().view(np.uint32).reshape(h, w).astype(np.int64), None
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    pkg.cone_trace_svo(img, fov, vm, ptr, center, edge, mode, counters=cnt)
    return img.cpu().numpy(), cnt.cpu().tolist()


# ---- pools: one alive at a time (a pool with bricks holds the 16 GiB field) ---------------------------------------------------
_LIVE = {}


def words_key(name):
    return name if name in M.BRICK_MAPS else {n: k for n, k, _ in M.NODE0}[name]


def pool_for(env, oracle, name):
    """the library's pool of a scene's map, rendered once at the default setting (its bricks exist and are current).  Brick maps
    are FUSED by the library (the bricks' retire bits come from the commit path); the saturated ones are rendered young and
    fused on, so the first render of the sweep is fed by the stale-brick refresh; the hand-saturated words and the edited
    node-0 words can only come through set_words."""
    pkg, torch = env
    key = words_key(name)
    if _LIVE.get("key") == key:
        return _LIVE["pool"]
    if "pool" in _LIVE:
        _LIVE.pop("pool").close()
    _LIVE.clear()
    ws, pool = pkg.Workspace(), pkg.Pool()

    def first_render(vm, w, h, center, edge):
        """(not compared: the sweep renders every map at the default setting too, and a failure there names the setting)"""
        render(env, pool.data_ptr, M.FOV, vm, w, h, center, edge)

    if name in M.BRICK_MAPS:
        depth, obs, hand, kind = M.BRICK_MAPS[name]
        pts, col = M.brick_cloud(depth, kind)
        tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
        for _ in range(M.YOUNG):
            pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, M.BRICK_CENTER, M.BRICK_EDGE)
        young = M.scene(oracle, name.rsplit("_", 1)[0] + "_young", 0)[0]
        assert np.array_equal(pool.words()[:2 * pool.size], young[:2 * pool.size])
        vm, w, h = M.brick_view(oracle, M.views_of(name)[-1])
        first_render(vm, w, h, M.BRICK_CENTER, M.BRICK_EDGE)
        for _ in range(obs - M.YOUNG):
            pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, M.BRICK_CENTER, M.BRICK_EDGE)
        words = M.scene(oracle, name, 0)[0]
        if hand:
            pool.set_words(words)
        assert np.array_equal(pool.words()[:2 * pool.size], words[:2 * pool.size])
    else:
        words = M.node0_words(oracle)[key]
        if key == "lod0":     # fused by the library, as tests/test_gpu_node0.py does: the grid built, then updated by the last commit
            (p0, c0, times), (p1, c1, _) = S.lod0_clouds()
            t0, k0 = torch.from_numpy(p0).cuda(), torch.from_numpy(c0).cuda()
            for _ in range(times):
                pkg.svo_from_point_cloud_async(ws, t0, k0, S.DEPTH, pool, S.CENTER, S.EDGE)
            img = torch.zeros((30, 40, 4), dtype=torch.uint8, device="cuda")
            pkg.cone_trace_svo(img, M.FOV, S.view_matrix(oracle, "lod0_plus")[0], pool.data_ptr, S.CENTER, S.EDGE, 0)
            pkg.svo_from_point_cloud_async(ws, torch.from_numpy(p1).cuda(), torch.from_numpy(c1).cuda(), S.DEPTH, pool, S.CENTER, S.EDGE)
            assert np.array_equal(pool.words(), words)
        else:
            pool.set_words(words)
            vm, w, h = S.view_matrix(oracle, "lod0_plus")
            first_render(vm, w, h, S.CENTER, S.EDGE)
    _LIVE.update(key=key, pool=pool, ws=ws)
    return pool


def bricks_in_use(pool, depth):
    """pool.march_accel(), checked as tests/test_gpu_bricks.py does.  False: the field did not fit beside other users of the
    device and the renders went through the tree march"""
    acc = pool.march_accel()
    assert acc["grid"], acc
    assert acc["bricks"] in (1, -1) and (acc["bricks"] == -1 or acc["brick_shift"] == (0 if depth <= 12 else 1)), acc
    return acc["bricks"] == 1


def depth_of(name):
    return M.BRICK_MAPS[name][0] if name in M.BRICK_MAPS else S.DEPTH


NO_BRICKS = "the brick field did not fit beside other users of the device: the renders went through the tree march (and equalled the oracle's)"


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,view", M.SCENES, ids=["%s-%s" % s for s in M.SCENES])
def test_every_burst_setting_renders_the_oracles_march(env, oracle, name, view):
    """image, [steps, levels] and per-pixel steps under every setting of march_ahead; all settings are rendered before anything
    is asserted, so a failure names every setting it shows under"""
    pkg, torch = env
    words, vm, w, h, center, edge = M.scene(oracle, name, view)
    ref, steps, levels, tr = M.rendered(oracle, name, view)
    pool = pool_for(env, oracle, name)
    with_bricks = bricks_in_use(pool, depth_of(name))
    wrong = []
    for ma in M.DEVICE_SWEEP:
        with configured(pkg, march_ahead=ma):
            got, cnt = render(env, pool.data_ptr, M.FOV, vm, w, h, center, edge)
            per_pixel = render(env, pool.data_ptr, M.FOV, vm, w, h, center, edge, 0x100)[0] if with_bricks else None
        print("%s %s march_ahead %d: [steps, levels] %s, oracle %s; image %s" % (name, view, ma, cnt, [steps, levels], describe_mismatch(got, ref)))
        if not np.array_equal(got, ref):
            wrong.append("march_ahead %d: image, %s" % (ma, describe_mismatch(got, ref)))
        if cnt != [steps, levels]:
            wrong.append("march_ahead %d: [steps, levels] %s, oracle %s" % (ma, cnt, [steps, levels]))
        if per_pixel is not None and not np.array_equal(per_pixel, tr.lengths):
            wrong.append("march_ahead %d: per-pixel steps, %s" % (ma, describe_mismatch(per_pixel, tr.lengths)))
    assert not wrong, (name, view, wrong)
    assert pkg.configure()["march_ahead"] == 60      # (the default stands again)
    if not with_bricks:
        pytest.skip(NO_BRICKS)


# ---- fields of view -----------------------------------------------------------------------------------------------------------
ORDINARY_FOVS = (20.0, 70.0)
DEGENERATE_FOVS = (0.0, 1e-30, 1e-33, 1e-37, 180.0, -45.0, 90.0)
# (map, view, (w, h)): the brick views near (a hand's breadth from the sheet) and far at small sizes; polarity True from the - side
FOV_SCENES = {"bricks12_young": ((2, (32, 60)), (0, (48, 36))), "bricks14_young": ((2, (32, 60)), (0, (48, 36))),
              "polarity_T_minus": (("lod0_minus", None),)}
_FOV_REF = {}


def fov_scene(oracle, name, view, size):
    words, vm, w, h, center, edge = M.scene(oracle, name, view)
    if size is not None:
        w, h = size
    return words, vm, w, h, center, edge


def fov_reference(oracle, name, view, size, fov, mode=0):
    """the oracle's render, once per (scene, fov, mode)"""
    k = (name, view, size, fov, mode)
    if k not in _FOV_REF:
        words, vm, w, h, center, edge = fov_scene(oracle, name, view, size)
        ref, steps, levels = oracle.cone_trace(words, w, h, fov, vm, center, edge, mode)
        assert steps <= S.MAX_ORACLE_STEPS, k
        ref.setflags(write=False)
        _FOV_REF[k] = (ref, steps, levels)
    return _FOV_REF[k]


def fov_check(env, oracle, ptr, name, view, size, fov, what, wrong, mode=0):
    words, vm, w, h, center, edge = fov_scene(oracle, name, view, size)
    ref, steps, levels = fov_reference(oracle, name, view, size, fov, mode)
    got, cnt = render(env, ptr, fov, vm, w, h, center, edge, mode)
    print("%s %s fov %g %s: [steps, levels] %s, oracle %s; image %s" % (name, view, fov, what, cnt, [steps, levels], describe_mismatch(got, ref)))
    if not np.array_equal(got, ref) or cnt != [steps, levels]:
        wrong.append((name, view, fov, what, cnt, [steps, levels], describe_mismatch(got, ref)))


@pytest.mark.parametrize("name", ["bricks12_young", "polarity_T_minus"])
def test_ordinary_fields_of_view(env, oracle, name):
    """fov 20 and 70 with bursts from the first step and at the default"""
    pkg, torch = env
    pool = pool_for(env, oracle, name)
    with_bricks = bricks_in_use(pool, depth_of(name))
    wrong = []
    for fov in ORDINARY_FOVS:
        for view, size in FOV_SCENES[name]:
            for ma in (0, 60):
                with configured(pkg, march_ahead=ma):
                    fov_check(env, oracle, pool.data_ptr, name, view, size, fov, "march_ahead %d" % ma, wrong)
    assert not wrong, wrong
    if not with_bricks:
        pytest.skip(NO_BRICKS)


@pytest.mark.parametrize("name", list(FOV_SCENES))
def test_degenerate_fields_of_view_through_the_brick_kernel(env, oracle, name):
    """`lod_always` false: cone_trace_brick_kernel<.., false, S, B> for S = 0 (depth 12, depth 10) and 1 (depth 14), B = 0
    (march_ahead -1) and 3 (march_ahead 0: every sample but the first inside a burst, on answer()'s rare path)"""
    pkg, torch = env
    pool = pool_for(env, oracle, name)
    with_bricks = bricks_in_use(pool, depth_of(name))
    wrong = []
    for fov in DEGENERATE_FOVS:
        for view, size in FOV_SCENES[name]:
            for ma in (-1, 0):
                with configured(pkg, march_ahead=ma):
                    fov_check(env, oracle, pool.data_ptr, name, view, size, fov, "march_ahead %d" % ma, wrong)
    assert not wrong, wrong
    if not with_bricks:
        pytest.skip(NO_BRICKS)


@pytest.mark.parametrize("name", list(FOV_SCENES))
def test_degenerate_fields_of_view_through_the_tree_kernel(env, oracle, name):
    """cone_trace_kernel's step_lod fallback: the same words as a plain device tensor (foreign memory: a grid built for the
    render) and the library's pool in carry mode"""
    pkg, torch = env
    pool = pool_for(env, oracle, name)
    foreign = torch.from_numpy(M.scene(oracle, name, FOV_SCENES[name][0][0])[0].view(np.int32).copy()).cuda()
    wrong = []
    for fov in DEGENERATE_FOVS:
        for view, size in FOV_SCENES[name]:
            fov_check(env, oracle, foreign.data_ptr(), name, view, size, fov, "foreign memory", wrong)
            fov_check(env, oracle, pool.data_ptr, name, view, size, fov, "carry mode", wrong, mode=1)
    assert not wrong, wrong


def test_degenerate_fields_of_view_depth16_pool(env, oracle):
    """a pool too deep for bricks: the library's level grid with cone_trace_kernel in reference mode"""
    pkg, torch = env
    depth = M.DEEP_MAPS["bricks16_young"][0]
    words = M.scene(oracle, "bricks16_young", 0)[0]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pts, col = M.brick_cloud(depth)
    for _ in range(M.YOUNG):
        pkg.svo_from_point_cloud_async(ws, torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda(), depth, pool, M.BRICK_CENTER, M.BRICK_EDGE)
    assert np.array_equal(pool.words()[:2 * pool.size], words[:2 * pool.size])
    wrong = []
    for fov in DEGENERATE_FOVS + ORDINARY_FOVS:
        for view, size in FOV_SCENES["bricks12_young"]:
            fov_check(env, oracle, pool.data_ptr, "bricks16_young", view, size, fov, "depth 16", wrong)
    acc = pool.march_accel()
    assert acc["grid"] and acc["bricks"] == 0 and acc["brick_shift"] == -1, acc
    assert not wrong, wrong
