"""The census of the node-0 scenes (tests/node0_scenes.py), on the CPU: the reference's own march must REACH the case each GPU
test of tests/test_gpu_node0.py is named for, at least once per ten pixels of the render -- a GPU test cannot pass by missing
its case.  The census march is held to the C oracle (image, steps, levels of every render) and, on a lattice of pixels, to
the scalar march of test_oracle_second_opinion.py sample by sample."""
import numpy as np
import pytest

import node0_scenes as S
from test_oracle_second_opinion import march


@pytest.fixture(scope="module")
def lod0_words(oracle):
    opool = oracle.Pool()
    S.fuse_all(opool, S.lod0_clouds())
    return opool.words()


@pytest.fixture(scope="module")
def stale_states(oracle):
    return {False: S.stale_sequence(oracle), True: S.stale_sequence(oracle, S.stale_first_frame_with_octant0())}


def counted(oracle, words, view):
    vm, w, h = S.view_matrix(oracle, view)
    ref, steps, levels = oracle.cone_trace(words, w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)
    assert steps <= S.MAX_ORACLE_STEPS
    img, s, l, counts = S.census(words, w, h, S.FOV, oracle.mat4_inverse(vm), S.CENTER, S.EDGE)
    assert (s, l) == (steps, levels) and np.array_equal(img, ref)      # the census march IS the reference's
    assert counts["pixels"] == w * h
    print(view, steps, levels, counts)
    return counts


def enough(counts, name):
    return 10 * counts[name] >= counts["pixels"]


def test_census_march_agrees_with_the_scalar_march_sample_by_sample(oracle, lod0_words):
    """twelve pixels of the LOD-0 scene (one sample each) and three of the opposite polarity (some two hundred each)"""
    for words, view, pixels in ((lod0_words, "lod0_plus", [(x, y) for x in (0, 13, 26, 39) for y in (0, 15, 29)]),
                                (S.opposite_polarity_words(lod0_words, True), "lod0_minus", [(0, 0), (21, 14), (39, 29)])):
        vm, w, h = S.view_matrix(oracle, view)
        inv = oracle.mat4_inverse(vm)
        mine = dict(lod_le0=0, lod1_octant0=0, lod_le_m1=0)

        def hook(px, py, lod, node, level, target):
            mine["lod_le0"] += lod <= 0
            mine["lod1_octant0"] += lod == 1 and node == 0
            mine["lod_le_m1"] += lod <= -1
            assert node == 0 or lod >= 1

        img, steps, levels = march(words, w, h, S.FOV, inv, S.CENTER, S.EDGE, hook=hook, pixels=pixels)
        # the census of the same pixels alone: an image of one row per pixel cannot be formed, so compare per-pixel results of the
        # full census with the scalar march's pixels and its sample counts with a census restricted by masking
        full, s, l, counts = S.census(words, w, h, S.FOV, inv, S.CENTER, S.EDGE)
        for px, py in pixels:
            assert tuple(img[py, px]) == tuple(full[py, px])
        if view == "lod0_plus":       # every ray: one LOD <= 0 sample, the last of its march
            assert mine["lod_le0"] == len(pixels) and counts["lod_le0"] == w * h
        else:                           # every ray takes the same LODs at the same lengths: counts scale with the pixels
            for k, v in mine.items():
                assert v * w * h == counts[k] * len(pixels), (k, v, counts[k])


def test_lod0_scene_reaches_lod_le0_over_cells_with_children(oracle, lod0_words):
    assert S.alpha_of(lod0_words, 0) >= S.SATURATED > S.alpha_of(lod0_words, 7)
    for view in ("lod0_plus", "lod0_minus"):
        c = counted(oracle, lod0_words, view)
        if view == "lod0_plus":
            assert enough(c, "lod_le0_over_children_other_saturation")


@pytest.mark.parametrize("raise_corner", [True, False])
def test_opposite_polarity_reaches_negative_lods(oracle, lod0_words, raise_corner):
    words = S.opposite_polarity_words(lod0_words, raise_corner)
    assert S.alpha_of(words, 0) < S.SATURATED
    c = counted(oracle, words, "lod0_minus")
    assert enough(c, "lod_le_m1") and enough(c, "lod_le0")
    if raise_corner:
        assert enough(c, "lod_le0_over_children_other_saturation")
    else:
        assert c["lod_le0_over_children_other_saturation"] == 0     # only the level count can tell
    counted(oracle, words, "lod0_plus")


def test_stale_scene_reaches_octant0_while_node0_is_childless(oracle, stale_states):
    frames, words = stale_states[False]
    assert all(not (int(w[0]) & S.FLAG) for w in words)                         # node 0 childless throughout
    assert S.alpha_of(words[-2], 0) < S.SATURATED <= S.alpha_of(words[-1], 0)   # the last frame crosses saturation
    assert frames >= 3
    for k in (0, frames - 2, frames - 1):
        for view in ("stale_coarse", "stale_fine"):
            vm, w, h = S.view_matrix(oracle, view)
            if view == "stale_fine" and k < frames - 1:     # (3 M samples: the oracle alone, the census below)
                assert oracle.cone_trace(words[k], w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)[1] <= S.MAX_ORACLE_STEPS
                continue
            c = counted(oracle, words[k], view)
            assert enough(c, "st1_octant0_lod_ge8")
            if view == "stale_coarse" and k < frames - 1:
                assert enough(c, "lod1_octant0")
    # what a stale entry serves: the last words with node 0's word of the frame before -- the march differs
    stale = words[-1].copy()
    stale[1] = words[-2][1]
    for view in ("stale_coarse", "stale_fine"):
        vm, w, h = S.view_matrix(oracle, view)
        fresh = oracle.cone_trace(words[-1], w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)
        old = oracle.cone_trace(stale, w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)
        assert fresh[1:] != old[1:]


def test_stale_scene_with_children_reaches_lod1_in_octant0(oracle, stale_states):
    frames, words = stale_states[True]
    assert all(int(w[0]) & S.FLAG for w in words)
    assert S.alpha_of(words[-2], 0) < S.SATURATED <= S.alpha_of(words[-1], 0)
    for k in (0, frames - 2, frames - 1):
        assert enough(counted(oracle, words[k], "stale_coarse"), "lod1_octant0")
    stale = words[-1].copy()
    stale[1] = words[-2][1]
    vm, w, h = S.view_matrix(oracle, "stale_coarse")
    assert oracle.cone_trace(words[-1], w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)[1:] != oracle.cone_trace(stale, w, h, S.FOV, vm, S.CENTER, S.EDGE, 0)[1:]
