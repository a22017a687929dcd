"""The tracker in every form it can take -- launch chain, one launch with register-resident pixels, its chain-replay fallback,
the streaming form, the hybrid -- at worker counts on the fan-in's edges and at odd and tiny image sizes, bit for bit against the
oracle's camera over six frames of which two lose every pyramid level (tracker_cases.py: the frames, the record, the table).
Every case also asserts, through svoslam_camera_last_track_plan, that the form and plan it was written for is the one that ran:
on a device too small for a plan the case fails rather than passing on another form."""
import numpy as np
import pytest

import tracker_cases as tc
from util import configured, same_bits_or_nan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    import importlib
    synth = importlib.import_module("octree_slam_amd.synth")
    return pkg, torch, synth


@pytest.fixture(scope="module")
def device_frames(env):
    """frames of a size on the device, uploaded once per size"""
    _, torch, _ = env
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = [(torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(c).cuda()) for d, c in tc.frames(w, h)]
        return cache[(w, h)]
    return get


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_frame(pkg, cam, want, k, tag):
    """the camera after frame k against the oracle's record, bit for bit; in the last system of a lost frame NaN where the
    oracle has NaN (sign and payload of a generated NaN are the FPU's choice)"""
    p, o = cam.pose()
    assert np.array_equal(bits(p), bits(want["position"])), (tag, k, p, want["position"])
    assert np.array_equal(bits(o), bits(want["orientation"])), (tag, k, o, want["orientation"])
    assert cam.tracking_lost_count() == want["lost"], (tag, k)
    if k >= 1:
        A, b, x = cam.last_system()
        assert same_bits_or_nan(A, want["A"]) and same_bits_or_nan(b, want["b"]), (tag, k)
        assert same_bits_or_nan(x, want["x"]), (tag, k, x, want["x"])
    fus = pkg.copy_from_device(cam.fusion_transform_ptr(), (16,), np.float32)
    assert np.array_equal(bits(fus), bits(want["fusion"])), (tag, k)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_tracker_form_matches_oracle(env, device_frames, case):
    pkg, torch, synth = env
    w, h = case["w"], case["h"]
    rec = tc.oracle_record(w, h)
    f = synth.focal_length(w)
    with configured(pkg, **case["config"]):
        cam = pkg.Camera(w, h, f, f)
        try:
            assert cam.last_track_plan()["form"] == tc.FORM_NONE
            for k, (d, c) in enumerate(device_frames(w, h)):
                assert cam.update(d, c, k) == 1
                check_frame(pkg, cam, rec[k], k, tc.case_id(case))
                assert cam.last_track_plan()["form"] == (case["plan"]["form"] if k >= 1 else tc.FORM_NONE), k
            assert cam.last_track_plan() == case["plan"]
            cam.reset()
            assert cam.last_track_plan() == {"form": tc.FORM_NONE, "workers": 0, "participants": [0, 0, 0], "slots": [0, 0, 0]}
        finally:
            cam.close()


def test_two_cameras_of_different_forms_alternate(env, device_frames):
    """a register-form camera (152x120, 9 workers) and a streaming camera (160x120, 4 workers) updated alternately in one
    process on one stream: they share the per-device launch chaining and nothing else -- generation, accumulator banks and
    broadcast granules are per camera -- so each follows its own oracle record"""
    pkg, torch, synth = env
    a, b = (152, 120), (160, 120)
    want_a = {"form": tc.FORM_ONE_LAUNCH, "workers": 9, "participants": [9, 5, 2], "slots": [4, 2, 2]}
    want_b = {"form": tc.FORM_STREAM, "workers": 4, "participants": [4, 4, 2], "slots": [10, 3, 2]}
    assert want_a in [c["plan"] for c in tc.CASES if (c["w"], c["h"]) == a and not c["config"]]
    assert want_b in [c["plan"] for c in tc.CASES if (c["w"], c["h"]) == b]
    rec_a, rec_b = tc.oracle_record(*a), tc.oracle_record(*b)
    cam_a = pkg.Camera(a[0], a[1], synth.focal_length(a[0]), synth.focal_length(a[0]))
    cam_b = pkg.Camera(b[0], b[1], synth.focal_length(b[0]), synth.focal_length(b[0]))
    try:
        for k in range(tc.FRAMES):
            d, c = device_frames(*a)[k]
            assert cam_a.update(d, c, k) == 1           # enqueued back to back: no readback between the two launches
            d, c = device_frames(*b)[k]
            with configured(pkg, track_mode=0, track_stream=1, track_workers=4):
                assert cam_b.update(d, c, k) == 1
            check_frame(pkg, cam_a, rec_a[k], k, "register")
            check_frame(pkg, cam_b, rec_b[k], k, "streaming")
        assert cam_a.last_track_plan() == want_a
        assert cam_b.last_track_plan() == want_b
    finally:
        cam_a.close(); cam_b.close()
