"""The frames of the tracker-form cases (tracker_cases.py) do what the GPU cases rely on, by the oracle alone: frames 1, 2 and
5 are tracked, frames 3 and 4 lose all three pyramid levels each, and the pose moves between tracked frames.  A change of
synth that turned the GPU cases into all-lost (or never-lost) runs fails here."""
import numpy as np
import pytest

import tracker_cases as tc

# lost-level count after each frame.  32x24 is the exception: its coarsest levels (16x12, 8x6) hold too little for the
# solve, so the oracle already abandons two levels on frame 1 (the finest among them: its last x is NaN, the pose still moves
# by the level that held) and all three on frames 3 and 4 -- written out.
LOST_USUAL = [0, 0, 0, 3, 6, 6]
LOST = {(32, 24): [0, 2, 2, 5, 8, 8]}


def test_case_table_is_complete():
    assert tc.SIZES == [(32, 24), (128, 96), (136, 104), (144, 112), (152, 120), (160, 120), (262, 198)]
    assert len(tc.CASES) == 21 and len({tc.case_id(c) for c in tc.CASES}) == 21
    for c in tc.CASES:
        p = c["plan"]
        assert max(p["participants"]) == p["workers"]                       # the finest level present takes every worker
        assert all((n == 0) == (s == 0) for n, s in zip(p["participants"], p["slots"]))


@pytest.mark.parametrize("w,h", tc.SIZES)
def test_oracle_tracks_loses_and_recovers(oracle, w, h):
    fr = tc.frames(w, h)
    assert len(fr) == tc.FRAMES and not fr[3][0].any() and all(fr[k][0].any() for k in (0, 1, 2, 4, 5))
    rec = tc.oracle_record(w, h)
    lost = [r["lost"] for r in rec]
    assert lost == LOST.get((w, h), LOST_USUAL), lost
    for k in ((1, 2, 5) if (w, h) not in LOST else (2, 5)):               # tracked: the finest level's last solve is finite
        assert np.isfinite(rec[k]["x"]).all() and np.isfinite(rec[k]["A"]).all() and np.abs(rec[k]["A"]).max() > 0, k
    for k in (3, 4):                                                      # lost: 0 / 0 in the Cholesky
        assert np.isnan(rec[k]["x"]).all(), k
    # the pose moves between tracked frames and stands still over the lost ones
    for a, b in ((0, 1), (1, 2), (4, 5)):
        assert not np.array_equal(rec[a]["orientation"], rec[b]["orientation"]), (a, b)
        assert not np.array_equal(rec[a]["fusion"], rec[b]["fusion"]), (a, b)
    for a, b in ((2, 3), (3, 4)):
        assert np.array_equal(rec[a]["orientation"], rec[b]["orientation"]) and np.array_equal(rec[a]["position"], rec[b]["position"])
    assert all(np.isfinite(r["position"]).all() and np.isfinite(r["orientation"]).all() for r in rec)


def test_last_track_plan_is_exported_and_refuses_null():
    import ctypes as C
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    assert "svoslam_camera_last_track_plan" in pkg.SIGNATURES and hasattr(pkg.Camera, "last_track_plan")
    out = (C.c_int32 * 8)()
    assert pkg.lib().svoslam_camera_last_track_plan(None, out) != 0            # no camera: refused, no device needed
    assert (pkg.TRACK_FORM_NONE, pkg.TRACK_FORM_CHAIN, pkg.TRACK_FORM_ONE_LAUNCH, pkg.TRACK_FORM_STREAM, pkg.TRACK_FORM_HYBRID) == \
        (tc.FORM_NONE, tc.FORM_CHAIN, tc.FORM_ONE_LAUNCH, tc.FORM_STREAM, tc.FORM_HYBRID) == (0, 1, 2, 3, 4)
