"""The frames, the oracle's record and the case table of the tracker-form tests (test_gpu_tracker_forms.py compares the device
with the record, test_tracker_cases_cpu.py keeps the record meaningful).

A case is one image size under one setting of svoslam_config.track_mode / track_stream / track_workers; the oracle's answer
does not depend on the setting, so every case of a size is compared with the same record.  The expected plans are written
out: they were derived by hand from track_persistent_plan / _plan_stream / _plan_coarse (csrc/track_persistent.hip) and
accumulate_range (csrc/icp.hip) with kTrkThreads = 512, kTrkSlots = 4, kTrkStreamSlots = 2 and a capacity of at least 27
workgroups:

  pixels of level l: n_l = (w >> l) * (h >> l), less the Q15 tail n_l mod (20 * (w >> l) / 640)
     32x24   768 / 192 / 48        128x96  12288 / 3072 / 768      136x104 14144 / 3536 / 884    144x112 16128 / 4032 / 1008
     152x120 18240 / 4560 / 1140   160x120 19200 / 4800 / 1200     262x198 51872 (of 51876) / 12968 (of 12969) / 3184 (of 3185)
  register form:  W = ceil(n_0 / 2048) (<= track_workers); P_0 = W, P_l = min(W, ceil(n_l / 1024)); slots_l = ceil(n_l / (512 P_l))
  streaming form: P_l = min(track_workers, ceil(n_l / 1024), P_(l-1)); slots likewise; taken when the register plan has
                  slots_0 > 4, track_mode = 0 and track_stream = 1
  hybrid:         level 2 alone, P_2 = min(track_workers, ceil(n_2 / 2048)); taken likewise with track_stream = 0
"""
import functools

import numpy as np

FRAMES = 6          # frame 3 has no depth: frames 3 and 4 lose all three levels (4 has no valid partner), frame 5 tracks again
FORM_NONE, FORM_CHAIN, FORM_ONE_LAUNCH, FORM_STREAM, FORM_HYBRID = range(5)


def case(w, h, form, workers, participants, slots, **config):
    return {"w": w, "h": h, "config": config, "plan": {"form": form, "workers": workers, "participants": list(participants),
                                                       "slots": list(slots)}}


def case_id(c):
    return "%dx%d-%s" % (c["w"], c["h"], ",".join("%s=%d" % kv for kv in sorted(c["config"].items())) or "default")


CASES = [
    # default settings, register form: fewer pixels than lanes; slots exactly full; the fan-in's edges P = 7, 8, 9; odd sizes
    case(32, 24, FORM_ONE_LAUNCH, 1, (1, 1, 1), (2, 1, 1)),
    case(128, 96, FORM_ONE_LAUNCH, 6, (6, 3, 1), (4, 2, 2)),
    case(136, 104, FORM_ONE_LAUNCH, 7, (7, 4, 1), (4, 2, 2)),
    case(144, 112, FORM_ONE_LAUNCH, 8, (8, 4, 1), (4, 2, 2)),
    case(152, 120, FORM_ONE_LAUNCH, 9, (9, 5, 2), (4, 2, 2)),
    case(262, 198, FORM_ONE_LAUNCH, 26, (26, 13, 4), (4, 2, 2)),
    # the chain-replay fallback inside the register kernel (levels with slots > 4).  A replayed level 0 starts from a chain of one
    # (update_trans) and gains nine over its 10 iterations: nchain reaches kMaxChain in every one of these.  At 262x198 with one
    # worker level 2 replays too: its 4 iterations, from an EMPTY chain (nchain = 0), the only case that does
    case(160, 120, FORM_ONE_LAUNCH, 1, (1, 1, 1), (38, 10, 3), track_mode=2, track_workers=1),
    case(160, 120, FORM_ONE_LAUNCH, 7, (7, 5, 2), (6, 2, 2), track_mode=2, track_workers=7),
    case(160, 120, FORM_ONE_LAUNCH, 8, (8, 5, 2), (5, 2, 2), track_mode=2, track_workers=8),
    case(160, 120, FORM_ONE_LAUNCH, 9, (9, 5, 2), (5, 2, 2), track_mode=2, track_workers=9),
    case(262, 198, FORM_ONE_LAUNCH, 1, (1, 1, 1), (102, 26, 7), track_mode=2, track_workers=1),
    # the streaming form (levels with slots > 2 stream); with 1 and 3 workers the coarsest level streams too
    case(160, 120, FORM_STREAM, 1, (1, 1, 1), (38, 10, 3), track_mode=0, track_stream=1, track_workers=1),
    case(160, 120, FORM_STREAM, 4, (4, 4, 2), (10, 3, 2), track_mode=0, track_stream=1, track_workers=4),
    case(160, 120, FORM_STREAM, 7, (7, 5, 2), (6, 2, 2), track_mode=0, track_stream=1, track_workers=7),
    case(160, 120, FORM_STREAM, 8, (8, 5, 2), (5, 2, 2), track_mode=0, track_stream=1, track_workers=8),
    case(160, 120, FORM_STREAM, 9, (9, 5, 2), (5, 2, 2), track_mode=0, track_stream=1, track_workers=9),
    case(262, 198, FORM_STREAM, 3, (3, 3, 3), (34, 9, 3), track_mode=0, track_stream=1, track_workers=3),
    # the hybrid: level 2 in the one launch, levels 1 and 0 by the launch chain from the CamState the solver left
    case(160, 120, FORM_HYBRID, 1, (0, 0, 1), (0, 0, 3), track_mode=0, track_stream=0, track_workers=4),
    case(262, 198, FORM_HYBRID, 2, (0, 0, 2), (0, 0, 4), track_mode=0, track_stream=0, track_workers=3),
    # the launch chain, which the hybrid hands over to
    case(262, 198, FORM_CHAIN, 0, (0, 0, 0), (0, 0, 0), track_mode=1),
    case(32, 24, FORM_CHAIN, 0, (0, 0, 0), (0, 0, 0), track_mode=1),
]
SIZES = sorted({(c["w"], c["h"]) for c in CASES})


@functools.lru_cache(maxsize=None)
def frames(w, h):
    """[(depth uint16 [h, w], rgb uint8 [h, w, 3])] * FRAMES as numpy arrays: synth.render_frame(2 k), frame 3 without depth"""
    import svoslam_pkg
    svoslam_pkg.load()
    import importlib
    synth = importlib.import_module("octree_slam_amd.synth")
    out = []
    for k in range(FRAMES):
        d, c = synth.render_frame(2 * k, w, h)
        d = d.numpy().view(np.uint16).copy()
        if k == 3:
            d[:] = 0
        out.append((d, c.numpy().copy()))
    return out


@functools.lru_cache(maxsize=None)
def oracle_record(w, h):
    """the oracle's camera over frames(w, h), run once per size: per frame position, orientation, last system, fusion transform
    and lost-level count.  Read-only for its users."""
    import svoslam_pkg
    svoslam_pkg.load()
    import importlib
    synth = importlib.import_module("octree_slam_amd.synth")
    from oracle import oracle as ora
    f = synth.focal_length(w)
    ocam = ora.Camera(w, h, f, f)
    rec = []
    for k, (d, c) in enumerate(frames(w, h)):
        assert ocam.update(d, c, k) == 1
        p, o = ocam.pose()
        A, b, x = ocam.last_system()
        r = {"position": p, "orientation": o, "A": A, "b": b, "x": x, "fusion": ocam.fusion_transform(),
             "lost": ocam.tracking_lost_count()}
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        rec.append(r)
    return rec
