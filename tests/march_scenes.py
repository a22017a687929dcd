"""Scenes, per-ray trace and burst model for the brick march's bursts (csrc/cone_trace.hip cone_trace_brick_kernel, phase 2), for
tests/test_march_bursts_cpu.py (the census) and tests/test_gpu_march_bursts.py (the sweep on the device): both import the scenes
from here, so the census runs on what the GPU renders.

`trace()` is node0_scenes.lockstep -- the reference's march, held to the C oracle by the census test -- recording every sample
of every ray: its LOD, the level its walk ends on as the reference counts it (the LOD itself where no level stops the walk, so
negative for negative LODs) and how the ray went on.  `burst_model()` is the kernel's SCHEDULE in plain numpy: which samples the
burst code answers under a setting of svoslam_config.march_ahead, at which burst position, as a hit or a miss of the prediction.
It knows nothing of the kernel's entries; what a wavefront adds (the `need` second trip depends on the other lanes) has a
reference-side proxy only."""
import numpy as np

import node0_scenes as S
from util import surface_cloud

GO_ON, RETIRED, RANGE = 0, 1, 2
SWEEP = (0, 2, 3, 7)            # the burst settings of the census; the device sweep adds -1 (bursts off) and 60 (the default)
DEVICE_SWEEP = (-1, 0, 2, 3, 7, 60)
FOV = 45.0
# (eye, target, (w, h)): tests/test_gpu_bricks.py VIEWS -- far / one metre / a hand's breadth / grazing the sphere
VIEWS = (((0.1, 0.2, -2.6), (0, 0, 0), (96, 72)),
         ((0.1, 0.2, -1.2), (0, 0, 0), (24, 480)),
         ((0.3, 0.1, 0.62), (0.28, 0.05, 0.2), (32, 480)),
         ((0.12, -0.18, 0.14), (0.1, -0.2, -0.3), (24, 480)),
         # the dense patch (patch_cloud) head-on from 0.2 m and 0.08 m: LOD 12 and 13 (the march is not conservative: from 0.1 m its steps jump the patch) on a surface with about one point per level-12 cell
         ((0.3, 0.1, 0.2), (0.3, 0.1, 0.4), (32, 480)),
         ((0.3, 0.1, 0.32), (0.3, 0.1, 0.4), (32, 480)))
SURFACE_VIEWS, PATCH_VIEWS = (0, 1, 2, 3), (4, 5)
CLOSE = (2, 3)                  # the two close views of the surface cloud
TALL = (1, 2, 3)                # its three 480-row views
BRICK_CENTER, BRICK_EDGE = (0.0, 0.0, 0.0), 1.0
YOUNG, SATURATED_OBS = 3, 130   # observations of the cloud: leaves pass A = 254 at observation 127


class Trace:
    """the march of one render, ray by ray: ray r's samples are [start[r], start[r + 1]) of lod / end / exit / kids8 (kids8: the
    sample's level-8 ancestor exists and has children)"""

    def __init__(self, img, steps, levels, w, h, start, lod, end, exit_, kids8):
        self.img, self.steps, self.levels, self.w, self.h = img, steps, levels, w, h
        self.start, self.lod, self.end, self.exit, self.kids8 = start, lod, end, exit_, kids8

    @property
    def lengths(self):
        """steps per ray, [h, w]"""
        return np.diff(self.start).reshape(self.h, self.w)

    def ray(self, r):
        """[(lod, end_level_raw, exit)] of ray r"""
        a, b = int(self.start[r]), int(self.start[r + 1])
        return list(zip(self.lod[a:b].tolist(), self.end[a:b].tolist(), self.exit[a:b].tolist()))


def trace(words, w, h, fov, inv_view, center, size):
    words = np.ascontiguousarray(words, np.uint32)
    result = {}
    rays, lods, ends, exits, kids = [], [], [], [], []
    for active, target, lod, node, end, retire, out in S.lockstep(words, w, h, fov, inv_view, center, size, result):
        # the level-8 ancestor: a walk of an LOD > 8 that ends below level 8 has passed it; one of LOD 8 ends ON it; a coarser LOD
        # says nothing about it -- those samples are walked once more, with LOD 8
        k8 = end > 8
        at8 = (lod == 8) & (end == 8)
        k8[at8] = (words[2 * node[at8]] & S.FLAG) != 0
        low = lod < 8
        if low.any():
            n8, e8 = S.walk(words, target[low], np.full(int(low.sum()), 8, np.int64), center, size)
            k8[low] = (e8 == 8) & ((words[2 * n8] & S.FLAG) != 0)
        rays.append(active); lods.append(lod); ends.append(end); kids.append(k8)
        exits.append(np.where(retire, RETIRED, np.where(out, RANGE, GO_ON)))
    rays = np.concatenate(rays)
    order = np.argsort(rays, kind="stable")     # ray-major, the steps of a ray in their order
    start = np.zeros(w * h + 1, np.int64)
    np.cumsum(np.bincount(rays, minlength=w * h), out=start[1:])
    pick = lambda parts, dt: np.concatenate(parts)[order].astype(dt)
    tr = Trace(result["img"], result["steps"], result["levels"], w, h, start, pick(lods, np.int32), pick(ends, np.int32),
               pick(exits, np.int8), pick(kids, bool))
    assert int(start[-1]) == tr.steps and (tr.exit[start[1:] - 1] != GO_ON).all()
    return tr


LOD_CLASSES = ("lod_le0", "lod_1_7", "lod_8", "lod_9_12", "lod_ge13")


def burst_model(seq, march_ahead, B=3):
    """what phase 2 of cone_trace_brick_kernel<.., B> answers of the rays of `seq` (a Trace) when bursts begin after step
    march_ahead (< 0: never).  Phase 1, the plain loop, always runs one step, so it answers steps 1 .. max(march_ahead, 1); a ray
    that ended there has no phase 2.  At the handover dprev is the raw level of phase 1's last step.  A burst answers samples
    j = 0 .. B - 1 while the chain holds: sample j is a HIT iff j + 1 < B, its raw level equals dprev and that level is >= -60;
    dprev becomes the sample's level either way.  A retire or range exit ends the ray, a miss ends the burst, and the next burst
    starts at the sample after the last one answered.  Returns counts (per burst position j where that matters)."""
    c = dict(burst_samples=0, lod_le_m1=0, hits_level_le0=0, rays=0, pixels=seq.w * seq.h, hits=[0] * B, misses=[0] * B,
             retires=[0] * B, ranges=[0] * B, entries=[0] * B)
    c.update({k: 0 for k in LOD_CLASSES})
    c["end_level"] = [0] * 17            # burst samples by the level their walk ends on (clipped to 0 .. 16)
    if march_ahead < 0:
        return c
    n1 = max(int(march_ahead), 1)
    length = np.diff(seq.start)
    rays = np.flatnonzero(length > n1)
    c["rays"] = len(rays)
    pos = seq.start[rays] + n1
    dprev = seq.end[pos - 1].astype(np.int64)
    while len(pos):
        chain = np.ones(len(pos), bool)
        done = np.zeros(len(pos), bool)
        for j in range(B):
            m = np.flatnonzero(chain)
            if not len(m):
                break
            at = pos[m]
            lod, end, ex = seq.lod[at], seq.end[at].astype(np.int64), seq.exit[at]
            c["burst_samples"] += len(m)
            c["lod_le0"] += int((lod <= 0).sum()); c["lod_le_m1"] += int((lod <= -1).sum())
            c["lod_1_7"] += int(((lod >= 1) & (lod <= 7)).sum()); c["lod_8"] += int((lod == 8).sum())
            c["lod_9_12"] += int(((lod >= 9) & (lod <= 12)).sum()); c["lod_ge13"] += int((lod >= 13).sum())
            c["end_level"] = (np.asarray(c["end_level"]) + np.bincount(np.clip(end, 0, 16), minlength=17)).tolist()
            c["entries"][j] += int((seq.kids8[at] & ~seq.kids8[at - 1]).sum())
            hit = (j + 1 < B) & (end == dprev[m]) & (end >= -60)
            dprev[m] = end
            over = ex != GO_ON
            c["retires"][j] += int((ex == RETIRED).sum()); c["ranges"][j] += int((ex == RANGE).sum())
            c["hits"][j] += int((hit & ~over).sum()); c["misses"][j] += int((~hit & ~over).sum()) if j + 1 < B else 0
            c["hits_level_le0"] += int((hit & ~over & (end <= 0)).sum())
            pos[m] += 1
            done[m] = over
            chain[m] = hit & ~over
        keep = ~done
        pos, dprev = pos[keep], dprev[keep]
    return c


def add(total, c):
    """counts summed over settings or scenes"""
    for k, v in c.items():
        if isinstance(v, list):
            total[k] = [x + y for x, y in zip(total.get(k, [0] * len(v)), v)]
        else:
            total[k] = total.get(k, 0) + v
    return total


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def brick_cloud(depth, kind="surface"):
    """surface: util.surface_cloud, a wavy sheet and a sphere over the whole root cube, a point per 6 cm^2 -- rays pass between its
    leaves and end on levels .. 10.  patch: a piece of a plane 3 cm x 10 cm with about one point per 0.5 mm cell (as
    tests/test_gpu_bricks.py test_foreign_words_are_not_trusted), which walks end ON at levels 11 .."""
    rng = np.random.default_rng(depth)
    if kind == "surface":
        return surface_cloud(rng, 5000, jitter=0.002)
    n = 10000
    pts = np.stack([rng.uniform(0.285, 0.315, n), rng.uniform(0.05, 0.15, n), 0.4 + rng.normal(scale=0.0003, size=n)], 1).astype(np.float32)
    return pts, rng.integers(1, 256, (n, 3), dtype=np.uint8)


def brick_words(oracle, depth, observations, kind="surface"):
    """the brick cloud observed `observations` times"""
    opool = oracle.Pool()
    pts, col = brick_cloud(depth, kind)
    for _ in range(observations):
        opool.insert_cloud(pts, col, depth, BRICK_CENTER, BRICK_EDGE)
    return opool.words()


def node_levels(words):
    """the level of every node reachable from the root (0: not reachable)"""
    level = np.zeros(len(words) // 2, np.int64)
    tile, lv = np.arange(8), 1
    while len(tile):
        level[tile] = lv
        w0 = words[2 * tile].astype(np.int64)
        first = w0[(w0 & S.FLAG) != 0] & S.MASK
        tile, lv = (first[:, None] + np.arange(8)[None, :]).ravel(), lv + 1
    return level


def hand_saturated(words):
    """three of ten observed nodes of levels 4 .. saturated by hand, with or without children, their parents and children
    untouched: words only set_words can bring into a pool (tests/test_gpu_bricks.py test_foreign_words_are_not_trusted).  Rays
    retire at every level from the pyramid's down to the leaves, on nodes whose ancestors and descendants say otherwise"""
    words = words.copy()
    seen = np.flatnonzero((node_levels(words) >= 4) & ((words[1::2] >> 24) > 127))
    pick = seen[np.random.default_rng(3).random(len(seen)) < 0.3]
    words[2 * pick + 1] = (words[2 * pick + 1] & np.uint32(0x00FFFFFF)) | np.uint32(0xFF000000)
    return words


def brick_view(oracle, k):
    eye, tgt, (w, h) = VIEWS[k]
    return oracle.look_at(eye, tgt, (0, 1, 0)), w, h


# node-0 scenes (tests/node0_scenes.py): (name, words key, view); words keys: ("polarity", raise_corner), "lod0", ("stale", state)
NODE0 = (("polarity_T_minus", ("polarity", True), "lod0_minus"),
         ("polarity_F_minus", ("polarity", False), "lod0_minus"),
         ("polarity_F_plus", ("polarity", False), "lod0_plus"),
         ("lod0_minus", "lod0", "lod0_minus"),
         ("stale_coarse_first", ("stale", 0), "stale_coarse"),
         ("stale_coarse_last", ("stale", -1), "stale_coarse"),
         ("stale_fine_last", ("stale", -1), "stale_fine"))


def node0_words(oracle, cache={}):
    """{words key: words} of the node-0 scenes"""
    if not cache:
        opool = oracle.Pool()
        S.fuse_all(opool, S.lod0_clouds())
        lod0 = opool.words()
        states = S.stale_sequence(oracle)[1]
        cache.update({"lod0": lod0, ("polarity", True): S.opposite_polarity_words(lod0, True),
                      ("polarity", False): S.opposite_polarity_words(lod0, False), ("stale", 0): states[0], ("stale", -1): states[-1]})
        for v in cache.values():
            v.setflags(write=False)
    return cache


# brick maps: name -> (depth, observations, saturated by hand, cloud)
BRICK_MAPS = {"bricks12_young": (12, YOUNG, False, "surface"), "bricks12_saturated": (12, SATURATED_OBS, False, "surface"),
              "bricks12_hand": (12, YOUNG, True, "surface"),
              "bricks14_young": (14, YOUNG, False, "surface"), "bricks14_saturated": (14, SATURATED_OBS, False, "surface"),
              "patch12_young": (12, YOUNG, False, "patch"), "patch12_saturated": (12, SATURATED_OBS, False, "patch"),
              "patch14_young": (14, YOUNG, False, "patch"), "patch14_saturated": (14, SATURATED_OBS, False, "patch")}
DEEP_MAPS = {"bricks16_young": (16, YOUNG, False, "surface")}    # too deep for bricks: the tree march (not part of the sweep)


def views_of(name):
    return PATCH_VIEWS if BRICK_MAPS[name][3] == "patch" else SURFACE_VIEWS


# every scene of the sweep: (map or node-0 scene name, view index or view name)
SCENES = [(m, k) for m in BRICK_MAPS for k in views_of(m)] + [(name, view) for name, _, view in NODE0]


def scene(oracle, name, view, fov=FOV, cache={}):
    """(words, view matrix, w, h, centre, half edge) of a scene; the words are computed once per map"""
    if name in BRICK_MAPS or name in DEEP_MAPS:
        if name not in cache:
            depth, obs, hand, kind = BRICK_MAPS[name] if name in BRICK_MAPS else DEEP_MAPS[name]
            words = brick_words(oracle, depth, obs, kind)
            cache[name] = hand_saturated(words) if hand else words
            cache[name].setflags(write=False)
        vm, w, h = brick_view(oracle, view)
        return cache[name], vm, w, h, BRICK_CENTER, BRICK_EDGE
    key = {n: k for n, k, _ in NODE0}[name]
    vm, w, h = S.view_matrix(oracle, view)
    return node0_words(oracle)[key], vm, w, h, S.CENTER, S.EDGE


def rendered(oracle, name, view, cache={}):
    """(oracle image, steps, levels, Trace) of a scene at fov 45, computed once and shared; the trace is held to the oracle here,
    so whoever uses it uses the reference's march"""
    if (name, view) not in cache:
        words, vm, w, h, center, edge = scene(oracle, name, view)
        ref, steps, levels = oracle.cone_trace(words, w, h, FOV, vm, center, edge, 0)
        assert steps <= S.MAX_ORACLE_STEPS, (name, view, steps)
        tr = trace(words, w, h, FOV, oracle.mat4_inverse(vm), center, edge)
        assert (tr.steps, tr.levels) == (steps, levels) and np.array_equal(tr.img, ref), (name, view)
        assert int(np.maximum(tr.end, 0).sum()) == levels and len(tr.end) == steps
        ref.setflags(write=False)
        cache[(name, view)] = (ref, steps, levels, tr)
    return cache[(name, view)]
