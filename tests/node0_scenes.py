"""Scenes in which the reference's march reads NODE 0's colour word, for tests/test_node0_scenes_cpu.py (the census) and
tests/test_gpu_node0.py (the GPU parity tests): both import the scenes from here, so the census runs on what the GPU renders.

Node 0's word is special: every commit with a valid key rewrites it (the root pass Q6, the mean of the root's children with
the maximum of their alphas), and the reference's walk reads it whenever a sample's LOD is <= 0 (no level is walked: node_idx
stays 0) and whenever a sample lies in octant 0 and the walk stops on level 1 (LOD 1, or node 0 childless).

All scenes: root cube centre (0, 0, 0), half edge 0.05, depth 10, fov 45.  With 30 image rows the LOD is
ceil(log2(1.5 / ray_len)): 1 from 0.75 m, 0 from 1.5 m, -1 from 3 m, -2 from 6 m; with 480 rows sixteen times closer.

`census()` is a third statement of the reference's march (after the C oracle and the scalar `march` of
test_oracle_second_opinion.py), in numpy binary32 with all rays of an image in lockstep: fast enough to record every sample of
every render here.  The census test first holds it to the oracle's image and counters, and to the scalar march's samples."""
import ctypes

import numpy as np

F = np.float32
FLAG, MASK = 0x40000000, 0x3FFFFFFF
MAX_RANGE, START_DIST = F(10.0), F(0.002)
CENTER, EDGE, DEPTH, FOV = (0.0, 0.0, 0.0), 0.05, 10, 45.0
MAX_ORACLE_STEPS = 1 << 23      # per render: keeps the CPU side of every test to seconds
SATURATED = 254                 # A - 127 >= 127 retires a ray

COARSE, FINE = (40, 30), (16, 480)
# (eye, target, (w, h)) by name
VIEWS = {
    # from the + side, 2.2 m away: every sample up to the cube lies beyond the + faces (clamped into the deep boundary cells), LOD 0 from 1.5 m
    "lod0_plus": ((0.6, 0.7, 2.0), (0.025, 0.025, 0.025), COARSE),
    # from the - side through the cube and out of its + corner: LOD 0 in front of, inside and behind the cube, then -1 and -2 out to the range
    "lod0_minus": ((-0.6, -0.7, -2.0), (0.025, 0.025, 0.025), COARSE),
    # from the - side, 1.1 m away: all samples up to the cube lie in octant 0, LOD 1 from 0.75 m
    "stale_coarse": ((-0.5, -0.6, -0.8), (0.025, 0.025, 0.025), COARSE),
    # close by, tall image: the eye in octant 0's clamp region, LOD 12 at the first sample; looking along -x, so that an unsaturated
    # march stays in the childless octants 0, 2, 4, 6 (steps of half the edge: 400 per ray to the range, 3.1 M in all -- through the
    # points of octant 7 the same image takes 16 M oracle steps)
    "stale_fine": ((-0.06, -0.07, -0.09), (-0.3, 0.0, 0.05), FINE),
}


def alpha_of(words, node):
    return int(words[2 * node + 1]) >> 24


# ---- clouds (deterministic) -----------------------------------------------------------------------------------------------
def _cloud(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3)) * (hi - lo) + lo).astype(np.float32)
    col = rng.integers(1, 256, (n, 3), dtype=np.uint8)
    return pts, col


def lod0_clouds():
    """[(points, colours, times fused)]: octant 0 fused until node 0's word saturates, then ONE frame that reaches and leaves the
    + faces -- the clamped boundary cells (Q11) are deep and unsaturated"""
    return [_cloud(101, 1500, -0.04, -0.01) + (70,), _cloud(102, 20000, 0.0, 0.06) + (1,)]


def stale_cloud():
    """octant 7 only: node 0 stays childless"""
    return _cloud(103, 6000, 0.002, 0.047)


def stale_first_frame_with_octant0():
    """the stale cloud plus a few hundred points in the middle of octant 0: node 0 has children"""
    p7, c7 = stale_cloud()
    p0, c0 = _cloud(104, 300, -0.035, -0.015)
    return np.concatenate([p7, p0]), np.concatenate([c7, c0])


def fuse_all(opool, clouds):
    for pts, col, times in clouds:
        for _ in range(times):
            opool.insert_cloud(pts, col, DEPTH, CENTER, EDGE)


def corner_path(words, levels=DEPTH):
    """node indices of levels 1 .. on the path into the + + + corner of the root cube (octant 7 at every level), down to the
    first childless node"""
    path, child = [], 0
    for _ in range(levels):
        node = child + 7
        path.append(node)
        if not (int(words[2 * node]) & FLAG):
            break
        child = int(words[2 * node]) & MASK
    return path


def with_alpha(words, nodes, alpha):
    words = words.copy()
    idx = 2 * np.asarray(nodes, np.int64) + 1
    words[idx] = (words[idx] & np.uint32(0x00FFFFFF)) | np.uint32(alpha << 24)
    return words


def opposite_polarity_words(words, raise_corner):
    """the LOD0 tree with every saturated alpha -- node 0's and those of octant 0's nodes -- lowered below saturation.
    raise_corner: the nodes of levels 4 .. on the + corner's path saturated (the level-8 ancestor included): a march that takes
    the level-8 cell's word for an LOD <= 0 retires where the reference runs on to LODs -1 and -2.  Without: no word differs in
    saturation, only the level count can go wrong."""
    out = with_alpha(words, np.flatnonzero((words[1::2] >> 24) >= SATURATED), 129)
    assert alpha_of(out, 0) == 129
    if raise_corner:
        path = corner_path(out)
        assert len(path) >= 9, path     # the corner cell is deep: its level-8 node has children
        out = with_alpha(out, path[3:], 255)
    return out


def stale_sequence(oracle, first=None):
    """the words after frame 1 and after every later frame up to the one in which node 0's alpha crosses saturation.
    Returns (frames, [words after frame 1, .., words after frame N]); frame k >= 2 is the stale cloud."""
    opool = oracle.Pool()
    pts, col = stale_cloud()
    fp, fc = first if first is not None else (pts, col)
    opool.insert_cloud(fp, fc, DEPTH, CENTER, EDGE)
    states = [opool.words()]
    while alpha_of(states[-1], 0) < SATURATED:
        assert len(states) < 100
        opool.insert_cloud(pts, col, DEPTH, CENTER, EDGE)
        states.append(opool.words())
    return len(states), states


def view_matrix(oracle, name):
    eye, tgt, (w, h) = VIEWS[name]
    return oracle.look_at(eye, tgt, (0, 1, 0)), w, h


# ---- the march, all rays of an image in lockstep ---------------------------------------------------------------------------
def _length(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def _f2u8(x):
    """(uint8_t) of a float as the CUDA compiler emits it (test_oracle_second_opinion.f2u8), element-wise"""
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape, np.int64)
    ok = (x == x) & (x > 0.0)
    big = ok & (x >= 4294967295.0)
    out[big] = 0xFF
    ok &= ~big
    out[ok] = x[ok].astype(np.int64) & 0xFF
    return out


def walk(words, target, lod, center, size):
    """the reference's walk (cone_tracing_kernels.cu:76-105) for samples `target` [n, 3] with LODs `lod` [n]: the node each walk
    ends on and its level (the LOD itself where no level is walked or none stops it)"""
    n = len(lod)
    node, child = np.zeros(n, np.int64), np.zeros(n, np.int64)
    c = np.tile(np.asarray(center, F), (n, 1))
    t = np.full(n, F(size), F)
    end = lod.astype(np.int64).copy()
    walking = lod > 0
    for i in range(max(int(lod.max()) if n else 0, 0)):
        m = walking & (i < lod)
        if not m.any():
            break
        gt = target > c
        octant = gt[:, 0].astype(np.int64) + 2 * gt[:, 1] + 4 * gt[:, 2]
        node[m] = child[m] + octant[m]
        w0 = words[2 * node].astype(np.int64)
        stop = m & ((w0 & FLAG) == 0)
        end[stop] = i + 1
        walking &= ~stop
        go = m & ~stop
        child[go] = w0[go] & MASK
        t[go] = t[go] / F(2.0)
        sign = np.where(gt, F(1), F(-1)).astype(F)
        c[go] += t[go, None] * sign[go]
    return node, end


def lockstep(words, w, h, fov, inv_view, center, size, result):
    """the reference's march with all rays of an image in lockstep, one iteration per step: yields (rays, target, lod, node, end,
    retire, out) of the rays still marching -- their pixel indices, samples, LODs, the node and level each walk ends on, and which
    of them retire on this sample or leave the range behind it.  `result` receives img, steps and levels (final when exhausted)"""
    tanf = ctypes.CDLL("libm.so.6").tanf
    tanf.restype, tanf.argtypes = ctypes.c_float, [ctypes.c_float]
    words = np.ascontiguousarray(words, np.uint32)
    inv = np.asarray(inv_view, F).reshape(16)
    x_dir, y_dir, origin = -inv[0:3], -inv[4:7], inv[12:15].copy()
    ny = -y_dir
    fwd = np.array([x_dir[1] * ny[2] - ny[1] * x_dir[2], x_dir[2] * ny[0] - ny[2] * x_dir[0], x_dir[0] * ny[1] - ny[0] * x_dir[1]], F)
    pix_scale = F(tanf(F(F(fov) * F(3.14159)) / F(180.0))) / F(h)
    size = F(size)
    py, px = np.divmod(np.arange(w * h), w)
    mx = (px.astype(F) - F(w) / F(2.0)) / F(532.57)
    my = (py.astype(F) - F(h) / F(2.0)) / F(531.54)
    d = (mx[:, None] * x_dir[None, :] + my[:, None] * y_dir[None, :]) + fwd[None, :]
    ray = START_DIST * (d * (F(1.0) / _length(d))[:, None])
    img = np.zeros((w * h, 4), np.uint8)
    active = np.arange(w * h)
    result.update(img=img.reshape(h, w, 4), steps=0, levels=0)
    size_m, size_e = np.frexp(np.float64(size))
    while len(active):
        result["steps"] += len(active)
        assert result["steps"] <= MAX_ORACLE_STEPS
        r = ray[active]
        target = origin[None, :] + r
        ray_len = _length(r)
        mb, eb = np.frexp((ray_len * pix_scale).astype(np.float64))
        lod = ((size_e - eb) + (size_m > mb)).astype(np.int64)       # ceil(log2) of the real quotient (R5)
        node, end = walk(words, target, lod, center, size)
        result["levels"] += int(np.maximum(end, 0).sum())
        # ---- the sample's value, retirement, advance (:107-138) ----
        val = words[2 * node + 1].astype(np.int64)
        alpha = (val >> 24) - 127
        a = alpha.astype(F) / F(127.0)
        v = np.stack([_f2u8(a * (val & 0xFF).astype(F)), _f2u8(a * ((val >> 8) & 0xFF).astype(F)), _f2u8(a * ((val >> 16) & 0xFF).astype(F))], 1)
        retire = ~(alpha < 127)
        img[active[retire], :3] = v[retire]
        img[active[retire], 3] = 255
        new_dist = size / np.ldexp(F(1.0), end.astype(np.int32)).astype(F)
        r = r * ((ray_len + new_dist) / ray_len)[:, None]
        ray[active] = r
        out = ~retire & (_length(r) > MAX_RANGE)
        if out.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = F(127.0) / (alpha[out] & 0xFF).astype(F)
                img[active[out], :3] = _f2u8(v[out].astype(F) * sc[:, None])
            img[active[out], 3] = 255
        yield active, target, lod, node, end, retire, out
        active = active[~retire & ~out]


def census(words, w, h, fov, inv_view, center, size):
    """image, steps, levels of the reference's march, and the census of its samples (a dict of counts)"""
    words = np.ascontiguousarray(words, np.uint32)
    sat0 = alpha_of(words, 0) >= SATURATED
    counts = dict(lod_le0=0, lod_le0_over_children_other_saturation=0, lod1_octant0=0, st1_octant0_lod_ge8=0, lod_le_m1=0, pixels=w * h)
    result = {}
    for _, target, lod, node, end, _, _ in lockstep(words, w, h, fov, inv_view, center, size, result):
        le0 = lod <= 0
        counts["lod_le0"] += int(le0.sum())
        if le0.any():
            n8, e8 = walk(words, target[le0], np.full(int(le0.sum()), 8, np.int64), center, size)
            deep = (e8 == 8) & ((words[2 * n8] & FLAG) != 0)
            counts["lod_le0_over_children_other_saturation"] += int((deep & (((words[2 * n8 + 1] >> 24) >= SATURATED) != sat0)).sum())
        counts["lod1_octant0"] += int(((lod == 1) & (node == 0)).sum())
        counts["st1_octant0_lod_ge8"] += int(((lod >= 8) & (end == 1) & (node == 0)).sum())
        counts["lod_le_m1"] += int((lod <= -1).sum())
    return result["img"], result["steps"], result["levels"], counts
