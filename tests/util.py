"""Shared helpers for the parity tests."""
import contextlib

import numpy as np


def rgba(word1):
    return [int(word1 & 0xFF), int((word1 >> 8) & 0xFF), int((word1 >> 16) & 0xFF), int(word1 >> 24)]


def same_bits_or_nan(a, b):
    """float arrays equal bit for bit where finite/inf, and NaN exactly where the other is NaN
    (NaN payload/sign differs between x86 and gfx950)."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def describe_mismatch(a, b, limit=5):
    a = np.asarray(a); b = np.asarray(b)
    if a.shape != b.shape:
        return "shape %s vs %s" % (a.shape, b.shape)
    idx = np.argwhere(a != b)
    return "%d mismatches, first: %s" % (len(idx), [(tuple(i), a[tuple(i)], b[tuple(i)]) for i in idx[:limit]])


def random_cloud(rng, n, lo=-0.95, hi=0.95, nan_every=0, dup_frac=0.0):
    pts = (rng.random((n, 3)) * (hi - lo) + lo).astype(np.float32)
    if dup_frac > 0 and n > 4:
        k = int(n * dup_frac)
        src = rng.integers(0, n, k)
        dst = rng.integers(0, n, k)
        pts[dst] = pts[src]
    if nan_every:
        pts[::nan_every, 0] = np.nan
        pts[1::nan_every * 2, 2] = np.inf
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return pts, col


def surface_cloud(rng, n, jitter=0.01):
    """points on a wavy sheet + a sphere: surface-like occupancy, as depth images produce"""
    u = rng.random(n) * 1.8 - 0.9
    v = rng.random(n) * 1.8 - 0.9
    z = 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.2
    pts = np.stack([u, v, z], 1)
    k = n // 3
    d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts[:k] = d * 0.4 + np.array([0.1, -0.2, -0.3])
    pts += rng.normal(scale=jitter, size=pts.shape)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return pts.astype(np.float32), col


def reference_obj(name, out_dir):
    """path of the reference's objs/<name> (data fixtures: tests/data/, or packed in tests/golden/ref_objs.npz as the
    file's bytes, unpacked into out_dir)"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "data", name)
    if os.path.exists(path):
        return path
    packed = np.load(os.path.join(here, "golden", "ref_objs.npz"))
    path = os.path.join(str(out_dir), name)
    with open(path, "wb") as fp:
        fp.write(packed[name[:-len(".obj")]].tobytes())
    return path


# ---- ICP maps whose Q15 tail can matter ------------------------------------------------------------------------------------
def noisy_depth(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    d = 1800 + 600 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + rng.normal(scale=3.0, size=(h, w))
    d[(xx // 40 + yy // 30) % 5 == 0] += 900      # depth discontinuities
    d = np.clip(d, 0, 65535)
    d[rng.random((h, w)) < 0.02] = 0              # dropouts
    d[0:3, 0:5] = 20000                           # > 15000 -> invalid
    return d.astype(np.uint16)


def live_last_row(m):
    """oracle.normal_map leaves +INF in the last row and the last column (no forward neighbour), so the ICP gates reject those
    pixels whatever the kernel does with them -- and Q15's tail, shorter than a row, lies in the last row.  Row h-2 copied over
    row h-1 and column w-2 over column w-1 (in place; returns m) makes them count."""
    m[-1, :, :] = m[-2, :, :]
    m[:, -1, :] = m[:, -2, :]
    return m


def q15_geometry(h, w):
    """(n, load_size, limit, tail): computeICPCost2 reduces floor(n / load_size) partials of load_size = 20 w / 640 pixels
    (localization_kernels.cu:303-326), so the last `tail` = n - limit pixels are left out"""
    n, load = w * h, 20 * w // 640
    limit = n // load * load if load > 0 else n
    return n, load, limit, n - limit


def icp_cost2_maps(oracle, h, w):
    """last and current vertex / normal maps [h, w, 3] of the computeICPCost2 tests: a noisy depth image and its copy under a
    small rigid motion, the normals with a live last row and column"""
    rng = np.random.default_rng(w)
    f = 570.3 * w / 640.0
    d1 = noisy_depth(rng, h, w)
    v1 = oracle.vertex_map(d1, f, f, w, h); n1 = live_last_row(oracle.normal_map(v1))
    T = oracle.icp_update_transform(np.array([0.004, -0.003, 0.002, 0.004, -0.002, 0.003], np.float32))
    v2 = oracle.transform_vertex_map(v1, T); n2 = live_last_row(oracle.transform_normal_map(n1, T))
    return v1, n1, v2, n2


def q15_bands(h, w):
    """pixel bands (first, num) that cover the image, one of them ending inside the tail (on the image's end for a tail of one
    pixel) and one starting there: svoslam_icp_accumulate clamps first + num to the limit with the line that clamps w * h"""
    n, load, limit, tail = q15_geometry(h, w)
    cuts = [0, (h // 3) * w, (h // 2 + 1) * w + 5, max(limit - load - 3, (h // 2 + 1) * w + 6), limit + (tail + 1) // 2, n]
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def cfg4_icp_maps(oracle, synth, w, h):
    """the maps of test_cfg4_icp_cost2_load_size_60: two 1920x1080 frames, subsampled (960, 480) or cropped (1919x1079), their
    normals with a live last row and column"""
    f = synth.focal_length(1920)
    d0, _ = synth.render_frame(0, 1920, 1080)
    d1, _ = synth.render_frame(3, 1920, 1080)
    step = 1920 // w if w in (960, 480) else 1
    a0 = np.ascontiguousarray(d0.numpy().view(np.uint16)[::step, ::step][:h, :w])
    a1 = np.ascontiguousarray(d1.numpy().view(np.uint16)[::step, ::step][:h, :w])
    v1 = oracle.vertex_map(a0, f, f, 1920, 1080); n1 = live_last_row(oracle.normal_map(v1))
    v2 = oracle.vertex_map(a1, f, f, 1920, 1080); n2 = live_last_row(oracle.normal_map(v2))
    return v1, n1, v2, n2


@contextlib.contextmanager
def configured(pkg, **settings):
    """svoslam_config set in-process for the block, the previous values restored after it"""
    before = pkg.configure(**settings)
    try:
        yield
    finally:
        pkg.configure(**before)
