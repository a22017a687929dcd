"""svoslam_extract_surface_mesh on the device: vertices (as bits), quads, colours and stats equal the host restatement of the
specification (tests/test_surface_cpu.py: surface_words) applied to the pool's own words -- never a second device result alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_surface_cpu import CENTER, EDGE, HAND, occupied_cells, read_ply, surface_face_masks, surface_words
from util import surface_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def same_mesh(got, want):
    (v, q, c, s), (rv, rq, rc, rs) = got, want
    assert s == rs, (s, rs)
    assert v.dtype == np.float32 and q.dtype == np.uint32 and c.dtype == np.uint32
    assert v.shape == rv.shape and q.shape == rq.shape and c.shape == rc.shape
    assert np.array_equal(c, rc)
    assert np.array_equal(q, rq)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))


def fuse(pkg, torch, ws, pool, pts, col, depth, times=2, opool=None):
    tp, tc = torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda()
    for _ in range(times):
        pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, CENTER, EDGE)
        if opool is not None:
            opool.insert_cloud(pts, col, depth, CENTER, EDGE)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_pools(env, name):
    pkg, torch = env
    words, depth = HAND[name][:2]
    ws, pool = pkg.Workspace(), pkg.Pool()
    pool.set_words(words)
    same_mesh(pkg.extract_surface_mesh(ws, pool, depth, CENTER, EDGE), surface_words(words, depth, CENTER, EDGE))
    if depth > 1:                                                  # the level above, from the same words
        same_mesh(pkg.extract_surface_mesh(ws, pool, depth - 1, CENTER, EDGE), surface_words(words, depth - 1, CENTER, EDGE))


@pytest.mark.parametrize("depth", [6, 9])
def test_fused_cloud(env, depth):
    pkg, torch = env
    pts, col = surface_cloud(np.random.default_rng(41), 15000)
    ws, pool = pkg.Workspace(), pkg.Pool()
    fuse(pkg, torch, ws, pool, pts, col, depth)
    words = pool.words()
    for d in (depth, depth - 2):
        want = surface_words(words, d, CENTER, EDGE)
        cells = want[3]["cells"]
        assert cells > 256 and cells % 256 != 0                    # the scans cross workgroups, the last one is ragged
        assert want[3]["faces"] * 4 > 4096 and want[3]["vertices"] > 256
        got = pkg.extract_surface_mesh(ws, pool, d, CENTER, EDGE)
        same_mesh(got, want)
        # cells and per-cell colours are the voxel extraction's
        ce, co = pkg.extract_voxel_grid(ws, pool, d, CENTER, EDGE)
        assert ce.shape[0] == got[3]["cells"]
        # directly: the voxel grid's colour of each cell, repeated once per face of that cell (the restatement's face counts,
        # which same_mesh has just tied to the device's), is the device's face colour converted the way the voxel grid converts
        faces_per_cell = np.unpackbits(surface_face_masks(words, d)[:, None], axis=1).sum(1).astype(np.int64)
        c = got[2]
        mine = np.stack([((c >> s) & 0xFF).astype(np.float32) / np.float32(255.0) for s in (0, 8, 16, 24)], 1)
        assert faces_per_cell.sum() == c.shape[0] and np.array_equal(np.repeat(co, faces_per_cell, axis=0), mine)
        w1 = words[1::2][occupied_cells(words, d)[1]]              # the restatement's cells, in key order
        assert np.array_equal(co, np.stack([((w1 >> s) & 0xFF).astype(np.float32) / np.float32(255.0) for s in (0, 8, 16, 24)], 1))


def test_depth_16_vertex_keys_beyond_32_bits(env):
    pkg, torch = env
    pts, col = surface_cloud(np.random.default_rng(43), 2000)
    ws, pool = pkg.Workspace(), pkg.Pool()
    fuse(pkg, torch, ws, pool, pts, col, 16)
    words = pool.words()
    want = surface_words(words, 16, CENTER, EDGE)
    got = pkg.extract_surface_mesh(ws, pool, 16, CENTER, EDGE)
    assert got[3]["vertices"] > 0
    same_mesh(got, want)


def test_fresh_pool_is_an_empty_surface(env):
    import ctypes as C
    pkg, torch = env
    ws, pool = pkg.Workspace(), pkg.Pool()
    v, q, c, stats = pkg.extract_surface_mesh(ws, pool, 5, CENTER, EDGE)
    assert stats == {"cells": 0, "faces": 0, "vertices": 0} and v.shape == (0, 3) and q.shape == (0, 4) and c.shape == (0,)
    pv, pq, pc, st = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), pkg.SurfaceStats(7, 7, 7)
    args = (ws._h, C.byref(pool._p), 5, pkg._fa(CENTER, 3), float(EDGE), C.byref(pv), C.byref(pq), C.byref(pc), C.byref(st), pkg._stream())
    assert pkg.lib().svoslam_extract_surface_mesh(*args) == 0
    assert pv.value is None and pq.value is None and pc.value is None and (st.cells, st.faces, st.vertices) == (0, 0, 0)
    for bad_depth in (0, 17):                                      # the voxel extraction's errors
        a = list(args)
        a[2] = bad_depth
        assert pkg.lib().svoslam_extract_surface_mesh(*a) == -5
    a = list(args)
    a[8] = None
    assert pkg.lib().svoslam_extract_surface_mesh(*a) == -1


def test_unsynced_pool_second_call_and_fusion_afterwards(env, oracle):
    pkg, torch = env
    depth = 8
    pts, col = surface_cloud(np.random.default_rng(47), 15000)
    ws, pool, opool = pkg.Workspace(), pkg.Pool(), oracle.Pool()
    fuse(pkg, torch, ws, pool, pts, col, depth, opool=opool)
    assert pool._p.pending > 0                                     # straight after the asynchronous calls, no sync
    unsynced = pkg.extract_surface_mesh(ws, pool, depth, CENTER, EDGE)
    size = pool.size                                               # svoslam_pool_sync
    assert pool._p.pending == 0 and size == opool.size
    synced = pkg.extract_surface_mesh(ws, pool, depth, CENTER, EDGE)   # also: a second call on the same workspace
    want = surface_words(opool.words(), depth, CENTER, EDGE)
    same_mesh(unsynced, want)
    same_mesh(synced, want)
    # the workspace is left fit for fusion: its sort and plan buffers are the fusion's own
    pts2 = (pts * np.float32(0.97) + np.float32(0.01)).astype(np.float32)
    tp, tc = torch.from_numpy(pts2).cuda(), torch.from_numpy(col).cuda()
    pkg.svo_from_point_cloud_async(ws, tp, tc, depth, pool, CENTER, EDGE)
    opool.insert_cloud(pts2, col, depth, CENTER, EDGE)
    pkg.svo_from_point_cloud(ws, tp, tc, depth, pool, CENTER, EDGE)
    opool.insert_cloud(pts2, col, depth, CENTER, EDGE)
    assert pool.size == opool.size and np.array_equal(pool.words(), opool.words())
    same_mesh(pkg.extract_surface_mesh(ws, pool, depth, CENTER, EDGE), surface_words(opool.words(), depth, CENTER, EDGE))


def test_map_to_ply_tool(env, tmp_path):
    pkg, torch = env
    depth = 7
    pts, col = surface_cloud(np.random.default_rng(53), 6000)
    ws, pool = pkg.Workspace(), pkg.Pool()
    fuse(pkg, torch, ws, pool, pts, col, depth)
    ckpt, out = tmp_path / "map.svopool", tmp_path / "map.ply"
    pool.save(ckpt, CENTER, EDGE, depth)
    v, q, c, stats = pkg.extract_surface_mesh(ws, pool, depth, CENTER, EDGE)
    same_mesh((v, q, c, stats), surface_words(pool.words(), depth, CENTER, EDGE))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "map_to_ply.py"), str(ckpt), str(out)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "%d cells, %d faces, %d vertices" % (stats["cells"], stats["faces"], stats["vertices"]) in r.stdout
    assert "(%d bytes" % os.path.getsize(out) in r.stdout
    pv, pf, pc = read_ply(out)
    assert np.array_equal(pv.view(np.uint32), v.view(np.uint32))
    assert pf == [tuple(row) for row in q.tolist()]
    assert np.array_equal(pc, np.stack([(c >> s) & 0xFF for s in (0, 8, 16, 24)], 1).astype(np.uint8))
