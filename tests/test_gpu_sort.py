"""The stable radix sort (both forms) and the exclusive scan of csrc/radix_sort.hip on the device, through svoslam_sort_words and
svoslam_exclusive_scan_u32 and through the fusion's own sort phase: every sorted and every scanned array equals the host restatement
(tests/test_sort_cpu.py: sort_words_host, scan_host, and a stable argsort of the oracle's keys) bit for bit -- never a second device
result alone.  The shapes are the smallest at which a pass can go wrong: one element, a wavefront, a tile of either form (2048,
1024) and one element more, several tiles, every digit width, one to five passes, a full 64-bit word; the two large cases are the
two sides of the packed sort's chunked column scan, whose threshold is hard-coded."""
import numpy as np
import pytest

from test_sort_cpu import (CENTER, COLUMN_SCAN_CASES, EDGE, FUSE_DEPTHS, FUSE_SIZES, FUSE_SIZES_DEPTH16, PACKED_CASES, PAIR_CASES,
                           SCAN_SIZES, SCAN_VALUES, U64, fuse_cloud, mask, packed_words, pair_inputs, scan_host, scan_input,
                           sort_words_host)
from util import configured, noisy_depth

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


@pytest.fixture(scope="module")
def shared_ws(env):
    """one workspace for the whole module: every case below sorts or scans in slots that an earlier case of another size, form and
    digit width has used"""
    return env[0].Workspace()


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d differ, first at %s: got %s, want %s" % (
        what, bad.size, got.size, bad[:4].tolist(), [hex(int(v)) for v in got[bad[:4]]], [hex(int(v)) for v in want[bad[:4]]])


def check_packed(pkg, torch, ws, n, key_bits, idx_bits, digit_bits, want_vals, words, what):
    want_k, want_v = sort_words_host(words, None, key_bits, idx_bits, bool(want_vals))
    keys, vals = pkg.sort_words(ws, dev(torch, words), key_bits, idx_bits, digit_bits, bool(want_vals))
    torch.cuda.synchronize()
    same(host(keys, U64), want_k, "%s keys" % (what,))
    if want_vals:
        same(host(vals, np.uint32), (want_v & U64(0xFFFFFFFF)).astype(np.uint32), "%s vals" % (what,))
    else:
        assert vals is None


def check_pairs(pkg, torch, ws, n, key_bits, words, vals, what):
    want_k, want_v = sort_words_host(words, vals, key_bits, -1)
    keys, out = pkg.sort_words(ws, dev(torch, words), key_bits, -1, vals=None if vals is None else dev(torch, vals))
    torch.cuda.synchronize()
    same(host(keys, U64), want_k, "%s words" % (what,))
    same(host(out, np.uint32), want_v, "%s vals" % (what,))


def fuse_expected(oracle, depth, n):
    """(points, sorted keys, sorted point indices) of a fusion case: the oracle's computeKeys and a stable argsort"""
    pts, _ = fuse_cloud(depth, n)
    keys = oracle.compute_keys(pts, depth, CENTER, EDGE).view(U64)
    order = np.argsort(keys, kind="stable")
    return pts, keys[order], order.astype(np.uint32)


def check_fuse_sort(pkg, torch, ws, depth, pts, want_k, want_i, what):
    n = pts.shape[0]
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    pkg.svo_fuse_sort(ws, torch.from_numpy(pts).cuda(), depth, CENTER, EDGE)
    pkg.svo_fuse_export_sorted(ws, n, keys, idx)
    torch.cuda.synchronize()
    same(host(keys, U64), want_k, "%s keys" % (what,))
    same(host(idx, np.uint32), want_i, "%s point indices" % (what,))


# ---- a. the packed sort ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: "%d-%d-%d-%d-%d-%s" % c)
def test_packed_sort_equals_the_host_sort(env, shared_ws, case):
    """svoslam_sort_words, packed form: keys (word >> idx_bits, bits above the key included) and unpacked indices equal a stable
    host sort on the key bits -- so equal keys leave in ascending index order (R1) at every digit width and pass count"""
    pkg, torch = env
    n, key_bits, idx_bits, digit_bits, want_vals, dist = case
    check_packed(pkg, torch, shared_ws, n, key_bits, idx_bits, digit_bits, want_vals, packed_words(n, key_bits, idx_bits, dist), case)


def test_packed_sort_ignores_and_keeps_the_bits_above_the_key(env, shared_ws):
    """the sort is `on bits [idx_bits, idx_bits + key_bits)`: bits of the word above them order nothing and leave in the keys"""
    pkg, torch = env
    n, key_bits, idx_bits = 4097, 12, 13
    words = packed_words(n, key_bits, idx_bits, "heavy")
    words |= np.random.default_rng(2).integers(0, 1 << (64 - key_bits - idx_bits), n, dtype=U64) << U64(key_bits + idx_bits)
    assert not np.array_equal(sort_words_host(words, None, key_bits, idx_bits)[0], np.sort(words) >> U64(idx_bits))
    for digit_bits in (11, 5):
        check_packed(pkg, torch, shared_ws, n, key_bits, idx_bits, digit_bits, 1, words, ("high bits", digit_bits))


# ---- b. the chunked column scan --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", COLUMN_SCAN_CASES, ids=lambda c: "%d-%d-%d-%d" % c)
def test_packed_sort_on_both_sides_of_the_chunked_column_scan(env, shared_ws, case):
    """More than 8192 tiles of 2048 words take the column scan in chunks (three launches per pass); up to 8192 tiles one launch
    scans the whole matrix.  The threshold is hard-coded in radix_sort.hip, which is why this case is large: 8192 * 2048 + 1 words
    (134 MB) is the smallest input on the far side, 8192 * 2048 the largest on the near side.  The words are unique by their index
    bits, so the host result is np.sort of the words."""
    pkg, torch = env
    n, key_bits, idx_bits, digit_bits = case
    words = np.random.default_rng(n).integers(0, 1 << key_bits, n, dtype=U64)
    words <<= U64(idx_bits)
    words |= np.arange(n, dtype=U64)
    keys, vals = pkg.sort_words(shared_ws, dev(torch, words), key_bits, idx_bits, digit_bits)
    torch.cuda.synchronize()
    words.sort()
    got_k, got_v = host(keys, U64), host(vals, np.uint32)
    del keys, vals
    same(got_k, words >> U64(idx_bits), "keys")
    same(got_v, (words & mask(idx_bits)).astype(np.uint32), "vals")


# ---- c. the pair sort ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: "%d-%d-%s-%s-%d" % c)
def test_pair_sort_equals_the_host_sort(env, shared_ws, case):
    """svoslam_sort_words, pair form: the whole words in the stable order of their bits [0, key_bits), each with the value it
    came with (its element number, or a given value: 0 and 0xFFFFFFFF among them)"""
    pkg, torch = env
    n, key_bits, values, dist, high = case
    words, vals = pair_inputs(n, key_bits, values, dist, high)
    check_pairs(pkg, torch, shared_ws, n, key_bits, words, vals, case)


# ---- d. the fusion's own path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", FUSE_DEPTHS)
def test_fusion_sort_phase_equals_the_host_sort(env, oracle, shared_ws, depth):
    """svoslam_svo_fuse_sort + _export_sorted on points with designed keys: the first pass's histogram comes from the key kernel
    (have_first_hist), the widths from 3 depth + 1 bits.  Expected: the oracle's keys in stable order, the point indices beside
    them.  Then the same under sort_pairs = 1 (the pair sort), with the same expected arrays.  At depth 16, 32768 points are the
    last size whose index fits the packed word (49 + 15 bits); 32769 take the pair sort on their own."""
    pkg, torch = env
    for n in FUSE_SIZES + (FUSE_SIZES_DEPTH16 if depth == 16 else ()):
        pts, want_k, want_i = fuse_expected(oracle, depth, n)
        check_fuse_sort(pkg, torch, shared_ws, depth, pts, want_k, want_i, ("packed", depth, n))
        with configured(pkg, sort_pairs=1):
            check_fuse_sort(pkg, torch, shared_ws, depth, pts, want_k, want_i, ("sort_pairs", depth, n))


def test_fusion_sort_phase_of_no_points(env):
    pkg, torch = env
    ws = pkg.Workspace()
    none = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    pkg.svo_fuse_sort(ws, none, 8, CENTER, EDGE)
    pkg.svo_fuse_export_sorted(ws, 0, torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"))
    pkg.svo_fuse_sort(ws, None, 8, CENTER, EDGE)
    pkg.svo_fuse_export_sorted(ws, 0, None, None)
    torch.cuda.synchronize()


# ---- e. one workspace, many sorts ------------------------------------------------------------------------------------------
def test_one_workspace_sorts_large_then_small_then_in_the_other_form(env, oracle):
    """a fresh workspace through packed 100 003, packed 65, pairs 1025, packed 2049 at another key width, the fusion's sort of
    6145 points, pairs 50 001: the slots only grow, so each sort runs in what the sorts before it left in tile_hist, keys_b and
    vals_a -- and none of it may show"""
    pkg, torch = env
    ws = pkg.Workspace()
    check_packed(pkg, torch, ws, 100003, 37, 17, 11, 1, packed_words(100003, 37, 17, "uniform"), "packed 100003")
    check_packed(pkg, torch, ws, 65, 12, 7, 8, 1, packed_words(65, 12, 7, "heavy"), "packed 65")
    words, vals = pair_inputs(1025, 37, "iota", "wave_runs", False)
    check_pairs(pkg, torch, ws, 1025, 37, words, vals, "pairs 1025")
    check_packed(pkg, torch, ws, 2049, 23, 12, 5, 1, packed_words(2049, 23, 12, "two_alternating"), "packed 2049")
    pts, want_k, want_i = fuse_expected(oracle, 12, 3 * 2048 + 1)
    check_fuse_sort(pkg, torch, ws, 12, pts, want_k, want_i, "fusion 6145")
    words, vals = pair_inputs(50001, 51, "given", "heavy", False)
    check_pairs(pkg, torch, ws, 50001, 51, words, vals, "pairs 50001")
    check_packed(pkg, torch, ws, 4097, 43, 0, 11, 0, packed_words(4097, 43, 0, "heavy"), "keys only 4097")


# ---- f. the frame front end ------------------------------------------------------------------------------------------------
def test_frame_sort_phase_equals_the_oracle_chain(env, oracle):
    """svoslam_svo_fuse_sort_frame on a 97 x 61 depth image under a pose that is not the identity: the exported arrays equal
    generateVertexMap, transformVertexMap and computeKeys of the oracle in stable order.  svoslam_svo_fuse_sort_frame_band for rows
    [7, 40) gives the whole frame's result filtered, in order, to those rows' pixels (whole-image pixel indices)."""
    pkg, torch = env
    w, h, depth, center, edge = 97, 61, 6, (0.0, 0.0, 2.0), 2.0
    f = 570.3 * w / 640.0
    d = noisy_depth(np.random.default_rng(97), h, w)
    T = np.asarray(oracle.icp_update_transform(np.array([0.04, -0.03, 0.02, 0.05, -0.02, 0.03], np.float32)), np.float32).reshape(16)
    assert not np.array_equal(T, np.eye(4, dtype=np.float32).reshape(16))
    pts = oracle.transform_vertex_map(oracle.vertex_map(d, f, f, w, h), T).reshape(-1, 3)
    keys = oracle.compute_keys(pts, depth, center, edge).view(U64)
    order = np.argsort(keys, kind="stable")
    want_k, want_i = keys[order], order.astype(np.uint32)
    assert 1000 < np.unique(keys).size < w * h // 2 and (keys == 1).sum() > 50       # many cells, most of them hit more than once
    dd, pose, ws = torch.from_numpy(d.view(np.int16)).cuda(), torch.from_numpy(T).cuda(), pkg.Workspace()
    n = w * h
    gk, gi = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    pkg.svo_fuse_sort_frame(ws, dd, pose.data_ptr(), f, f, depth, center, edge)
    pkg.svo_fuse_export_sorted(ws, n, gk, gi)
    torch.cuda.synchronize()
    same(host(gk, U64), want_k, "frame keys")
    same(host(gi, np.uint32), want_i, "frame pixel indices")
    first, rows = 7, 33
    inside = (want_i >= first * w) & (want_i < (first + rows) * w)
    nb = rows * w
    pkg.svo_fuse_sort_frame_band(ws, dd, pose.data_ptr(), f, f, depth, center, edge, first, rows)
    pkg.svo_fuse_export_sorted(ws, nb, gk[:nb], gi[:nb])
    torch.cuda.synchronize()
    same(host(gk[:nb], U64), want_k[inside], "band keys")
    same(host(gi[:nb], np.uint32), want_i[inside], "band pixel indices")


# ---- g. the scan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_equals_the_host_scan(env, shared_ws, n):
    """svoslam_exclusive_scan_u32 at every size where it takes another path (one workgroup's loop up to 8192, chunks of 2048 beyond,
    more than 256 chunk sums) with small values, zeros, ones, 0xFFFFFFFF (the sums wrap modulo 2^32) and any values; the total too"""
    pkg, torch = env
    for kind in SCAN_VALUES:
        data = scan_input(n, kind)
        want, want_total = scan_host(data)
        t = dev(torch, data)
        total = pkg.exclusive_scan_u32(shared_ws, t)
        torch.cuda.synchronize()
        same(host(t, np.uint32), want, "scan of %d x %s" % (n, kind))
        assert int(host(total, np.uint32)[0]) == want_total, (n, kind, int(host(total, np.uint32)[0]), want_total)


def test_scans_of_different_sizes_share_one_workspace(env):
    """scan_tmp (the chunk sums) is grow-only: a long scan, a shorter chunked one, a one-workgroup one and the long one again"""
    pkg, torch = env
    ws = pkg.Workspace()
    for n, kind in ((256 * 2048 + 3, "max"), (10 * 2048 + 1, "any"), (8192, "one"), (256 * 2048 + 3, "small"), (8193, "max")):
        data = scan_input(n, kind)
        want, want_total = scan_host(data)
        t = dev(torch, data)
        total = pkg.exclusive_scan_u32(ws, t)
        torch.cuda.synchronize()
        same(host(t, np.uint32), want, "scan of %d x %s" % (n, kind))
        assert int(host(total, np.uint32)[0]) == want_total, (n, kind)


# ---- h. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_sort(env):
    pkg, torch = env
    L, ws = pkg.lib(), pkg.Workspace()
    n = 100
    words = dev(torch, packed_words(n, 12, 7, "uniform"))
    keys = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    vals = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    W, K, V, NULL = words.data_ptr(), keys.data_ptr(), vals.data_ptr(), None

    def call(ws_h=ws._h, d_words=W, d_vals=NULL, n=n, key_bits=12, idx_bits=7, digit_bits=0, want_vals=1, d_keys=K, d_out=V):
        return L.svoslam_sort_words(ws_h, d_words, d_vals, n, key_bits, idx_bits, digit_bits, want_vals, d_keys, d_out, None)

    bad = [dict(ws_h=None), dict(d_words=NULL), dict(d_keys=NULL), dict(d_out=NULL), dict(n=-1), dict(key_bits=0), dict(key_bits=-3),
           dict(key_bits=58), dict(key_bits=65, idx_bits=0), dict(key_bits=65, idx_bits=-1), dict(idx_bits=-2),
           dict(digit_bits=-1), dict(digit_bits=12), dict(idx_bits=-1, digit_bits=12), dict(idx_bits=-1, d_out=NULL)]
    for kw in bad:
        assert call(**kw) == INVALID_ARG, kw
    torch.cuda.synchronize()
    assert (keys == -1).all() and (vals == -1).all()                                # nothing was launched
    # n == 0 is OK whatever the pointers, if the other arguments are valid -- and not if they are not
    assert call(n=0, d_words=NULL, d_keys=NULL, d_out=NULL) == 0 and call(n=0, idx_bits=-1, d_words=NULL, d_keys=NULL, d_out=NULL) == 0
    assert call(n=0, key_bits=0) == INVALID_ARG and call(n=0, digit_bits=12) == INVALID_ARG
    torch.cuda.synchronize()
    assert (keys == -1).all() and (vals == -1).all()
    # the edges that are valid: a full word, 64 key bits in the pair form, d_vals_out NULL without values
    assert call(key_bits=57) == 0 and call(key_bits=64, idx_bits=-1) == 0 and call(want_vals=0, d_out=NULL) == 0
    assert call(digit_bits=11) == 0 and call(digit_bits=1) == 0
    torch.cuda.synchronize()
    want_k, want_v = sort_words_host(host(words, U64), None, 12, 7)
    same(host(keys, U64), want_k, "keys after the refused calls")
    same(host(vals, np.uint32), want_v.astype(np.uint32), "vals after the refused calls")


def test_argument_errors_of_the_scan(env):
    pkg, torch = env
    L, ws = pkg.lib(), pkg.Workspace()
    data = torch.full((10,), 3, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    assert L.svoslam_exclusive_scan_u32(None, data.data_ptr(), 10, total.data_ptr(), None) == INVALID_ARG
    assert L.svoslam_exclusive_scan_u32(ws._h, None, 10, total.data_ptr(), None) == INVALID_ARG
    assert L.svoslam_exclusive_scan_u32(ws._h, data.data_ptr(), 10, None, None) == INVALID_ARG
    assert L.svoslam_exclusive_scan_u32(ws._h, data.data_ptr(), 0xFFFFFFFF, total.data_ptr(), None) == INVALID_ARG
    torch.cuda.synchronize()
    assert int(total.item()) == -1 and (data == 3).all()
    assert L.svoslam_exclusive_scan_u32(ws._h, None, 0, total.data_ptr(), None) == 0       # no elements: the total is 0
    torch.cuda.synchronize()
    assert int(total.item()) == 0 and (data == 3).all()
    assert L.svoslam_exclusive_scan_u32(ws._h, data.data_ptr(), 10, total.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(total.item()) == 30 and data.tolist() == list(range(0, 30, 3))
