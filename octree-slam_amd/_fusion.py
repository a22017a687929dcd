"""Fusion: the workspace and the node pool, the phases of svoFromPointCloud, the radix sort and the scan behind them, key-range
sharded commits, and the voxel grid and surface mesh taken back out of a pool."""
import ctypes as C
import os

import numpy as np

from ._abi import (AccelView, CompactStats, FuseStats, SurfaceStats, SvoslamError, _close_quietly, _PoolStruct, _fa, _fp, _hip, _i32, _ptr,
                   _stream, _vp, check, copy_from_device, lib)
from ._args import stats_dict


class Workspace:
    def __init__(self):
        self._h = C.c_void_p()
        check(lib().svoslam_workspace_create(C.byref(self._h)))

    def close(self):
        if self._h:
            lib().svoslam_workspace_destroy(self._h)
            self._h = C.c_void_p()

    def _buffers(self, call, slots):
        """[(device pointer, bytes)] of the `slots` buffers one of the svoslam_workspace_*_buffers calls reports"""
        ptrs, sizes = (_vp * slots)(), (C.c_uint64 * slots)()
        check(call(self._h, ptrs, sizes))
        return [(int(ptrs[k] or 0), int(sizes[k])) for k in range(slots)]

    def field_buffers(self):
        """svoslam_workspace_field_buffers: [(device pointer, bytes)] of the three distance-field slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_field_buffers, 3)

    def reach_buffers(self):
        """svoslam_workspace_reach_buffers: [(device pointer, bytes)] of the two reach-field slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_reach_buffers, 2)

    def plan_buffers(self):
        """svoslam_workspace_plan_buffers: [(device pointer, bytes)] of the three cost-field slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_plan_buffers, 3)

    def ground_buffers(self):
        """svoslam_workspace_ground_buffers: [(device pointer, bytes)] of the six ground-field slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_ground_buffers, 6)

    def component_buffers(self):
        """svoslam_workspace_component_buffers: [(device pointer, bytes)] of the two component slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_component_buffers, 2)

    def nearest_buffers(self):
        """svoslam_workspace_nearest_buffers: [(device pointer, bytes)] of the three nearest-cell slots (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_nearest_buffers, 3)

    def visibility_buffers(self):
        """svoslam_workspace_visibility_buffers: [(device pointer, bytes)] of the visibility field's one slot (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_visibility_buffers, 1)

    def cover_buffers(self):
        """svoslam_workspace_cover_buffers: [(device pointer, bytes)] of the view cover's four slots -- the bit rows, the flags / ranks
        and the target list, the matrix, the covered words and round records (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_cover_buffers, 4)

    def observe_buffers(self):
        """svoslam_workspace_observe_buffers: [(device pointer, bytes)] of the ray observation's one slot, the two bit planes (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_observe_buffers, 1)

    def frontier_buffers(self):
        """svoslam_workspace_frontier_buffers: [(device pointer, bytes)] of the frontier field's one slot, the bit rows (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_frontier_buffers, 1)

    def score_buffers(self):
        """svoslam_workspace_score_buffers: [(device pointer, bytes)] of the pose scoring's one slot (diagnostics)"""
        return self._buffers(lib().svoslam_workspace_score_buffers, 1)

    __del__ = _close_quietly


class Pool:
    """Device node pool (svoslam_pool).  words() copies it to the host as uint32."""

    def __init__(self, capacity_nodes=8):
        self._p = _PoolStruct(None, 0, 0, None, 0, 0)
        check(lib().svoslam_pool_init(C.byref(self._p), capacity_nodes, _stream()))

    @property
    def size(self):
        if self._p.pending > 0:   # asynchronous fusion calls in flight: fetch the exact size (blocking)
            check(lib().svoslam_pool_sync(C.byref(self._p), _stream()))
        return int(self._p.size)

    @property
    def capacity(self):
        return int(self._p.capacity)

    @property
    def data_ptr(self):
        return int(self._p.d_data)

    def reserve(self, capacity_nodes):
        check(lib().svoslam_pool_reserve(C.byref(self._p), capacity_nodes, _stream()))

    def words(self):
        return copy_from_device(self.data_ptr, (2 * self.size,), np.uint32)

    def set_words(self, words):
        """replace the pool's contents (svoslam_pool_set_nodes: validates child pointers, resets the device-resident size
        and the reservations of asynchronous fusions, so fusing into the loaded tree allocates after it)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        check(lib().svoslam_pool_set_nodes(C.byref(self._p), words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size // 2, _stream()))

    def evict_subtree(self, path, file):
        """page the sub-tree below the node reached by the octant `path` out to `file` (svoslam_pool_evict_subtree)"""
        p = (C.c_uint8 * len(path))(*[int(o) for o in path])
        check(lib().svoslam_pool_evict_subtree(C.byref(self._p), p, len(path), str(file).encode(), _stream()))

    def restore_subtree(self, file):
        check(lib().svoslam_pool_restore_subtree(C.byref(self._p), str(file).encode(), _stream()))

    def graft_subtree(self, file):
        """bring a paged-out sub-tree back as new tiles at the end of the pool (svoslam_pool_graft_subtree): independent of node
        numbering, so it works after compact() where restore_subtree refuses"""
        check(lib().svoslam_pool_graft_subtree(C.byref(self._p), str(file).encode(), _stream()))

    def compact(self, capacity_nodes=0, want_map=False):
        """re-index the pool to the tiles reachable from the root, in canonical breadth-first order (svoslam_pool_compact).
        capacity_nodes <= 0 keeps the capacity, otherwise the new one is max(capacity_nodes, size after): 1 shrinks to fit.
        Returns the stats as a dict; with want_map also an int32 device tensor, entry k = old first-node index of new tile k."""
        st = CompactStats()
        old_tile, ptr = None, None
        if want_map:
            import torch
            # the call writes size_before / 8 entries, size_before being the size AFTER its own sync: take the same one here
            # (every commit in flight reports through the pool's tracker, which the sync drains), not a host-side size that lags
            check(lib().svoslam_pool_sync(C.byref(self._p), _stream()))
            old_tile = torch.zeros(max(int(self._p.size) // 8, 1), dtype=torch.int32, device="cuda")
            ptr = C.c_void_p(old_tile.data_ptr())
        check(lib().svoslam_pool_compact(C.byref(self._p), int(capacity_nodes), ptr, C.byref(st), _stream()))
        stats = stats_dict(st)
        if want_map:
            return stats, old_tile[:stats["size_after"] // 8]
        return stats

    def copy_from(self, other):
        """become a byte-identical replica of `other` (blocking)"""
        check(lib().svoslam_pool_copy(C.byref(self._p), C.byref(other._p), _stream()))

    def reset(self):
        """empty map (8 zeroed root children), same allocation"""
        check(lib().svoslam_pool_reset(C.byref(self._p), _stream()))

    def march_accel(self):
        """what the ray march of this pool runs on: {grid: bool, bricks: 1 in use / 0 not built / -1 allocation failed (tree march),
        brick_shift}"""
        g, b, sh = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        check(lib().svoslam_pool_march_accel(C.byref(self._p), C.byref(g), C.byref(b), C.byref(sh)))
        return {"grid": bool(g.value), "bricks": int(b.value), "brick_shift": int(sh.value)}

    def accel_view(self):
        """svoslam_pool_accel_view: the march's tables and their upkeep state as the library holds them right now, as a dict of
        device addresses (0: none), host flags and word offsets into a dirty state.  Launches nothing and changes nothing."""
        v = AccelView()
        check(lib().svoslam_pool_accel_view(C.byref(self._p), C.byref(v)))
        out = {n: getattr(v, n) for n, _ in AccelView._fields_ if n not in ("dirty", "brick_served")}
        for n in ("grid", "bricks", "brick_touched"):
            out[n] = int(out[n] or 0)
        for n in ("valid", "bricks_valid", "mip_consistent", "deferred_pending", "bricks_failed"):
            out[n] = bool(out[n])
        out["dirty"] = [int(v.dirty[k] or 0) for k in range(2)]
        out["brick_served"] = [int(v.brick_served[k]) for k in range(2)]
        out["bricks_in_use"] = bool(out["bricks"]) and out["bricks_valid"] and out["brick_shift"] >= 0
        return out

    def accel_grid(self, view=None):
        """the level-8 grid and the pyramid behind it as host words: (uint32 [2^24, 2], uint32 [pyramid entries, 2]); None
        before the first render"""
        v = view or self.accel_view()
        if not v["grid"]:
            return None
        n8, npyr = 1 << 24, ((1 << 24) - 8) // 7
        both = copy_from_device(v["grid"], (n8 + npyr, 2), np.uint32)
        return both[:n8], both[n8:]

    def accel_brick_group(self, group, view=None):
        """one 64 KB group of the brick field (8^3 bricks of 64 entries) as host uint16 [32768]"""
        v = view or self.accel_view()
        if not v["bricks"] or not 0 <= int(group) < (1 << 18):
            raise SvoslamError("no brick field, or no such group")
        return copy_from_device(v["bricks"] + int(group) * 65536, (32768,), np.uint16)

    def accel_dirty_words(self, state, offset, count, view=None):
        """`count` words of dirty state `state` from word `offset` on (uint32)"""
        v = view or self.accel_view()
        if not v["dirty"][state] or offset < 0 or offset + count > v["state_words"]:
            raise SvoslamError("no such dirty state, or words outside it")
        return copy_from_device(v["dirty"][state] + 4 * int(offset), (int(count),), np.uint32)

    def expand(self, center, edge_length, toward):
        """doubles the root cube towards `toward` (re-rooting); returns the new (center, edge_length)"""
        c = _fa(center, 3)
        e = C.c_float(float(edge_length))
        check(lib().svoslam_pool_expand(C.byref(self._p), c, C.byref(e), _fa(toward, 3), _stream()))
        return tuple(float(v) for v in c), float(e.value)

    def save(self, path, center, edge_length, max_depth):
        """checkpoint: linear tree + root parameters (svoslam_pool_save)"""
        check(lib().svoslam_pool_save(C.byref(self._p), str(path).encode(), _fa(center, 3), float(edge_length), int(max_depth),
                                      _stream()))

    def load(self, path):
        """resume from a checkpoint; returns (center, edge_length, max_depth)"""
        c, e, d = (C.c_float * 3)(), C.c_float(0), C.c_int32(0)
        check(lib().svoslam_pool_load(C.byref(self._p), str(path).encode(), c, C.byref(e), C.byref(d), _stream()))
        return tuple(float(v) for v in c), float(e.value), int(d.value)

    def close(self):
        if self._p.d_data:
            lib().svoslam_pool_free(C.byref(self._p))

    __del__ = _close_quietly


def svo_from_point_cloud(ws, points, colors, max_depth, pool, center, edge_length):
    """svo::svoFromPointCloud.  points: cuda float32 [n,3]; colors: cuda uint8 [n,3]."""
    n = int(points.shape[0]) if points is not None else 0
    stats = FuseStats()
    check(lib().svoslam_svo_from_point_cloud(ws._h, _ptr(points), _ptr(colors), n, max_depth, C.byref(pool._p),
                                             _fa(center, 3), float(edge_length), C.byref(stats), _stream()))
    return stats


def svo_from_point_cloud_async(ws, points, colors, max_depth, pool, center, edge_length):
    """svoFromPointCloud without any host round trip (size stays on the device until pool.size is read)."""
    n = int(points.shape[0]) if points is not None else 0
    check(lib().svoslam_svo_from_point_cloud_async(ws._h, _ptr(points), _ptr(colors), n, max_depth, C.byref(pool._p),
                                                   _fa(center, 3), float(edge_length), _stream()))


def svo_fuse_sort(ws, points, max_depth, center, edge_length):
    """phase 1 of the asynchronous fusion: keys + sort (workspace only)."""
    n = int(points.shape[0]) if points is not None else 0
    check(lib().svoslam_svo_fuse_sort(ws._h, _ptr(points), n, max_depth, _fa(center, 3), float(edge_length), _stream()))


def svo_fuse_sort_frame(ws, depth_image, pose_ptr, fx, fy, max_depth, center, edge_length, bbox7=None):
    """sort phase straight from a depth frame and a device-resident pose (vertex map + transform + bbox + keys in one launch)"""
    h, w = depth_image.shape[-2], depth_image.shape[-1]
    check(lib().svoslam_svo_fuse_sort_frame(ws._h, _ptr(depth_image), C.c_void_p(int(pose_ptr)), w, h, float(fx), float(fy),
                                            int(max_depth), _fa(center, 3), float(edge_length), _ptr(bbox7), _stream()))


def svo_fuse_sort_frame_band(ws, depth_image, pose_ptr, fx, fy, max_depth, center, edge_length, first_row, rows):
    """svo_fuse_sort_frame for one row band of the frame; the sorted point indices are whole-image indices"""
    h, w = depth_image.shape[-2], depth_image.shape[-1]
    check(lib().svoslam_svo_fuse_sort_frame_band(ws._h, _ptr(depth_image), C.c_void_p(int(pose_ptr)), w, h, float(fx), float(fy),
                                                 int(max_depth), _fa(center, 3), float(edge_length), int(first_row), int(rows), _stream()))


def svo_fuse_merge_sorted(keys_lists, idx_lists, keys_out, idx_out):
    """merge sorted (key, index) lists with ascending, disjoint index ranges (row bands in order) -> keys_out, idx_out"""
    n = len(keys_lists)
    kp = (C.c_void_p * n)(*[k.data_ptr() for k in keys_lists])
    ip = (C.c_void_p * n)(*[k.data_ptr() for k in idx_lists])
    cn = (C.c_int32 * n)(*[int(k.shape[0]) for k in keys_lists])
    check(lib().svoslam_svo_fuse_merge_sorted(kp, ip, cn, n, _ptr(keys_out), _ptr(idx_out), _stream()))


def svo_fuse_export_sorted(ws, n, keys_out, idx_out):
    """the outcome of the workspace's sort phase -> keys_out (int64 cuda tensor [n]), idx_out (int32 cuda tensor [n])"""
    check(lib().svoslam_svo_fuse_export_sorted(ws._h, int(n), _ptr(keys_out), _ptr(idx_out), _stream()))


def sort_words(ws, words, key_bits, idx_bits, digit_bits=0, want_vals=True, vals=None, keys_out=None, vals_out=None):
    """svoslam_sort_words: the library's stable radix sort on `words` (int64 cuda tensor [n]).  idx_bits >= 0: the packed form
    (key << idx_bits | index; digit_bits 1..11, 0 = by size); idx_bits == -1: the pair form carrying `vals` (int32 cuda tensor
    [n]; None: 0..n-1).  -> (keys, vals) as int64 / int32 cuda tensors (vals None when want_vals is false)"""
    import torch
    n = int(words.shape[0])
    if keys_out is None:
        keys_out = torch.empty(n, dtype=torch.int64, device=words.device)
    if vals_out is None and want_vals:
        vals_out = torch.empty(n, dtype=torch.int32, device=words.device)
    check(lib().svoslam_sort_words(ws._h, _ptr(words), _ptr(vals), n, int(key_bits), int(idx_bits), int(digit_bits), 1 if want_vals else 0,
                                   _ptr(keys_out), _ptr(vals_out), _stream()))
    return keys_out, vals_out


def exclusive_scan_u32(ws, data, total=None):
    """svoslam_exclusive_scan_u32: `data` (int32 cuda tensor [n], read as uint32) becomes its exclusive prefix sums mod 2^32, in
    place.  -> total (int32 cuda tensor [1]: the sum mod 2^32)"""
    import torch
    if total is None:
        total = torch.empty(1, dtype=torch.int32, device=data.device)
    check(lib().svoslam_exclusive_scan_u32(ws._h, _ptr(data), int(data.shape[0]), _ptr(total), _stream()))
    return total


def svo_fuse_adopt_sorted(ws, keys, idx, max_depth):
    """sorted keys / point indices from elsewhere become the outcome of the workspace's sort phase (they must stay alive
    until the commit has run)"""
    check(lib().svoslam_svo_fuse_adopt_sorted(ws._h, _ptr(keys), _ptr(idx), int(keys.shape[0]), int(max_depth)))


def svo_fuse_plan(ws, n, max_depth, pool):
    """phase 2: split planning against the pool's current tree (reads the pool)."""
    check(lib().svoslam_svo_fuse_plan(ws._h, int(n), max_depth, C.byref(pool._p), _stream()))


def pool_structure_begin(pool):
    """before a sequence of svo_fuse_plan_structure calls: the structure-side size := the pool's size"""
    check(lib().svoslam_pool_structure_begin(C.byref(pool._p), _stream()))


def svo_fuse_plan_structure(ws, n, max_depth, pool):
    """plan + every split with its links, independent of the previous frame's commit (colour words)"""
    check(lib().svoslam_svo_fuse_plan_structure(ws._h, int(n), int(max_depth), C.byref(pool._p), _stream()))


def svo_fuse_split_early(ws, n, max_depth, pool):
    """between plan and commit: the planned splits' child tiles, written where no ray march can see them yet"""
    check(lib().svoslam_svo_fuse_split_early(ws._h, int(n), int(max_depth), C.byref(pool._p), _stream()))


def svo_fuse_commit(ws, colors, max_depth, pool):
    """phase 3: splits, leaf blend, mip levels (writes the pool)."""
    n = int(colors.shape[0]) if colors is not None else 0
    check(lib().svoslam_svo_fuse_commit(ws._h, _ptr(colors), n, max_depth, C.byref(pool._p), _stream()))


def svo_fuse_commit_deferred(ws, colors, max_depth, pool):
    """phase 3 without a store a concurrent render of the pool's present state can see; svo_fuse_apply publishes it"""
    n = int(colors.shape[0]) if colors is not None else 0
    check(lib().svoslam_svo_fuse_commit_deferred(ws._h, _ptr(colors), n, max_depth, C.byref(pool._p), _stream()))


def svo_fuse_apply(ws, pool):
    check(lib().svoslam_svo_fuse_apply(ws._h, C.byref(pool._p), _stream()))


KEYRANGE_OVERFLOW, KEYRANGE_MISMATCH, KEYRANGE_USED_WORD = 2, 4, 10
KEYRANGE_FIXED_WORDS = 11264    # header + fixed-size lists of a delta; its tiles, links and words follow


def svo_fuse_keyrange_commit(ws, sorted_keys, sorted_idx, colors, max_depth, pool, rank, world, delta):
    """key-range sharded fusion, first half: plan + (invisible) commit of rank's slice of the frame's sorted keys, its delta into `delta`
    (a uint32 / int32 device tensor with room: 64 bytes per key of the slice is ample)"""
    n = int(sorted_keys.shape[0])
    check(lib().svoslam_svo_fuse_keyrange_commit(ws._h, _ptr(sorted_keys), _ptr(sorted_idx), _ptr(colors), n, int(max_depth), C.byref(pool._p),
                                                 int(rank), int(world), _ptr(delta), int(delta.numel() * delta.element_size()), _stream()))


def svo_fuse_keyrange_apply(ws, sorted_keys, max_depth, pool, deltas):
    """second half, after the all-gather: every rank's delta (rank order, the own one included) into this replica"""
    n = int(sorted_keys.shape[0])
    arr = (C.c_void_p * len(deltas))(*[int(d.data_ptr()) for d in deltas])
    check(lib().svoslam_svo_fuse_keyrange_apply(ws._h, _ptr(sorted_keys), n, int(max_depth), C.byref(pool._p), arr, len(deltas), _stream()))


def svo_fuse_keyrange_discard(ws, pool):
    """the delta of the last keyrange_commit was all that was wanted: no apply follows on this pool"""
    check(lib().svoslam_svo_fuse_keyrange_discard(ws._h, C.byref(pool._p)))


def svo_fuse_keyrange_status(ws):
    """flags of the last apply on this workspace (blocking): 0 = applied"""
    f = C.c_int32(0)
    check(lib().svoslam_svo_fuse_keyrange_status(ws._h, C.byref(f), _stream()))
    return int(f.value)


def svo_from_voxel_grid(ws, centers, colors, max_depth, pool, center, edge_length):
    """svo::svoFromVoxelGrid.  centers, colors: cuda float32 [n,4]."""
    n = int(centers.shape[0]) if centers is not None else 0
    stats = FuseStats()
    check(lib().svoslam_svo_from_voxel_grid(ws._h, _ptr(centers), _ptr(colors), n, max_depth, C.byref(pool._p),
                                            _fa(center, 3), float(edge_length), C.byref(stats), _stream()))
    return stats


def extract_voxel_grid(ws, pool, max_depth, center, edge_length):
    """svo::extractVoxelGridFromSVO -> (centers[n,4], colors[n,4]) numpy float32."""
    import torch
    pc, pk, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    check(lib().svoslam_extract_voxel_grid(ws._h, C.byref(pool._p), max_depth, _fa(center, 3), float(edge_length),
                                           C.byref(pc), C.byref(pk), C.byref(n), _stream()))
    torch.cuda.synchronize()
    ce = np.zeros((n.value, 4), np.float32)
    co = np.zeros((n.value, 4), np.float32)
    if n.value > 0:
        _hip().hipMemcpy(C.c_void_p(ce.ctypes.data), pc, C.c_size_t(ce.nbytes), 2)
        _hip().hipMemcpy(C.c_void_p(co.ctypes.data), pk, C.c_size_t(co.nbytes), 2)
        lib().svoslam_free(pc)
        lib().svoslam_free(pk)
    return ce, co


def extract_surface_mesh(ws, pool, max_depth, center, edge_length):
    """svoslam_extract_surface_mesh: the surface of the occupied cells at max_depth as a welded quad mesh ->
    (vertices[n,3] float32, quads[m,4] uint32, colors[m] uint32 (the cells' colour words), stats dict) as numpy arrays"""
    pv, pq, pc, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), SurfaceStats()
    check(lib().svoslam_extract_surface_mesh(ws._h, C.byref(pool._p), max_depth, _fa(center, 3), float(edge_length),
                                             C.byref(pv), C.byref(pq), C.byref(pc), C.byref(st), _stream()))
    stats = stats_dict(st)
    try:
        vertices = copy_from_device(pv.value, (stats["vertices"], 3), np.float32) if pv.value else np.zeros((0, 3), np.float32)
        quads = copy_from_device(pq.value, (stats["faces"], 4), np.uint32) if pq.value else np.zeros((0, 4), np.uint32)
        colors = copy_from_device(pc.value, (stats["faces"],), np.uint32) if pc.value else np.zeros(0, np.uint32)
    finally:
        for p in (pv, pq, pc):
            if p.value:
                lib().svoslam_free(p)
    return vertices, quads, colors, stats


def write_ply(path, vertices, quads, colors, triangulate=False):
    """svoslam_mesh_write_ply: binary little-endian PLY of a mesh held in numpy arrays (needs no device)"""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 4)
    c = np.ascontiguousarray(colors, dtype=np.uint32).reshape(-1)
    if c.shape[0] != q.shape[0]:
        raise ValueError("one colour per quad: %d colours, %d quads" % (c.shape[0], q.shape[0]))
    u32p = C.POINTER(C.c_uint32)
    check(lib().svoslam_mesh_write_ply(os.fsencode(str(path)), v.ctypes.data_as(_fp), v.shape[0], q.ctypes.data_as(u32p),
                                       c.ctypes.data_as(u32p), q.shape[0], 1 if triangulate else 0))


def subtree_file_words(file):
    """the stand-alone linear tree stored in a paged-out sub-tree file, as uint32 words (2 per node)"""
    w, n = C.POINTER(C.c_uint32)(), _i32(0)
    check(lib().svoslam_subtree_file_nodes(str(file).encode(), C.byref(w), C.byref(n)))
    try:
        return np.ctypeslib.as_array(w, shape=(2 * n.value,)).copy()
    finally:
        C.CDLL(None).free(w)
