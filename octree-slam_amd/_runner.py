"""The native frame scheduler, and the mailbox the ranks of a node exchange small records through."""
import ctypes as C

import numpy as np

from ._abi import _close_quietly, _fa, _fp, _i32, _ptr, _stream, check, lib


def _frames(depths, rgbs, timestamps, views):
    """what every run call starts with: the number of frames, their depth and colour pointers, timestamps, and views as float32 [n, 16]"""
    n = len(timestamps)
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in depths])
    rp = (C.c_void_p * n)(*[r.data_ptr() for r in rgbs])
    ts = (C.c_longlong * n)(*[int(t) for t in timestamps])
    vw = np.ascontiguousarray(np.stack([np.asarray(v, np.float32).reshape(16) for v in views]), np.float32)
    return n, dp, rp, ts, vw


def _shards(n, deltas, delta_events, march, images):
    """a sharded run's per-frame delta pointers, their events (None: no events at all), march flags and image pointers; None is NULL"""
    dl = (C.c_void_p * n)(*[(d.data_ptr() if d is not None else None) for d in deltas])
    ev = (C.c_void_p * n)(*[(e.cuda_event if e is not None else None) for e in delta_events]) if delta_events is not None else None
    mf = (C.c_uint8 * n)(*[1 if m else 0 for m in march])
    im = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in images])
    return dl, ev, mf, im


class Runner:
    """Native frame scheduler (csrc/runner.hip): track -> back-project -> fuse -> raycast of a list of frames on four
    HIP streams, enqueued by ONE call."""

    def __init__(self, cam, pool, width, height, max_depth, center, edge, fx, fy, render_mode):
        self._h = C.c_void_p()
        self._cam, self._pool = cam, pool          # keep the handles alive
        check(lib().svoslam_runner_create(C.byref(self._h), cam._h, C.byref(pool._p), width, height, max_depth, _fa(center, 3),
                                          float(edge), float(fx), float(fy), int(render_mode)))

    def run(self, depths, rgbs, timestamps, views, image, row_first, rows, counters=None):
        n, dp, rp, ts, vw = _frames(depths, rgbs, timestamps, views)
        check(lib().svoslam_runner_run(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, _ptr(image), int(row_first), int(rows),
                                       _ptr(counters), _stream()))

    def run_sharded(self, depths, rgbs, timestamps, views, deltas, delta_events, march, images, row_first, rows, counters=None):
        """one rank of a frame-sharded session (svoslam_runner_run_sharded): deltas = per-frame tensors (or None) of
        DELTA_FLOATS floats, delta_events = per-frame torch.cuda.Event (recorded) or None, march = per-frame bool,
        images = per-frame output tensor (or None where march is False)"""
        n, dp, rp, ts, vw = _frames(depths, rgbs, timestamps, views)
        dl, ev, mf, im = _shards(n, deltas, delta_events, march, images)
        self._keep = (depths, rgbs, deltas, delta_events, images)   # alive until the next call (the work is asynchronous)
        check(lib().svoslam_runner_run_sharded(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, dl, ev, mf, im, int(row_first), int(rows),
                                               _ptr(counters), _stream()))

    def run_sharded_presorted(self, depths, rgbs, timestamps, views, deltas, delta_events, march, images, sorted_keys, sorted_idx,
                              sorted_events, row_first, rows, counters=None):
        """run_sharded with every frame's sorted keys / point indices supplied (svoslam_runner_run_sharded_presorted):
        sorted_keys / sorted_idx = per-frame int64 / int32 cuda tensors, sorted_events = per-frame torch.cuda.Event or None"""
        n, dp, rp, ts, vw = _frames(depths, rgbs, timestamps, views)
        dl, ev, mf, im = _shards(n, deltas, delta_events, march, images)
        sk = (C.c_void_p * n)(*[k.data_ptr() for k in sorted_keys])
        si = (C.c_void_p * n)(*[k.data_ptr() for k in sorted_idx])
        se = (C.c_void_p * n)(*[(e.cuda_event if e is not None else None) for e in sorted_events]) if sorted_events is not None else None
        self._keep = (depths, rgbs, deltas, delta_events, images, sorted_keys, sorted_idx, sorted_events)
        check(lib().svoslam_runner_run_sharded_presorted(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, dl, ev, mf, im, sk, si, se,
                                                         int(row_first), int(rows), _ptr(counters), _stream()))

    def run_model(self, depths, rgbs, timestamps, views, image, row_first, rows, min_coverage=0.5, counters=None):
        """the frame loop with frame-to-model tracking inside the library (svoslam_runner_run_model); returns the number of frames
        whose ray-cast model was accepted.  Blocking."""
        n, dp, rp, ts, vw = _frames(depths, rgbs, timestamps, views)
        used = C.c_int32(0)
        check(lib().svoslam_runner_run_model(self._h, dp, rp, ts, vw.ctypes.data_as(_fp), n, _ptr(image), int(row_first), int(rows),
                                             _ptr(counters), float(min_coverage), C.byref(used), _stream()))
        return int(used.value)

    def bbox(self):
        """{min xyz, max xyz, any} of the last frame's point cloud (main.cpp:43)"""
        b = (C.c_float * 7)()
        check(lib().svoslam_runner_bbox(self._h, b))
        return np.array(list(b), np.float32)

    def timeline(self, max_frames=4096):
        """[frames, 10] stage times in ms of the last run (svoslam_config.runner_timeline = 1 when the runner was created)"""
        out = np.full((max_frames, 10), -1.0, np.float32)
        n = _i32(0)
        check(lib().svoslam_runner_timeline(self._h, out.ctypes.data_as(_fp), max_frames, C.byref(n)))
        return out[: n.value]

    def close(self):
        if self._h:
            lib().svoslam_runner_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = _close_quietly


class Mailbox:
    """One-shot peer-to-peer exchange of small records between the ranks of a node (csrc/mailbox.hip): all_gather of up to
    2 KB per rank, all_reduce of up to 256 float64 added in rank order; enqueued on the current stream, no host round trip."""

    def __init__(self, rank, world):
        self._h = C.c_void_p()
        self.rank, self.world = int(rank), int(world)
        check(lib().svoslam_mailbox_create(C.byref(self._h), self.rank, self.world))

    def handle(self):
        """64 bytes (numpy uint8) that the other PROCESSES need to map this rank's inbox"""
        buf = (C.c_uint8 * 64)()
        check(lib().svoslam_mailbox_handle(self._h, buf))
        return np.frombuffer(bytes(buf), dtype=np.uint8).copy()

    def connect(self, handles):
        """handles: uint8 array [world, 64], row r from rank r (this rank's own row is ignored)"""
        h = np.ascontiguousarray(handles, dtype=np.uint8)
        assert h.shape == (self.world, 64)
        check(lib().svoslam_mailbox_connect(self._h, h.ctypes.data_as(C.c_void_p)))

    def connect_local(self, boxes):
        """all mailboxes of the session live in this process (tests; one process driving several devices)"""
        arr = (C.c_void_p * self.world)(*[b._h for b in boxes])
        check(lib().svoslam_mailbox_connect_local(self._h, arr))

    def all_gather(self, src, dst):
        """dst[world, ...] <- every rank's src (same byte count on every rank, a multiple of 4, <= 2048)"""
        nbytes = src.numel() * src.element_size()
        assert dst.numel() * dst.element_size() == nbytes * self.world
        check(lib().svoslam_mailbox_all_gather(self._h, _ptr(src), nbytes, _ptr(dst), _stream()))

    def all_reduce_f64(self, values):
        """values (float64 cuda tensor, <= 256 entries) <- sum over ranks, added in rank order: the same bits everywhere"""
        check(lib().svoslam_mailbox_all_reduce_f64(self._h, _ptr(values), int(values.numel()), _stream()))

    def post(self, src):
        """first half of a collective: this rank's record into every inbox"""
        check(lib().svoslam_mailbox_post(self._h, _ptr(src), src.numel() * src.element_size(), _stream()))

    def collect(self, dst, nbytes, reduce_f64=False):
        """second half: every rank's record of the epoch just posted -> dst[world, ...] (or their rank-ordered float64 sum)"""
        check(lib().svoslam_mailbox_collect(self._h, _ptr(dst), int(nbytes), 1 if reduce_f64 else 0, _stream()))

    def set_wait_limit(self, polls):
        check(lib().svoslam_mailbox_set_wait_limit(self._h, int(polls)))

    def failed(self):
        f = _i32(0)
        check(lib().svoslam_mailbox_failed(self._h, C.byref(f)))
        return bool(f.value)

    def close(self):
        if self._h:
            lib().svoslam_mailbox_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = _close_quietly
