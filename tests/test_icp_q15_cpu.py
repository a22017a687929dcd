"""Q15 (the last n mod load_size pixels are left out of computeICPCost2's reduce) can be seen in the maps the GPU tests use --
proved here on the oracle alone, so that the GPU tests only have to compare device and oracle.

The tail is shorter than an image row, so it lies in the last row, where oracle.normal_map leaves +INF: with such maps the
gates reject the tail anyway and a kernel that clamped its range to w * h instead of floor(n / load) * load would pass.
util.live_last_row makes the last row and column count.  For every size with a tail:
  - the last KEPT group of load_size pixels is live: NaN-ing it changes the sums;
  - the oracle leaves the tail out: NaN-ing the tail changes nothing;
  - the tail WOULD count: its pixels' twelve values moved onto the first pixels of the last kept group (the rest of the group
    NaN) give other sums than the group NaN'd altogether -- so a kernel that counted the tail would differ from the oracle."""
import importlib

import numpy as np
import pytest

from util import cfg4_icp_maps, icp_cost2_maps, q15_bands, q15_geometry

SIZES = [(99, 131, 4, 1), (49, 65, 2, 1), (198, 262, 8, 4), (269, 479, 14, 9)]    # h, w, load_size, tail


def check_tail_is_observable(oracle, maps, h, w):
    n, load, limit, tail = q15_geometry(h, w)
    assert 0 < tail < load <= w and limit + tail == n
    flat = [m.reshape(-1, 3) for m in maps]

    def raw(edit=None):
        ms = [m.copy() for m in flat]
        if edit:
            edit(ms)
        return oracle.icp_cost2_raw(*(m.reshape(h, w, 3) for m in ms))

    def kill(lo, hi):
        def edit(ms):
            ms[2][lo:hi] = np.nan                 # a non-finite current vertex fails the first gate
        return edit

    def tail_into_group(ms):
        for m in ms:
            m[limit - load:limit - load + tail] = m[limit:]
        ms[2][limit - load + tail:limit] = np.nan

    base = raw()
    group_dead = raw(kill(limit - load, limit))
    assert base.any() and not np.array_equal(base, group_dead)                 # the last kept group is live
    assert np.array_equal(base, raw(kill(limit, n)))                           # the tail is left out
    assert not np.array_equal(raw(tail_into_group), group_dead)                # ... although it would pass the gates
    return limit, tail


@pytest.mark.parametrize("h,w,load,tail", SIZES)
def test_q15_tail_is_observable_in_the_icp_cost2_maps(oracle, h, w, load, tail):
    assert q15_geometry(h, w)[1:] == (load, w * h - tail, tail)
    maps = icp_cost2_maps(oracle, h, w)
    limit, _ = check_tail_is_observable(oracle, maps, h, w)
    # the pixel bands of the GPU test: they cover the image, one ends inside the tail or on the image's end, the next begins there
    bands = q15_bands(h, w)
    assert bands[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(bands[:-1], bands[1:])) and sum(bands[-1]) == w * h
    ends_in_tail = [(a, n) for a, n in bands if a < limit - load and limit < a + n <= w * h - (tail > 1)]
    assert len(ends_in_tail) == 1 and (tail == 1 or bands[-1][0] == sum(ends_in_tail[0]))
    total = sum(oracle.icp_cost2_raw(*maps, first, num) for first, num in bands)
    assert np.array_equal(total, oracle.icp_cost2_raw(*maps))
    # with the normals as oracle.normal_map leaves them the same edits change nothing: the hole these maps close
    dead = [m.copy() for m in maps]
    for m in (dead[1], dead[3]):
        m[-1, :, :] = np.inf; m[:, -1, :] = np.inf
    a = oracle.icp_cost2_raw(*dead)
    dead[2].reshape(-1, 3)[limit - load:] = np.nan
    assert np.array_equal(a, oracle.icp_cost2_raw(*dead))


def test_q15_tail_is_observable_in_the_ragged_cfg4_maps(oracle):
    import svoslam_pkg
    svoslam_pkg.load()
    synth = importlib.import_module("octree_slam_amd.synth")
    w, h = 1919, 1079
    assert q15_geometry(h, w)[1:] == (59, w * h - 55, 55)
    check_tail_is_observable(oracle, cfg4_icp_maps(oracle, synth, w, h), h, w)
