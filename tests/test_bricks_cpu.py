"""CPU check of the occupancy bricks' RULES (csrc/pool_grid.hpp "occupancy bricks", decode() of cone_trace_brick_kernel):
brick entries and level-grid entries are built from an oracle pool exactly as brick_rebuild / grid_entry define them, and
the kernel's decode rule -- restated in Python, tests/accel_ref.py -- must give, for every sample it decides, the level and the
saturation of the node the reference's walk ends on (cone_tracing_kernels.cu:76-119, restated below as walk()).  A sample
it does not decide goes to the tree walk in the kernel; the test also checks that the samples the design promises to
decide (LOD 8..12 among nodes, empty space at or above level 8) are decided; likewise for the shape of deeper pools (shift 1:
bricks of level-10 nodes, level-12 cells, bits for level 13, inside the field's window).  No device code runs here."""
import numpy as np
import pytest

from util import surface_cloud
from accel_ref import FLAG, MASK, brick_entry, decode, grid_entry, walk   # the rules, shared with the device tests


@pytest.mark.parametrize("depth,passes,shift", [(10, 3, 0), (12, 130, 0), (13, 2, 0), (13, 130, 1), (14, 3, 1), (11, 2, 1)])
def test_brick_and_grid_entries_decide_what_the_reference_walk_finds(oracle, depth, passes, shift):
    rng = np.random.default_rng(depth)
    pool = oracle.Pool()
    pts, col = surface_cloud(rng, 1500, jitter=0.002)
    for _ in range(passes):   # 130 passes: leaves saturate (A += 2 per observation), Q4 gives octant-7 leaves children
        pool.insert_cloud(pts, col, depth, (0, 0, 0), 1.0)
    words = pool.words()
    # samples: on and around the inserted points, and uniformly in the cube; octant bits straight from coordinates (the
    # rule under test does not depend on how the kernel obtains the bits)
    near = pts[rng.integers(0, len(pts), 700)] + rng.normal(scale=0.004, size=(700, 3)).astype(np.float32)
    samples = np.concatenate([near, rng.uniform(-0.99, 0.99, size=(300, 3))]).clip(-0.999, 0.999)
    decided_among_nodes = total_among_nodes = decided_empty = total_empty = outside = 0
    cl = 11 + shift
    org, span = ((1 << cl) - 2048) // 2, 2048           # the window of the brick field, in cells of level cl (pool_grid.hpp)
    for p in samples:
        cell = np.floor((p + 1.0) * 0.5 * (1 << 16)).astype(np.int64)      # 16 levels of octant bits per axis
        bits = [int(((cell[0] >> (15 - l)) & 1) | (((cell[1] >> (15 - l)) & 1) << 1) | (((cell[2] >> (15 - l)) & 1) << 2)) for l in range(16)]
        g = grid_entry(words, bits[:8])
        inside = all(org <= int(c >> (16 - cl)) < org + span for c in cell)
        e = brick_entry(words, g, bits[8:], shift) if inside else 0
        outside += not inside
        for lod in range(1, 16):
            want_depth, want_word = walk(words, bits, lod)
            ok, got_depth, got_ret = decode(e, g, lod, bits[11 + shift], shift)
            if ok:
                assert got_depth == want_depth, (p, lod, hex(e), g, want_depth)
                assert got_ret == (1 if (want_word >> 24) >= 254 else 0), (p, lod, hex(e), g, hex(want_word))
            among = bool(g[0] & FLAG)
            if among and inside and 8 <= lod <= 12 + shift and not (shift == 1 and lod == 9):
                total_among_nodes += 1
                decided_among_nodes += ok
            if not among and lod >= 8:
                total_empty += 1
                decided_empty += ok
    # LOD 8..12 + shift among nodes inside the window: always the bricks' (or the grid's, at 8) -- except LOD 9 of shift 1 (a level-9
    # node's alpha is not kept current in the eight bricks below it)
    assert total_among_nodes > (500 if shift == 0 else 250) and decided_among_nodes == total_among_nodes
    assert total_empty > 100 and decided_empty == total_empty                       # empty space at or above level 8: always the grid's
    assert (outside > 50) == (shift == 1)                                           # shift 1: some samples lie outside the window and take the tree walk
