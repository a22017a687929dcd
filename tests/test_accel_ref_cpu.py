"""CPU check of tests/accel_ref.py: the vectorised builders of the march's tables (grid_table, pyramid_table, brick_lines)
against the scalar rules they restate (grid_entry, grid_entry_level, brick_entry), on oracle pools of depth 10 .. 14 including
saturated ones; and the premise of the brick rebuild's shortcut (PoolAccel::mip_consistent): on pools the oracle fused from
empty, trusted and untrusted lines differ in bit 3 only.  No device code runs here."""
import numpy as np
import pytest

import accel_ref as R
from util import surface_cloud

# (depth, passes): 130 passes saturate the leaves (A += 2 per observation) and give octant-7 leaves children (Q4)
POOLS = [(10, 3), (12, 130), (13, 2), (13, 130), (14, 3)]
_CACHE = {}


def pool_words(oracle, depth, passes):
    key = (depth, passes)
    if key not in _CACHE:
        rng = np.random.default_rng(depth)
        pool = oracle.Pool()
        pts, col = surface_cloud(rng, 1500, jitter=0.002)
        for _ in range(passes):
            pool.insert_cloud(pts, col, depth, (0, 0, 0), 1.0)
        words = pool.words().copy()
        words.setflags(write=False)
        _CACHE[key] = (words, pts, R.level_states(words))
    return _CACHE[key]


def octants(x, y, z, level):
    """octant per level 1 .. `level` of cell (x, y, z) of that level"""
    return [int(((x >> (level - l)) & 1) | (((y >> (level - l)) & 1) << 1) | (((z >> (level - l)) & 1) << 2)) for l in range(1, level + 1)]


def sample_cells(rng, pts, level, n):
    """cells of `level`: those of the points, their neighbours, and uniform ones"""
    near = R.cell_of_points(pts[rng.integers(0, len(pts), n // 2)], level) + rng.integers(-2, 3, (n // 2, 3))
    cells = np.concatenate([near, rng.integers(0, 1 << level, (n - n // 2, 3))]).clip(0, (1 << level) - 1)
    return np.unique(cells, axis=0)


@pytest.mark.parametrize("center,edge", [((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 0.0), 0.05), ((0.3, -0.1, 1.5), 4.096)])
def test_cell_of_points_is_the_cell_of_the_oracles_key(oracle, center, edge):
    """the points of the device tests are placed in blocks and bricks by cell_of_points: it must name the cell the fusion's key names,
    also for points on cell boundaries and for roots whose half edge is no power of two"""
    rng = np.random.default_rng(7)
    pts = (rng.uniform(-1.0, 1.0, (4000, 3)) * edge + np.asarray(center)).astype(np.float32)
    k = np.arange(1000)
    pts[:1000, 0] = (np.float32(center[0]) + np.float32(edge) * ((k % 64) - 32).astype(np.float32) / np.float32(32.0)).astype(np.float32)   # on boundaries
    for level in (5, 9, 10, 14):
        keys = oracle.compute_keys(pts, level, center, edge)
        want = np.zeros((len(pts), 3), np.int64)
        for l in range(level):
            o = (keys >> (3 * (level - 1 - l))) & 7
            want = (want << 1) | np.stack([o & 1, (o >> 1) & 1, o >> 2], 1)
        assert np.array_equal(R.cell_of_points(pts, level, center, edge), want)


def test_brick_entry_index_and_its_inverse():
    rng = np.random.default_rng(3)
    c = rng.integers(0, R.WINDOW_CELLS, (5000, 3))
    i = R.brick_entry_index(c[:, 0], c[:, 1], c[:, 2])
    assert len(np.unique(i)) == len(np.unique(c, axis=0)) and i.max() < (1 << 33)
    assert np.array_equal(np.stack(R.brick_entry_cell(i), 1), c)
    # a brick is one 128-byte line, the 8^3 bricks of a level-6 cube of the window one 64 KB group
    assert (i >> 6 == R.brick_entry_index(c[:, 0] & ~3, c[:, 1] & ~3, c[:, 2] & ~3) >> 6).all()
    assert (i >> 15 == ((c[:, 2] >> 5) << 12 | (c[:, 1] >> 5) << 6 | (c[:, 0] >> 5))).all()


@pytest.mark.parametrize("depth,passes", POOLS)
def test_grid_and_pyramid_tables_equal_the_scalar_entries(oracle, depth, passes):
    words, pts, states = pool_words(oracle, depth, passes)
    rng = np.random.default_rng(100 + depth)
    grid = R.grid_table(words, states=states).numpy()
    pyr = R.pyramid_table(words, states=states).numpy()
    assert grid.shape == (1 << 24, 2) and pyr.shape == (R.pyr_offset(8), 2)
    flagged = 0
    for level in range(1, 9):
        cells = sample_cells(rng, pts, level, 3000) if level > 2 else np.argwhere(np.ones((1 << level,) * 3, bool))
        for x, y, z in cells.tolist():
            bits = octants(x, y, z, level)
            c = (z << (2 * level)) | (y << level) | x
            if level == 8:
                want, got = R.grid_entry(words, bits), tuple(grid[c].tolist())
                assert want == R.grid_entry_level(words, bits)
            else:
                want, got = R.grid_entry_level(words, bits), tuple(pyr[R.pyr_offset(level) + c].tolist())
            assert got == want, "level %d cell (%d, %d, %d): table %s, rule %s" % (level, x, y, z, got, want)
            flagged += bool(want[0] & R.FLAG)
    assert flagged > 500        # (the samples reach the map's nodes with children, not only empty space)


@pytest.mark.parametrize("depth,passes", POOLS)
@pytest.mark.parametrize("shift", [0, 1])
def test_brick_lines_equal_the_scalar_entries(oracle, depth, passes, shift):
    words, pts, states = pool_words(oracle, depth, passes)
    rng = np.random.default_rng(200 + depth + shift)
    cl = 11 + shift
    org = R.window_origin(shift)
    grid = R.grid_table(words, states=states).numpy()
    for trust in (False, True):
        bricks, index, value = (t.numpy() for t in R.brick_lines(words, shift, trust, states=states))
        assert len(np.unique(index)) == index.size                       # no entry is defined twice
        assert (value > 0).all() and (value < 65536).all()               # a defined entry is never "ask the level grid"
        assert ((bricks >= 0) & (bricks < 512)).all()
        table = dict(zip(index.reshape(-1).tolist(), value.reshape(-1).tolist()))
        cells = np.unique(np.concatenate([sample_cells(rng, pts, cl, 4000), R.cell_of_points(pts, cl)]), axis=0)   # every point's own cell too
        defined = stops = 0
        for x, y, z in cells.tolist():
            bits = octants(x, y, z, cl)
            g = R.grid_entry(words, bits[:8])
            inside = all(org <= c < org + R.WINDOW_CELLS for c in (x, y, z))
            want = R.brick_entry(words, g, bits[8:], shift, trust) if inside else 0
            got = table.get(int(R.brick_entry_index(x - org, y - org, z - org)), 0) if inside else 0
            assert got == want, "shift %d trust %s cell (%d, %d, %d): lines %#x, rule %#x" % (shift, trust, x, y, z, got, want)
            defined += want != 0
            stops += (want & 7) == 4
        print("shift %d trust %s: %d sampled cells, %d with an entry, %d of them at a cell-level node with children" % (shift, trust, len(cells), defined, stops))
        assert defined > 300 and (stops > 100 or depth <= cl)         # (the samples reach the lines, and the part of the rule below the cell level)
        # every flagged level-8 cell inside the window has all its 8^(1 + shift) bricks, and nothing else has any
        m8 = np.arange(1 << 24)
        x8, y8, z8 = m8 & 255, (m8 >> 8) & 255, m8 >> 16
        o8, s8 = org >> (3 + shift), R.WINDOW_CELLS >> (3 + shift)
        inside8 = (x8 >= o8) & (x8 < o8 + s8) & (y8 >= o8) & (y8 < o8 + s8) & (z8 >= o8) & (z8 < o8 + s8)
        n8 = int((((grid[:, 0] & R.FLAG) != 0) & inside8).sum())
        assert len(bricks) == n8 * 8 ** (1 + shift)


@pytest.mark.parametrize("depth,passes", POOLS + [(12, 127), (13, 128), (11, 130)])
def test_trusted_and_untrusted_lines_differ_in_bit3_only(oracle, depth, passes):
    """the premise of PoolAccel::mip_consistent: a node with children carries the maximum of its children's alphas, so a cell-level
    node with A < 254 has no saturated child -- skipping its tile loses no bit 8..15, and bit 3 is set where it might be clear"""
    words, _, states = pool_words(oracle, depth, passes)
    for shift in (0, 1):
        _, ia, a = R.brick_lines(words, shift, False, states=states)
        _, ib, b = R.brick_lines(words, shift, True, states=states)
        assert (ia == ib).all()
        diff = (a ^ b).numpy()
        bad = np.argwhere(diff & ~8)
        assert len(bad) == 0, "shift %d: %d entries differ beyond bit 3, first %s: untrusted %#x trusted %#x" % (
            shift, len(bad), tuple(bad[0]), int(a[tuple(bad[0])]), int(b[tuple(bad[0])]))
        assert ((b.numpy() & 8) >= (a.numpy() & 8)).all()                 # the trusted bit 3 is never clear where the computed one is set
        if passes >= 127 and depth >= 12 + shift:
            assert (a.numpy() >> 8).any()                                  # saturated nodes of the bits level exist: the premise is exercised
