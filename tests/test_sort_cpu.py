"""The library's own sort and scan (svoslam_sort_words, svoslam_exclusive_scan_u32; include/svoslam.h, csrc/radix_sort.hip) restated
on the host, the case tables of tests/test_gpu_sort.py and the generators of their inputs.  No GPU.

sort_words_host and scan_host below are what the device calls must produce; tests/test_gpu_sort.py compares against them bit for
bit.  The tests here are about the INPUTS: that every distribution is what its name says, that cells_cloud's points have the keys
they were designed to have (by the oracle's computeKeys), and that the tables are not degenerate -- a sorted result that differs
from its input, runs of equal keys across a tile boundary wherever a case has duplicates by design, bit 63 in use where the packed
word is full.  A wrong generator then cannot make a device test vacuous."""
import ctypes as C
import os

import numpy as np
import pytest

U64 = np.uint64
PACKED_TILE, PAIR_TILE = 2048, 1024          # elements per workgroup of the two forms (radix_sort.hip: kPkTile, kSortTile)
SCAN_ONE_WORKGROUP, SCAN_CHUNK = 8192, 2048  # exclusive_scan_u32: one workgroup up to 8192 elements, chunks of 2048 beyond
CENTER, EDGE = (0.0, 0.0, 0.0), 1.0          # the root cube of cells_cloud: [-1, 1]^3 (a child's centre is its parent's +- edge / 2)


def load_pkg():
    import svoslam_pkg
    return svoslam_pkg.load()


def mask(bits):
    return U64((1 << bits) - 1)


def ceil_log2(n):
    return int(n - 1).bit_length()


# ---- the specification, restated -------------------------------------------------------------------------------------------
def sort_words_host(words, vals, key_bits, idx_bits, want_vals=True):
    """svoslam_sort_words in numpy -> (keys uint64, vals or None).  Packed form (idx_bits >= 0): stable order of
    (word >> idx_bits) & mask(key_bits); keys = word >> idx_bits, vals = word & mask(idx_bits) (uint64: the device keeps their low
    32 bits).  Pair form (idx_bits == -1): stable order of word & mask(key_bits); keys = the whole words, vals = the carried values
    (uint32; `vals` None: 0..n-1)."""
    words = np.ascontiguousarray(words, dtype=U64)
    if idx_bits >= 0:
        order = np.argsort((words >> U64(idx_bits)) & mask(key_bits), kind="stable")
        s = words[order]
        return s >> U64(idx_bits), ((s & mask(idx_bits)) if want_vals else None)
    assert idx_bits == -1
    order = np.argsort(words & mask(key_bits), kind="stable")
    carried = np.arange(words.shape[0], dtype=np.uint32) if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
    return words[order], (carried[order] if want_vals else None)


def scan_host(data):
    """svoslam_exclusive_scan_u32 in numpy -> (exclusive prefix sums mod 2^32 as uint32, the total mod 2^32)"""
    data = np.ascontiguousarray(data, dtype=np.uint32)
    inc = np.cumsum(data.astype(U64), dtype=U64)          # < 2^32 * n: no wrap in 64 bits for any n a test uses
    ex = np.zeros(data.shape[0], dtype=U64)
    ex[1:] = inc[:-1]
    total = int(inc[-1]) if data.shape[0] else 0
    return (ex & U64(0xFFFFFFFF)).astype(np.uint32), total & 0xFFFFFFFF


# ---- key distributions: (n, key_bits, seed) -> uint64 keys below 2^key_bits ---------------------------------------------------
def _pattern(key_bits):
    return U64(0x5A5A5A5A5A5A5A5A) & mask(key_bits)


def uniform(n, key_bits, seed):
    return np.random.default_rng(seed).integers(0, int(mask(key_bits)), n, dtype=U64, endpoint=True)


def all_equal(n, key_bits, seed):
    return np.full(n, _pattern(key_bits) | U64(1 if key_bits < 2 else 0), dtype=U64)


def two_alternating(n, key_bits, seed):
    """the larger value first: mask, mask >> 1 (1, 0 at one bit), so the sort has to swap every pair"""
    k = np.empty(n, dtype=U64)
    k[0::2] = mask(key_bits)
    k[1::2] = mask(key_bits) >> U64(1)
    return k


def top_digit(n, key_bits, seed):
    """only the top min(key_bits, 4) bits vary: every pass below the last sees one digit value"""
    top = min(key_bits, 4)
    low = _pattern(key_bits) & mask(key_bits - top)
    return (np.random.default_rng(seed).integers(0, 1 << top, n, dtype=U64) << U64(key_bits - top)) | low


def bit0(n, key_bits, seed):
    """only bit 0 varies: every pass above the first sees one digit value"""
    return (_pattern(key_bits) & ~U64(1)) | np.random.default_rng(seed).integers(0, 2, n, dtype=U64)


def all_equal_ones(n, key_bits, seed):
    """every bit set: every digit of every pass is bins - 1"""
    return np.full(n, mask(key_bits), dtype=U64)


def ascending(n, key_bits, seed):
    i = np.arange(n, dtype=U64)
    if (1 << key_bits) >= n:
        return i * U64((1 << key_bits) // max(n, 1))
    return (i << U64(key_bits)) // U64(n)      # more elements than values: nondecreasing, with duplicates


def descending(n, key_bits, seed):
    return ascending(n, key_bits, seed)[::-1].copy()


def wave_runs(n, key_bits, seed):
    """blocks of 128 = two wavefronts: 64 equal keys beside 64 distinct ones (as distinct as key_bits allows), so the ballot match
    loop of a downsweep sees a wavefront of one digit and a wavefront of many in one tile"""
    rng = np.random.default_rng(seed)
    blocks = (n + 127) // 128
    # (three base keys for all blocks: the equal halves of blocks that share one make runs far longer than a tile)
    base = rng.integers(0, int(mask(key_bits)), 3, dtype=U64, endpoint=True)[rng.integers(0, 3, blocks)]
    k = np.repeat(base, 128)
    j = np.arange(blocks * 128, dtype=U64) % U64(128)
    distinct = (k + (j - U64(63)) * U64(0x9E3779B97F4A7C15 & int(mask(key_bits)) | 1)) & mask(key_bits)
    return np.where(j < U64(64), k, distinct)[:n].copy()


def heavy(n, key_bits, seed):
    """one key takes 90 % of the array"""
    rng = np.random.default_rng(seed)
    k = uniform(n, key_bits, seed + 1)
    k[rng.random(n) < 0.9] = _pattern(key_bits)
    return k


DISTRIBUTIONS = {f.__name__: f for f in (uniform, all_equal, two_alternating, top_digit, bit0, all_equal_ones, ascending, descending,
                                          wave_runs, heavy)}
SORTED_BY_NAME = ("ascending", "all_equal", "all_equal_ones")    # the sorted result IS the input: the name says so
DUPLICATES_BY_NAME = ("all_equal", "two_alternating", "top_digit", "bit0", "all_equal_ones", "wave_runs", "heavy")


def has_designed_duplicates(n, key_bits, dist):
    """duplicates by design: the distribution repeats keys whatever key_bits is, or there are at least four elements per value
    (so that a run of equal keys is long enough to lie across a given position; two uniform keys that merely happen to be equal
    do not make a case `one with duplicates`)"""
    return n > 1 and (dist in DUPLICATES_BY_NAME or n >= 4 * (1 << min(key_bits, 40)))


# ---- the tables of tests/test_gpu_sort.py --------------------------------------------------------------------------------------
# (n, key_bits, idx_bits, digit_bits, want_vals, distribution); idx_bits = ceil(log2 n) unless the comment says otherwise
PACKED_CASES = [
    (1, 1, 0, 11, 1, "uniform"),
    (1, 49, 15, 11, 1, "all_equal_ones"),               # idx_bits = 64 - key_bits
    (2, 1, 1, 1, 1, "descending"),
    (2, 37, 1, 11, 1, "descending"),
    (63, 4, 6, 5, 1, "descending"),
    (64, 11, 6, 11, 1, "uniform"),
    (65, 12, 7, 8, 1, "descending"),
    (65, 23, 7, 9, 1, "uniform"),
    (2047, 11, 11, 11, 1, "uniform"),
    (2047, 22, 11, 5, 1, "heavy"),
    (2048, 12, 11, 11, 1, "two_alternating"),
    (2048, 37, 11, 8, 1, "uniform"),
    (2049, 1, 12, 1, 1, "bit0"),
    (2049, 4, 12, 5, 1, "uniform"),
    (2049, 23, 12, 11, 1, "all_equal"),
    (2049, 43, 12, 9, 1, "descending"),
    (2049, 49, 12, 11, 1, "top_digit"),
    (4095, 12, 12, 1, 1, "uniform"),                    # twelve passes of one bit
    (4095, 37, 12, 11, 1, "wave_runs"),
    (4097, 11, 13, 8, 1, "heavy"),
    (4097, 22, 13, 11, 1, "two_alternating"),
    (4097, 22, 13, 11, 0, "uniform"),                   # index bits in the word, not unpacked
    (4097, 43, 13, 11, 1, "uniform"),
    (4097, 49, 13, 5, 1, "bit0"),                       # ten passes
    (3 * 2048 + 1, 12, 13, 9, 1, "all_equal_ones"),
    (3 * 2048 + 1, 23, 13, 8, 1, "wave_runs"),
    (3 * 2048 + 1, 37, 13, 11, 1, "descending"),
    (100003, 4, 17, 11, 1, "uniform"),
    (100003, 11, 17, 5, 1, "ascending"),
    (100003, 12, 17, 0, 1, "two_alternating"),          # digit_bits 0: the width the map's calls take (11 at this size)
    (100003, 22, 17, 11, 1, "uniform"),
    (100003, 23, 17, 8, 1, "top_digit"),
    (100003, 37, 17, 11, 1, "heavy"),
    (100003, 43, 17, 9, 1, "wave_runs"),
    # idx_bits = 0, want_vals = 0: the voxel-grid form, the words are the keys and repeat
    (2049, 37, 0, 8, 0, "wave_runs"),
    (4097, 22, 0, 11, 0, "heavy"),
    (100003, 12, 0, 9, 0, "uniform"),
    (100003, 43, 0, 11, 0, "heavy"),
    # idx_bits = 64 - key_bits: the word is full, keys with their top bit set put bit 63 to use
    (65, 37, 27, 8, 1, "two_alternating"),
    (2049, 49, 15, 11, 1, "uniform"),
    (4097, 43, 21, 11, 1, "descending"),
    (3 * 2048 + 1, 12, 52, 5, 1, "heavy"),
    (100003, 23, 41, 9, 1, "wave_runs"),
]

# the chunked column scan of the packed sort is taken above 8192 tiles (hard-coded in radix_sort.hip): one case on either side
COLUMN_SCAN_CASES = [(8192 * PACKED_TILE + 1, 16, 25, 8), (8192 * PACKED_TILE, 16, 25, 8)]   # (n, key_bits, idx_bits, digit_bits)

# (n, key_bits, values, distribution, bits above key_bits in the words)
PAIR_CASES = [
    (1, 8, "iota", "uniform", False),
    (1, 64, "given", "uniform", False),
    (255, 1, "iota", "bit0", False),
    (255, 37, "given", "uniform", False),
    (256, 8, "iota", "descending", False),
    (256, 64, "iota", "uniform", False),
    (257, 9, "given", "wave_runs", False),
    (257, 51, "iota", "two_alternating", False),
    (1023, 8, "iota", "uniform", False),
    (1023, 49, "given", "heavy", False),
    (1024, 9, "iota", "two_alternating", False),
    (1024, 37, "given", "descending", False),
    (1025, 1, "iota", "bit0", False),
    (1025, 8, "given", "all_equal", False),
    (1025, 51, "iota", "top_digit", False),
    (1025, 64, "given", "wave_runs", False),
    (4 * 1024 + 1, 9, "iota", "uniform", False),
    (4 * 1024 + 1, 37, "given", "wave_runs", False),
    (4 * 1024 + 1, 49, "iota", "descending", False),
    (4 * 1024 + 1, 64, "iota", "all_equal_ones", False),
    (50001, 8, "given", "uniform", False),
    (50001, 37, "iota", "heavy", False),
    (50001, 49, "given", "top_digit", False),
    (50001, 51, "given", "uniform", False),               # the surface weld's corner key at depth 16
    (50001, 64, "iota", "heavy", False),
    # the contract is `on bits [0, key_bits)`: what lies above must order nothing and arrive intact
    (1025, 9, "given", "two_alternating", True),
    (4 * 1024 + 1, 37, "iota", "uniform", True),
]

SCAN_SIZES = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 8192 + 2048, 10 * 2048 + 1, 256 * 2048 + 3, 1000003]
SCAN_VALUES = ("small", "zero", "one", "max", "any")

FUSE_DEPTHS = (1, 3, 4, 8, 12, 14, 16)
FUSE_SIZES = (1, 2, 2047, 2048, 2049, 3 * 2048 + 1)
FUSE_SIZES_DEPTH16 = (32768, 32769)      # 49 + 15 bits: the last packed size; 49 + 16: the pair sort takes over on its own


def case_seed(*parts):
    s = 0
    for p in parts:
        s = (s * 1000003 + (sum(p.encode()) if isinstance(p, str) else int(p))) & 0x7FFFFFFF
    return s


def packed_words(n, key_bits, idx_bits, dist):
    """the words of a packed case: key << idx_bits | element number (the keys alone at idx_bits = 0)"""
    keys = DISTRIBUTIONS[dist](n, key_bits, case_seed(n, key_bits, dist))
    if idx_bits == 0:
        return keys
    assert n <= (1 << idx_bits)
    return (keys << U64(idx_bits)) | np.arange(n, dtype=U64)


def pair_inputs(n, key_bits, values, dist, high):
    """(words, vals or None) of a pair case"""
    rng = np.random.default_rng(case_seed(n, key_bits, dist, 7))
    words = DISTRIBUTIONS[dist](n, key_bits, case_seed(n, key_bits, dist))
    if high:
        assert key_bits < 64
        words = words | (rng.integers(0, 1 << (64 - key_bits), n, dtype=U64) << U64(key_bits))
    vals = None
    if values == "given":
        vals = rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint32, endpoint=True)
        vals[-1] = 0xFFFFFFFF
        if n > 1:
            vals[0] = 0
    return words, vals


def scan_input(n, kind):
    rng = np.random.default_rng(case_seed(n, kind))
    if kind == "small":
        return rng.integers(0, 1000, n, dtype=np.uint32)
    if kind == "any":
        return rng.integers(0, 0xFFFFFFFF, n, dtype=np.uint32, endpoint=True)
    return np.full(n, {"zero": 0, "one": 1, "max": 0xFFFFFFFF}[kind], dtype=np.uint32)


# ---- points with designed keys ---------------------------------------------------------------------------------------------
def cells_cloud(depth, cells, nan_every=0):
    """-> (points float32 [n, 3], designed keys uint64 [n]).  Point i sits at the centre of the depth-`depth` cell of the root cube
    (CENTER, EDGE) whose Morton code (3 bits per level, x + 2 y + 4 z, the top level first) is cells[i]: its key is
    1 << 3 depth | cells[i].  A cell's centre is -1 + (2 c + 1) 2^-depth per axis: exact in float32 up to depth 16, and never equal
    to the centre of an enclosing cell, so no comparison of computeKeys is a tie.  nan_every > 0: every nan_every-th point is made
    special, in turn: x = NaN, z = +inf, x = -inf (key 1: the finite test reads x and z), and y = NaN, which the finite test does
    not read (Q1) -- the point keeps its key with every y bit cleared, since no comparison with a NaN holds."""
    cells = np.ascontiguousarray(cells, dtype=U64)
    n = cells.shape[0]
    assert 1 <= depth <= 16 and (n == 0 or int(cells.max()) < (1 << (3 * depth)))
    coord = np.zeros((n, 3), dtype=np.int64)
    for level in range(depth):                      # level 0 = the root's octant = the top three bits
        octant = ((cells >> U64(3 * (depth - 1 - level))) & U64(7)).astype(np.int64)
        for a in range(3):
            coord[:, a] = (coord[:, a] << 1) | ((octant >> a) & 1)
    pts = (-1.0 + (2 * coord + 1) * 2.0 ** -depth).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), -1.0 + (2 * coord + 1) * 2.0 ** -depth)      # exact
    keys = cells | U64(1 << (3 * depth))
    if nan_every:
        y_bits = U64(sum(2 << (3 * level) for level in range(depth)))
        for j, i in enumerate(range(nan_every - 1, n, nan_every)):
            kind = j % 4
            if kind == 0:
                pts[i, 0] = np.nan; keys[i] = 1
            elif kind == 1:
                pts[i, 2] = np.inf; keys[i] = 1
            elif kind == 2:
                pts[i, 0] = -np.inf; keys[i] = 1
            else:
                pts[i, 1] = np.nan; keys[i] = keys[i] & ~y_bits
    return pts, keys


FUSE_DISTRIBUTIONS = ("uniform", "wave_runs", "descending", "two_alternating", "top_digit", "bit0", "all_equal")


def fuse_distribution(depth, n):
    sizes = FUSE_SIZES + FUSE_SIZES_DEPTH16
    return "descending" if n == 2 else FUSE_DISTRIBUTIONS[(FUSE_DEPTHS.index(depth) + sizes.index(n)) % len(FUSE_DISTRIBUTIONS)]


def fuse_cloud(depth, n):
    """the points of one case of the fusion's own sort path, and their designed keys"""
    dist = fuse_distribution(depth, n)
    cells = DISTRIBUTIONS[dist](n, 3 * depth, case_seed(depth, n, dist))
    return cells_cloud(depth, cells, nan_every=7 if n >= 7 else 0)


def fuse_cases():
    return [(d, n) for d in FUSE_DEPTHS for n in FUSE_SIZES + (FUSE_SIZES_DEPTH16 if d == 16 else ())]


def crosses_a_tile_boundary(sorted_keys, tile):
    """a run of equal keys of the sorted array lies on both sides of a multiple of `tile`"""
    edges = np.arange(tile, sorted_keys.shape[0], tile)
    return bool(edges.size) and bool((sorted_keys[edges - 1] == sorted_keys[edges]).any())


# ---- tests of the restatement ----------------------------------------------------------------------------------------------
def test_sort_words_host_by_hand():
    # packed: keys 2, 1, 2, 1 with indices 0..3 in two index bits, a bit above the key that must order nothing
    words = np.array([2 << 2 | 0, 1 << 2 | 1, (4 | 2) << 2 | 2, 1 << 2 | 3], dtype=U64)
    keys, vals = sort_words_host(words, None, 2, 2)
    assert keys.tolist() == [1, 1, 2, 6] and vals.tolist() == [1, 3, 0, 2] and keys.dtype == U64
    keys, vals = sort_words_host(words, None, 2, 2, want_vals=False)
    assert keys.tolist() == [1, 1, 2, 6] and vals is None
    # bit 63
    words = np.array([0x8000000000000001, 0x0000000000000003, 0x8000000000000000], dtype=U64)
    keys, vals = sort_words_host(words, None, 63, 1)
    assert keys.tolist() == [1, 0x4000000000000000, 0x4000000000000000] and vals.tolist() == [1, 1, 0]
    # pairs: on the low bits alone, the whole word travels, equal keys keep their order
    words = np.array([0x8000000000000001, 0x30, 0x0000000000000001, 0xF0], dtype=U64)
    keys, vals = sort_words_host(words, None, 4, -1)
    assert keys.tolist() == [0x30, 0xF0, 0x8000000000000001, 1] and vals.tolist() == [1, 3, 0, 2] and vals.dtype == np.uint32
    keys, vals = sort_words_host(words, np.array([0xFFFFFFFF, 7, 0, 9], np.uint32), 64, -1)
    assert keys.tolist() == [1, 0x30, 0xF0, 0x8000000000000001] and vals.tolist() == [0, 7, 9, 0xFFFFFFFF]


def test_sort_words_host_against_python_sorted():
    rng = np.random.default_rng(5)
    for key_bits, idx_bits in ((3, 9), (11, 9), (54, 9), (5, 0)):
        words = packed_words(500, key_bits, idx_bits, "uniform") | (rng.integers(0, 2, 500, dtype=U64) << U64(key_bits + idx_bits))
        keys, vals = sort_words_host(words, None, key_bits, idx_bits)
        want = sorted(range(500), key=lambda i: (int(words[i]) >> idx_bits) & ((1 << key_bits) - 1))     # sorted() is stable
        assert keys.tolist() == [int(words[i]) >> idx_bits for i in want]
        assert vals.tolist() == [int(words[i]) & ((1 << idx_bits) - 1) for i in want]


def test_scan_host_by_hand():
    ex, total = scan_host(np.array([3, 0, 5, 1], np.uint32))
    assert ex.tolist() == [0, 3, 3, 8] and total == 9 and ex.dtype == np.uint32
    ex, total = scan_host(np.array([0xFFFFFFFF, 0xFFFFFFFF, 2, 0xFFFFFFFF], np.uint32))
    assert ex.tolist() == [0, 0xFFFFFFFF, 0xFFFFFFFE, 0] and total == 0xFFFFFFFF
    ex, total = scan_host(np.zeros(0, np.uint32))
    assert ex.shape == (0,) and total == 0
    big = scan_input(70000, "max")
    ex, total = scan_host(big)
    assert ex[65536] == 0xFFFF0000 and ex[65537] == 0xFFFEFFFF and total == (70000 * 0xFFFFFFFF) % (1 << 32)


# ---- tests of the generators -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits", [1, 4, 11, 37, 64])
def test_every_distribution_is_what_its_name_says(key_bits):
    n, m = 1000, int(mask(key_bits))
    for name, f in DISTRIBUTIONS.items():
        k = f(n, key_bits, 3)
        assert k.dtype == U64 and k.shape == (n,) and int(k.max()) <= m, name
        assert np.array_equal(k, f(n, key_bits, 3)), name                     # a function of its arguments
    assert np.unique(all_equal(n, key_bits, 0)).size == 1
    assert np.unique(all_equal_ones(n, key_bits, 0)).tolist() == [m]
    k = two_alternating(n, key_bits, 0)
    assert np.unique(k).size == 2 and (k[0::2] > k[1::2]).all() and (k[0::2] == k[0]).all() and (k[1::2] == k[1]).all()
    top = min(key_bits, 4)
    k = top_digit(n, key_bits, 0)
    assert np.unique(k & mask(key_bits - top)).size == 1 and np.unique(k >> U64(key_bits - top)).size == 1 << top
    k = bit0(n, key_bits, 0)
    assert np.unique(k >> U64(1)).size == 1 and np.unique(k & U64(1)).size == 2
    k = ascending(n, key_bits, 0)
    assert (k[1:] >= k[:-1]).all() and k[-1] > k[0] and np.array_equal(descending(n, key_bits, 0), k[::-1])
    if (1 << key_bits) >= n:
        assert (k[1:] > k[:-1]).all()
    k = heavy(n, key_bits, 0)
    assert 0.85 * n <= np.bincount(np.unique(k, return_inverse=True)[1]).max() <= (0.95 * n if key_bits > 4 else n)
    k = uniform(4000, key_bits, 0)
    distinct = np.unique(k).size
    assert distinct == 1 << key_bits if key_bits <= 4 else (distinct == 4000 if key_bits >= 37 else distinct > 1000)
    assert int(k.max()) >> (key_bits - 1) == 1 and int(k.min()) >> (key_bits - 1) == 0


@pytest.mark.parametrize("key_bits", [9, 23, 64])
def test_wave_runs_puts_a_wavefront_of_one_key_beside_a_wavefront_of_many(key_bits):
    k = wave_runs(1000, key_bits, 1)
    for b in range(0, 896, 128):
        assert np.unique(k[b:b + 64]).size == 1 and np.unique(k[b + 64:b + 128]).size == 64
        assert k[b] not in k[b + 64:b + 128]


def test_cells_cloud_has_its_designed_keys(oracle):
    """the oracle's computeKeys gives every point of every fusion case the key it was designed to have (the special points
    included), and the points are the centres of their cells"""
    for depth, n in fuse_cases():
        pts, keys = fuse_cloud(depth, n)
        assert pts.dtype == np.float32 and pts.shape == (n, 3) and keys.dtype == U64
        got = oracle.compute_keys(pts, depth, CENTER, EDGE).view(U64)
        assert np.array_equal(got, keys), (depth, n, np.nonzero(got != keys)[0][:5])
        if n >= 28:
            special = np.arange(6, n, 7)
            assert (keys[special[0::4]] == 1).all() and (keys[special[1::4]] == 1).all() and (keys[special[2::4]] == 1).all()
            assert (keys[special[3::4]] >> U64(3 * depth) == 1).all() and np.isnan(pts[special[3::4], 1]).all()
            ordinary = np.setdiff1d(np.arange(n), special)
            assert np.isfinite(pts[ordinary]).all() and (keys[ordinary] >> U64(3 * depth) == 1).all()


def test_cells_cloud_by_hand(oracle):
    # depth 2: code 0b110_001 = octant 6 (y, z high) then octant 1 (x high): x = 01 -> cell 1, y = 10 -> cell 2, z = 10 -> cell 2
    pts, keys = cells_cloud(2, [0b110001, 0, 63])
    assert pts.tolist() == [[-0.25, 0.25, 0.25], [-0.75, -0.75, -0.75], [0.75, 0.75, 0.75]]
    assert keys.tolist() == [64 | 0b110001, 64, 127]
    for p, k in zip(pts, keys):
        assert oracle.compute_key(p, CENTER, 2, EDGE) == int(k)
    pts, keys = cells_cloud(16, [(1 << 48) - 1, 0x5A5A5A5A5A5A], nan_every=2)
    assert pts[0].tolist() == [1.0 - 2.0 ** -16] * 3 and keys[0] == (1 << 49) - 1 and keys[1] == 1 and np.isnan(pts[1, 0])


# ---- the tables are not degenerate -----------------------------------------------------------------------------------------
def test_the_packed_table_holds_what_it_must():
    ns = {c[0] for c in PACKED_CASES}
    assert ns == {1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4097, 3 * 2048 + 1, 100003}
    assert {c[1] for c in PACKED_CASES} == {1, 4, 11, 12, 22, 23, 37, 43, 49}
    assert {c[3] for c in PACKED_CASES} >= {1, 5, 8, 9, 11}
    assert set(DISTRIBUTIONS) == {c[5] for c in PACKED_CASES} | {c[3] for c in PAIR_CASES}
    assert 38 <= len(PACKED_CASES) <= 48 and len(set(PACKED_CASES)) == len(PACKED_CASES)
    for n, key_bits, idx_bits, digit_bits, want_vals, dist in PACKED_CASES:
        assert key_bits + idx_bits <= 64 and 0 <= digit_bits <= 11
        assert idx_bits in (ceil_log2(n), 64 - key_bits) or (idx_bits == 0 and not want_vals), (n, key_bits, idx_bits)
    assert sum(1 for c in PACKED_CASES if c[2] == ceil_log2(c[0]) and c[0] > 1) >= 25
    assert sum(1 for c in PACKED_CASES if c[2] == 0 and not c[4] and c[0] > 1) >= 3
    assert sum(1 for c in PACKED_CASES if c[1] + c[2] == 64 and c[0] > 1) >= 4
    # one to five passes at 11 bits, of even and uneven widths
    assert {-(-c[1] // 11) for c in PACKED_CASES if c[3] == 11} == {1, 2, 3, 4, 5}
    for n, key_bits, idx_bits, digit_bits in COLUMN_SCAN_CASES:
        assert key_bits + idx_bits <= 64 and n <= (1 << idx_bits)
    assert [-(-c[0] // PACKED_TILE) for c in COLUMN_SCAN_CASES] == [8193, 8192]


@pytest.mark.parametrize("case", PACKED_CASES, ids=lambda c: "%d-%d-%d-%d-%d-%s" % c)
def test_packed_case_is_not_degenerate(case):
    n, key_bits, idx_bits, digit_bits, want_vals, dist = case
    words = packed_words(n, key_bits, idx_bits, dist)
    keys, vals = sort_words_host(words, None, key_bits, idx_bits, bool(want_vals))
    assert int((words >> U64(idx_bits)).max()) < (1 << key_bits)
    assert ((keys[1:] & mask(key_bits)) >= (keys[:-1] & mask(key_bits))).all()
    if want_vals and idx_bits:
        assert np.array_equal(np.sort(vals), np.arange(n, dtype=U64))             # a permutation of the element numbers
    if n > 1 and dist not in SORTED_BY_NAME:
        assert not np.array_equal(keys, words >> U64(idx_bits)), "the sorted keys are the input"
    if key_bits + idx_bits == 64 and n > 1 and dist not in SORTED_BY_NAME:
        top = words >> U64(63)
        assert top.any() and not top.all(), "bit 63 is not in use"
    if has_designed_duplicates(n, key_bits, dist):
        assert (keys[1:] == keys[:-1]).any()
        if n > PACKED_TILE:
            assert crosses_a_tile_boundary(keys, PACKED_TILE), "no run of equal keys across a multiple of 2048"
    if idx_bits == 0 and n > 1:
        assert np.unique(words).size < n                                           # the voxel-grid form: the words repeat


def test_the_pair_table_holds_what_it_must():
    assert {c[0] for c in PAIR_CASES} == {1, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 1, 50001}
    assert {c[1] for c in PAIR_CASES} == {1, 8, 9, 37, 49, 51, 64}
    assert {c[2] for c in PAIR_CASES} == {"iota", "given"} and sum(1 for c in PAIR_CASES if c[4]) >= 1
    assert len(set(PAIR_CASES)) == len(PAIR_CASES)


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: "%d-%d-%s-%s-%d" % c)
def test_pair_case_is_not_degenerate(case):
    n, key_bits, values, dist, high = case
    words, vals = pair_inputs(n, key_bits, values, dist, high)
    keys, out = sort_words_host(words, vals, key_bits, -1)
    low = keys & mask(key_bits)
    assert (low[1:] >= low[:-1]).all() and np.array_equal(np.sort(keys), np.sort(words))
    if vals is not None:
        assert int(vals.max()) == 0xFFFFFFFF and (n == 1 or int(vals.min()) == 0)
    if n > 1 and dist not in SORTED_BY_NAME:
        assert not np.array_equal(keys, words), "the sorted words are the input"
    if high:
        assert np.unique(words >> U64(key_bits)).size > n // 2
        assert not np.array_equal(keys, np.sort(words)), "the bits above the key would order the same way"
    if has_designed_duplicates(n, key_bits, dist):
        assert (low[1:] == low[:-1]).any()
        if n > PAIR_TILE:
            assert crosses_a_tile_boundary(low, PAIR_TILE), "no run of equal keys across a multiple of 1024"


def test_fusion_cases_are_not_degenerate():
    assert set(fuse_cases()) >= {(16, 32768), (16, 32769)} and len(fuse_cases()) == 7 * 6 + 2
    assert ceil_log2(32768) + 49 == 64 and ceil_log2(32769) + 49 == 65
    for depth, n in fuse_cases():
        _, keys = fuse_cloud(depth, n)
        order = np.argsort(keys, kind="stable")
        if n > 1:
            assert not np.array_equal(order, np.arange(n)), (depth, n)
        if n > PACKED_TILE and has_designed_duplicates(n, 3 * depth, fuse_distribution(depth, n)):
            assert crosses_a_tile_boundary(keys[order], PACKED_TILE), (depth, n)


def test_scan_sizes_sit_on_both_sides_of_every_switch():
    s = set(SCAN_SIZES)
    assert {0, 1, SCAN_ONE_WORKGROUP - 1, SCAN_ONE_WORKGROUP, SCAN_ONE_WORKGROUP + 1} <= s
    assert {255, 256, 257, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1} <= s
    assert any(-(-n // SCAN_CHUNK) > 256 and n % SCAN_CHUNK for n in s)      # more chunk sums than one round of the sums' scan
    for kind in SCAN_VALUES:
        assert scan_input(5000, kind).dtype == np.uint32
    assert scan_host(scan_input(1000003, "max"))[1] == (1000003 * 0xFFFFFFFF) % (1 << 32)
    assert scan_host(scan_input(8193, "one"))[0][-1] == 8192


def test_library_exports_the_sort_and_scan_calls():
    pkg = load_pkg()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_sort_words", "svoslam_exclusive_scan_u32"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert hasattr(pkg, "sort_words") and hasattr(pkg, "exclusive_scan_u32")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svoslam.h")).read()
    assert "int svoslam_sort_words(svoslam_workspace *ws, const unsigned long long *d_words, const uint32_t *d_vals, int32_t n," in header
    assert "int svoslam_exclusive_scan_u32(svoslam_workspace *ws, uint32_t *d_data, uint32_t n, uint32_t *d_total, void *stream);" in header
    assert "#define SVOSLAM_ABI_VERSION 1" in header
