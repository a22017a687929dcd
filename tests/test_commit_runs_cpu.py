"""The clouds of commit_runs.py are what they claim to be, by the oracle's keys alone: the heads of the sorted keys stand at the
designed positions, the families put their runs where test_gpu_commit_runs.py needs them -- whole groups without a head, heads on
the cuts and one beside them, every common-prefix length at a tile's and at a group's edge, more tiles than the single-workgroup
straddler pass keeps in registers.  A change of the generator that moved a run off its cut fails here, without a GPU."""
import numpy as np
import pytest

import commit_runs as cr

T, G = cr.T, cr.G


def sorted_keys(oracle, pts, depth):
    return np.sort(oracle.compute_keys(pts, depth, cr.CENTER, cr.EDGE))


def heads_of(keys):
    return [0] + (np.flatnonzero(keys[1:] != keys[:-1]) + 1).tolist()


def shared_levels(a, b, depth):
    return cr.common_levels(int(a), int(b), depth)      # (both keys carry the same leading 1)


def groups_without_head(heads, n, valid_from=0):
    """straddle groups none of whose keys is a head at or after valid_from"""
    heads = np.asarray([h for h in heads if h >= valid_from])
    return [g for g in range(-(-n // G)) if not ((heads >= g * G) & (heads < min(n, (g + 1) * G))).any()]


@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c["id"])
def test_heads_are_where_the_case_puts_them(oracle, case):
    depth = case["depth"]
    assert depth in (cr.DEPTHS_MORE if case["family"] in ("on_the_cuts", "staircase", "random_runs") else cr.DEPTHS_ALL)
    clouds = cr.frames(case)
    assert len(clouds) == 3 and clouds[0][0] is clouds[1][0]
    for c, (pts, col) in ((case, clouds[0]), (cr.rotated(case), clouds[2])):
        n = cr.size(c)
        assert pts.shape == (n, 3) and pts.dtype == np.float32 and col.shape == (n, 3) and col.dtype == np.uint8
        assert len(np.unique(col.astype(np.int64) @ np.array([1, 256, 65536]))) == n         # a colour of its own for every point
        keys = sorted_keys(oracle, pts, depth)
        assert heads_of(keys) == cr.heads(c), (heads_of(keys)[:12], cr.heads(c)[:12])
        # the keys themselves: 1 for the invalid points, then the leading 1 in front of each run's rank, the outside points in the last cell
        want = ([1] if c["invalid"] else []) + [(1 << (3 * depth)) | r for r, _ in cr.all_runs(c)]
        assert keys[cr.heads(c)].tolist() == want
        assert int(np.isnan(pts).any(1).sum()) == c["invalid"] and int((np.abs(pts) > 1).any(1).sum()) == c["outside"]
    assert cr.size(case) <= 60000


def test_case_table_is_complete():
    ids = [c["id"] for c in cr.CASES]
    assert len(set(ids)) == len(ids)
    for d in cr.DEPTHS_ALL:
        assert sorted(cr.size(c) for c in cr.family("one_leaf", d)) == [T, T + 1, G - 1, G, G + 1, 2 * G + 1]
        assert sorted(c["invalid"] for c in cr.family("invalid_front", d)) == [T, G, G + T + 1]
        assert len(cr.family("invalid_only_tail", d)) == 1 and len(cr.family("siblings", d)) == 6
        assert sorted(cr.size(c) for c in cr.family("ragged_end", d)) == [G + 1, G + 1, 2 * G + T + 1, 2 * G + T + 1]
    for d in cr.DEPTHS_MORE:
        assert len(cr.family("on_the_cuts", d)) == 3 and len(cr.family("random_runs", d)) == 3 and len(cr.family("staircase", d)) >= 1
    assert {c["depth"] for c in cr.CASES} == set(cr.DEPTHS_MORE)


@pytest.mark.parametrize("name", ["one_leaf", "invalid_front"])
def test_whole_groups_without_a_head(oracle, name):
    """from a run of more than G keys on (one_leaf: n > G; invalid_front: k >= G) a whole straddle group holds no valid head;
    the shorter members hold a whole TILE without one, or are a single tile"""
    seen = 0
    for case in cr.family(name):
        pts, _ = cr.frames(case)[0]
        keys = sorted_keys(oracle, pts, case["depth"])
        n, hs = len(keys), heads_of(keys)
        valid_from = int(np.searchsorted(keys, 2))      # behind the run of key 1
        none = groups_without_head(hs, n, valid_from)
        long_run = cr.size(case) > G if name == "one_leaf" else case["invalid"] >= G
        if long_run:
            assert none, case["id"]
            assert (0 in none) == (name == "invalid_front")      # one_leaf: the groups BEHIND the head; invalid_front: group 0
            seen += 1
        elif n > T:
            tiles = [t for t in range(-(-n // T)) if not any(t * T <= h < (t + 1) * T and h >= valid_from for h in hs)]
            assert tiles, case["id"]
    assert seen >= 4      # two sizes, two depths


def test_outside_points_sort_behind_every_run_into_the_last_cell(oracle):
    for case in cr.family("invalid_only_tail"):
        depth = case["depth"]
        pts, _ = cr.frames(case)[0]
        keys = oracle.compute_keys(pts, depth, cr.CENTER, cr.EDGE)
        outside = (np.abs(pts) > 1).any(1)
        assert outside.sum() == 2 * G and (keys[outside] == ((1 << (3 * depth)) | cr.last_cell(depth))).all()
        assert keys[~outside].max() < keys[outside].min()
        s = np.sort(keys)
        hs = heads_of(s)
        assert hs[-1] == G and groups_without_head(hs, len(s)) == [2]       # the run starts ON the cut: group 1 has its head, group 2 none


@pytest.mark.parametrize("depth", cr.DEPTHS_MORE)
def test_staircase_shows_every_prefix_length_at_a_tile_and_at_a_group_edge(oracle, depth):
    at_tile, at_group = set(), set()
    for case in cr.family("staircase", depth):
        pts, _ = cr.frames(case)[0]
        keys = sorted_keys(oracle, pts, depth)
        hs = heads_of(keys)
        assert all(h % T == 0 for h in hs) and (depth == 1 or hs == list(range(0, len(keys), T)))      # run i is tile i
        for h in hs[1:]:
            c = shared_levels(keys[h], keys[h - 1], depth)
            at_tile.add(c)
            if h % G == 0:
                at_group.add(c)
        if depth > 1:
            assert len(keys) == 3 * G + T          # the last group holds one tile
    assert at_tile == set(range(depth)) and at_group == set(range(depth)), (sorted(at_tile), sorted(at_group))


@pytest.mark.parametrize("depth", cr.DEPTHS_MORE)
def test_on_the_cuts_has_a_head_on_every_cut_and_beside_it(oracle, depth):
    for case in cr.family("on_the_cuts", depth):
        shift = {"exact": 0, "plus1": 1, "minus1": -1}[case["variant"]]
        pts, _ = cr.frames(case)[0]
        hs = heads_of(sorted_keys(oracle, pts, depth))
        assert hs == [0] + [cut + shift for cut in cr.CUTS]
        assert cr.CUTS == (T, 2 * T, G - T, G, G + T, 2 * G)


@pytest.mark.parametrize("depth", cr.DEPTHS_ALL)
def test_siblings_and_ragged_ends(oracle, depth):
    want = {"siblings": depth - 1, "cousins": 1, "strangers": 0}
    for case in cr.family("siblings", depth):
        relation, _, where = case["variant"].partition("_at_")
        pts, _ = cr.frames(case)[0]
        keys = sorted_keys(oracle, pts, depth)
        hs = heads_of(keys)
        assert hs == [0, G if where == "G" else G - 1]
        assert shared_levels(keys[hs[1]], keys[hs[1] - 1], depth) == want[relation]
    for case in cr.family("ragged_end", depth):
        pts, _ = cr.frames(case)[0]
        keys = sorted_keys(oracle, pts, depth)
        n, hs = len(keys), heads_of(keys)
        assert n % T == 1                                     # the last tile holds one key,
        assert (hs[-1] == n - 1) == case["variant"].endswith("head")      # a head or the tail of a run that began tiles before
        assert case["variant"].endswith("head") or hs[-1] < n - 1 - T


def test_random_runs_have_long_and_short_runs_and_shared_prefixes(oracle):
    for case in cr.family("random_runs"):
        counts = [k for _, k in case["runs"]]
        assert case["invalid"] == 3000 and cr.size(case) == 60000
        if case["depth"] >= 3:      # (depths 1 and 2: 8 and 64 cells, the last run takes what is left)
            assert max(counts) <= 3 * G
            assert min(counts) < 64 and max(counts) > T
            ranks = [r for r, _ in case["runs"]]
            assert any(cr.common_levels(a, b, case["depth"]) >= case["depth"] - 2 for a, b in zip(ranks, ranks[1:]))


def test_huge_passes_the_register_slots_and_one_pass_of_tier_two(oracle):
    """mip_straddle_kernel keeps kSlots x kStradThreads = 8 x 1024 tiles in registers, tier 2 of mip_straddle2_kernel takes
    kStrad2Threads = 256 groups a pass"""
    case = cr.HUGE
    n = cr.size(case)
    tiles = -(-n // T)
    assert n == 8192 * T + T + 1 and tiles > 8 * 1024 and -(-tiles // 16) > 256 and n % T == 1
    clouds = cr.frames(case)
    assert len(clouds) == 2 and not np.array_equal(clouds[0][0], clouds[1][0])
    pts, col = clouds[0]
    assert pts.shape == (n, 3) and col.shape == (n, 3) and np.isfinite(pts).all() and np.abs(pts).max() < 1
    keys = sorted_keys(oracle, pts, case["depth"])
    assert len(heads_of(keys)) == 512           # every cell of depth 3, in runs of about G keys
