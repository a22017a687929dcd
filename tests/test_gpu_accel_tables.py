"""The tables the ray march reads instead of the octree (csrc/pool_grid.hpp: the level-8 grid, the pyramid of levels 1..7 behind it,
the occupancy bricks in both shapes), ENTRY BY ENTRY against the rules of tests/accel_ref.py, after every kind of upkeep: dirty
level-5 blocks, the stale-brick ring and its dedupe bits, the sibling ring, node 0's colour word, the mip_consistent shortcut, a
lapped ring, full rebuilds on invalidation and on a change of shape, deferred commits, re-indexing and growth.  A render reads only
the entries its rays touch; these tests read all of them through Pool.accel_view() (svoslam_pool_accel_view: addresses and host
state, nothing launched), so a failure names the table, the cell and its level, and the value found beside the one wanted.

What is asserted of the bricks (check_tables): every entry of every line the rules define is the rule's value or 0 ("ask the level
grid"); the bricks on the paths of the keys committed since the previous check are exact and nonzero; where no ring was lapped no
defined entry reads 0 (pool_grid.hpp: the sibling ring completes the childless siblings a commit's splits create); nothing else
in the 16 GiB field is nonzero, and a 64 KB group whose touched bit is clear is all zero.  ONE bit is compared only where the march
reads it: bit 4 of the second shape (A >= 254 of the level-9 node above the brick node) lives in the eight bricks below that node, of
which a commit rebuilds the one on its key's path -- the march takes it only from an entry whose path stops AT level 9 (stop code 5,
decode() in accel_ref.py), and there it is compared; in a rebuilt brick every bit is."""
import numpy as np
import pytest

import accel_ref as R
import node0_scenes as S
from accel_check import CENTER, EDGE, SCAN_GROUPS, DeviceMem, Rig, cell_text, check_marks, check_tables
from util import surface_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


def new_points(rng, n, jitter=0.004):
    return surface_cloud(rng, n, jitter=jitter)


# ---- scenarios ----------------------------------------------------------------------------------------------------------------
def test_device_mem_reads_the_same_in_place_and_by_copies(env):
    """DeviceMem's two ways to the memory, held to a tensor whose contents are known (three parts of a scan, the last one short)"""
    pkg, torch = env
    n = 2 * SCAN_GROUPS * R.GROUP_ENTRIES + 12345
    src = torch.randint(-32768, 32768, (n,), dtype=torch.int16, device="cuda")
    idx = torch.randint(0, n, (1000, 64), dtype=torch.int64, device="cuda")
    want = src[idx].to(torch.int64) & 0xFFFF
    for in_place in (True, False):
        mem = DeviceMem(env, src.data_ptr(), 2 * n)
        if not in_place:
            mem.view = None
        assert torch.equal(mem.part(64, 2 * n - 2).view(torch.int16), src[32:n - 1])
        assert torch.equal(mem.gather16(idx), want)



@pytest.mark.parametrize("depth", [10, 12, 14])
def test_incremental_direct_commits(env, oracle, depth):
    """an empty pool rendered, a first commit (its splits above level 5 mark whole cubes), three commits of a few hundred new points"""
    rng = np.random.default_rng(depth)
    rig = Rig(env, oracle)
    rig.render()
    seen = rig.check("empty pool, first render", words=np.zeros(16, np.uint32))
    assert seen["lines"] == 0
    pts, col = surface_cloud(rng, 5000, jitter=0.002)
    rig.fuse(pts, col, depth)
    marked = rig.marks("first commit")
    assert len(marked) > len(np.unique(R.cell_of_points(pts, 5), axis=0))     # splits above level 5 marked whole cubes
    rig.render()
    seen = rig.check("first commit")
    assert seen["bricks"] and seen["view"]["brick_shift"] == (0 if depth <= 12 else 1) and seen["lines"] > 0
    for k in range(3):
        extra, ecol = new_points(rng, 300)
        rig.fuse(extra, ecol, depth)
        rig.marks("commit %d" % (k + 2))
        rig.render()
        seen = rig.check("commit %d of a few hundred new points" % (k + 2))
        assert seen["recent"] > 0
    assert seen["view"]["mip_consistent"]


@pytest.mark.parametrize("depth", [10, 12, 14])
def test_two_commits_between_renders_and_a_render_without_a_commit(env, oracle, depth):
    rng = np.random.default_rng(100 + depth)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 4000, jitter=0.002)
    rig.fuse(pts, col, depth)
    rig.render()
    rig.recent = []
    for k in range(2):     # the second commit finds the first one's marks and ring entries unserved
        extra, ecol = new_points(rng, 400)
        rig.fuse(np.concatenate([pts[:500], extra]), np.concatenate([col[:500], ecol]), depth)
        rig.marks("commit %d without a render" % (k + 1))
    rig.render()
    rig.check("two commits, then one render")
    grid_before = rig.pool.accel_grid()
    rig.render()           # nothing is dirty: the tables are unchanged
    seen = rig.check("a second render without a commit")
    grid_after = rig.pool.accel_grid()
    assert np.array_equal(grid_before[0], grid_after[0]) and np.array_equal(grid_before[1], grid_after[1])
    assert seen["missing"] == 0


@pytest.mark.parametrize("depth", [12, 13])
def test_saturation_flips_the_alpha_bits(env, oracle, depth):
    """the same cloud 130 times, rendered after every pass (incremental upkeep throughout).  A leaf's alpha is 127 + 2 per observation
    (the oracle's words: 253 after pass 63, 255 after pass 64), so the A >= 254 bits -- bits 4..6 of the path, bit 7 of the second
    shape, bits 8..15 of the bits level -- flip between passes 63 and 64: checked at 63, 64, 65, and at 126, 127, 128, where a leaf has
    been observed 127 times and every alpha has long stopped at 255"""
    rng = np.random.default_rng(depth)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 1500, jitter=0.002)
    sat = {}
    for p in range(1, 131):
        rig.fuse(pts, col, depth)
        rig.render()
        if p in (63, 64, 65, 126, 127, 128):
            sat[p] = rig.check("pass %d of the same cloud" % p)
        else:
            rig.recent = []
    counts = {p: (s["sat_bits"], s["bit7"], s["deep_bits"]) for p, s in sat.items()}
    assert sat[63]["sat_bits"] == 0 < sat[64]["sat_bits"] <= sat[128]["sat_bits"], counts      # (of the rules' lines: the scenario reaches the flip)
    assert sat[63]["deep_bits"] == 0 < sat[64]["deep_bits"], counts
    if depth == 13:
        assert sat[63]["bit7"] == 0 < sat[64]["bit7"], counts
    assert sat[128]["view"]["mip_consistent"]


def octant0_entries(level):
    """numbers of the level-`level` cells under octant 0 of the root"""
    h = np.arange(1 << (level - 1), dtype=np.int64)
    return ((h[:, None, None] << (2 * level)) | (h[None, :, None] << level) | h[None, None, :]).reshape(-1)


def test_node0_word_in_every_entry_that_holds_it(env, oracle):
    """tests/node0_scenes.py "stale": commits into octant 7 rewrite node 0's colour word (the root pass Q6) and mark no block of octant
    0; while node 0 is childless every grid and pyramid entry under octant 0 is (1, that word), and the pyramid's level-1 cell 0
    carries it whether or not node 0 has children"""
    pkg, torch = env
    rig = Rig(env, oracle, S.CENTER, S.EDGE)
    pts, col = S.stale_cloud()

    def octant0(what, word, childless):
        grid, pyr = rig.pool.accel_grid()
        e = pyr[R.pyr_offset(1)]
        assert int(e[1]) == word, "%s: pyramid level 1 cell (0, 0, 0): got (%#x, %#x), wanted node 0's word %#x" % (what, e[0], e[1], word)
        assert (int(e[0]) == 1) == childless
        if childless:
            want = np.array([1, word], np.uint32)
            for level in range(1, 9):
                table = grid if level == 8 else pyr[R.pyr_offset(level):R.pyr_offset(level + 1)]
                cells = octant0_entries(level)
                bad = cells[(table[cells] != want).any(1)]
                assert len(bad) == 0, "%s: %s: %d entries under octant 0 do not hold node 0's word, first %s: got (%#x, %#x), wanted (1, %#x)" % (
                    what, "grid" if level == 8 else "pyramid", len(bad), cell_text(level, int(bad[0])), table[bad[0], 0], table[bad[0], 1], word)

    rig.fuse(pts, col, S.DEPTH)
    rig.render()
    rig.check("stale frame 1")
    last = int(rig.opool.words()[1])
    for k in range(2, 6):
        rig.fuse(pts, col, S.DEPTH)
        marked = rig.marks("stale frame %d" % k)
        assert len(marked) > 0 and not (((marked & 31) < 16) & (((marked >> 5) & 31) < 16) & ((marked >> 10) < 16)).any()   # no block of octant 0
        words = rig.words()
        assert not (int(words[0]) & R.FLAG) and int(words[1]) != last      # node 0 childless, its word changed
        last = int(words[1])
        rig.render()
        octant0("stale frame %d" % k, last, True)
        if k in (2, 5):
            rig.check("stale frame %d" % k)
        else:
            rig.recent = []
    p0, c0 = S.stale_first_frame_with_octant0()                          # a few hundred points in the middle of octant 0 too: node 0 gets children
    rig.fuse(p0, c0, S.DEPTH)
    rig.render()
    words = rig.words()
    assert int(words[0]) & R.FLAG
    octant0("node 0 with children", int(words[1]), False)
    rig.check("node 0 with children")
    rig.fuse(pts, col, S.DEPTH)                                           # octant 7 again: level-1 cell 0 still follows
    rig.render()
    words = rig.words()
    assert int(words[1]) != last
    octant0("octant 7 again, node 0 with children", int(words[1]), False)
    rig.check("octant 7 again, node 0 with children")


@pytest.mark.parametrize("depth", [11, 14])
def test_deferred_commits(env, oracle, depth):
    """commit_deferred / apply with a render between them: that render's tables describe the OLD map and leave the pending commit's
    dirty state -- bitmap, list, count, rings -- as it was; after the apply the tables describe the new map"""
    pkg, torch = env
    rng = np.random.default_rng(77)
    rig = Rig(env, oracle)
    pool, ws = rig.pool, rig.ws
    for it in range(4):
        pts, col = surface_cloud(rng, 4000, jitter=0.003)
        tp, tc = rig.dev(pts, col)
        old = rig.opool.words().copy() if rig.opool.size else np.zeros(16, np.uint32)
        pkg.svo_fuse_sort(ws, tp, depth, CENTER, EDGE)
        pkg.svo_fuse_plan(ws, len(pts), depth, pool)
        pkg.svo_fuse_commit_deferred(ws, tc, depth, pool)
        torch.cuda.synchronize()
        v = pool.accel_view()
        assert v["deferred_pending"]
        state = v["epoch"] & 1
        check_marks(env, pool, state, pts, "deferred commit %d" % it)
        before = pool.accel_dirty_words(state, 0, v["state_words"], v)
        rig.render()
        after = pool.accel_dirty_words(state, 0, v["state_words"], v)
        # (state 0 also keeps node 0's colour word as each refresh saw it, two words that are no part of any commit's marks: pool_grid.hpp)
        mine = np.ones(len(before), bool)
        mine[v["node0_offset"]:v["node0_offset"] + 2] = False
        changed = np.flatnonzero((before != after) & mine)
        assert len(changed) == 0, "round %d: the refresh between commit and apply changed %d words of the pending commit's dirty state %d, first word %d: %#x -> %#x" % (
            it, len(changed), state, changed[0], before[changed[0]], after[changed[0]])
        if it in (1, 3):
            check_tables(env, pool, old, "round %d, between commit and apply (the old map)" % it)
        pkg.svo_fuse_apply(ws, pool)
        rig.opool.insert_cloud(pts, col, depth, CENTER, EDGE)
        rig.recent = [pts]
        rig.render()
        if it != 2:
            seen = rig.check("round %d, applied" % it)
            assert seen["bricks"] and not seen["view"]["deferred_pending"]


@pytest.mark.parametrize("depth", [12, 14])
def test_reset_leaves_no_brick_of_the_old_map(env, oracle, depth):
    rng = np.random.default_rng(300 + depth)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 4000, jitter=0.003)
    rig.fuse(pts, col, depth)
    rig.render()
    rig.check("before the reset")
    rig.pool.reset()
    rig.opool = oracle.Pool()
    pts, col = surface_cloud(rng, 3000, jitter=0.003)
    pts = (pts * np.float32(0.5) + np.float32(0.3)).astype(np.float32)
    rig.fuse(pts, col, depth)
    rig.render()
    seen = rig.check("a different cloud after the reset")      # (the field's hygiene: nothing nonzero but the new map's lines)
    assert seen["lines"] > 0 and seen["missing"] == 0


def test_change_of_shape_and_outgrowing_the_bricks(env, oracle):
    """depths 12, 12, 14, 14, 13, 16, 12 into one pool: each change of shape leaves exact lines in the new shape and none of the old
    one; from depth 16 on no bricks are in use and the grid and the pyramid stay exact"""
    rng = np.random.default_rng(5)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 4000, jitter=0.002)
    for step, depth in enumerate((12, 12, 14, 14, 13, 16, 12)):
        rig.fuse(pts, col, depth)
        rig.render()
        if step == 1:          # (six full checks per test: the second depth-12 commit goes unchecked)
            rig.recent = []
            continue
        seen = rig.check("step %d, depth %d" % (step, depth))
        if step < 5:
            assert seen["bricks"] and seen["view"]["brick_shift"] == (0 if step < 2 else 1) and seen["lines"] > 0 and seen["missing"] == 0
        else:
            assert not seen["bricks"] and seen["view"]["max_depth"] == 16


def test_commit_shallower_than_the_brick_node(env, oracle):
    """a depth-9 fusion into a depth-14 pool changes nodes between the level grid and the brick nodes that no key lists a brick for:
    pool_accel_dirty_bitmap clears bricks_valid, the next refresh rebuilds every line"""
    rng = np.random.default_rng(9)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 4000, jitter=0.002)
    rig.fuse(pts, col, 14)
    rig.render()
    assert rig.pool.accel_view()["bricks_valid"]
    rig.check("depth 14")
    extra, ecol = new_points(rng, 1500)
    rig.fuse(extra, ecol, 9)
    assert not rig.pool.accel_view()["bricks_valid"]
    rig.render()
    seen = rig.check("a depth-9 commit into the depth-14 pool")
    assert seen["view"]["brick_shift"] == 1 and seen["code5"] > 0 and seen["missing"] == 0


def test_lapped_sibling_ring(env, oracle):
    """more than 65536 sibling-ring entries between two renders (150 000 scattered points inside the window, depth 13): the refresh zeroes
    every group instead of trusting lines whose sibling entries are lost -- every entry is the rule's value or 0, completeness is NOT
    asserted -- and a further small commit brings exact, nonzero lines back on its keys' paths"""
    pkg, torch = env
    depth = 13
    rng = np.random.default_rng(900 + depth)
    rig = Rig(env, oracle)
    pts, col = surface_cloud(rng, 4000, jitter=0.003)
    rig.fuse(pts, col, depth)
    rig.render()
    rig.recent = []
    big = (rng.random((150000, 3), dtype=np.float32) * np.float32(0.96) - np.float32(0.48)).astype(np.float32)
    bcol = rng.integers(0, 256, (150000, 3), dtype=np.uint8)
    rig.fuse(big, bcol, depth)
    torch.cuda.synchronize()
    v = rig.pool.accel_view()
    r = rig.pool.accel_dirty_words(0, v["sib_count_offset"], 3, v)
    pending = int(r[0]) - int(r[1 + ((v["brick_served"][0] - 1) & 1)])
    assert pending > v["sib_list_cap"], "the sibling ring is not lapped: %d entries pending" % pending
    rig.render()
    seen = rig.check("the lapping refresh", complete=False, exact_recent=False)
    assert seen["missing"] == seen["lines"] * 64 > 0          # every group zeroed
    near = (big[:3000] + np.float32(0.0009)).astype(np.float32)
    rig.fuse(near, bcol[:3000], depth)
    rig.render()
    seen = rig.check("a small commit after the lapped ring", complete=False)
    assert seen["recent"] > 1000


def test_foreign_words_lines_are_computed_not_assumed(env, oracle):
    """set_words with leaves saturated by hand under unsaturated parents (test_gpu_bricks.py test_foreign_words_are_not_trusted): the view
    reports mip_consistent false, and the lines are the UNTRUSTED rule's -- bits 8..15 under unsaturated cell-level nodes, bit 3 read"""
    pkg, torch = env
    rng = np.random.default_rng(21)
    rig = Rig(env, oracle)
    depth = 12
    pts = np.stack([rng.uniform(0.27, 0.33, 40000), rng.uniform(0.0, 0.2, 40000), 0.4 + rng.normal(scale=0.0003, size=40000)], 1).astype(np.float32)
    col = rng.integers(1, 256, (40000, 3), dtype=np.uint8)
    for _ in range(3):
        rig.fuse(pts, col, depth)
    rig.render()
    seen = rig.check("fused")
    assert seen["view"]["mip_consistent"] and seen["deep_bits"] == 0
    words = rig.opool.words().copy()
    leaves = np.flatnonzero(((words[0::2] & 0x40000000) == 0) & ((words[1::2] >> 24) > 127))
    pick = leaves[rng.random(len(leaves)) < 0.3]
    words[2 * pick + 1] = (words[2 * pick + 1] & np.uint32(0x00FFFFFF)) | np.uint32(0xFF000000)
    rig.pool.set_words(words)
    rig.render()
    assert not rig.pool.accel_view()["mip_consistent"]
    seen = check_tables(env, rig.pool, words, "hand-saturated leaves")
    assert seen["deep_bits"] > 0
    # the trusted rule would give other lines for these words: the check above tells the two apart
    w = R.split_words(words, "cuda")
    a, b = R.brick_lines(w, 0, False)[2], R.brick_lines(w, 0, True)[2]
    assert int(((a ^ b) & ~8).ne(0).sum()) > 0 and int(((a ^ b) & 8).ne(0).sum()) > 0


def test_compaction_reindexes_the_grid(env, oracle):
    """compact() renumbers the tiles (breadth-first order): after the next render every grid x field carries the NEW indices"""
    rng = np.random.default_rng(31)
    rig = Rig(env, oracle)
    for k in range(3):
        pts, col = surface_cloud(rng, 3000, jitter=0.003)
        rig.fuse(pts, col, 12)
        rig.render()
    before = rig.pool.words().copy()
    rig.pool.compact()
    after = rig.pool.words().copy()
    assert len(after) == len(before) and not np.array_equal(after[0::2], before[0::2])     # the links changed
    rig.render()
    seen = check_tables(env, rig.pool, after, "after compact()")
    assert seen["lines"] > 0 and seen["missing"] == 0


def test_growth_between_renders_keeps_the_tables(env, oracle):
    """a pool of 8 nodes grows with its commits (pool_accel_rebind moves the entry to the new allocation): the tables stay valid across
    the growth -- no full rebuild -- and exact after the incremental refresh"""
    rng = np.random.default_rng(41)
    pkg, torch = env
    rig = Rig(env, oracle, pool=pkg.Pool(capacity_nodes=8))
    # (a commit that finds too little room reserves for sixteen commits of its own size: a cloud of 50 points, then one eighty times
    # as large, which cannot fit into what the first one reserved)
    pts, col = surface_cloud(rng, 50, jitter=0.003)
    rig.fuse(pts, col, 12)
    rig.render()
    rig.check("small map")
    ptr, cap = rig.pool.data_ptr, rig.pool.capacity
    pts, col = surface_cloud(rng, 4000, jitter=0.003)
    rig.fuse(pts, col, 12)
    torch.cuda.synchronize()
    assert rig.pool.capacity > cap and rig.pool.data_ptr != ptr, "the pool did not grow"
    v = rig.pool.accel_view()
    assert v["valid"] and v["bricks_valid"] and v["grid"], "the growth invalidated the tables: %s" % v
    rig.marks("the commit that grew the pool")
    rig.render()
    seen = rig.check("after the growth")
    assert seen["recent"] > 0 and seen["missing"] == 0
