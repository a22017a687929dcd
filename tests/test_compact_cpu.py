"""Pool compaction and sub-tree grafting: the specification restated on host words, and checked against the restatement
of the reference's reader (oracle/formats.py: pullFromLinearTree) on pools built by the CPU oracle.  No GPU.

compact_words / graft_words below are what svoslam_pool_compact / svoslam_pool_graft_subtree (include/svoslam.h) must
produce; tests/test_gpu_compact.py compares the device against them bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from util import surface_cloud

FLAG, MASK = 0x40000000, 0x3FFFFFFF


def compact_words(words, want_map=False):
    """The canonical order: exactly the tiles reachable from the root tile (nodes 0..7), breadth-first from tile 0, each level
    in the order of the parent nodes' new indices, then octant 0..7.  Colour words and word0 of childless nodes are copied,
    word0 of a node with children becomes FLAG | 8 * (new index of its child tile).  want_map: also the old first-node index
    of every new tile."""
    words = np.asarray(words, dtype=np.uint32)
    cap = words.size // 16                                  # no tree visits more tiles than the pool holds
    old_tile, out, level = [0], [], [0]
    while level:
        nxt = []
        for t in level:
            for j in range(8):
                a, b = int(words[2 * (t + j)]), int(words[2 * (t + j) + 1])
                if a & FLAG:
                    child = a & MASK
                    if child & 7 or child + 8 > words.size // 2:
                        raise ValueError("child index outside the pool")
                    a = FLAG | (8 * (len(old_tile) + len(nxt)))
                    nxt.append(child)
                out.extend((a, b))
        if len(old_tile) + len(nxt) > cap:
            raise ValueError("a cycle or a shared tile")
        old_tile.extend(nxt)
        level = nxt
    out = np.array(out, dtype=np.uint32)
    return (out, np.array(old_tile, dtype=np.uint32)) if want_map else out


def graft_words(words, sub):
    """The sub-tree of oracle.formats.read_subtree_file appended at base = size of the pool: flagged word0 = FLAG | (base +
    relative index), the node at the file's path gets FLAG | base and keeps its colour.  Nothing of the file's numbering
    (node_index, pool_size, tiles) is used."""
    from oracle import formats as fm
    words = np.asarray(words, dtype=np.uint32)
    node, w0 = fm.walk_path(words, sub["path"])
    if w0 & FLAG:
        raise ValueError("the cube was fused into while it was paged out")
    base = words.size // 2
    nodes = np.array(sub["nodes"], dtype=np.uint32)
    flagged = (nodes[0::2] & FLAG) != 0
    nodes[0::2][flagged] = FLAG | (base + (nodes[0::2][flagged] & MASK))
    out = np.concatenate([words, nodes])
    out[2 * node] = FLAG | base
    return out


# ------------------------------------------------------------------------------------------------------------------------
CENTER, EDGE, DEPTH = (0.05, -0.02, 0.01), 1.0, 7


def clouds(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pts, col = surface_cloud(rng, 12000)
        out.append((pts + np.float32(0.01 * k), col))
    return out


@pytest.fixture(scope="module")
def built(oracle):
    """an oracle pool of three clouds; its words with gaps (two sub-trees evicted) come from formats.evict_subtree"""
    pool = oracle.Pool()
    for pts, col in clouds(91, 3):
        pool.insert_cloud(pts, col, DEPTH, CENTER, EDGE)
    return pool.words()


def test_compaction_keeps_the_host_tree(built):
    from oracle import formats as fm
    w = built
    c, old_tile = compact_words(w, want_map=True)
    tree = fm.pull_to_cpu(w)
    assert fm.pull_to_cpu(c) == tree                                    # the same tree through pullFromLinearTree
    assert c.size // 2 == sum(fm.count_nodes(t) for t in tree)          # and nothing but the tree
    assert np.array_equal(compact_words(c), c)                          # idempotent
    # the old-tile map: new tile k holds old tile map[k], up to re-pointed word0
    assert old_tile.size == c.size // 16 and len(set(old_tile.tolist())) == old_tile.size
    for k in (0, 1, old_tile.size // 2, old_tile.size - 1):
        t = int(old_tile[k])
        assert np.array_equal(c[16 * k + 1:16 * k + 16:2], w[2 * t + 1:2 * t + 16:2])
        assert np.array_equal(c[16 * k:16 * k + 16:2] & FLAG, w[2 * t:2 * t + 16:2] & FLAG)
    fresh = np.zeros(16, dtype=np.uint32)
    assert np.array_equal(compact_words(fresh), fresh)                  # an empty map stays 8 nodes


def test_compaction_renders_the_same(built, oracle):
    w, c = built, compact_words(built)
    view = oracle.look_at((0.1, 0.2, -2.5), (0, 0, 0), (0, 1, 0))
    for mode in (oracle.RENDER_REFERENCE, oracle.RENDER_CARRY):
        a, sa, la = oracle.cone_trace(w, 64, 48, 45.0, view, CENTER, EDGE, mode)
        b, sb, lb = oracle.cone_trace(c, 64, 48, 45.0, view, CENTER, EDGE, mode)
        assert a.any() and a.tobytes() == b.tobytes() and (sa, la) == (sb, lb)


def test_eviction_then_compaction_then_graft(built):
    from oracle import formats as fm
    w = built
    tree = fm.pull_to_cpu(w)
    top = next(k for k in range(8) if tree[k][1] is not None)
    inner = next(k for k in range(8) if tree[top][1][k][1] is not None)
    full = compact_words(w)
    for path in ([top], [top, inner]):
        tiles, blob, after, node = fm.evict_subtree(w, path)
        small = compact_words(after)
        assert full.size // 2 - small.size // 2 == 8 * len(tiles)       # exactly the evicted tiles are gone
        sub = {"path": path, "nodes": blob, "tiles": tiles, "node_index": node, "pool_size": w.size // 2}
        for target in (small, after):                                   # compacted and never-compacted pools alike
            g = graft_words(target, sub)
            assert g.size == target.size + blob.size and fm.pull_to_cpu(g) == tree
        assert np.array_equal(compact_words(graft_words(small, sub)), full)   # canonical: the same tree is the same bytes
    with pytest.raises(ValueError):
        graft_words(w, sub)                                             # the node has children


def test_fusion_after_compaction_is_well_defined(built, oracle):
    """numbering is the only thing compaction changes: one more cloud into the pool and into its compacted copy gives the
    same host tree -- and the same bytes once both are compacted"""
    from oracle import formats as fm
    tiles, blob, after, node = fm.evict_subtree(built, [next(k for k in range(8) if built[2 * k] & FLAG)])
    A, B = oracle.Pool(), oracle.Pool()
    A.load_words(after)
    B.load_words(compact_words(after))
    pts, col = clouds(17, 1)[0]
    for p in (A, B):
        p.insert_cloud(pts + np.float32(0.02), col, DEPTH, CENTER, EDGE)
    assert A.size > after.size // 2
    assert fm.pull_to_cpu(A.words()) == fm.pull_to_cpu(B.words())
    assert np.array_equal(compact_words(A.words()), compact_words(B.words()))


def test_malformed_pools_are_refused():
    w = np.zeros(32, dtype=np.uint32)
    w[0] = FLAG | 8
    w[16] = FLAG | 0                                                    # node 8 points back at tile 0
    with pytest.raises(ValueError):
        compact_words(w)
    w[16] = FLAG | 12                                                   # not a tile boundary
    with pytest.raises(ValueError):
        compact_words(w)
    w[16] = FLAG | 16                                                   # outside the pool
    with pytest.raises(ValueError):
        compact_words(w)


def test_library_exports_compact_and_graft():
    import svoslam_pkg
    pkg = svoslam_pkg.load()
    if not os.path.exists(pkg.LIB_PATH):
        pkg.build()
    L = C.CDLL(pkg.LIB_PATH)
    for name in ("svoslam_pool_compact", "svoslam_pool_graft_subtree"):
        assert hasattr(L, name), "%s is not exported" % name
        assert name in pkg.SIGNATURES
    assert [n for n, _ in pkg.CompactStats._fields_] == ["size_before", "size_after", "capacity_before", "capacity_after", "levels",
                                                         "tiles_dropped"]
    assert C.sizeof(pkg.CompactStats) == 24
    assert hasattr(pkg.Pool, "compact") and hasattr(pkg.Pool, "graft_subtree")
