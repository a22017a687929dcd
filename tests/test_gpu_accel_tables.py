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
import ctypes as C

import numpy as np
import pytest

import accel_ref as R
import node0_scenes as S
from util import surface_cloud

pytestmark = pytest.mark.gpu

CENTER, EDGE = (0.0, 0.0, 0.0), 1.0
FIELD_ENTRIES = 1 << 33             # 16-bit entries of the brick field
GROUPS = 1 << 18                    # 64 KB groups
SCAN_GROUPS = 4096                  # groups per part of a whole-field scan (256 MiB)
LINES_PART = 4096                   # level-8 cells per part of the reference lines (<= 4096 * 64 bricks * 64 entries)


@pytest.fixture(scope="module")
def env():
    import torch
    import svoslam_pkg
    return svoslam_pkg.load(), torch


# ---- raw device memory as tensors ---------------------------------------------------------------------------------------------
class _Raw:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}


class DeviceMem:
    """`nbytes` at a raw device address as torch tensors on the device: zero-copy through __cuda_array_interface__ where torch takes
    it, otherwise a device-to-device copy of each part asked for (the brick field as a whole is never copied, nor brought to the host)"""

    def __init__(self, env, ptr, nbytes):
        self.pkg, self.torch = env
        self.ptr, self.nbytes, self.view = int(ptr), int(nbytes), None
        try:
            t = self.torch.as_tensor(_Raw(ptr, nbytes), device="cuda")
            if t.data_ptr() == self.ptr and t.numel() == self.nbytes and t.dtype == self.torch.uint8:
                self.view = t
        except Exception:
            self.view = None

    def part(self, lo, hi):
        if self.view is not None:
            return self.view[lo:hi]
        out = self.torch.empty(hi - lo, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        r = self.pkg._hip().hipMemcpy(C.c_void_p(out.data_ptr()), C.c_void_p(self.ptr + lo), C.c_size_t(hi - lo), 3)
        assert r == 0, "hipMemcpy D2D failed: %d" % r
        return out

    def gather16(self, idx):
        """the 16-bit entries number idx (int64 tensor, any shape) as int64"""
        torch = self.torch
        if self.view is not None:
            return self.view.view(torch.int16)[idx].to(torch.int64) & 0xFFFF
        flat = idx.reshape(-1)
        s, order = torch.sort(flat)
        out = torch.empty_like(flat)
        per = SCAN_GROUPS * R.GROUP_ENTRIES
        total = self.nbytes // 2
        edges = list(range(0, total, per)) + [total]
        bounds = torch.searchsorted(s, torch.tensor(edges, device=flat.device)).tolist()
        for c in range(len(edges) - 1):
            a, b = bounds[c], bounds[c + 1]
            if a < b:
                chunk = self.part(2 * edges[c], 2 * edges[c + 1]).view(torch.int16)
                out[order[a:b]] = chunk[s[a:b] - edges[c]].to(torch.int64) & 0xFFFF
        return out.reshape(idx.shape)


def group_nonzero_counts(mem):
    """nonzero entries of every 64 KB group of the field: int64 [GROUPS] on the device (the whole field is read there, in parts)"""
    torch = mem.torch
    counts = torch.empty(GROUPS, dtype=torch.int64, device="cuda")
    for c in range(GROUPS // SCAN_GROUPS):
        p = mem.part(c * SCAN_GROUPS * 65536, (c + 1) * SCAN_GROUPS * 65536).view(torch.int16).reshape(SCAN_GROUPS, R.GROUP_ENTRIES)
        counts[c * SCAN_GROUPS:(c + 1) * SCAN_GROUPS] = (p != 0).sum(1)
    return counts


def to_host_u32(torch, t):
    """an int64 tensor of 32-bit values as host uint32"""
    return torch.where(t >= (1 << 31), t - (1 << 32), t).to(torch.int32).cpu().numpy().view(np.uint32)


# ---- messages -----------------------------------------------------------------------------------------------------------------
def cell_text(level, c):
    m = (1 << level) - 1
    return "level %d cell (%d, %d, %d)" % (level, c & m, (c >> level) & m, c >> (2 * level))


def assert_entries_equal(table, got, want, what, level_of):
    if np.array_equal(got, want):
        return
    rows = np.flatnonzero((got != want).any(1))
    first = []
    for r in rows[:5].tolist():
        level, c = level_of(r)
        first.append("%s: got (%#x, %#x), wanted (%#x, %#x)" % (cell_text(level, c), got[r, 0], got[r, 1], want[r, 0], want[r, 1]))
    pytest.fail("%s: %s: %d of %d entries wrong; %s" % (what, table, len(rows), len(got), "; ".join(first)))


def pyramid_level_of(r):
    level = max(l for l in range(1, R.GRID_LEVEL) if R.pyr_offset(l) <= r)
    return level, r - R.pyr_offset(level)


def brick_text(shift, index, got=None, want=None):
    x, y, z = R.brick_entry_cell(int(index))
    org = R.window_origin(shift)
    s = "level %d cell (%d, %d, %d) [brick node (%d, %d, %d) of level %d, entry %d of its line, group %d]" % (
        11 + shift, x + org, y + org, z + org, (x + org) >> 2, (y + org) >> 2, (z + org) >> 2, 9 + shift, int(index) & 63, int(index) >> 15)
    if got is not None:
        s += ": got %#06x, wanted %#06x" % (int(got), int(want))
    return s


def brick_class(shift, want):
    code, nl = int(want) & 7, 9 + shift
    if code == 5:
        return "a brick under a CHILDLESS level-9 node (stop code 5: a sibling line)"
    if code == 1:
        return "the line of a CHILDLESS brick node of level %d (stop code 1: a sibling line, or a leaf at that level)" % nl
    return "a brick node WITH children (stop code %d in this entry)" % code


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def recent_brick_bases(shift, pts, center, edge):
    """field index of the first entry of the brick on the path of every point (those inside the window), sorted and unique"""
    if pts is None or len(pts) == 0:
        return np.zeros(0, np.int64)
    b = R.cell_of_points(pts, 9 + shift, center, edge) - (R.window_origin(shift) >> 2)
    b = b[((b >= 0) & (b < (R.WINDOW_CELLS >> 2))).all(1)]
    return np.unique(R.brick_entry_index(b[:, 0] << 2, b[:, 1] << 2, b[:, 2] << 2))


def check_tables(env, pool, words, what, recent=None, complete=True, center=CENTER, edge=EDGE):
    """the tables `pool` holds right now against the rules applied to `words` (see the module's docstring); recent: the points
    committed since the previous check; complete: no ring was lapped, every defined brick entry must be there.
    Returns what it saw, for the scenario's own assertions."""
    pkg, torch = env
    torch.cuda.synchronize()
    v = pool.accel_view()
    assert v["grid"] and v["valid"], (what, v)
    w = R.split_words(words, "cuda")
    states = R.level_states(w, R.GRID_LEVEL)
    # 1, 2: the grid and the pyramid, both words of every entry
    got_grid, got_pyr = pool.accel_grid(v)
    assert_entries_equal("grid", got_grid, to_host_u32(torch, R.grid_table(w, states=states)), what, lambda r: (R.GRID_LEVEL, r))
    assert_entries_equal("pyramid", got_pyr, to_host_u32(torch, R.pyramid_table(w, states=states)), what, pyramid_level_of)
    seen = dict(view=v, bricks=v["bricks_in_use"], lines=0, missing=0, stale_bit4=0, sat_bits=0, bit7=0, code5=0, deep_bits=0, recent=0)
    # 5: the upkeep state of the dirty states this refresh served
    served = [(v["epoch"] + 1) & 1] if v["deferred_pending"] else [0, 1]
    for s in served:
        if not v["dirty"][s]:
            continue
        bitmap = pool.accel_dirty_words(s, 0, v["dirty_words"], v)
        left = np.flatnonzero(np.unpackbits(bitmap.view(np.uint8), bitorder="little"))
        assert len(left) == 0, "%s: dirty state %d: %d level-5 blocks still marked after the refresh, first %s" % (what, s, len(left), cell_text(5, int(left[0])))
        if v["bricks_in_use"] and v["brick_served"][s] > 0:
            par = (v["brick_served"][s] - 1) & 1
            for ring, off in (("stale-brick ring", v["brick_count_offset"]), ("sibling ring", v["sib_count_offset"])):
                r = pool.accel_dirty_words(s, off, 3, v)
                assert r[1 + par] == r[0], "%s: dirty state %d: %s: mark %d after the refresh, count %d" % (what, s, ring, r[1 + par], r[0])
            bits = DeviceMem(env, v["dirty"][s] + 4 * v["brick_bits_offset"], 4 * v["brick_bits_words"]).part(0, 4 * v["brick_bits_words"]).view(torch.int32)
            still = torch.nonzero(bits).reshape(-1)
            assert len(still) == 0, "%s: dirty state %d: %d words of the 'in this ring' bits still set after the refresh, first word %d = %#x" % (
                what, s, len(still), int(still[0]), int(bits[still[0]]) & 0xFFFFFFFF)
    if not v["bricks_in_use"]:
        return seen
    # 3, 4: the bricks
    shift, trust = v["brick_shift"], v["mip_consistent"]
    mem = DeviceMem(env, v["bricks"], 2 * FIELD_ENTRIES)
    touched_words = pkg.copy_from_device(v["brick_touched"], (GROUPS // 32,), np.uint32)
    touched = torch.from_numpy(np.unpackbits(touched_words.view(np.uint8), bitorder="little").astype(bool)).cuda()
    counts = group_nonzero_counts(mem)
    stray = torch.nonzero((counts > 0) & ~touched).reshape(-1)
    assert len(stray) == 0, "%s: bricks: %d groups hold entries but their touched bit is clear, first group %d (%d nonzero entries), e.g. %s" % (
        what, len(stray), int(stray[0]), int(counts[stray[0]]), brick_text(shift, int(stray[0]) << 15))
    held = torch.nonzero(counts > 0).reshape(-1)
    if len(held):     # (the host copy of a single group, Pool.accel_brick_group, reads the same memory)
        g = int(held[len(held) // 2])
        assert int(np.count_nonzero(pool.accel_brick_group(g, v))) == int(counts[g]), (what, g)
    bases = torch.from_numpy(recent_brick_bases(shift, recent, center, edge)).cuda()
    care_rest = 0xFFFF & ~(0x10 if shift == 1 else 0)      # bit 4 of shape 1: only where the path stops at level 9 (module docstring)
    nonzero_at_lines, first_missing = 0, None
    for part in R.brick_cells(shift, states).split(LINES_PART):
        _, index, want = R.brick_lines(w, shift, trust, states=states, cells=part)
        got = mem.gather16(index)
        care = torch.where((want & 7) == 5, torch.full_like(want, 0xFFFF), torch.full_like(want, care_rest))
        there = got != 0
        bad = torch.nonzero(there & (((got ^ want) & care) != 0))
        if len(bad):
            i, j = int(bad[0, 0]), int(bad[0, 1])
            pytest.fail("%s: bricks (shape %d, trust_mip %s): %d entries hold neither the rule's value nor 0, first %s" % (
                what, shift, trust, len(bad), brick_text(shift, index[i, j], got[i, j], want[i, j])))
        if len(bases):
            hit = torch.isin(index[:, 0], bases)
            wrong = torch.nonzero(got[hit] != want[hit])
            if len(wrong):
                i, j = int(wrong[0, 0]), int(wrong[0, 1])
                pytest.fail("%s: bricks (shape %d): %d entries of bricks on the path of a key just committed are not exact, first %s" % (
                    what, shift, len(wrong), brick_text(shift, index[hit][i, j], got[hit][i, j], want[hit][i, j])))
            seen["recent"] += int(hit.sum())
        gone = torch.nonzero(~there)
        if len(gone) and first_missing is None:
            i, j = int(gone[0, 0]), int(gone[0, 1])
            first_missing = "%s, which belongs to %s" % (brick_text(shift, index[i, j], 0, want[i, j]), brick_class(shift, want[i, j]))
        seen["missing"] += len(gone)
        seen["lines"] += len(index)
        nonzero_at_lines += int(there.sum())
        seen["stale_bit4"] += int((there & (got != want)).sum())
        seen["sat_bits"] += int(((want & 0xFFF0) != 0).sum())
        seen["bit7"] += int(((want & 0x80) != 0).sum())
        seen["code5"] += int(((want & 7) == 5).sum())
        seen["deep_bits"] += int(((want >> 8) != 0).sum())
    print("%s: shape %d, trust_mip %s: %d lines, %d defined entries read 0, %d differ in bit 4 only, %d bricks of recent keys, field read %s" % (
        what, shift, trust, seen["lines"], seen["missing"], seen["stale_bit4"], seen["recent"], "in place" if mem.view is not None else "by copies"))
    assert seen["recent"] == len(bases), "%s: bricks: %d bricks of recent keys inside the window, the rules define lines for %d of them" % (what, len(bases), seen["recent"])
    if complete:
        assert seen["missing"] == 0, "%s: bricks (shape %d): %d defined entries read 0 though no ring was lapped, first %s" % (what, shift, seen["missing"], first_missing)
    total = int(counts.sum())
    if total != nonzero_at_lines:   # 4b: something nonzero where the rules define no line
        for g in torch.nonzero(counts > 0).reshape(-1).tolist():
            entries = (g << 15) + torch.nonzero(mem.part(g * 65536, (g + 1) * 65536).view(torch.int16)).reshape(-1)
            defined = torch.zeros_like(entries, dtype=torch.bool)
            for part in R.brick_cells(shift, states).split(LINES_PART):
                defined |= torch.isin(entries, R.brick_lines(w, shift, trust, states=states, cells=part)[1].reshape(-1))
            if not bool(defined.all()):
                e = int(entries[~defined][0])
                pytest.fail("%s: bricks (shape %d): %d nonzero entries in the field, %d of them where the rules define a line; first stray %s holds %#06x" % (
                    what, shift, total, nonzero_at_lines, brick_text(shift, e), int(mem.gather16(torch.tensor([e], device="cuda"))[0])))
        pytest.fail("%s: bricks: %d nonzero entries in the field, %d where the rules define a line" % (what, total, nonzero_at_lines))
    return seen


def check_marks(env, pool, state, pts, what, center=CENTER, edge=EDGE):
    """after a commit, before the render that serves it: the block list of dirty state `state` is its bitmap's set bits in ascending
    order, its count their number, and the level-5 block of every point committed since the last render is among them"""
    pkg, torch = env
    torch.cuda.synchronize()
    v = pool.accel_view()
    words = pool.accel_dirty_words(state, 0, v["count_offset"] + 1, v)
    marked = np.flatnonzero(np.unpackbits(words[:v["dirty_words"]].view(np.uint8), bitorder="little"))
    count = int(words[v["count_offset"]])
    assert count == len(marked), "%s: dirty state %d: count %d, %d bits set in the bitmap" % (what, state, count, len(marked))
    listed = words[v["list_offset"]:v["list_offset"] + count].astype(np.int64)
    assert np.array_equal(listed, marked), "%s: dirty state %d: the list is not the bitmap's set bits in ascending order: %s" % (
        what, state, [(i, int(listed[i]), int(marked[i])) for i in np.flatnonzero(listed != marked)[:5]])
    c = R.cell_of_points(pts, 5, center, edge)
    blocks = np.unique((c[:, 2] << 10) | (c[:, 1] << 5) | c[:, 0])
    lost = np.setdiff1d(blocks, marked)
    assert len(lost) == 0, "%s: dirty state %d: %d level-5 blocks of inserted points are not marked, first %s" % (what, state, len(lost), cell_text(5, int(lost[0])))
    return marked


class Rig:
    """a device pool and the oracle pool that follows it"""

    def __init__(self, env, oracle, center=CENTER, edge=EDGE, pool=None):
        self.env, self.oracle = env, oracle
        self.pkg, self.torch = env
        self.center, self.edge = center, edge
        self.ws, self.pool, self.opool = self.pkg.Workspace(), pool or self.pkg.Pool(), oracle.Pool()
        self.view = oracle.look_at((0.1, 0.2, -1.2), (0, 0, 0), (0, 1, 0))
        self.recent = []

    def dev(self, pts, col):
        return self.torch.from_numpy(pts).cuda(), self.torch.from_numpy(col).cuda()

    def fuse(self, pts, col, depth):
        tp, tc = self.dev(pts, col)
        self.pkg.svo_from_point_cloud_async(self.ws, tp, tc, depth, self.pool, self.center, self.edge)
        self.opool.insert_cloud(pts, col, depth, self.center, self.edge)
        self.recent.append(pts)

    def render(self):
        """a tiny reference-mode render: what it shows is not the subject, the refresh before it is"""
        img = self.torch.zeros((8, 8, 4), dtype=self.torch.uint8, device="cuda")
        self.pkg.cone_trace_svo(img, 45.0, self.view, self.pool.data_ptr, self.center, self.edge, 0)
        self.torch.cuda.synchronize()

    def words(self):
        """the oracle's words, which the device pool must hold too (so that tile indices are comparable)"""
        want, got = self.opool.words(), self.pool.words()
        assert len(got) == len(want) and np.array_equal(got, want), "the device pool's words are not the oracle's"
        return want

    def marks(self, what, state=0):
        return check_marks(self.env, self.pool, state, np.concatenate(self.recent), what, self.center, self.edge)

    def check(self, what, complete=True, words=None, exact_recent=True):
        recent = np.concatenate(self.recent) if self.recent and exact_recent else None
        seen = check_tables(self.env, self.pool, self.words() if words is None else words, what, recent, complete, self.center, self.edge)
        self.recent = []
        return seen


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
