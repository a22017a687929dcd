"""The entry-by-entry checker of the tables the ray march reads instead of the octree (csrc/pool_grid.hpp), for the tests that commit
into a pool and then hold its level grid, pyramid, occupancy bricks and dirty marks to the rules of tests/accel_ref.py:
test_gpu_accel_tables.py (every kind of upkeep; its docstring says what is asserted of the bricks) and test_gpu_commit_runs.py
(commits with few heads).  No test here."""
import ctypes as C

import numpy as np
import pytest

import accel_ref as R


CENTER, EDGE = (0.0, 0.0, 0.0), 1.0
FIELD_ENTRIES = 1 << 33             # 16-bit entries of the brick field
GROUPS = 1 << 18                    # 64 KB groups
SCAN_GROUPS = 4096                  # groups per part of a whole-field scan (256 MiB)
LINES_PART = 4096                   # level-8 cells per part of the reference lines (<= 4096 * 64 bricks * 64 entries)


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
