"""The rules of the march's tables (csrc/pool_grid.hpp, csrc/pool_grid.hip), stated once for every test that needs them:

 * scalar, cell by cell: walk() = the reference's descent (cone_tracing_kernels.cu:76-105), grid_entry() / grid_entry_level() =
   an entry of the level-8 grid / of the pyramid, brick_entry() = a 16-bit entry of an occupancy brick, decode() = what the
   march's kernel makes of the two (tests/test_bricks_cpu.py proves that the rules decide what the walk finds);
 * vectorised, whole tables from a pool's words in plain torch indexing, so that the same code runs on the CPU and on the
   device: grid_table(), pyramid_table(), brick_lines().  They expand level by level from the parent level's result.
   tests/test_accel_ref_cpu.py holds them to the scalar functions; tests/test_gpu_accel_tables.py holds the tables the device
   keeps to them, entry by entry.

Cells of level l are numbered (z << 2 l) | (y << l) | x, as the grid and the pyramid number them; the octant of a node is
x | y << 1 | z << 2 of its lowest coordinate bits."""
import numpy as np

FLAG, MASK = 0x40000000, 0x3FFFFFFF
GRID_LEVEL = 8
WINDOW_CELLS = 2048          # the brick field's window, in cells of level 11 + shift per axis (pool_grid.hpp kBrickWindowCells)
GROUP_ENTRIES = 32768        # 16-bit entries of a 64 KB group: 8^3 bricks of 64


def pyr_offset(l):
    """entries of the pyramid's levels 1 .. l - 1 (pool_grid.hpp)"""
    return ((1 << (3 * l)) - 8) // 7


def window_origin(shift):
    """first cell of the window on every axis, in cells of level 11 + shift"""
    return ((1 << (11 + shift)) - WINDOW_CELLS) >> 1


# ---- scalar rules -------------------------------------------------------------------------------------------------------------
def walk(words, bits, lod):
    """the reference's descent for a sample whose octant bits per level are bits[l] (l = 1..): (level it ends on, colour word)"""
    node, child = 0, 0
    depth = lod
    for i in range(lod):
        node = child + bits[i]
        if not (int(words[2 * node]) & FLAG):
            depth = i + 1
            break
        child = int(words[2 * node]) & MASK
    return depth, int(words[2 * node + 1]) if lod >= 1 else int(words[1])


def grid_entry(words, bits8):
    """pool_grid.hip grid_entry(): x = flag | children tile of the level-8 node, or the level of the first childless node; y = colour"""
    base, out = 0, (0, 0)
    for l in range(1, 9):
        nd0, nd1 = int(words[2 * (base + bits8[l - 1])]), int(words[2 * (base + bits8[l - 1]) + 1])
        if not (nd0 & FLAG):
            return (l, nd1)
        base = nd0 & MASK
        out = (FLAG | base, nd1)
    return out


def grid_entry_level(words, bits):
    """pool_grid.hip grid_entry_level() for a cell of level len(bits): (st, word) at the first childless node, otherwise
    (flag | children tile, word) of the cell's own node"""
    base, out = 0, (0, 0)
    for l in range(1, len(bits) + 1):
        nd0, nd1 = int(words[2 * (base + bits[l - 1])]), int(words[2 * (base + bits[l - 1]) + 1])
        if not (nd0 & FLAG):
            return (l, nd1)
        base = nd0 & MASK
        out = (FLAG | base, nd1)
    return out


def brick_entry(words, g, bits_below_8, shift, trust_mip=False):
    """brick_rebuild<.., S>(): the 16-bit entry of the cell at level 11 + shift below the level-8 node whose grid entry is g
    (0 = no brick): the levels 9 .. 9 + shift are the same for the whole brick (a childless node there: code 5 for level 9 of
    shift 1, 1 for the brick node itself), then two levels per cell, then the tile of the bits level.
    trust_mip (PoolAccel::mip_consistent): a cell-level node with children and A < 254 has no saturated child, its tile is not
    read: stop 4 | bit 3 ("a node of the bits level may have children") and no bits 8..15"""
    if not (g[0] & FLAG):
        return 0
    sat = lambda w: 1 if (w >> 24) >= 254 else 0
    nl = 9 + shift
    tile, v, w1 = g[0] & MASK, 0, 0
    for l in range(9, nl + 3):                      # levels 9 .. cell level
        n = tile + bits_below_8[l - 9]
        w0, w1 = int(words[2 * n]), int(words[2 * n + 1])
        v |= sat(w1) << (l - 5)
        if not (w0 & FLAG):
            return v | ((4 + (l - 8)) if l < nl else (l - nl + 1))
        tile = w0 & MASK
    v |= 4
    if trust_mip and (w1 >> 24) < 254:
        return v | 8
    for q in range(8):
        c0, c1 = int(words[2 * (tile + q)]), int(words[2 * (tile + q) + 1])
        v |= sat(c1) << (8 + q)
        if c0 & FLAG:
            v |= 8
    return v


def decode(e, g, lod, oct_bl, shift):
    """decode() of cone_trace_brick_kernel<.., S>: (decided, level, retired)"""
    bl = 12 + shift
    st = ((e & 7) | 8) if shift == 0 else (0x009DCBA8 >> ((e & 7) << 2)) & 15
    depth_b = min(lod, st)
    bit = depth_b - 5
    nl = 9 + shift
    # the brick node's level and its cells' two levels; a level above the brick node only where the path stops there
    by_brick = 0 <= depth_b - nl < 3 or (8 < st < nl and depth_b == st)
    if lod >= bl:
        deep = depth_b == bl and (lod == bl or not (e & 8))
        by_brick = by_brick or deep
        bit = 8 + oct_bl if deep else bit
    depth_g = min(g[0], 8)
    top_g = 127 if g[0] < FLAG else 8
    by_grid = depth_g <= lod <= top_g
    depth = depth_b if by_brick else depth_g
    retired = ((e >> bit) & 1) if by_brick else (1 if g[1] >= 0xFE000000 else 0)
    return by_brick or by_grid, depth, retired


def brick_entry_index(x, y, z):
    """pool_grid.hpp brick_entry_index(): entry of window cell (x, y, z) (11 bits each, relative to the window's origin) in the
    field -- [z >> 5 | y >> 5 | x >> 5] group, [z y x bits 4..2] brick in the group, [z y x bits 1..0] cell in the brick.  Works
    on ints, numpy arrays and torch tensors alike"""
    lo = (((y >> 5) << 21) | ((x >> 5) << 15) | (((z >> 2) & 7) << 12) | (((y >> 2) & 7) << 9) | (((x >> 2) & 7) << 6) |
          ((z & 3) << 4) | ((y & 3) << 2) | (x & 3))
    return ((z >> 5) << 27) | lo


def brick_entry_cell(i):
    """the inverse: window cell (x, y, z) of field entry i"""
    x = (((i >> 15) & 63) << 5) | (((i >> 6) & 7) << 2) | (i & 3)
    y = (((i >> 21) & 63) << 5) | (((i >> 9) & 7) << 2) | ((i >> 2) & 3)
    z = ((i >> 27) << 5) | (((i >> 12) & 7) << 2) | ((i >> 4) & 3)
    return x, y, z


def cell_of_points(pts, level, center=(0.0, 0.0, 0.0), edge=1.0):
    """cell coordinates int64 [n, 3] at `level` of the keys svo.cu:33-66 gives finite points: the descent itself, in binary32 as the
    reference runs it (octant bit = p > centre, the half edge halved and the centre moved by it level by level)"""
    p = np.asarray(pts, np.float32)
    c = np.tile(np.asarray(center, np.float32), (len(p), 1))
    e = np.float32(edge)
    cell = np.zeros(p.shape, np.int64)
    for _ in range(level):
        up = p > c
        cell = (cell << 1) | up
        e = np.float32(e / np.float32(2.0))
        c = (c + np.where(up, e, -e).astype(np.float32)).astype(np.float32)
    return cell


# ---- whole tables -------------------------------------------------------------------------------------------------------------
def split_words(words, device=None):
    """(word 0, word 1) of every node as int64 tensors on `device`; a pool that holds no node yet is the empty root tile"""
    import torch
    if isinstance(words, tuple):
        return words
    if isinstance(words, torch.Tensor):
        w = words.to(torch.int64) & 0xFFFFFFFF
    else:
        w = torch.from_numpy(np.ascontiguousarray(words, np.uint32).astype(np.int64))
    if w.numel() < 16:
        w = torch.zeros(16, dtype=torch.int64)
    if device is not None:
        w = w.to(device)
    w = w.reshape(-1, 2)
    return w[:, 0].contiguous(), w[:, 1].contiguous()


def _expand(w0, w1, parent, l):
    """the state of level l + 1 from that of level l.  A state = (st, tile, word) per cell: st = level of the first childless
    node on the cell's path (0: every node down to the cell's own has children), tile = the children tile of the cell's node
    (st == 0), word = the colour word of the node the walk stops on, or of the cell's own node"""
    import torch
    st, tile, word = parent
    L = l + 1
    idx = torch.arange(1 << (3 * L), dtype=torch.int64, device=w0.device)
    m = (1 << L) - 1
    x, y, z = idx & m, (idx >> L) & m, idx >> (2 * L)
    par = ((z >> 1) << (2 * l)) | ((y >> 1) << l) | (x >> 1)
    octant = (x & 1) | ((y & 1) << 1) | ((z & 1) << 2)
    del idx, x, y, z
    p_st = st[par]
    alive = p_st == 0
    node = torch.where(alive, tile[par] + octant, torch.zeros_like(par))
    n0, n1 = w0[node], w1[node]
    has = (n0 & FLAG) != 0
    new_st = torch.where(alive, torch.where(has, torch.zeros_like(p_st), torch.full_like(p_st, L)), p_st)
    new_word = torch.where(alive, n1, word[par])
    new_tile = torch.where(alive & has, n0 & MASK, torch.zeros_like(n0))
    return new_st, new_tile, new_word


def level_states(words, upto=GRID_LEVEL, device=None):
    """states of levels 0 .. upto (see _expand), each expanded from the one above"""
    import torch
    w0, w1 = split_words(words, device)
    z = torch.zeros(1, dtype=torch.int64, device=w0.device)
    states = [(z, z.clone(), z.clone())]     # the root: has children (the tile at node 0), no word of its own in any entry
    for l in range(upto):
        states.append(_expand(w0, w1, states[-1], l))
    return states


def _entries(state):
    import torch
    st, tile, word = state
    return torch.stack([torch.where(st > 0, st, FLAG | tile), word], 1)


def grid_table(words, device=None, states=None):
    """the level-8 grid: int64 [2^24, 2] = (x, y) of every cell (grid_entry)"""
    states = states or level_states(words, GRID_LEVEL, device)
    return _entries(states[GRID_LEVEL])


def pyramid_table(words, device=None, states=None):
    """the pyramid: int64 [pyr_offset(8), 2], the entries of levels 1 .. 7 in pyr_offset order (grid_entry_level)"""
    import torch
    states = states or level_states(words, GRID_LEVEL - 1, device)
    return torch.cat([_entries(states[l]) for l in range(1, GRID_LEVEL)])


def brick_cells(shift, states):
    """the level-8 cells that have brick lines: those whose node has children, inside the window (which holds whole level-8 cells)"""
    import torch
    G = GRID_LEVEL
    cells = torch.nonzero(states[G][0] == 0).reshape(-1)
    m8 = (1 << G) - 1
    x, y, z = cells & m8, (cells >> G) & m8, cells >> (2 * G)
    org8, span8 = window_origin(shift) >> (3 + shift), WINDOW_CELLS >> (3 + shift)
    keep = (x >= org8) & (x < org8 + span8) & (y >= org8) & (y < org8 + span8) & (z >= org8) & (z < org8 + span8)
    return cells[keep]


def brick_lines(words, shift, trust_mip, device=None, states=None, cells=None):
    """every brick line the rules define: for each brick node (level 9 + shift) inside the window whose level-8 ancestor has
    children -- the childless siblings beside the paths included -- its window-relative brick coordinates int64 [n, 3], the
    field indices of its 64 entries int64 [n, 64] (brick_entry_index) and their values int64 [n, 64] (brick_entry).
    cells: a part of brick_cells() (large maps are taken in parts), default all of them"""
    import torch
    w0, w1 = split_words(words, device)
    states = states or level_states((w0, w1), GRID_LEVEL)
    G, NL = GRID_LEVEL, 9 + shift
    sat = lambda w: ((w >> 24) >= 254).to(torch.int64)
    if cells is None:
        cells = brick_cells(shift, states)
    m8 = (1 << G) - 1
    x, y, z, tile = cells & m8, (cells >> G) & m8, cells >> (2 * G), states[G][1][cells]
    v, code = torch.zeros_like(x), torch.zeros_like(x)      # code != 0: the path has stopped, the entry is v | code from there on
    q8 = torch.arange(8, dtype=torch.int64, device=w0.device)
    for l in range(G + 1, NL + 1):                          # the levels every cell of a brick shares
        x = ((x << 1)[:, None] | (q8 & 1)[None, :]).reshape(-1)
        y = ((y << 1)[:, None] | ((q8 >> 1) & 1)[None, :]).reshape(-1)
        z = ((z << 1)[:, None] | (q8 >> 2)[None, :]).reshape(-1)
        alive = (code == 0).repeat_interleave(8)
        node = torch.where(alive, tile.repeat_interleave(8) + q8.repeat(len(tile)), torch.zeros_like(x))
        n0, n1 = w0[node], w1[node]
        v = v.repeat_interleave(8) | torch.where(alive, sat(n1) << (l - 5), torch.zeros_like(x))
        stop = alive & ((n0 & FLAG) == 0)
        code = torch.where(stop, torch.full_like(x, 1 if l == NL else 4 + (l - G)), code.repeat_interleave(8))
        tile = torch.where(alive & ~stop, n0 & MASK, torch.zeros_like(x))
    # the two levels of a brick's own cells, then the tile of the bits level: lane = octant at level NL + 1 (bits 5..3), at NL + 2 (bits 2..0)
    lane = torch.arange(64, dtype=torch.int64, device=w0.device)
    o1, o2 = lane >> 3, lane & 7
    on = (code == 0)[:, None].expand(-1, 64)
    zero = torch.zeros((len(x), 64), dtype=torch.int64, device=w0.device)
    n10 = torch.where(on, tile[:, None] + o1[None, :], zero)
    a0, a1 = w0[n10], w1[n10]
    val = (v | code)[:, None] | torch.where(on, sat(a1) << (NL + 1 - 5), zero)
    on11 = on & ((a0 & FLAG) != 0)
    val = val | torch.where(on & ~on11, zero + 2, zero)
    n11 = torch.where(on11, (a0 & MASK) + o2[None, :], zero)
    b0, b1 = w0[n11], w1[n11]
    val = val | torch.where(on11, sat(b1) << (NL + 2 - 5), zero)
    on12 = on11 & ((b0 & FLAG) != 0)
    val = val | torch.where(on11 & ~on12, zero + 3, zero) | torch.where(on12, zero + 4, zero)
    if trust_mip:
        skip = on12 & ((b1 >> 24) < 254)
        val = val | torch.where(skip, zero + 8, zero)
        on12 = on12 & ~skip
    t12 = torch.where(on12, b0 & MASK, zero)
    for q in range(8):
        c0, c1 = w0[t12 + q], w1[t12 + q]
        val = val | torch.where(on12, (sat(c1) << (8 + q)) | (((c0 & FLAG) != 0).to(torch.int64) << 3), zero)
    org = window_origin(shift) >> 2                         # in bricks
    xr, yr, zr = x - org, y - org, z - org
    cx = (xr << 2)[:, None] | (((lane >> 3) & 1) << 1)[None, :] | (lane & 1)[None, :]
    cy = (yr << 2)[:, None] | (((lane >> 4) & 1) << 1)[None, :] | ((lane >> 1) & 1)[None, :]
    cz = (zr << 2)[:, None] | (((lane >> 5) & 1) << 1)[None, :] | ((lane >> 2) & 1)[None, :]
    return torch.stack([xr, yr, zr], 1), brick_entry_index(cx, cy, cz), val
