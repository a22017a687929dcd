"""Point clouds designed by their RUNS of equal keys, for the tests of the fusion commit (csrc/svo_build.hip: plan_count /
plan_emit, split_all_kernel, fill_mip_local_kernel, mip_straddle_kernel, mip_straddle2_kernel, commit_apply_kernel):
test_commit_runs_cpu.py holds the cases to what they claim by the oracle's keys alone, test_gpu_commit_runs.py commits them in
every form.  No test here, and no GPU.

The commit works on the frame's SORTED keys, and what it has to get right is how runs of equal or prefix-sharing keys lie across
three fixed cuts of that array: T = 512 keys (one workgroup of the plan and of the leaf kernel), G = 16 T = 8192 keys (one tier-1
group of mip_straddle2_kernel) and the array's end.  A case therefore says where its runs lie, not where its points are:

  runs     [(cell, count)] in key order; a cell is its RANK among the cells of its depth in key order, that is the key without
           its leading 1: the octants of the path from the root, three bits a level, x + 2 y + 4 z (cell_index gives the
           integer coordinates).  Every point of a run is the exact centre of the cell
  invalid  points of NaN: key 1, which sorts in front of every cell
  outside  points beyond the +x +y +z corner of the root cube: every level takes them for octant 7, so they join the LAST cell
           of the depth and sort behind every run
  depth    of the leaves

so the sorted array is [invalid | run 0 | run 1 | ... | outside] and its heads (first key of each run) are at the cumulative
counts: heads().  With center (0, 0, 0) and edge 1.0 the root cube is [-1, 1]^3 and the centre of cell i along an axis is
(i + 0.5) / 2^depth * 2 - 1, exact in float32 up to depth 16 and never on a splitting plane.

Cells are made from the COMMON-PREFIX LENGTHS wanted between neighbouring runs (cells_from_steps): a level-d node continues
across a cut iff the first head behind it shares >= d levels with its predecessor, so that number, c, is what a case chooses
at each cut."""
import functools

import numpy as np

T = 512                 # kPlanThreads, kFillThreads
G = 16 * T              # kStradGroup tiles
CENTER, EDGE = (0.0, 0.0, 0.0), 1.0
FORMS = ("blocking", "async", "early", "deferred", "structure")
DEPTHS_ALL = (3, 12)                    # 12: the last depth of fill_mip_local_kernel<12>
DEPTHS_MORE = (1, 2, 3, 12, 13, 16)     # 1: no mip level at all; 13: the first depth of <16>
HUGE_N = 8192 * T + T + 1               # one tile more than mip_straddle_kernel keeps in registers, and a ragged one


# ---- cells ----------------------------------------------------------------------------------------------------------------------
def cell_index(rank, depth):
    """integer coordinates (ix, iy, iz) of the cell of this rank: octant x + 2 y + 4 z of level l is digit l of the rank"""
    ix = iy = iz = 0
    for l in range(depth):
        o = (rank >> (3 * (depth - 1 - l))) & 7
        ix, iy, iz = (ix << 1) | (o & 1), (iy << 1) | ((o >> 1) & 1), (iz << 1) | (o >> 2)
    return ix, iy, iz


def cell_centre(rank, depth):
    return np.array([(i + 0.5) / (1 << depth) * 2.0 - 1.0 for i in cell_index(rank, depth)], np.float32)


def last_cell(depth):
    return (1 << (3 * depth)) - 1


def common_levels(a, b, depth):
    """levels the cells of ranks a and b share, 0 ... depth"""
    x = a ^ b
    return depth if x == 0 else depth - (x.bit_length() + 2) // 3


def cells_from_steps(depth, steps, first=None):
    """ranks of len(steps) + 1 cells in ascending key order, cell i + 1 sharing exactly steps[i] levels with cell i: the octant
    of level steps[i] + 1 goes up by one and the levels below start again at octant 0.  `first`: the first cell's octants"""
    digits = list(first) if first is not None else [0] * depth
    assert len(digits) == depth
    out = [digits[:]]
    for c in steps:
        assert 0 <= c < depth and digits[c] < 7, "no cell left that shares %d levels: %s" % (c, digits)
        digits[c] += 1
        digits[c + 1:] = [0] * (depth - c - 1)
        out.append(digits[:])
    return [functools.reduce(lambda r, o: (r << 3) | o, d, 0) for d in out]


def first_octants(depth, rng):
    """a random first cell that leaves room for four steps at every level (depth 1, with eight cells in all: the first one)"""
    return [int(o) for o in rng.integers(0, 4, depth)] if depth > 1 else [0]


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def case(family, variant, depth, runs, invalid=0, outside=0):
    runs = [(int(r), int(k)) for r, k in runs]
    assert all(k > 0 for _, k in runs) and all(a[0] < b[0] for a, b in zip(runs, runs[1:])), runs
    assert not runs or (0 <= runs[0][0] and runs[-1][0] <= last_cell(depth))
    assert not (outside and runs and runs[-1][0] == last_cell(depth))
    return {"id": "%s-%s-d%d" % (family, variant, depth), "family": family, "variant": variant, "depth": depth, "runs": runs,
            "invalid": int(invalid), "outside": int(outside)}


def size(c):
    return c.get("uniform", 0) + c["invalid"] + sum(k for _, k in c["runs"]) + c["outside"]


def all_runs(c):
    """the runs of the sorted array behind the invalid points, the outside points among them"""
    return c["runs"] + ([(last_cell(c["depth"]), c["outside"])] if c["outside"] else [])


def heads(c):
    """designed positions of the first key of every run of the sorted array, the run of key 1 included"""
    counts = ([c["invalid"]] if c["invalid"] else []) + [k for _, k in all_runs(c)]
    return [0] + np.cumsum(counts)[:-1].tolist() if counts else []


def rotated(c):
    """frame 3: the same cells with the run lengths moved on by one place, so the cuts fall on other cells of the tree"""
    counts = [k for _, k in c["runs"]]
    counts = counts[-1:] + counts[:-1]
    return dict(c, runs=[(r, k) for (r, _), k in zip(c["runs"], counts)])


def build(c, rng):
    """(pts float32 [n, 3], col uint8 [n, 3]): a distinct random colour for every point (the blend of a leaf depends on which
    point of its run comes first), the whole cloud shuffled"""
    n, depth = size(c), c["depth"]
    pts = np.empty((n, 3), np.float32)
    at = 0
    if c.get("uniform"):
        pts[:c["uniform"]] = rng.random((c["uniform"], 3), dtype=np.float32) * np.float32(1.998) - np.float32(0.999)
        at = c["uniform"]
    pts[at:at + c["invalid"]] = np.nan
    at += c["invalid"]
    for rank, k in c["runs"]:
        pts[at:at + k] = cell_centre(rank, depth)
        at += k
    if c["outside"]:    # beyond the corner by different amounts, on every axis
        pts[at:] = (1.5 + 40.0 * rng.random((c["outside"], 3))).astype(np.float32)
    rgb = rng.choice(1 << 24, n, replace=False)
    col = np.stack([rgb & 255, (rgb >> 8) & 255, rgb >> 16], 1).astype(np.uint8)
    perm = rng.permutation(n)
    return pts[perm], col[perm]


def rng_of(c):
    return np.random.default_rng([ord(ch) for ch in c["id"]])


def frames(c):
    """the three frames a case is committed as: the cloud, the same cloud again (no split but the one-off ones of octant-7 leaves,
    every leaf blends with what is there), the cloud with rotated run lengths (`huge`: two frames, both its own)"""
    rng = rng_of(c)
    if c["family"] == "huge":
        return [build(c, rng), build(c, rng)]
    first = build(c, rng)
    return [first, first, build(rotated(c), rng)]


# ---- the families ---------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng(list(seed))


def one_leaf(depth, n):
    """all n points in one cell: from n = G + 1 on a whole straddle group lies inside the run"""
    rank = int(_rng(1, depth, n).integers(0, last_cell(depth) + 1))
    return case("one_leaf", "n%d" % n, depth, [(rank, n)])


def invalid_front(depth, k):
    """k invalid points, three short runs, one run of G + 100 to the end: from k = G on group 0 has no valid head"""
    d = depth
    cells = cells_from_steps(d, [d - 1, min(1, d - 1), max(d - 2, 0)], first_octants(d, _rng(2, d, k)))
    return case("invalid_front", "k%d" % k, d, zip(cells, (3, 1, 40, G + 100)), invalid=k)


def invalid_only_tail(depth):
    """valid runs of G keys in all, then 2 G points outside the cube: one run in the last cell that starts ON the group cut and
    covers the whole of groups 1 and 2"""
    d = depth
    cells = cells_from_steps(d, [max(d - 2, 0), d - 1, 0, min(1, d - 1)], first_octants(d, _rng(3, d)))
    return case("invalid_only_tail", "2G", d, zip(cells, (1000, 3000, 1, 4000, G - 8001)), outside=2 * G)


CUTS = (T, 2 * T, G - T, G, G + T, 2 * G)


def on_the_cuts(depth, shift, first=None):
    """run boundaries at T, 2T, G-T, G, G+T, 2G (+ shift: the first run is that much longer), a ragged last run.  Siblings meet
    at T and at G, cells sharing half their levels at 2G, one level at 2T, none at G+T.  `first`: the first cell's octants"""
    d = depth
    steps = [d - 1, min(1, d - 1), max(d - 2, 0), d - 1, 0, d // 2]
    cells = cells_from_steps(d, steps, first or first_octants(d, _rng(4, d)))
    counts = (T + shift, T, G - 3 * T, T, T, G - T, T + 37)
    return case("on_the_cuts", {0: "exact", 1: "plus1", -1: "minus1"}[shift], d, zip(cells, counts))


SIBLING_RELATIONS = ("siblings", "cousins", "strangers")


def siblings(depth, relation, boundary):
    """two runs that share all levels but the last (the parent straddles the cut, the leaves do not), only level 1, or nothing,
    the first ending exactly at `boundary` (G or G - 1)"""
    d = depth
    c = {"siblings": d - 1, "cousins": min(1, d - 1), "strangers": 0}[relation]
    cells = cells_from_steps(d, [c], first_octants(d, _rng(5, d, c)))
    return case("siblings", "%s_at_%s" % (relation, "G" if boundary == G else "G-1"), d, zip(cells, (boundary, T + 5)))


def staircase_walk(depth):
    """the common-prefix lengths of neighbouring runs, one period: 0, 1, ..., depth-1, ..., 1.  A step of 0 needs a new octant of
    the root, of which there are eight: below depth 5 the walk turns round at 1 instead, until the period is at least 8"""
    if depth == 1:
        return [0]
    inner = list(range(1, depth)) + list(range(depth - 2, 1, -1))       # 1 ... depth-1 ... 2
    walk, i = [0], 0
    while len(walk) < 8 or walk[-1] != 1:
        walk.append(inner[i % len(inner)])
        i += 1
    return walk


STAIR_TILES = 3 * 16
STAIR_EDGES = (16, 32, 48)      # the tiles that begin a straddle group


def staircase_steps(depth, phase):
    w = staircase_walk(depth)
    return [w[(t - 1 + phase) % len(w)] for t in range(1, STAIR_TILES + 1)]


@functools.lru_cache(maxsize=None)
def staircase_phases(depth):
    """phases of the walk, fewest first found, after which every common-prefix length has stood at a group's edge"""
    w = staircase_walk(depth)
    want, phases = set(w), []
    while want:
        best = max(range(len(w)), key=lambda p: len(want & {staircase_steps(depth, p)[t - 1] for t in STAIR_EDGES}))
        phases.append(best)
        want -= {staircase_steps(depth, best)[t - 1] for t in STAIR_EDGES}
    return tuple(phases)


def staircase(depth, phase):
    """3 x 16 + 1 runs of exactly T keys: run i is tile i, the last one a group of a single tile.  Depth 1 has eight cells: eight
    runs of 4 T, the fifth beginning group 1"""
    if depth == 1:
        return case("staircase", "p0", 1, [(r, 4 * T) for r in range(8)])
    cells = cells_from_steps(depth, staircase_steps(depth, phase))
    return case("staircase", "p%d" % phase, depth, [(r, T) for r in cells])


def ragged_end(depth, n, last):
    """n = G + 1 or 2 G + T + 1: the last tile holds one key, `head`: a run of its own, `tail`: the end of a long run"""
    d = depth
    cells = cells_from_steps(d, [d - 1, min(1, d - 1)], first_octants(d, _rng(6, d, n)))
    a = G - 700 if n == G + 1 else G + 300
    counts = (a, n - a - 1, 1) if last == "head" else (a, n - a)
    return case("ragged_end", "n%d_%s" % (n, last), d, zip(cells, counts))


def random_runs(depth, seed, total=60000):
    """run lengths log-uniform in [1, 3 G], random cells (every other one a near neighbour of the one before, so that prefixes
    are shared), 5 % invalid points"""
    rng = _rng(7, depth, seed)
    invalid = total // 20
    counts, left = [], total - invalid
    most = min(last_cell(depth) + 1, 4096)
    while left > 0 and len(counts) < most:
        k = min(left, int(np.exp(rng.uniform(0.0, np.log(3 * G)))))
        counts.append(k)
        left -= k
    counts[-1] += left      # (depth 1: eight cells take what is there)
    cells = set()
    while len(cells) < len(counts):
        r = int(rng.integers(0, last_cell(depth) + 1))
        cells.add(r)
        if len(cells) < len(counts):
            cells.add(min(last_cell(depth), r + int(rng.integers(1, 9))))
    return case("random_runs", "s%d" % seed, depth, zip(sorted(cells), counts), invalid=invalid)


def huge():
    """uniformly random points, not designed by runs: 8194 fill tiles, 513 straddle groups"""
    c = case("huge", "uniform", 3, [])
    c["uniform"] = HUGE_N
    return c


def _table():
    out = []
    for d in DEPTHS_ALL:
        out += [one_leaf(d, n) for n in (T, T + 1, G - 1, G, G + 1, 2 * G + 1)]
        out += [invalid_front(d, k) for k in (T, G, G + T + 1)]
        out.append(invalid_only_tail(d))
        out += [siblings(d, r, b) for r in SIBLING_RELATIONS for b in (G, G - 1)]
        out += [ragged_end(d, n, last) for n in (G + 1, 2 * G + T + 1) for last in ("head", "tail")]
    for d in DEPTHS_MORE:
        out += [on_the_cuts(d, s) for s in (0, 1, -1)]
        out += [staircase(d, p) for p in staircase_phases(d)]
        out += [random_runs(d, s) for s in (1, 2, 3)]
    return out


CASES = _table()
HUGE = huge()
BY_ID = {c["id"]: c for c in CASES + [HUGE]}
assert len(BY_ID) == len(CASES) + 1


def family(name, depth=None):
    return [c for c in CASES if c["family"] == name and depth in (None, c["depth"])]
