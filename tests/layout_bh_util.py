"""What tests/test_layout_bh_host.py and tests/test_gpu_layout_bh.py share: the input bodies -- the smallest at which the
tree, the walk or a kernel of csrc/nem_layout_bh.hip can go wrong -- each a symmetric master as arrays (tests/layout_util.py)
with start positions, the statement's answers computed once per case, and the checks of a tree that both sides run.

LARGE_CASES are the sizes at which the device's large-n paths begin (the cell numbering is one scan over (DEPTH + 1) n
flags, tests/master_shapes.py: SCAN_PASS items per pass of k_scan_partials; k_bh_box and k_layout_speed stride over the
blocks of 256 bodies above 256 of them); large_properties / check_large hold each to what it is there for."""
import functools

import numpy as np

from pangenomenem_amd import synth
from pangenomenem_amd.layout import layout_graph
from pangenomenem_amd.layout_bh import DEPTH, LEAF, cell_bound, layout_bh_arrays, tree_arrays
from tests.layout_util import arrays_of, ring_with_chords
from tests.master_shapes import SCAN_PASS, scan_passes

D = 9
SIZES = (0, 1, 2, 3, LEAF, LEAF + 1, 255, 256, 257, 1500)
SHAPED = ("coincident", "horizontal", "vertical", "far_edges", "bucket", "chain", "centre")
CASES = ["n%d" % n for n in SIZES] + list(SHAPED)
DEVICE_CASES = [c for c in CASES if c != "n0"]                # (a master of no family cannot be made)
TREE_KEYS = ("key", "order", "level", "lo", "hi", "M", "Sx", "Sy", "child", "rope")
# name: (n, the passes of the scan over (DEPTH + 1) n flags).  Kept out of CASES: those feed the theta 0 walks (n^2)
LARGE = {"clustered30840": (30840, 1),                        # one below the scan's second pass
         "clustered30841": (30841, 2),                        # one above: the carry begins
         "clustered32768": (32768, 2),                        # the second pass is level DEPTH alone
         "uniform65793": (65793, 3),                          # 258 blocks of bodies; the first pass ends inside level 7
         "clustered65793": (65793, 3)}                        # the same with a deep tree
LARGE_CASES = list(LARGE)
HALF = 1.0e5                                                  # the large cases' square is [-HALF, HALF]^2: the extent such a layout settles at
CENTRES = 32
BLOCK = 256                                                   # kLayoutTile: the bodies of one block of k_bh_box_blocks / k_layout_forces


def _graph(n, seed):
    """(x, (ptr, idx), edge_bits, counts or None): nothing below 2 families, a ring with chords below 255, above it a
    master with self-loops and counts (uneven masses)"""
    if n < 2:
        return arrays_of(n, [], D) + (None,)
    if n < 255:
        return ring_with_chords(n, D, seed) + (None,)
    return synth.master_pangenome_counts(n, D, seed, loops=0.05, multi_frac=0.1)


def _clustered(rng, n):
    """CENTRES centres, around each bodies at spreads from 2^-8 to 2^12 grid cells (a cell: side / 2^DEPTH), so that
    levels 9 .. DEPTH hold cells and a level-DEPTH leaf holds hundreds; bodies 0 and 1 pin the square's corners, and
    bodies 2 .. 8 fill the 2 x 2 grid cells at the far corner -- the last sorted positions -- with 2 (body 1 included), 2, 2
    and 3 bodies, LEAF + 1 in all: four level-DEPTH cells that start within the last LEAF + 1 sorted positions, behind
    every pass boundary"""
    cell = 2.0 * HALF / 2 ** DEPTH
    centres = (rng.random((CENTRES, 2)) * 1.6 - 0.8) * HALF
    spread = cell * 2.0 ** rng.choice([-8.0, -5.0, -2.0, 1.0, 4.0, 7.0, 10.0, 12.0], n)
    pos = centres[rng.integers(0, CENTRES, n)] + rng.standard_normal((n, 2)) * spread[:, None]
    np.clip(pos, -HALF, HALF - 4.0 * cell, out=pos)
    pos[0], pos[1] = (-HALF, -HALF), (HALF, HALF)
    at = 2
    for (cx, cy), count in (((1, 1), 1), ((0, 1), 2), ((1, 0), 2), ((0, 0), 3)):
        corner = HALF - np.array([2 - cx, 2 - cy]) * cell
        pos[at:at + count] = corner + (0.05 + 0.9 * rng.random((count, 2))) * cell
        at += count
    return pos


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: name, n, d, x, graph, eb, counts, mass, pos float64 [n][2]"""
    rng = np.random.default_rng(sum(name.encode()))
    if name in LARGE:
        n = LARGE[name][0]
        x, graph, eb, counts = _graph(n, 100 + n)
        pos = _clustered(rng, n) if name.startswith("clustered") else (rng.random((n, 2)) * 2.0 - 1.0) * HALF
    elif name.startswith("n"):
        n = int(name[1:])
        x, graph, eb, counts = _graph(n, 100 + n)
        pos = rng.random((n, 2)) * 40.0 - 20.0
    else:
        n = 30 + LEAF + 4 if name in ("bucket", "chain") else 40
        x, graph, eb, counts = ring_with_chords(n, D, 7, chords=0.0 if name == "centre" else 0.2) + (None,)
        pos = rng.random((n, 2))
        if name == "coincident":
            pos[:] = (0.3, -0.7)
        elif name == "horizontal":
            pos[:, 1] = 0.25
        elif name == "vertical":
            pos[:, 0] = -3.0
        elif name == "far_edges":                             # one body exactly at max x, one exactly at max y of a square: the clamp
            pos[0] = (0.0, 0.0)
            pos[3] = (2.0, 0.5)
            pos[5] = (0.5, 2.0)
        elif name == "bucket":                                # LEAF + 4 coincident bodies: a level-DEPTH leaf above LEAF
            pos[4:4 + LEAF + 4] = pos[4]
        elif name == "chain":                                 # LEAF + 4 distinct bodies within side * 2^-20: single-child cells down to DEPTH
            side = float((pos.max(axis=0) - pos.min(axis=0)).max())
            pos[4:4 + LEAF + 4] = pos[4] + (np.arange(LEAF + 4)[:, None] * np.array([1.0, 0.5])) * side * 2.0 ** -25
        elif name == "centre":                                # every mass is 3: nine bodies whose centre of mass is one of them, exactly
            pos[:, 0] = 0.5 + 0.5 * pos[:, 0]
            pos[0], pos[1] = (0.0, 0.0), (1.0, 1.0)
            off = np.array([(1, 1), (1, -2), (2, 1), (3, 3)], np.float64) / 64.0
            pos[2:6], pos[6:10], pos[10] = 0.375 + off, 0.375 - off, (0.375, 0.375)
    mass = layout_graph(graph, eb, D)["mass"]
    pos.setflags(write=False)
    return dict(name=name, n=n, d=D, x=x, graph=graph, eb=eb, counts=counts, mass=mass, pos=pos)


@functools.lru_cache(maxsize=None)
def statement_tree(name):
    c = case(name)
    return tree_arrays(c["pos"], c["mass"])


@functools.lru_cache(maxsize=None)
def statement_step(name, theta):
    """one iteration of the statement from the case's start (S and T exactly rounded)"""
    c = case(name)
    return layout_bh_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=c["pos"], theta=theta, order="fsum")


def check_tree(t, mass, what):
    """the invariants of a tree, the statement's or the device's"""
    n, cells = t["n"], t["cells"]
    level, lo, hi, child = t["level"], t["lo"], t["hi"], t["child"]
    assert cells <= t["bound"] == cell_bound(n), what
    assert sorted(t["order"].tolist()) == list(range(n)), what
    skey = t["key"][t["order"]].astype(np.uint64)
    assert (np.diff(skey.astype(np.int64)) >= 0).all(), what
    same = np.diff(skey.astype(np.int64)) == 0
    assert (np.diff(t["order"])[same] > 0).all(), what + ": equal keys keep the order of their indices"
    if not t["side"] > 0.0:
        assert cells == 0 and not t["key"].any(), what
        return
    assert cells >= 1 and (level[0], lo[0], hi[0]) == (0, 0, n), what
    assert (np.diff(level * (n + 1) + lo) > 0).all(), what + ": numbered by level, then by run order"
    # a cell exists iff its prefix's run lies under a run of more than LEAF bodies: rebuild the cells from the keys alone
    # (per level the runs of equal prefixes; np.unique counts the bodies of the run one level up: linear in n)
    want = []
    for l in range(DEPTH + 1):
        pre = skey >> np.uint64(2 * (DEPTH - l))
        starts = np.nonzero(np.append(True, pre[1:] != pre[:-1]))[0]
        ends = np.append(starts[1:], n)
        if l > 0:
            _, inverse, counts = np.unique(skey >> np.uint64(2 * (DEPTH - l + 1)), return_inverse=True, return_counts=True)
            exists = counts[inverse.ravel()][starts] > LEAF
            starts, ends = starts[exists], ends[exists]
        want.append(np.stack([np.full(len(starts), l, np.int64), starts, ends], axis=1))
    want = np.concatenate(want)                               # (by level, then by run order: the cells' own numbering)
    assert np.array_equal(np.stack([level, lo, hi], axis=1), want), what
    leaf = child < 0
    assert np.array_equal(leaf, (hi - lo <= LEAF) | (level == DEPTH)), what
    # the leaves partition the sorted bodies; the children partition their parent
    cover = np.zeros(n, np.int64)
    for c in np.nonzero(leaf)[0]:
        cover[lo[c]:hi[c]] += 1
    assert (cover == 1).all(), what
    for c in np.nonzero(~leaf)[0]:
        k, at = int(child[c]), int(lo[c])
        while at < hi[c]:
            assert level[k] == level[c] + 1 and lo[k] == at and hi[k] <= hi[c], (what, c, k)
            at, k = int(hi[k]), k + 1
        assert at == hi[c], (what, c)
    below = np.append(0, np.cumsum(np.asarray(mass)[t["order"]].astype(np.int64)))      # (the masses are whole numbers)
    assert np.array_equal(t["M"], (below[hi] - below[lo]).astype(np.float64)), what


def same_tree(got, want, what):
    for k in ("n", "x0", "y0", "side", "cells", "bound"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in TREE_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


@functools.lru_cache(maxsize=None)
def large_properties(name):
    """what a large case is there for, from the statement's tree alone: passes (of the scan over (DEPTH + 1) n flags), per
    pass the cells whose flag lies in it (flat index level * n + lo), the deepest level, the largest level-DEPTH leaf,
    cells, bound, blocks (of 256 bodies), equal_keys (sorted neighbours with one key: the sort must keep their indices in
    order), level_of_pass (the level each pass begins in)"""
    c, t = case(name), statement_tree(name)
    n = c["n"]
    flat = t["level"] * n + t["lo"]
    passes = scan_passes((DEPTH + 1) * n)
    deep = t["level"] == DEPTH
    return dict(n=n, passes=passes, cells_in_pass=[int(((flat >= k * SCAN_PASS) & (flat < (k + 1) * SCAN_PASS)).sum()) for k in range(passes)],
                deepest=int(t["level"].max()), deep_leaf=int((t["hi"] - t["lo"])[deep].max()) if deep.any() else 0, cells=t["cells"],
                bound=cell_bound(n), blocks=-(-n // BLOCK), equal_keys=int((np.diff(np.sort(t["key"])) == 0).sum()),
                level_of_pass=[k * SCAN_PASS // n for k in range(passes)])


def check_large(name):
    """a large case is what it claims (LARGE's comments)"""
    n, passes = LARGE[name]
    p = large_properties(name)
    assert (p["n"], p["passes"]) == (n, passes) and scan_passes((DEPTH + 1) * n) == passes, (name, p)
    assert p["cells"] <= p["bound"] and p["cells"] > 1000, (name, p)
    # cells whose flags lie behind a pass boundary: a lost carry shows in their numbers -- child, rope -- not only in the total
    assert passes == 1 or sum(p["cells_in_pass"][1:]) > 0, (name, p)
    if name.startswith("clustered"):
        assert p["deepest"] == DEPTH and p["deep_leaf"] > 64 and p["equal_keys"] > 1000, (name, p)
        assert p["cells_in_pass"][-1] >= 4, (name, p)         # (the far corner's cells: the last sorted positions at level DEPTH)
    if name == "clustered32768":
        assert p["level_of_pass"] == [0, DEPTH] and SCAN_PASS == DEPTH * n
    if n == 65793:
        assert p["blocks"] == 258 and p["level_of_pass"][1] == 7, (name, p)
    if name == "uniform65793":
        assert p["cells_in_pass"][1] > 1000, (name, p)        # (level 7 holds thousands of cells; hundreds of them behind the boundary)
