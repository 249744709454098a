"""What tests/test_layout_bh_host.py and tests/test_gpu_layout_bh.py share: the input bodies -- the smallest at which the
tree, the walk or a kernel of csrc/nem_layout_bh.hip can go wrong -- each a symmetric master as arrays (tests/layout_util.py)
with start positions, the statement's answers computed once per case, and the checks of a tree that both sides run."""
import functools

import numpy as np

from pangenomenem_amd import synth
from pangenomenem_amd.layout import layout_graph
from pangenomenem_amd.layout_bh import DEPTH, LEAF, cell_bound, layout_bh_arrays, tree_arrays
from tests.layout_util import arrays_of, ring_with_chords

D = 9
SIZES = (0, 1, 2, 3, LEAF, LEAF + 1, 255, 256, 257, 1500)
SHAPED = ("coincident", "horizontal", "vertical", "far_edges", "bucket", "chain", "centre")
CASES = ["n%d" % n for n in SIZES] + list(SHAPED)
DEVICE_CASES = [c for c in CASES if c != "n0"]                # (a master of no family cannot be made)
TREE_KEYS = ("key", "order", "level", "lo", "hi", "M", "Sx", "Sy", "child", "rope")


def _graph(n, seed):
    """(x, (ptr, idx), edge_bits, counts or None): nothing below 2 families, a ring with chords below 255, above it a
    master with self-loops and counts (uneven masses)"""
    if n < 2:
        return arrays_of(n, [], D) + (None,)
    if n < 255:
        return ring_with_chords(n, D, seed) + (None,)
    return synth.master_pangenome_counts(n, D, seed, loops=0.05, multi_frac=0.1)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: name, n, d, x, graph, eb, counts, mass, pos float64 [n][2]"""
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("n"):
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
    # a cell exists iff its prefix's run lies under a run of more than LEAF bodies: rebuild the set from the keys alone
    want = set()
    for l in range(DEPTH + 1):
        pre = skey >> np.uint64(2 * (DEPTH - l))
        starts = np.nonzero(np.append(True, pre[1:] != pre[:-1]))[0]
        ends = np.append(starts[1:], n)
        for a, z in zip(starts.tolist(), ends.tolist()):
            if l == 0:
                want.add((0, a, z))
                continue
            up = skey >> np.uint64(2 * (DEPTH - l + 1))
            if int((up == up[a]).sum()) > LEAF:
                want.add((l, a, z))
    assert set(zip(level.tolist(), lo.tolist(), hi.tolist())) == want, what
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
    smass = np.asarray(mass)[t["order"]]
    for c in range(cells):
        assert t["M"][c] == float(int(smass[lo[c]:hi[c]].sum())), (what, c)


def same_tree(got, want, what):
    for k in ("n", "x0", "y0", "side", "cells", "bound"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in TREE_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
