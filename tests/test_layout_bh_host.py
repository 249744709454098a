"""The Barnes-Hut statement (pangenomenem_amd/layout_bh.py: tree_arrays, walk, layout_bh_arrays) held to what it says of
itself, on the CPU: the tree's invariants, that every walk covers every body exactly once (what a wrong rope or a
skipped sibling breaks), theta = 0 as the exact pair set in another order, the inputs without a tree, and that the error
against the exact statement does not grow as theta shrinks.  tests/test_gpu_layout_bh.py holds the device to this
statement bit for bit; the inputs are tests/layout_bh_util.py's."""
import ctypes as C
import types

import numpy as np
import pytest

from pangenomenem_amd import layout as ly
from pangenomenem_amd import layout_bh as bh
from pangenomenem_amd.engine import load_library
from pangenomenem_amd.layout import layout_arrays
from pangenomenem_amd.layout_bh import DEPTH, LEAF, layout_bh_arrays, tree_arrays, walk
from tests.layout_bh_util import CASES, LARGE_CASES, case, check_large, check_tree, large_properties, statement_step, statement_tree
from tests.layout_util import U, ring_with_chords


@pytest.mark.parametrize("name", CASES)
def test_tree_invariants(name):
    c, t = case(name), statement_tree(name)
    check_tree(t, c["mass"], name)
    if name in ("bucket", "chain"):                           # a level-DEPTH leaf above LEAF under a chain of single-child cells
        deep = np.nonzero((t["level"] == DEPTH) & (t["hi"] - t["lo"] == LEAF + 4))[0]
        assert len(deep) == 1
        chain = [k for k in range(t["cells"]) if t["lo"][k] == t["lo"][deep[0]] and t["hi"][k] == t["hi"][deep[0]]]
        assert len(chain) > DEPTH // 2 and all(t["child"][k] == chain[j + 1] for j, k in enumerate(chain[:-1]))
    if name == "far_edges":                                   # the far edge gives G before the clamp
        x = t["key"][[3, 5]].astype(np.uint64)
        assert int(x[0]) & 0x55555555 == 0x55555555 and int(x[1]) & 0xAAAAAAAA == 0xAAAAAAAA
    if name == "centre":
        cx, cy = t["Sx"] / t["M"], t["Sy"] / t["M"]
        hit = [k for k in range(t["cells"]) if t["child"][k] >= 0 and cx[k] == c["pos"][10, 0] and cy[k] == c["pos"][10, 1]]
        assert hit, "no inner cell has the body at its centre"
    if name in ("horizontal", "vertical"):
        keep = 0x55555555 if name == "horizontal" else 0xAAAAAAAA
        assert not (t["key"] & np.uint32(0xFFFFFFFF ^ keep)).any()


@pytest.mark.parametrize("name", LARGE_CASES)
def test_the_large_inputs_are_what_they_claim(name):
    """the scan's passes over the 17 n flags, cells behind every pass boundary, for the clustered ones a tree down to
    level DEPTH with a leaf of hundreds there, the bound on the cells -- and the invariants every tree is held to
    (check_tree is linear in n: it runs at every size here)"""
    check_large(name)
    p = large_properties(name)
    print("%s: %d scan passes over %d flags (they begin in levels %s), cells per pass %s, deepest level %d, its largest leaf %d, %d cells of at most %d, %d blocks"
          % (name, p["passes"], (DEPTH + 1) * p["n"], p["level_of_pass"], p["cells_in_pass"], p["deepest"], p["deep_leaf"], p["cells"], p["bound"], p["blocks"]))
    check_tree(statement_tree(name), case(name)["mass"], name)


def test_check_tree_sees_a_wrong_cell_a_wrong_moment_and_a_wrong_order():
    t, mass = statement_tree("n1500"), case("n1500")["mass"]
    check_tree(t, mass, "as it is")
    inner = int(np.nonzero((t["level"] == 3) & (t["child"] >= 0))[0][0])
    spoiled = []
    for key, at, by in (("hi", inner, -1), ("lo", t["cells"] - 1, 1), ("M", inner, 1.0), ("level", t["cells"] - 1, -1)):
        a = t[key].copy()
        a[at] += by
        spoiled.append(dict(t, **{key: a}))
    spoiled += [dict(t, level=t["level"][:-1], lo=t["lo"][:-1], hi=t["hi"][:-1], child=t["child"][:-1], cells=t["cells"] - 1)]
    for k, bad in enumerate(spoiled):
        with pytest.raises(AssertionError):
            check_tree(bad, mass, "spoiled %d" % k)
    t, mass = statement_tree("bucket"), case("bucket")["mass"]               # (bodies in one grid cell: their indices ascend)
    same = np.nonzero(np.diff(t["key"][t["order"]].astype(np.int64)) == 0)[0]
    swapped = t["order"].copy()
    swapped[[same[0], same[0] + 1]] = swapped[[same[0] + 1, same[0]]]
    with pytest.raises(AssertionError, match="equal keys"):
        check_tree(dict(t, order=swapped), mass, "two equal keys out of order")


@pytest.mark.parametrize("theta", [1.2, 0.5, 0.0])
@pytest.mark.parametrize("name", CASES)
def test_every_walk_covers_every_body_once(name, theta):
    c, t = case(name), statement_tree(name)
    n = c["n"]
    _, _, accepted, visited, covered = walk(t, c["pos"], c["mass"], 50000.0, theta, ranges=True)
    for i in range(n):
        if t["cells"] == 0:
            assert covered[i] == [] and accepted[i] == visited[i] == 0
            continue
        spans = covered[i]
        assert spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (name, i, spans)
    if theta == 0.0:
        assert not accepted.any() and (visited == (n if t["cells"] else 0)).all()
    if theta == 1.2 and name == "n1500":
        assert accepted.mean() > 4 and visited.mean() < n / 8


@pytest.mark.parametrize("name", CASES)
def test_theta_zero_is_the_exact_sum_in_another_order(name):
    """every pair term is layout_arrays', only the order is the tree's: within 2 n u B of the exactly rounded sum"""
    c = case(name)
    got = statement_step(name, 0.0)
    want = layout_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=c["pos"], order="fsum")
    assert not got["accepted"].any()
    assert (np.abs(got["forces"] - want["forces"]) <= 2.0 * c["n"] * U * want["bound"]).all()
    assert np.allclose(got["bound"], want["bound"], rtol=1e-12, atol=0.0)      # (the same terms' absolute values)


@pytest.mark.parametrize("name", ["n0", "n1", "coincident"])
def test_without_a_tree_there_is_no_repulsion(name):
    c, t = case(name), statement_tree(name)
    assert t["side"] == 0.0 and t["cells"] == 0
    # (one iteration: gravity then pulls families of unequal mass apart, and a tree appears)
    got = layout_bh_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=c["pos"])
    want = layout_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=c["pos"], order="left")
    assert not got["repulsion"].any()
    assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["forces"], want["forces"])
    assert (got["speed"], got["eff"], got["S"], got["T"]) == (want["speed"], want["eff"], want["S"], want["T"])


def test_the_error_does_not_grow_as_theta_shrinks():
    """a ring of 300 with chords after 20 exact iterations: the rms over the families of |F_bh - F_exact| / |F_exact| of the
    repulsion, along theta 1.2, 0.6, 0.3, 0 (the values are reported in profiles/layout.md; no bound is put on them)"""
    n, d = 300, 9
    x, graph, eb = ring_with_chords(n, d, 20241)
    start = np.random.default_rng(20242).random((n, 2))
    laid = layout_arrays(graph, eb, d, iterations=20, pos=start, order="left")["pos"]
    mass = ly.layout_graph(graph, eb, d)["mass"]
    dx, dy = laid[:, 0][:, None] - laid[:, 0][None, :], laid[:, 1][:, None] - laid[:, 1][None, :]
    d2 = dx * dx + dy * dy
    with np.errstate(divide="ignore", invalid="ignore"):
        coef = np.where(d2 > 0.0, ((50000.0 * mass)[:, None] * mass[None, :]) / d2, 0.0)
    want = np.stack([(dx * coef).sum(axis=1), (dy * coef).sum(axis=1)], axis=1)     # (layout_arrays' step 1)
    t = tree_arrays(laid, mass)
    errors = []
    for theta in (1.2, 0.6, 0.3, 0.0):
        rep = walk(t, laid, mass, 50000.0, theta)[0]
        rel = np.sqrt(((rep - want) ** 2).sum(axis=1) / (want ** 2).sum(axis=1))
        errors.append(float(np.sqrt((rel ** 2).mean())))
    print("rms relative error of the repulsion at theta 1.2, 0.6, 0.3, 0: %s" % ", ".join("%.3g" % e for e in errors))
    assert all(a >= b for a, b in zip(errors, errors[1:])), errors


def test_what_python_refuses():
    nobody = types.SimpleNamespace()                          # (refused before the master is looked at)
    with pytest.raises(ValueError, match="repulsion"):
        ly.Layout(nobody, repulsion="x")
    for theta in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="theta"):
            ly.Layout(nobody, repulsion="barnes_hut", theta=theta)
        with pytest.raises(ValueError, match="theta"):
            layout_bh_arrays((np.zeros(1, np.int32), np.zeros(0, np.int32)), np.zeros((0, 1), np.uint32), 3, iterations=0, theta=theta)
    with pytest.raises(TypeError):
        ly.Layout(nobody, repulsion="barnes_hut", barnes_hut_theta=1.2)


def test_the_shape_is_the_librarys():
    lib = ly._bind_layout(load_library())
    depth, leaf = C.c_int(), C.c_int()
    assert lib.nemgpu_layout_bh_shape(C.byref(depth), C.byref(leaf)) == 0
    assert (depth.value, leaf.value) == (DEPTH, LEAF) == (16, 8)
    assert [bh.cell_bound(n) for n in (0, 8, 9, 17, 18, 1500)] == [1, 1, 65, 65, 129, 1 + 16 * 664]
