"""The Barnes-Hut repulsion on the device (nemgpu_layout_create_bh, csrc/nem_layout_bh.hip; Master.layout(repulsion=
"barnes_hut")) against the numpy statement pangenomenem_amd/layout_bh.py, which tests/test_layout_bh_host.py holds to its
own rules.

The tree is the statement's bit for bit -- keys, order, cells, moments -- and so is every force: the walk accumulates in
the statement's order, and k_layout_forces adds gravity and the row's entries behind it as layout_bh_arrays does.  Only S
and T are summed in the device's own trees, so they, the speed and the positions are held as tests/layout_util.py's
step_tolerances holds the exact path, with the force term of the bound set to zero.  The inputs are
tests/layout_bh_util.py's: the smallest at which a kernel takes another path.

Its LARGE cases are the sizes at which the large-n paths begin -- the passes of the scan that numbers the cells over
17 n flags (524 288 per pass), the stride of k_bh_box and k_layout_speed over more than 256 blocks of bodies, rocPRIM's
radix sort at tens of thousands of pairs with equal keys -- at theta 1.2 only (theta 0 is n^2 per lane, and minutes of the
statement's walk).  The path each reaches, and the wall times on an MI355X host of its tree test / its two steps (the
statement on one core is nearly all of both):
  clustered30840   1 scan pass (8 flags below the second), 121 blocks, a tree down to level 16       0.6 s / 0.7 s
  clustered30841   2 scan passes: the carry's first n; four level-16 cells behind the boundary      0.6 s / 0.6 s
  clustered32768   2 scan passes, the second level 16 alone (753 cells), 128 blocks                  0.7 s / 0.7 s
  uniform65793     3 scan passes, the first boundary inside level 7 (1 700 cells behind), 258 blocks 0.3 s / 0.4 s
  clustered65793   3 scan passes with cells in each, 258 blocks, level-16 leaves of hundreds         1.5 s / 1.7 s
  clustered65793   three steps and two against five, the tree after them                            0.1 s"""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd import layout as ly
from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.gexf import write_gexf
from pangenomenem_amd.layout_bh import cell_bound, layout_bh_arrays, tree_arrays
from tests.gexf_util import contigs_orders, path_contigs, sizes_of
from tests.layout_bh_util import DEVICE_CASES, LARGE_CASES, case, check_large, check_tree, same_tree, statement_step, statement_tree
from tests.layout_util import LAYOUT_FIXTURES, U, base_record, branches, check_margins, ring_with_chords, step_tolerances
from tests.orders_util import load
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

E_ARG = 3
BH = dict(repulsion="barnes_hut")


def master_of(c):
    ptr, idx = c["graph"]
    return Master(c["x"], ptr, idx, c["eb"], edge_counts=c["counts"]) if c["counts"] is not None else Master(c["x"], ptr, idx, c["eb"])


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_the_tree_is_the_statements_bit_for_bit(gpu_lib, name):
    c = case(name)
    m = master_of(c)
    try:
        lay = m.layout(0, pos=c["pos"], **BH)
        got = lay.tree()
        lay.close()
    finally:
        m.close()
    same_tree(got, statement_tree(name), name)
    check_tree(got, c["mass"], name)


def steps_against_the_statement(name, theta, steps=2):
    """each step against one iteration of the statement from the device's own state before it: forces and counters equal,
    S, T, speed and positions within the bound that the order of S and T alone leaves"""
    c = case(name)
    n, mass = c["n"], c["mass"]
    m = master_of(c)
    try:
        lay = m.layout(0, pos=c["pos"], theta=theta, **BH)
        pos, old, speed, eff = np.array(c["pos"]), np.zeros((n, 2)), 1.0, 1.0
        for step in range(steps):
            want = layout_bh_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=pos, old=old, speed=speed, eff=eff, theta=theta, order="fsum")
            if want["moved"]:
                check_margins(want["comparisons"][0], not old.any(), "%s step %d" % (name, step))
            tol = step_tolerances(n, mass, dict(want, bound=np.zeros((n, 2))), old, speed)
            counted = lay.tree()
            assert np.array_equal(counted["accepted"], want["accepted"]) and np.array_equal(counted["visited"], want["visited"]), (name, step)
            lay.run(1)
            got_pos, got_f, st = lay.positions(), lay.forces(), lay.state()
            assert np.array_equal(got_f, want["forces"]), "%s step %d: a force is not the statement's" % (name, step)
            print("%s theta %g step %d: S off by %.3g (bound %.3g), T by %.3g (%.3g), speed %r / %r" %
                  (name, theta, step, abs(st["S"] - want["S"]), tol["S"], abs(st["T"] - want["T"]), tol["T"], st["speed"], want["speed"]))
            assert abs(st["S"] - want["S"]) <= tol["S"] and abs(st["T"] - want["T"]) <= tol["T"], (name, step, st, want["S"], want["T"])
            assert st["eff"] == want["eff"], (name, step)
            assert abs(st["speed"] - want["speed"]) <= tol["speed"], (name, step, st["speed"], want["speed"], tol["speed"])
            assert (np.abs(got_pos - want["pos"]) <= tol["pos"]).all(), "%s step %d: a position is off its bound" % (name, step)
            assert st["iterations"] == step + 1 and (st["T"] != 0.0) == want["moved"]
            if want["moved"]:
                old = got_f
            pos, speed, eff = got_pos, st["speed"], st["eff"]
        lay.close()
    finally:
        m.close()


@pytest.mark.parametrize("theta", [1.2, 0.0])
@pytest.mark.parametrize("name", DEVICE_CASES)
def test_one_step_and_two(gpu_lib, name, theta):
    steps_against_the_statement(name, theta)


@pytest.mark.parametrize("name", LARGE_CASES)
def test_the_tree_at_the_sizes_where_the_scan_carries_and_the_blocks_are_strided(gpu_lib, name):
    """tests/layout_bh_util.py's LARGE: the cell numbering's scan in one pass, in two from the first n that needs them, in
    two with the second all of level DEPTH, in three; 258 blocks of bodies for k_bh_box's stride; a radix sort of 30 000
    and 65 000 pairs with thousands of equal keys.  Keys, order, cells, links, moments, the box and the walk's counters
    at theta 1.2 are the statement's bit for bit (check_large: the cells behind the pass boundaries are there)."""
    check_large(name)
    c = case(name)
    m = master_of(c)
    try:
        lay = m.layout(0, pos=c["pos"], **BH)
        got = lay.tree()
        lay.close()
    finally:
        m.close()
    same_tree(got, statement_tree(name), name)
    check_tree(got, c["mass"], name)
    want = statement_step(name, 1.2)
    assert np.array_equal(got["accepted"], want["accepted"]) and np.array_equal(got["visited"], want["visited"]), name
    assert got["accepted"].any() and got["visited"].any()


@pytest.mark.parametrize("name", LARGE_CASES)
def test_two_steps_at_the_large_sizes(gpu_lib, name):
    """test_one_step_and_two's body at theta 1.2 (theta 0 is n^2 per lane and minutes of the statement's walk here): the
    65 793 cases run k_layout_forces in 258 blocks and k_layout_speed's stride over their sums, which the exact path shares"""
    steps_against_the_statement(name, 1.2)


@pytest.mark.parametrize("name", ["n256", "n257", "n1500"])
def test_theta_zero_against_the_exact_path_on_the_device(gpu_lib, name):
    """the same pair terms in two orders: each within n u B of the exact sum (n - 1 terms), so within 2 n u B of each other"""
    c = case(name)
    m = master_of(c)
    try:
        a, b = m.layout(1, pos=c["pos"], theta=0.0, **BH), m.layout(1, pos=c["pos"])
        fa, fb = a.forces(), b.forces()
        a.close()
        b.close()
    finally:
        m.close()
    B = ly.layout_arrays(c["graph"], c["eb"], c["d"], iterations=1, pos=c["pos"], order="left")["bound"]
    worst = float((np.abs(fa - fb) / (2.0 * c["n"] * U * B)).max())
    print("%s: theta 0 against the exact path at %.3f of the bound" % (name, worst))
    assert (np.abs(fa - fb) <= 2.0 * c["n"] * U * B).all()


def test_ten_steps_within_a_measured_tolerance(gpu_lib):
    """tests/test_gpu_layout.py's method: the forces being the statement's, what differs is the order of S and T alone; s is
    the largest deviation, relative to the layout's extent, of the statement with S and T summed left to right and in a
    seeded permutation of the families from the fsum run after 10 iterations, and the device, one more order, must lie
    within 8 s of the fsum run (one iteration of the ten takes its speed from S and T: the others halve or keep it)"""
    n, d, its = 300, 9, 10
    x, (ptr, idx), eb = ring_with_chords(n, d, 20241)
    pos = np.random.default_rng(20242).random((n, 2))
    perm = np.random.default_rng(20243).permutation(n)
    runs = {order: layout_bh_arrays((ptr, idx), eb, d, iterations=its, pos=pos, order=order, perm=perm) for order in ("fsum", "left", "perm")}
    assert branches(runs["fsum"]) == branches(runs["left"]) == branches(runs["perm"])
    for k, made in enumerate(runs["fsum"]["comparisons"]):
        check_margins(made, k == 0, "ring iteration %d" % k)
    ref = runs["fsum"]["pos"]
    extent = float((ref.max(axis=0) - ref.min(axis=0)).max())
    s = max(float(np.abs(runs[order]["pos"] - ref).max()) for order in ("left", "perm")) / extent
    assert 0.0 < s < 1e-9
    m = Master(x, ptr, idx, eb)
    try:
        lay = m.layout(its, pos=pos, **BH)
        got, st = lay.positions(), lay.state()
        lay.close()
    finally:
        m.close()
    dev = float(np.abs(got - ref).max()) / extent
    print("ten Barnes-Hut steps on a ring of %d with chords: s = %.3g, the device is %.3g from the fsum run (%.2f s)" % (n, s, dev, dev / s))
    assert dev <= 8.0 * s
    assert st["eff"] == runs["fsum"]["eff"] and st["iterations"] == its


def test_runs_repeat_bit_for_bit_and_a_tree_in_between_changes_nothing(gpu_lib):
    c = case("n1500")
    m = master_of(c)
    try:
        whole, again, parts = (m.layout(k, pos=c["pos"], **BH) for k in (5, 5, 3))
        try:
            between = parts.tree()
            assert between["cells"] > 1 and between["accepted"].any()
            parts.run(2)
            a, b, p = whole.positions(), again.positions(), parts.positions()
            assert np.array_equal(a, b) and np.array_equal(a, p) and not np.array_equal(a, c["pos"]) and np.isfinite(a).all()
            assert np.array_equal(whole.forces(), again.forces()) and np.array_equal(whole.forces(), parts.forces())
            assert whole.state() == again.state() == parts.state() and whole.state()["iterations"] == 5
            same_tree(whole.tree(), tree_arrays(a, c["mass"]), "after five steps")
            exact = m.layout(5, pos=c["pos"])
            assert not np.array_equal(exact.positions(), a)  # (theta 1.2 is an approximation: another layout)
            exact.close()
        finally:
            for lay in (whole, again, parts):
                lay.close()
    finally:
        m.close()


def test_runs_repeat_bit_for_bit_at_65793_clustered(gpu_lib):
    """three scan passes, 258 blocks, a tree down to level DEPTH: three steps then two are five, bit for bit, and the
    device's tree after them is the statement's tree of the device's positions"""
    c = case("clustered65793")
    m = master_of(c)
    try:
        whole, parts = m.layout(5, pos=c["pos"], **BH), m.layout(3, pos=c["pos"], **BH)
        try:
            parts.positions()                                 # (a fetch between the two runs)
            parts.run(2)
            a, p = whole.positions(), parts.positions()
            assert np.array_equal(a, p) and not np.array_equal(a, c["pos"]) and np.isfinite(a).all()
            assert np.array_equal(whole.forces(), parts.forces()) and whole.state() == parts.state() and whole.state()["iterations"] == 5
            after = whole.tree()
            same_tree(after, tree_arrays(a, c["mass"]), "after five steps")
            check_tree(after, c["mass"], "after five steps")
        finally:
            whole.close()
            parts.close()
    finally:
        m.close()


def test_refusals_return_e_arg_and_say_why(gpu_lib):
    n, d = 20, 5
    rng = np.random.default_rng(2)
    o = contigs_orders(path_contigs(rng, n - 1, d), d, rng)
    make = lambda **kw: Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)
    m, directed = make(), make(directed=True)
    lib = ly._bind_layout(m.lib)
    pos = np.random.default_rng(1).random((n, 2))
    cfg = ly.config_of(ly.DEFAULTS)

    def create(master, theta, cfg=cfg):
        h = C.c_void_p()
        rc = lib.nemgpu_layout_create_bh(C.byref(h), master._h, C.byref(cfg), pos.ctypes.data, theta)
        assert (rc == 0) == bool(h.value)
        return rc, lib.nemgpu_last_error().decode(), h

    try:
        for theta in (float("nan"), -0.5, float("inf")):
            rc, why, _ = create(m, theta)
            assert rc == E_ARG and "theta" in why, (rc, why)
        rc, why, _ = create(directed, 1.2)
        assert rc == E_ARG and "directed" in why
        rc, why, _ = create(m, 1.2, ly.config_of(dict(ly.DEFAULTS, lin_log=True)))
        assert rc == E_ARG and "LinLog" in why
        rc, _, h = create(m, 1.2)
        assert rc == 0 and lib.nemgpu_layout_run(h, 1) == 0
        cells = C.c_int()
        assert lib.nemgpu_layout_bh_tree(h, C.byref(cells), *([None] * 11)) == 0 and 1 <= cells.value <= cell_bound(n)
        lib.nemgpu_layout_destroy(h)
        h = C.c_void_p()
        assert lib.nemgpu_layout_create(C.byref(h), m._h, C.byref(cfg), pos.ctypes.data) == 0
        assert lib.nemgpu_layout_bh_tree(h, C.byref(cells), *([None] * 11)) == E_ARG and "nemgpu_layout_create_bh" in lib.nemgpu_last_error().decode()
        lib.nemgpu_layout_destroy(h)
        exact = m.layout(0, pos=pos)
        with pytest.raises(NemGpuError, match="no tree"):
            exact.tree()
        exact.close()
        with pytest.raises(ValueError, match="repulsion"):
            m.layout(1, pos=pos, repulsion="octree")
        with pytest.raises(ValueError, match="theta"):
            m.layout(1, pos=pos, theta=-1.0, **BH)
        m.layout(1, pos=pos, theta=-1.0).close()            # (theta is read for barnes_hut alone)
        with pytest.raises(ValueError, match="directed"):
            directed.layout(1, pos=pos, **BH)
    finally:
        m.close()
        directed.close()


def test_a_fixture_end_to_end(gpu_lib, tmp_path):
    rec = load(LAYOUT_FIXTURES[0])
    base = base_record(rec)
    ann = annotations_of(base)
    m = Master.from_annotations(annotations_of(base, base["organisms"]), base["organisms"], base["circular"], base["repeated"])
    try:
        if base["new_organisms"]:
            grown = m.add_annotations(annotations_of(base, base["new_organisms"]), base["new_organisms"],
                                      set(base["circular"]) | set(base["update_circular"]), set(base["repeated"]) | set(base["update_repeated"]))
            m.close()
            m = grown
        repeated = set(base["repeated"]) | set(base["update_repeated"])
        ft, et = m.family_table(ann, repeated), m.edge_table(ann, repeated, sizes_of(base))
        try:
            lay = m.layout(20, rng=__import__("random").Random(3), **BH)
            laid = lay.positions()
            lay.close()
            assert np.isfinite(laid).all()
            write_gexf(str(tmp_path / "bh"), rec["labels"], ft, et, ann, positions=laid)
            text = open(str(tmp_path / "bh.gexf"), newline="", encoding="utf-8").read()
            assert text.count("<viz:position") == m.n
            for i in (0, m.n - 1):
                assert '<viz:position x="%s" y="%s"' % (str(float(laid[i, 0])), str(float(laid[i, 1]))) in text
            import xml.dom.minidom
            xml.dom.minidom.parseString(text.encode("utf-8"))
        finally:
            ft.close()
            et.close()
    finally:
        m.close()
