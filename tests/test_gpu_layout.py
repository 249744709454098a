"""The layout on the device (nemgpu_layout_*, csrc/nem_layout.hip; Master.layout) against the numpy statement
layout.layout_arrays, which tests/test_layout_host.py holds to closed forms.

One step: every term of the device is the statement's bit for bit (IEEE division and square root, no contraction), only
the order of the sums is its own, so a force component lies within 2 n 2^-53 B of the exactly rounded sum (order="fsum"),
B the statement's sum of the terms' absolute values; S, T, the speed and the positions within that bound propagated
(tests/layout_util.py: step_tolerances) -- eff and, where the step is half the speed, the speed itself are EQUAL.  Ten
steps: the growth of a rounding difference is chaotic, so the yardstick is measured, from the statement alone.  The
shapes are the smallest at which a kernel takes another path: one family to three, one below / at / one above the tile
and the first slice boundary, several slices, bit rows that cross a word, an isolated family, masters grown and bits-only,
a coincident pair -- and the tile loop of k_layout_repulse, which below 8 193 families never makes a second trip (a slice
of the j range is at most 64 there).  Those sizes are held to the row-blocked statement in extended precision
(layout_arrays: order="extended", block_rows=), whose own error n 2^-64 B is added to the force bound; the path each
reaches, and the wall time of its test on an MI355X host (the statement on one core is nearly all of it):
  n  8 192   32 slices of 256: one full tile per slice                                1.6 s
  n  8 193   32 slices of 257: a second trip of the tile loop, a tile of one j         1.4 s
  n 12 500   21 slices of 596: two full tiles and one of 84                            3.3 s
  n  8 193   the exact path against the theta 0 walk over all 8 193 bodies per lane    0.7 s
Above 65 536 families the exact path's only further path is the stride of k_layout_speed over more than 256 blocks; the
launches it sits in are shared with the Barnes-Hut path, and tests/test_gpu_layout_bh.py runs them at 65 793."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd import layout as ly
from pangenomenem_amd import synth
from pangenomenem_amd.chunks import Master
from pangenomenem_amd.gexf import write_gexf
from pangenomenem_amd.layout import SLICE_GRAIN, TILE, layout_arrays, layout_graph, slices_of
from tests.gexf_util import contigs_orders, host_tables, path_contigs, same_gexf_text, sizes_of
from tests.layout_util import (LAYOUT_FIXTURES, U, arrays_of, base_record, branches, check_margins, positions_in_master_order,
                               ring_with_chords, statement_step, step_tolerances)
from tests.orders_util import load, same_master
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

E_ARG, E_FUNCARG = 3, 8


def counts_master(n, d, seed, **kw):
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(n, d, seed, loops=0.05, multi_frac=0.1, **kw)
    return Master(x, ptr, idx, eb, edge_counts=counts)


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def held_to_the_statement(m, pos, what, steps=2, order="fsum", block_rows=None, **params):
    """`steps` single iterations on the device from pos, each against one iteration of the statement (fsum order; for a
    large n order="extended" in blocks of block_rows rows, its own error added to the force bound) from the device's own
    state before it: the first from old = 0, the next from the old the first left"""
    _, graph, eb, _, _ = m.arrays()
    n = m.n
    mass = layout_graph(graph, eb, m.d)["mass"]
    pos = np.ascontiguousarray(pos, np.float64)
    lay = m.layout(0, pos=pos, **params)
    try:
        assert np.array_equal(lay.positions(), pos), what + ": iterations=0 returns the start"
        assert lay.state() == dict(speed=1.0, eff=1.0, S=0.0, T=0.0, iterations=0)
        old, speed, eff = np.zeros((n, 2)), 1.0, 1.0
        for step in range(steps):
            want = statement_step(graph, eb, m.d, pos, old, speed, eff, order=order, block_rows=block_rows, **params)
            if want["moved"]:
                check_margins(want["comparisons"][0], not old.any(), "%s step %d" % (what, step))
            tol = step_tolerances(n, mass, want, old, speed, order=order)
            lay.run(1)
            got_pos, got_f, st = lay.positions(), lay.forces(), lay.state()
            worst = float(np.max(np.abs(got_f - want["forces"]) / np.maximum(tol["forces"], 1e-300))) if n else 0.0
            print("%s step %d: n %d, forces at %.3f of the bound, S off by %.3g (bound %.3g), T by %.3g (%.3g), speed %r / %r, eff %r"
                  % (what, step, n, worst, abs(st["S"] - want["S"]), tol["S"], abs(st["T"] - want["T"]), tol["T"], st["speed"], want["speed"], st["eff"]))
            assert (np.abs(got_f - want["forces"]) <= tol["forces"]).all(), "%s step %d: a force is off its bound" % (what, step)
            assert abs(st["S"] - want["S"]) <= tol["S"] and abs(st["T"] - want["T"]) <= tol["T"], (what, step, st, want["S"], want["T"])
            if not old.any():
                assert st["S"] == 2.0 * st["T"]               # (from old = 0, in any order: layout_util.check_margins)
            assert st["eff"] == want["eff"], (what, step)
            assert abs(st["speed"] - want["speed"]) <= tol["speed"], (what, step, st["speed"], want["speed"], tol["speed"])
            assert (np.abs(got_pos - want["pos"]) <= tol["pos"]).all(), "%s step %d: a position is off its bound" % (what, step)
            assert st["iterations"] == step + 1 and (st["T"] != 0.0) == want["moved"]
            if want["moved"]:
                old = got_f
            pos, speed, eff = got_pos, st["speed"], st["eff"]
    finally:
        lay.close()


def start(n, seed, coincident=False):
    pos = np.random.default_rng(seed).random((n, 2))
    if coincident and n > 2:
        pos[n // 2] = pos[0]
    return pos


def test_no_master_has_no_family_and_the_statement_gives_an_empty_layout(gpu_lib):
    """n = 0: a master of no family cannot be made (nemgpu_master_create refuses n <= 0), so the device's empty layout is
    not reachable; the statement's is empty"""
    with pytest.raises(Exception):
        Master(np.zeros((0, 3), np.uint8), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 1), np.uint32))
    empty = layout_arrays((np.zeros(1, np.int32), np.zeros(0, np.int32)), np.zeros((0, 1), np.uint32), 3, iterations=3)
    assert empty["pos"].shape == (0, 2) and empty["iterations"] == 3


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_family_to_three(gpu_lib, n):
    d = 3
    edges = [(a, a + 1, [a % d, 2]) for a in range(n - 1)] + ([(0, 0, [1])] if n == 3 else [])
    x, (ptr, idx), eb = arrays_of(n, edges, d)
    m = Master(x, ptr, idx, eb)
    try:
        held_to_the_statement(m, start(n, 40 + n) - 0.5, "n %d" % n)
        if n == 1:
            held_to_the_statement(m, [[0.0, 0.0]], "one family at the origin")      # T == 0: nothing moves
    finally:
        m.close()


SHAPES = [(n, d) for n in (TILE - 1, TILE, TILE + 1, SLICE_GRAIN - 1, SLICE_GRAIN, SLICE_GRAIN + 1) for d in (3, 70, 200)] + [(1500, 70)]


@pytest.mark.parametrize("n, d", SHAPES)
def test_around_the_tile_and_the_first_slice_boundary(gpu_lib, n, d):
    """one below, at and one above the repulsion kernel's tile width (TILE) and the n above which a node's j range is cut
    into more than one slice (SLICE_GRAIN), and one n that spans many slices; masters with self-loops and counts above 1,
    bit rows inside one word, across two, across seven; a coincident pair in the start"""
    assert (slices_of(SLICE_GRAIN), slices_of(SLICE_GRAIN + 1)) == (1, 2) and slices_of(1500) > 8 and slices_of(TILE + 1) > 1
    m = counts_master(n, d, 1000 * d + n)
    try:
        _, (ptr, idx), eb, counts, _ = m.arrays()
        g = layout_graph((ptr, idx), eb, d)
        assert (g["col"] == g["row"]).any() and len(counts[1]) > 0 and (d < 33 or (eb[:, 1:] != 0).any())
        held_to_the_statement(m, start(n, n + d, coincident=True), "n %d d %d" % (n, d))
    finally:
        m.close()


TILED = {8192: (32, 256, 1), 8193: (32, 257, 2), 12500: (21, 596, 3)}         # n: slices, slice_len, tiles per slice
TILED_D = 9


def tiled_master(n):
    return counts_master(n, TILED_D, 9000 + n)


def tiled_start(n):
    return start(n, n + TILED_D, coincident=True)


@pytest.mark.parametrize("n", sorted(TILED))
def test_the_tile_loop_of_a_slice(gpu_lib, n):
    """k_layout_repulse's loop over the LDS tiles of one slice: at 8192 a slice is one full tile of 256 j's, at 8193 the
    loop makes its second trip (a tile of one j, behind the barrier that guards the reload), at 12500 two full tiles and
    one of 84.  Two steps from a start with a coincident pair, a master with self-loops and counts above 1, against the
    row-blocked statement in extended precision: the force bound is 2 n u B + n 2^-64 B, about 1e-8 of one pair term
    (tests/test_layout_host.py shows that it rejects a dropped tile and a wrong term)."""
    slices, length, tiles = TILED[n]
    assert (slices_of(n), -(-n // slices_of(n)), -(-length // TILE)) == (slices, length, tiles)
    m = tiled_master(n)
    try:
        _, (ptr, idx), eb, counts, _ = m.arrays()
        g = layout_graph((ptr, idx), eb, TILED_D)
        assert (g["col"] == g["row"]).any() and len(counts[1]) > 0
        held_to_the_statement(m, tiled_start(n), "n %d" % n, order="extended", block_rows=256)
    finally:
        m.close()


def test_the_two_device_orders_past_one_tile(gpu_lib):
    """n = 8193: the exact path (32 slices of 257, two tiles each) against the Barnes-Hut walk at theta 0, which opens every
    cell and so sums the same 8192 pair terms per family in the tree's order: each within n u B of the exact sum, so
    within 2 n u B of each other (tests/test_gpu_layout_bh.py does this below one tile)"""
    n = 8193
    m = tiled_master(n)
    try:
        _, graph, eb, _, _ = m.arrays()
        pos = tiled_start(n)
        a, b = m.layout(1, pos=pos, theta=0.0, repulsion="barnes_hut"), m.layout(1, pos=pos)
        try:
            fa, fb = a.forces(), b.forces()
            walked = a.tree()["visited"]
        finally:
            a.close()
            b.close()
    finally:
        m.close()
    B = layout_arrays(graph, eb, TILED_D, iterations=1, pos=pos, order="left", block_rows=256)["bound"]
    worst = float((np.abs(fa - fb) / (2.0 * n * U * B)).max())
    print("n %d: theta 0 against the exact path at %.3f of the bound" % (n, worst))
    assert (np.abs(fa - fb) <= 2.0 * n * U * B).all()
    assert np.isfinite(fa).all() and fa.any() and not np.array_equal(fa, fb)       # (two orders of 8192 terms)


def test_an_isolated_family_a_grown_master_and_a_bits_only_one(gpu_lib):
    rng = np.random.default_rng(13)
    ne, d, d0 = 90, 40, 25
    o = contigs_orders(path_contigs(rng, ne, d) + [(d - 1, [ne + 1], -1), (d - 1, [ne + 2, ne + 2], -1)], d, rng)    # (ne + 1: no link at all)
    c0 = int(np.searchsorted(o["contig_org"], d0))
    g0 = int(o["contig_ptr"][c0])
    base = dict(o, genes=o["genes"][:g0], contig_ptr=o["contig_ptr"][:c0 + 1], contig_org=o["contig_org"][:c0], contig_circular=o["contig_circular"][:c0], d=d0)
    whole = from_orders(o)
    m0 = from_orders(base)
    grown = m0.add_orders(o["genes"][g0:], o["contig_ptr"][c0:] - g0, o["contig_org"][c0:], o["contig_circular"][c0:], d - d0, repeated=o["repeated"])
    m0.close()
    x, graph, eb, _, _ = whole.arrays()
    present = np.unpackbits(x.view(np.uint8).reshape(whole.n, -1), axis=1, bitorder="little")[:, :d]
    bits = Master(present, graph[0], graph[1], eb)
    try:
        assert (np.diff(graph[0]) == 0).sum() == 1 and whole.n == ne + 3
        pos = start(whole.n, 21)
        for m, what in ((whole, "from orders"), (grown, "grown"), (bits, "bits only")):
            before = m.arrays()
            held_to_the_statement(m, pos, what)
            same_master(m.arrays(), before, what)
        a, b = whole.layout(3, pos=pos), grown.layout(3, pos=pos)
        try:
            same_master(whole.arrays(), grown.arrays(), "grown")
            assert np.array_equal(a.positions(), b.positions())       # (the same master: the same layout, bit for bit)
        finally:
            a.close()
            b.close()
    finally:
        for m in (whole, grown, bits):
            m.close()


@pytest.mark.parametrize("params", [dict(edge_weight_influence=0.0), dict(outbound_attraction_distribution=False), dict(edge_weight_influence=0.5),
                                    dict(scaling_ratio=2.0, gravity=30.0, jitter_tolerance=0.1)], ids=lambda p: "-".join(p))
def test_the_other_parameters(gpu_lib, params):
    n, d = 130, 70
    m = counts_master(n, d, 77)
    try:
        held_to_the_statement(m, start(n, 5) * 40.0 - 20.0, str(params), steps=3, **params)
    finally:
        m.close()


def test_ten_steps_within_a_measured_tolerance(gpu_lib):
    """A rounding difference grows chaotically over the iterations, so no bound is derived: the statement is run three
    times on the CPU -- fsum, left to right, a seeded permutation of j -- and s is the largest deviation of the latter two
    from the first after 10 iterations, relative to the layout's extent.  The device, yet another order, must lie
    within 8 s of the fsum run: the 8 is room for one more order, not a precision claim.  The three runs must have
    decided every comparison of the speed control alike, none of them closely."""
    n, d, its = 300, 9, 10
    x, (ptr, idx), eb = ring_with_chords(n, d, 20241)
    pos = np.random.default_rng(20242).random((n, 2))
    perm = np.random.default_rng(20243).permutation(n)
    runs = {order: layout_arrays((ptr, idx), eb, d, iterations=its, pos=pos, order=order, perm=perm) for order in ("fsum", "left", "perm")}
    assert branches(runs["fsum"]) == branches(runs["left"]) == branches(runs["perm"])
    for k, made in enumerate(runs["fsum"]["comparisons"]):
        check_margins(made, k == 0, "ring iteration %d" % k)
    ref = runs["fsum"]["pos"]
    extent = float((ref.max(axis=0) - ref.min(axis=0)).max())
    s = max(float(np.abs(runs[order]["pos"] - ref).max()) for order in ("left", "perm")) / extent
    assert 0.0 < s < 1e-9
    m = Master(x, ptr, idx, eb)
    try:
        lay = m.layout(its, pos=pos)
        got, st = lay.positions(), lay.state()
        lay.close()
    finally:
        m.close()
    dev = float(np.abs(got - ref).max()) / extent
    print("ten steps on a ring of %d with chords: s = %.3g, the device is %.3g from the fsum run (%.2f s)" % (n, s, dev, dev / s))
    assert dev <= 8.0 * s
    assert st["eff"] == runs["fsum"]["eff"] and st["iterations"] == its


def test_runs_repeat_bit_for_bit_and_hand_over(gpu_lib):
    n, d = 700, 40
    m = counts_master(n, d, 9)
    try:
        before = m.arrays()
        pos = start(n, 3, coincident=True)
        whole, again, parts = m.layout(5, pos=pos), m.layout(5, pos=pos), m.layout(3, pos=pos)
        try:
            parts.positions()                                 # (a fetch between the two runs)
            parts.run(2)
            a, b, c = whole.positions(), again.positions(), parts.positions()
            assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, pos)
            assert np.array_equal(whole.forces(), again.forces()) and np.array_equal(whole.forces(), parts.forces())
            assert whole.state() == again.state() == parts.state() and whole.state()["iterations"] == 5
            assert np.isfinite(a).all()
            none = m.layout(0, pos=pos)
            assert np.array_equal(none.positions(), pos) and none.state()["iterations"] == 0
            none.close()
        finally:
            for lay in (whole, again, parts):
                lay.close()
        same_master(m.arrays(), before, "after the layouts")
        # drawn from a generator: x before y in master order
        import random
        drawn = m.layout(0, rng=random.Random(8))
        twin = random.Random(8)
        assert drawn.positions().ravel().tolist() == [twin.random() for _ in range(2 * n)]
        drawn.close()
    finally:
        m.close()


@pytest.mark.parametrize("path", LAYOUT_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixtures_end_to_end(gpu_lib, path, tmp_path):
    rec = load(path)
    base = base_record(rec)
    ann = annotations_of(base)
    everyone = base["organisms"] + base["new_organisms"]
    m = Master.from_annotations(annotations_of(base, base["organisms"]), base["organisms"], base["circular"], base["repeated"])
    try:
        if base["new_organisms"]:
            grown = m.add_annotations(annotations_of(base, base["new_organisms"]), base["new_organisms"],
                                      set(base["circular"]) | set(base["update_circular"]), set(base["repeated"]) | set(base["update_repeated"]))
            m.close()
            m = grown
        repeated = set(base["repeated"]) | set(base["update_repeated"])
        ft, et = m.family_table(ann, repeated), m.edge_table(ann, repeated, sizes_of(base))
        hft, het, _ = host_tables(base)
        try:
            read = lambda name: open(str(tmp_path / (name + ".gexf")), newline="", encoding="utf-8").read()
            # the recorded positions through the device tables: the reference's bytes
            pos = positions_in_master_order(rec, m.names)
            write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, positions=pos)
            write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, positions=pos)
            same_gexf_text(read("full"), rec["gexf"], everyone, rec["name"] + " full")
            same_gexf_text(read("light"), rec["gexf_light"], everyone, rec["name"] + " light")
            # a layout of the device through the device tables: the host writer's file
            lay = m.layout(20, rng=__import__("random").Random(3))
            laid = lay.positions()
            lay.close()
            assert np.isfinite(laid).all() and hft.names == m.names
            for name, kw in (("dev", {}), ("dev_light", dict(all_node_attributes=False, all_edge_attributes=False))):
                write_gexf(str(tmp_path / name), rec["labels"], ft, et, ann, positions=laid, **kw)
                write_gexf(str(tmp_path / (name + "_host")), rec["labels"], hft, het, ann, positions=laid, **kw)
                same_gexf_text(read(name), read(name + "_host"), everyone, rec["name"] + " " + name)
                assert read(name).count("<viz:position") == m.n and 'x="%s"' % str(float(laid[0, 0])) in read(name)
        finally:
            ft.close()
            et.close()
    finally:
        m.close()


def test_refusals_return_e_arg_and_say_why(gpu_lib):
    n, d = 20, 5
    rng = np.random.default_rng(2)
    o = contigs_orders(path_contigs(rng, n - 1, d), d, rng)
    m, directed = from_orders(o), from_orders(o, directed=True)
    lib = ly._bind_layout(m.lib)
    pos = start(n, 1)

    def create(master, pos, **params):
        cfg = ly.config_of(dict(ly.DEFAULTS, **params))
        h = C.c_void_p()
        rc = lib.nemgpu_layout_create(C.byref(h), master._h, C.byref(cfg), pos.ctypes.data if pos is not None else None)
        assert (rc == 0) == bool(h.value)
        return rc, lib.nemgpu_last_error().decode(), h

    try:
        before = m.arrays()
        rc, _, h = create(m, pos)
        assert rc == 0
        assert lib.nemgpu_layout_run(h, -1) == E_ARG and "iterations" in lib.nemgpu_last_error().decode()
        assert lib.nemgpu_layout_run(h, 0) == 0
        lib.nemgpu_layout_destroy(h)
        for params, word in ((dict(lin_log=True), "LinLog"), (dict(adjust_sizes=True), "adjust_sizes"), (dict(strong_gravity=False), "strong gravity"),
                             (dict(gravity=float("nan")), "not finite")):
            rc, why, _ = create(m, pos, **params)
            assert rc == E_ARG and word in why, (rc, why)
        for spoiled in (np.nan, np.inf, -np.inf):
            bad = pos.copy()
            bad[n - 1, 1] = spoiled
            rc, why, _ = create(m, bad)
            assert rc == E_ARG and "start position" in why
        rc, why, _ = create(directed, pos)
        assert rc == E_ARG and "directed" in why
        assert create(m, None)[0] == E_FUNCARG
        with pytest.raises(ValueError, match="directed"):
            directed.layout(1, pos=pos)
        with pytest.raises(ValueError, match="LinLog"):
            m.layout(1, pos=pos, lin_log=True)
        with pytest.raises(ValueError, match="not finite"):
            m.layout(1, pos=np.full((n, 2), np.nan))
        lay = m.layout(0, pos=pos)
        with pytest.raises(ValueError, match="iterations"):
            lay.run(-1)
        lay.close()
        same_master(m.arrays(), before, "after the refusals")
    finally:
        m.close()
        directed.close()
