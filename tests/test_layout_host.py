"""The layout's numpy statement (pangenomenem_amd/layout.py: layout_arrays, positions_3d, start_positions) and the GEXF
writer's positions= against what the reference determines -- the <viz:position> that networkx writes for the dict that
compute_layout's own loop makes (tests/golden/layout/, byte for byte except <meta> and the set-joined fields) -- and
against itself: closed forms worked by hand, the properties the device relies on, and what is refused."""
import math
import random

import numpy as np
import pytest

from pangenomenem_amd import layout as ly
from pangenomenem_amd import synth
from pangenomenem_amd.engine import load_library
from pangenomenem_amd.gexf import write_gexf
from tests.gexf_util import host_tables, same_gexf_text
from tests.layout_util import LAYOUT_FIXTURES, U, arrays_of, base_record, positions_in_master_order, ring_with_chords, step_tolerances
from tests.orders_util import load


def read(path):
    return open(str(path), newline="", encoding="utf-8").read()


@pytest.mark.parametrize("path", LAYOUT_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixture_exports_with_positions(path, tmp_path):
    rec = load(path)
    base = base_record(rec)
    everyone = base["organisms"] + base["new_organisms"]
    ft, et, ann = host_tables(base)
    pos = positions_in_master_order(rec, ft.names)
    write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, positions=pos)
    write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, positions=pos)
    same_gexf_text(read(tmp_path / "full.gexf"), rec["gexf"], everyone, rec["name"] + " full")
    same_gexf_text(read(tmp_path / "light.gexf"), rec["gexf_light"], everyone, rec["name"] + " light")
    # without positions the file is what it was
    write_gexf(str(tmp_path / "plain"), rec["labels"], ft, et, ann, positions=None)
    write_gexf(str(tmp_path / "plain_light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False)
    same_gexf_text(read(tmp_path / "plain.gexf"), base["gexf"], everyone, rec["name"] + " plain")
    same_gexf_text(read(tmp_path / "plain_light.gexf"), base["gexf_light"], everyone, rec["name"] + " plain light")
    assert "viz:position" not in read(tmp_path / "plain.gexf")
    with pytest.raises(ValueError, match="positions"):
        write_gexf(str(tmp_path / "bad"), rec["labels"], ft, et, ann, positions=pos[:-1])


def test_fixtures_cover_the_cases():
    recs = {r["name"]: r for r in map(load, LAYOUT_FIXTURES)}
    assert set(recs) == {"links", "duplicates", "repeated_late"}
    text = "".join(r["gexf"] for r in recs.values())
    for value in ('x="-1234.5"', 'y="3.0"', 'x="1e-05"', 'x="0.10000000000000002"', 'y="-0.0"'):
        assert value in text, value
    for z in ('z="0"', 'z="1"', 'z="2"'):
        assert z in text
    for r in recs.values():
        assert r["gexf"].count("<viz:position") == r["gexf_light"].count("<viz:position") == len(r["families"])


def one(graph, eb, d, pos, **kw):
    return ly.layout_arrays(graph, eb, d, iterations=kw.pop("iterations", 1), pos=pos, **kw)


def test_one_family_at_the_origin_does_not_move():
    _, graph, eb = arrays_of(1, [], 3)
    r = one(graph, eb, 3, [[0.0, 0.0]], iterations=4)
    assert r["T"] == 0.0 and r["S"] == 0.0 and not r["moved"] and r["comparisons"] == [[]] * 4
    assert (r["pos"] == 0.0).all() and (r["speed"], r["eff"]) == (1.0, 1.0) and r["iterations"] == 4


def test_one_family_off_the_origin_feels_gravity_alone():
    _, graph, eb = arrays_of(1, [], 3)
    r = one(graph, eb, 3, [[0.75, -1.0]])
    # mass 1: f = -1 * 1 * p; old = 0: sw = tr = |f| = 1.25, S = 1.25, T = 0.625
    assert r["forces"].tolist() == [[-0.75, 1.0]] and r["bound"].tolist() == [[0.75, 1.0]]
    assert (r["S"], r["T"]) == (1.25, 0.625)
    est = 0.05                                                # 0.05 sqrt(1)
    jt = max(math.sqrt(est), min(10.0, est * 0.625 / 1.0))    # sqrt(est): the traction is small
    assert jt == math.sqrt(0.05)
    target = jt * 1.0 * 0.625 / 1.25                          # S / T == 2: not above it
    speed = 1.0 + min(target - 1.0, 0.5)                      # about 0.1118: the step is target - speed
    assert r["eff"] == 0.7 and r["speed"] == speed and abs(speed - jt / 2) < 1e-15      # S > jt T: eff * 0.7
    den = 1.0 + math.sqrt(speed * 1.0 * 1.25)
    assert r["pos"].tolist() == [[0.75 + -0.75 * speed / den, -1.0 + 1.0 * speed / den]]
    assert r["old"].tolist() == r["forces"].tolist() and [c[0] for c in r["comparisons"][0]] == ["ratio", "swing", "step"]


@pytest.mark.parametrize("order", ly.ORDERS)
def test_two_families_joined_by_an_edge_of_weight_three(order):
    _, graph, eb = arrays_of(2, [(0, 1, [0, 2, 4])], 5)
    g = ly.layout_graph(graph, eb, 5)
    assert g["mass"].tolist() == [2.0, 2.0] and g["edge_weight"].tolist() == [3] and (g["src"].tolist(), g["dst"].tolist()) == ([0], [1])
    r = one(graph, eb, 5, [[-0.5, 0.0], [0.5, 0.0]], order=order, perm=[1, 0])
    # on family 0: repulsion (-1) * 50000 * 2 * 2 / 1 = -200000; gravity -(1 * 2 * -0.5) = +1; attraction: comp = mean(mass)
    # = 2, fac = -2 * 3 / mass[src] = -3, (p0 - p1) * fac = +3
    assert r["forces"].tolist() == [[-199996.0, 0.0], [199996.0, 0.0]]
    assert r["bound"].tolist() == [[200004.0, 0.0], [200004.0, 0.0]]
    assert (r["S"], r["T"]) == (2 * 2 * 199996.0, 2 * 199996.0)
    # est = 0.05 sqrt(2); est T / 4 is far above 10: jt = 10; S / T == 2; target = 10 T / S = 5; S > 10 T is false and the
    # speed is below 1000: eff * 1.3; the step is half the speed
    assert (r["speed"], r["eff"]) == (1.5, 1.3)
    assert [(name, left > right) for name, left, right in r["comparisons"][0]] == [("ratio", False), ("swing", False), ("fast", False), ("step", True)]
    move = 199996.0 * 1.5 / (1.0 + math.sqrt(1.5 * 2.0 * 199996.0))
    assert r["pos"].tolist() == [[-0.5 - move, 0.0], [0.5 + move, 0.0]]


def test_two_coincident_families_give_finite_forces():
    _, graph, eb = arrays_of(3, [(0, 1, [0]), (1, 2, [1])], 2)
    for order in ly.ORDERS:
        r = one(graph, eb, 2, [[0.25, 0.5], [0.25, 0.5], [0.75, 0.5]], order=order, perm=[2, 0, 1], iterations=3)
        assert np.isfinite(r["pos"]).all() and np.isfinite(r["forces"]).all() and np.isfinite(r["bound"]).all()
    r = one(graph, eb, 2, [[0.25, 0.5], [0.25, 0.5], [0.75, 0.5]], order="fsum")
    # the coincident pair repels and attracts nothing: families 0 and 1 differ by their edges to family 2 alone
    lone = one(graph, eb, 2, [[0.25, 0.5], [5.0, 5.0], [0.75, 0.5]], order="fsum")
    assert r["forces"][0, 1] == -(1.0 * 2.0) * 0.5 and lone["forces"][0, 1] != r["forces"][0, 1]


def test_a_self_loop_adds_mass_and_no_attraction():
    d = 4
    _, graph, eb = arrays_of(3, [(0, 1, [0, 1]), (1, 2, [2]), (1, 1, [0, 1, 2, 3])], d)
    g = ly.layout_graph(graph, eb, d)
    assert g["mass"].tolist() == [2.0, 4.0, 2.0] and g["src"].tolist() == [0, 1] and g["edge_weight"].tolist() == [2, 1]
    pos = [[0.1, 0.2], [0.7, 0.3], [0.4, 0.9]]
    r = one(graph, eb, d, pos, order="fsum")
    # by hand on family 1, x: the two pairs, gravity, the two edges (comp = 8 / 3; fac = -comp * w / mass[src])
    comp, (x0, y0), (x1, y1), (x2, y2) = 8.0 / 3.0, *pos
    d01, d12 = (x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0), (x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2)
    terms = [(x1 - x0) * (50000.0 * 4.0 * 2.0 / d01), (x1 - x2) * (50000.0 * 4.0 * 2.0 / d12), -(1.0 * 4.0) * x1, (x1 - x0) * (-comp * 2.0 / 2.0), (x1 - x2) * (-comp * 1.0 / 4.0)]
    assert r["forces"][1, 0] == math.fsum(terms) and abs(r["bound"][1, 0] - sum(abs(t) for t in terms)) < 1e-9


def test_the_gather_over_the_rows_is_the_scatter_over_the_edges():
    d = 70
    _, graph, eb = ring_with_chords(40, d, 3)
    pos = np.random.default_rng(4).random((40, 2))
    for influence in (1.0, 0.0, 0.5):
        for distributed in (True, False):
            kw = dict(edge_weight_influence=influence, outbound_attraction_distribution=distributed, order="fsum", iterations=2)
            a, b = one(graph, eb, d, pos, attraction="gather", **kw), one(graph, eb, d, pos, attraction="scatter", **kw)
            assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["forces"], b["forces"]) and (a["S"], a["T"]) == (b["S"], b["T"])
    near = one(graph, eb, d, pos, attraction="scatter", order="left")
    assert np.allclose(near["forces"], one(graph, eb, d, pos, order="fsum")["forces"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("order", ["numpy", "left", "fsum"])
def test_mirrored_start_positions_give_the_mirrored_layout(order):
    _, graph, eb = ring_with_chords(30, 9, 5)
    pos = np.random.default_rng(6).random((30, 2)) - 0.5
    a = one(graph, eb, 9, pos, order=order, iterations=5)
    b = one(graph, eb, 9, pos * [-1.0, 1.0], order=order, iterations=5)
    assert np.array_equal(b["pos"], a["pos"] * [-1.0, 1.0]) and (a["speed"], a["eff"], a["S"], a["T"]) == (b["speed"], b["eff"], b["S"], b["T"])


def test_the_generator_is_drawn_x_before_y_and_left_there():
    _, graph, eb = ring_with_chords(7, 3, 1)
    rng, twin = random.Random(5), random.Random(5)
    r = ly.layout_arrays(graph, eb, 3, iterations=0, rng=rng)
    drawn = [twin.random() for _ in range(14)]
    assert r["pos"].ravel().tolist() == drawn and rng.random() == twin.random()
    random.seed(11)
    module = ly.start_positions(3)
    twin = random.Random(11)
    assert module.ravel().tolist() == [twin.random() for _ in range(6)]
    with pytest.raises(ValueError, match="not both"):
        ly.start_positions(2, pos=[[0, 0], [1, 1]], rng=rng)


def test_z_follows_the_partition():
    names = ["a", "b", "c", "d"]
    pos = np.arange(8.0).reshape(4, 2)
    assert ly.positions_3d({"a": "P", "b": "S", "c": "C", "d": "U"}, names, pos)[1].tolist() == [2, 1, 0, 0]
    assert ly.positions_3d(np.asarray([1, 0, 3, 2], np.uint8), None, pos)[1].tolist() == [1, 2, 0, 0]
    assert ly.positions_3d(None, names, pos)[1].tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        ly.positions_3d(np.zeros(3, np.uint8), None, pos)


def test_what_is_refused():
    _, graph, eb = ring_with_chords(5, 3, 2)
    pos = np.random.default_rng(1).random((5, 2))
    for bad in (dict(lin_log=True), dict(adjust_sizes=True), dict(strong_gravity=False), dict(gravity=math.inf), dict(scaling_ratio=math.nan)):
        with pytest.raises(ValueError):
            one(graph, eb, 3, pos, **bad)
    with pytest.raises(TypeError):
        one(graph, eb, 3, pos, barnes_hut_theta=1.2)
    for spoiled in (math.nan, math.inf):
        start = pos.copy()
        start[3, 1] = spoiled
        with pytest.raises(ValueError, match="not finite"):
            one(graph, eb, 3, start)
    with pytest.raises(ValueError, match="iterations"):
        one(graph, eb, 3, pos, iterations=-1)
    with pytest.raises(ValueError):
        one(graph, eb, 3, pos[:4])
    with pytest.raises(ValueError, match="permutation"):
        one(graph, eb, 3, pos, order="perm", perm=[0, 1, 2, 3, 3])
    for rows in (0, -1, 2.5):
        with pytest.raises(ValueError, match="block_rows"):
            one(graph, eb, 3, pos, block_rows=rows)
    assert one(graph, eb, 3, pos, iterations=0)["pos"].tolist() == pos.tolist()
    empty = ly.layout_arrays((np.zeros(1, np.int32), np.zeros(0, np.int32)), np.zeros((0, 1), np.uint32), 3, iterations=2)
    assert empty["pos"].shape == (0, 2) and empty["iterations"] == 2


def test_the_slices_are_the_librarys():
    import ctypes as C
    lib = ly._bind_layout(load_library())
    tile, grain = C.c_int(), C.c_int()
    for n in (0, 1, 63, 64, 65, 128, 129, 255, 256, 257, 1500, 2000, 4096, 4097, 20000, 200000, 2 ** 31 - 1):
        assert lib.nemgpu_layout_slices(n, C.byref(tile), C.byref(grain)) == ly.slices_of(n), n
    assert (tile.value, grain.value) == (ly.TILE, ly.SLICE_GRAIN)
    assert ly.slices_of(ly.SLICE_GRAIN) == 1 and ly.slices_of(ly.SLICE_GRAIN + 1) == 2 and ly.slices_of(1500) > 8


SAME_KEYS = ("pos", "forces", "bound", "old")


@pytest.mark.parametrize("n", [300, 700])
def test_the_row_blocked_form_is_the_unblocked_one_bit_for_bit(n):
    """block_rows= changes what is held at a time, not one bit: a block size of one row, one that does not divide n, one
    that does, n itself and one above n; two iterations from a start with a coincident pair, a master with self-loops.
    The exactly rounded order is blocked too (one iteration: it is the slow one)."""
    d = 9
    _, graph, eb, _ = synth.master_pangenome_counts(n, d, n, loops=0.05, multi_frac=0.1)
    pos = np.random.default_rng(n).random((n, 2))
    pos[n // 2] = pos[0]
    perm = np.random.default_rng(1).permutation(n)
    assert n % 11 and n % 100 == 0
    for order, iterations, blocks in (("left", 2, (1, 11, 100, n, n + 5)), ("numpy", 2, (1, 11, 100, n, n + 5)), ("perm", 2, (1, 11, 100, n, n + 5)),
                                      ("extended", 2, (11, 100, n + 5)), ("fsum", 1, (11, n + 5))):
        whole = one(graph, eb, d, pos, order=order, perm=perm, iterations=iterations)
        for rows in blocks:
            cut = one(graph, eb, d, pos, order=order, perm=perm, iterations=iterations, block_rows=rows)
            for k in SAME_KEYS:
                assert np.array_equal(whole[k], cut[k]), (order, rows, k)
            assert [whole[k] for k in ("S", "T", "speed", "eff", "moved", "comparisons")] == [cut[k] for k in ("S", "T", "speed", "eff", "moved", "comparisons")]
            assert (cut["wide"] is None) == (order != "extended" or ly.extended_type() is None)


@pytest.mark.parametrize("n", [300, 700])
def test_the_extended_order_is_within_its_bound_of_the_exactly_rounded_one(n):
    """The float64 terms accumulated in 64 significant bits are within n 2^-64 B of the exact sum s (at most 2 n - 1 terms,
    summed pairwise: the bound has room).  The fsum order gives fl(s), itself within u |s| of s, so the unrounded
    extended sum ("wide") is held to n 2^-64 B + u |fl(s)| of it, and the rounded one is fl(s) or a neighbour of it.
    Where np.longdouble is no wider than float64 the order IS fsum per row."""
    d = 9
    _, graph, eb, _ = synth.master_pangenome_counts(n, d, n, loops=0.05, multi_frac=0.1)
    pos = np.random.default_rng(n).random((n, 2))
    pos[n // 2] = pos[0]
    exact = one(graph, eb, d, pos, order="fsum")
    wide = one(graph, eb, d, pos, order="extended", block_rows=64)
    if ly.extended_type() is None:
        assert np.array_equal(wide["forces"], exact["forces"]) and wide["wide"] is None
        return
    assert np.finfo(np.longdouble).nmant >= 63 and wide["wide"].dtype == np.longdouble
    B = exact["bound"]
    assert np.array_equal(wide["bound"], B)
    off = np.abs(wide["wide"] - exact["forces"].astype(np.longdouble))
    room = (n * 2.0 ** -64) * B + U * np.abs(exact["forces"])
    print("n %d: the extended sums are at most %.3g of n 2^-64 B + u |f| off the exactly rounded ones; %d of %d rounded ones differ"
          % (n, float((off / room).max()), int((wide["forces"] != exact["forces"]).sum()), 2 * n))
    assert (off <= room).all()
    assert np.array_equal(wide["forces"], wide["wide"].astype(np.float64))
    assert (np.abs(wide["forces"] - exact["forces"]) <= np.spacing(np.abs(exact["forces"]))).all()
    assert (wide["S"], wide["T"]) != (0.0, 0.0) and abs(wide["S"] - exact["S"]) <= step_tolerances(n, ly.layout_graph(graph, eb, d)["mass"], exact, np.zeros((n, 2)), 1.0)["S"]


def test_without_a_wide_longdouble_the_extended_order_is_fsum_per_row(monkeypatch):
    """where np.longdouble has fewer than 64 significant bits (extended_type() is None) order="extended" sums every row
    with math.fsum: the exactly rounded order, bit for bit"""
    n, d = 90, 9
    _, graph, eb = ring_with_chords(n, d, 3)
    pos = np.random.default_rng(2).random((n, 2))
    assert ly.extended_type() in (None, np.longdouble) and (ly.extended_type() is None) == (np.finfo(np.longdouble).nmant < 63)
    monkeypatch.setattr(ly, "extended_type", lambda: None)
    exact = one(graph, eb, d, pos, order="fsum", iterations=2)
    narrow = one(graph, eb, d, pos, order="extended", iterations=2, block_rows=32)
    assert narrow["wide"] is None
    for k in SAME_KEYS:
        assert np.array_equal(exact[k], narrow[k]), k
    assert (exact["S"], exact["T"], exact["speed"], exact["eff"]) == (narrow["S"], narrow["T"], narrow["speed"], narrow["eff"])


def slice_len(n):
    return -(-n // ly.slices_of(n))


def test_the_slice_arithmetic_the_large_shapes_rest_on():
    """k_layout_repulse walks a slice of the j range in tiles of TILE: 8192 is the largest n whose slice is one full tile,
    8193 the smallest with a second trip of the tile loop (a tile of one j), 12500 has two full tiles and one of 84; and
    no slice is empty (its block would still be launched: j0 = j1 = n), at any n below 2^20"""
    import ctypes as C
    lib = ly._bind_layout(load_library())
    for n, slices, length in ((8192, 32, 256), (8193, 32, 257), (12500, 21, 596)):
        assert (ly.slices_of(n), slice_len(n)) == (slices, length) and lib.nemgpu_layout_slices(n, None, None) == slices, n
    assert 596 == 2 * ly.TILE + 84
    first = next(n for n in range(1, 2 ** 20) if slice_len(n) > ly.TILE)
    assert first == 8193
    for n in range(1, 2 ** 20):
        s = ly.slices_of(n)
        assert (s - 1) * (-(-n // s)) < n, n                  # (the last slice starts below n)


def repulsion_rows(xy, mass, scaling, rows, keep=None, scale=None):
    """step 1 of layout_arrays for the rows `rows` alone, j ascending (order="left"), over the j's `keep` (all: None);
    scale: {(row, j): factor} multiplies single pair terms.  Returns float64 [len(rows)][2]."""
    out = np.zeros((len(rows), 2))
    for at, i in enumerate(rows):
        dx, dy = xy[i, 0] - xy[:, 0], xy[i, 1] - xy[:, 1]
        d2 = dx * dx + dy * dy
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = ((scaling * mass[i]) * mass) / d2
        coef[~(d2 > 0.0)] = 0.0
        for c, delta in ((0, dx), (1, dy)):
            terms = delta * coef
            for (row, j), factor in (scale or {}).items():
                if row == i:
                    terms[j] *= factor
            if keep is not None:
                terms = terms[keep]
            out[at, c] = np.cumsum(terms)[-1]
    return out


def test_the_force_bound_at_8193_rejects_a_wrong_pair_term_and_a_dropped_second_tile():
    """What tests/test_gpu_layout.py's comparison at n = 8193 can see, shown on the CPU: the yardstick is the row-blocked
    statement in extended precision, the bound step_tolerances' 2 n u B + n 2^-64 B.  A correct kernel in another order
    (the blocked statement, j ascending) lies inside it at every family.  Made wrong, it does not:
      one pair term of one row off by 2^-20 of itself, or missing;
      the j's behind the first TILE of one slice left out (slice_len - TILE = 1 of them at 8193: what a kernel that
      never makes the tile loop's second trip computes) -- at every family looked at, 300 of them."""
    n, d = 8193, 9
    _, graph, eb, _ = synth.master_pangenome_counts(n, d, 9000 + n, loops=0.05, multi_frac=0.1)
    g = ly.layout_graph(graph, eb, d)
    mass = g["mass"]
    pos = np.random.default_rng(n + 9).random((n, 2))
    pos[n // 2] = pos[0]
    want = one(graph, eb, d, pos, order="extended", block_rows=256)
    tol = step_tolerances(n, mass, want, np.zeros((n, 2)), 1.0, order="extended")["forces"]
    left = one(graph, eb, d, pos, order="left", block_rows=256)["forces"]
    inside = lambda f, rows: (np.abs(f - want["forces"][rows]) <= tol[rows]).all(axis=1)
    everyone = np.arange(n)
    worst = float((np.abs(left - want["forces"]) / tol).max())
    print("n %d: another order is at %.3g of the bound; the bound is %.3g of B; one pair term is about %.3g of B"
          % (n, worst, float((tol / want["bound"]).max()), 1.0 / n))
    assert inside(left, everyone).all()
    scaling = ly.DEFAULTS["scaling_ratio"]
    # the rows looked at: the first, the last, those around the slice's own j's, and a spread of others
    length, s = slice_len(n), 17
    gone = np.arange(s * length + ly.TILE, min(n, (s + 1) * length))
    assert length == ly.TILE + 1 and gone.tolist() == [s * length + ly.TILE]
    rows = np.unique(np.concatenate([[0, 1, n - 2, n - 1], np.arange(gone[0] - 3, gone[0] + 4), np.random.default_rng(5).integers(0, n, 300)]))
    rows = rows[(rows != gone[0]) & ~((pos[rows] == pos[gone[0]]).all(axis=1))]      # (its own term and a coincident pair's are 0 anyway)
    assert len(rows) >= 300
    full = repulsion_rows(pos, mass, scaling, rows)
    keep = np.setdiff1d(everyone, gone)
    dropped = left[rows] + (repulsion_rows(pos, mass, scaling, rows, keep=keep) - full)
    assert inside(left[rows] + (repulsion_rows(pos, mass, scaling, rows) - full), rows).all()      # (the method itself adds nothing)
    assert not inside(dropped, rows).any(), "a dropped second tile passes the bound at %d of %d families" % (int(inside(dropped, rows).sum()), len(rows))
    # one pair term of one row: the middle-sized term of that row
    i = int(rows[len(rows) // 2])
    dx, dy = pos[i] - pos[n - 7]
    assert dx != 0.0 and dy != 0.0
    k = int(np.nonzero(rows == i)[0][0])
    for factor in (1.0 + 2.0 ** -20, 0.0):
        wrong = left[rows] + (repulsion_rows(pos, mass, scaling, rows, scale={(i, n - 7): factor}) - full)
        verdict = inside(wrong, rows)
        assert not verdict[k] and verdict.sum() == len(rows) - 1, (factor, i)
