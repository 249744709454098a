"""The device master build, append and projection (csrc/nem_orders.hip, nem_project.hip and the scans of nem_scan.hpp
they share) at the shapes of tests/master_shapes.py where their kernels take another path -- scans of more items than
one pass of k_scan_partials takes, item counts on a tile's and a pass's end, runs of equal sorted keys over tile and
block ends, key fields at and one past a power of two, every set of wanted outputs, rows far apart, a hub's row that
an append lengthens by more than a block, extras over a word of organisms, appends to an appended master, the 2^24
bound across an append -- array for array against the numpy statements (chunks.master_arrays_from_orders,
master_arrays_append_orders, projection.projection_arrays); and the consumers of a master grown at that scale.
tests/test_master_shapes_host.py asserts on the CPU that every fixture reaches the branch it is here for."""
import random

import numpy as np
import pytest

from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.projection import projection_arrays
from tests import master_shapes as ms
from tests.orders_util import same_master
from tests.projection_util import random_part, same_projection
from tests.test_gpu_master_append import add_orders, device_equals_host as append_equals_host, from_orders
from tests.test_gpu_orders import device_equals_host as build_equals_host
from tests.test_gpu_projection import device_equals_host as projection_equals_host, raw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scan_device(gpu_lib):
    """the scan fixture's master on the device, built once"""
    m = from_orders(ms.scan_orders())
    yield m
    m.close()


def scan_part():
    return random_part(np.random.default_rng(61), ms.scan_master()[0].shape[0])


# ---- the projection
@pytest.mark.parametrize("size", ["more", "all", "pass", "pass+1", "tiles"])
def test_projection_scan_sizes(scan_device, size):
    """one scan item per projected gene: more kept genes than a pass of k_scan_partials takes (their runs' numbers need
    its carry), more genes than a pass, exactly a pass, a pass and one, whole tiles; the repeated families' genes sort
    behind the kept ones"""
    p = ms.scan_orders(size)
    g = len(p["genes"])
    assert {"more": ms.scan_passes(g) == 2, "all": ms.scan_passes(g) == 2, "pass": g == ms.SCAN_PASS, "pass+1": g == ms.SCAN_PASS + 1,
            "tiles": g == 3 * ms.SCAN_TILE}[size]
    want = projection_equals_host(scan_device, ms.scan_master(), scan_part(), p, "scan fixture, " + size)
    assert (want[0] == -1).any() and (want[1] >= 2).any() and want[3][:p["contig_org"].max(), 6].all()
    assert size != "more" or (want[0] >= 0).sum() > ms.SCAN_PASS + 2 * ms.SCAN_TILE


def test_projection_every_set_of_outputs(scan_device):
    """the outputs not wanted are NULL: what is wanted equals the call that wants everything"""
    p, part, host = ms.scan_orders("more"), scan_part(), ms.scan_master()
    n, d = host[0].shape
    g = len(p["genes"])
    full = dict(zip(("fam", "cop", "nei", "org"), projection_equals_host(scan_device, host, part, p, "all outputs")))
    shapes = dict(org=(d, 7), nei=(n, 3), fam=(g,), cop=(g,))
    for names in (("org",), ("nei",), ("cop",), ("fam",), ("org", "cop"), ("nei", "fam"), ("fam", "cop"), ("org", "nei")):
        outs = {name: np.full(shapes[name], -7, np.int32) for name in names}
        rc, msg = raw(scan_device, part, len(p["repeated"]), p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"], **outs)
        assert rc == 0, msg
        for name in names:
            assert np.array_equal(outs[name], full[name]), "%s of %s" % (name, names)


def test_projection_copies_over_a_tile_every_gene_kept_and_none(gpu_lib):
    """301 genes of one family in one organism, their sorted keys over a scan tile's end and two blocks' ends; every
    gene kept (the last sorted key closes the last run, no key sorts behind it); no gene kept"""
    o = ms.copies_orders()
    host = ms.host_master(o)
    part = random_part(np.random.default_rng(62), ms.COPIES_FAMILIES)
    m = from_orders(o)
    try:
        want = projection_equals_host(m, host, part, o, "every gene kept")
        assert (want[0] >= 0).all() and want[1].min() >= 1 and want[1].max() == ms.COPIES + 1
        assert (want[1][want[0] == ms.COPIES_FAMILY] == [ms.COPIES + 1] * (ms.COPIES + 1)).all() and want[1][-3:].tolist() == [3, 3, 3]
        assert want[3][:, 6].sum() == len(o["genes"])
        want = projection_equals_host(m, host, part, dict(o, repeated=None), "no repeated array")
        assert want[1].max() == ms.COPIES + 1
        want = projection_equals_host(m, host, part, dict(o, repeated=np.ones(ms.COPIES_FAMILIES, np.uint8)), "no gene kept")
        assert (want[0] == -1).all() and not want[1].any() and not want[3].any() and want[2].any()
    finally:
        m.close()


@pytest.mark.parametrize("n", ms.KEY_FAMILIES)
def test_projection_key_widths(gpu_lib, n):
    """n families and d organisms at and one past a power of two, d = 1, 2, 3: the key's organism and family fields, the
    key of the genes not counted and the sorted bits"""
    for d in ms.KEY_ORGANISMS:
        o, rep = ms.key_orders(n, d)
        host = ms.host_master(o)
        part = random_part(np.random.default_rng(n + d), n)
        m = from_orders(o)
        try:
            want = projection_equals_host(m, host, part, o, "%d x %d, every gene kept" % (n, d))
            assert want[1].min() >= 1 and want[1].max() >= 2
            want = projection_equals_host(m, host, part, dict(o, repeated=rep), "%d x %d, repeated" % (n, d))
            assert (want[0] == -1).any() == bool(rep.any()) and want[1].max() >= 2
        finally:
            m.close()


def test_projection_rows_far_apart(gpu_lib):
    """more than 131 072 rows, nearly all empty, before, between and behind two hubs whose rows span four blocks and more"""
    o, hubs = ms.wide_rows_orders()
    host = ms.host_master(o)
    n = host[0].shape[0]
    part = random_part(np.random.default_rng(63), n)
    idx, ptr = host[1][1], host[1][0]
    m = from_orders(o)
    try:
        want = projection_equals_host(m, host, part, o, "rows far apart")
    finally:
        m.close()
    for hub in hubs:
        cls = part[idx[ptr[hub]:ptr[hub + 1]]]
        assert want[2][hub].tolist() == [(cls == k).sum() for k in range(3)] and want[2][hub].min() > 150 and (cls == 3).sum() > 150
    assert not want[2][:hubs[0]].any() and not want[2][n - ms.WIDE_ROWS_EMPTY[2]:].any()


# ---- the build
@pytest.mark.parametrize("size", ["all", "pass", "half", "half+1"])
def test_build_scan_sizes(gpu_lib, size):
    """the build's scans (per gene, per record, per pair) over more than a pass; the genes exactly a pass; the records
    exactly a pass and two more"""
    o = ms.scan_orders(size)
    assert {"all": ms.scan_passes(len(o["genes"])) == 2, "pass": len(o["genes"]) == ms.SCAN_PASS, "half": ms.orders_records(o) == ms.SCAN_PASS,
            "half+1": ms.orders_records(o) == ms.SCAN_PASS + 2}[size]
    want = build_equals_host(o, False, "scan fixture, " + size)
    assert len(want[3][1]) > 0 and ms.plan_scans(o, want)["pairs"] > ms.SCAN_PASS // 2 - ms.SCAN_TILE * 8


# ---- the append
def test_append_scan_fixture(gpu_lib):
    """an update of more records than a pass: every scan of the plan carries; the grown master is the one build's"""
    base, upd = ms.scan_parts()
    assert ms.orders_records(upd) > ms.SCAN_PASS
    host = append_equals_host(base, [(upd, ms.SCAN_ORGANISMS - ms.SCAN_BASE)], "scan fixture")
    whole = ms.scan_master()
    assert np.array_equal(host[1][4], whole[4])
    same_master(host[1], whole, "one build")


def test_append_widens_the_keys(gpu_lib):
    """the families pass 4 096 and the organisms 32 with the update: its keys are wider than the base's were, the
    numbering goes on from the old master's"""
    base, upd = ms.key_bits_parts()
    n0, d0, n1, d1 = ms.KEY_BITS_PARTS
    host = append_equals_host(base, [(upd, d1 - d0)], "key bits")
    assert host[0][0].shape == (n0, d0) and host[1][0].shape == (n1, d1) and np.array_equal(host[1][4][:n0], host[0][4])


def test_append_to_a_hub_row(gpu_lib):
    """a row of 402 entries gains 322 in one append, their flags over a scan tile's end"""
    base, upd = ms.hub_parts()
    host = append_equals_host(base, [(upd, 2)], "hub")
    deg0, deg1 = np.diff(host[0][1][0]), np.diff(host[1][1][0])
    assert deg0[ms.HUB] == ms.HUB_OLD + 2 and deg1[ms.HUB] - deg0[ms.HUB] == ms.HUB_NEW + 22
    row = host[1][1][1][host[1][1][0][ms.HUB]:host[1][1][0][ms.HUB + 1]]
    assert np.array_equal(row[:deg0[ms.HUB]], host[0][1][1][host[0][1][0][ms.HUB]:host[0][1][0][ms.HUB + 1]]) and len(set(row.tolist())) == len(row)


def test_append_to_more_than_32_extras(gpu_lib):
    """an entry of 40 extras gains 30, the update's organisms on both sides of a word's end"""
    base, upd = ms.extras_parts()
    host = append_equals_host(base, [(upd, ms.EXTRAS_UPDATE)], "extras")
    assert np.diff(host[1][3][0]).max() == ms.EXTRAS_BASE + ms.EXTRAS_UPDATE


def test_three_appends_in_a_row(gpu_lib):
    """30 -> 45 -> 70 -> 100 organisms: every source but the first is a master an append made, none a multiple of 32"""
    parts = ms.triple_parts()
    steps = [(u, hi - lo) for u, lo, hi in zip(parts[1:], ms.TRIPLE_STAGES[:-1], ms.TRIPLE_STAGES[1:])]
    host = append_equals_host(parts[0], steps, "three appends")
    assert [m[0].shape[1] for m in host] == list(ms.TRIPLE_STAGES)
    whole = ms.host_master(ms.concat_orders(parts, ms.TRIPLE_STAGES[-1]))
    assert np.array_equal(host[-1][4], whole[4])
    same_master(host[-1], whole, "one build")


def test_append_masks_the_bits_above_the_last_organism(gpu_lib):
    """a master made of arrays whose edge_bits carry set bits above organism d - 1 (45 organisms: 19 such bits in every
    entry's last word, which are not data): the grown master's new organisms 45 .. 63 start from clear bits"""
    from pangenomenem_amd.chunks import Master
    old = ms.triple_masters()[1]
    upd = ms.triple_parts()[2]
    n0, d0 = old[0].shape
    assert d0 == 45 and old[2].shape[1] == 2
    dirty = old[2].copy()
    dirty[:, -1] |= np.uint32(0xffffffff) << np.uint32(d0 & 31)
    # the master's family i is id i: the update's ids in its numbering, the ids it lacks behind
    ids = np.concatenate([old[4], np.setdiff1d(np.arange(len(upd["repeated"])), old[4])])
    newid = np.empty(len(ids), np.int64)
    newid[ids] = np.arange(len(ids))
    u = dict(upd, genes=newid[upd["genes"]].astype(np.int32), repeated=upd["repeated"][ids])
    source = (old[0], old[1], dirty, old[3], np.arange(n0, dtype=np.int32))
    want = ms.host_append(source, n0, u, ms.TRIPLE_STAGES[2] - d0)
    clear = ((want[2][:, 1] >> np.uint32(d0 & 31)) & np.uint32(0x7ffff)) == 0      # entries none of organisms 45 .. 63 carries
    assert want[0].shape[0] > n0 and clear.sum() > 1000 and not clear.all()
    m = Master(old[0], old[1][0], old[1][1], dirty, edge_counts=old[3])
    try:
        g = add_orders(m, u, ms.TRIPLE_STAGES[2] - d0)
        try:
            got = g.arrays()
            assert np.array_equal(got[4], want[4])
            same_master(got, want, "bits above the last organism")
        finally:
            g.close()
        assert np.array_equal(m.arrays()[2].ravel(), dirty.ravel())             # (the source master as it was given)
    finally:
        m.close()


def test_count_bound_across_an_append(gpu_lib):
    """entry (0, 1) counts 2^23 in the master; an update that brings 2^23 more is taken (2^24 is exact in a float), one
    that brings 2^23 + 1 is refused though neither count alone passes the bound"""
    half = ms.COUNT_BOUND // 2
    m = from_orders(ms.alternating_orders(half, 0, 1))
    try:
        assert m.shape() == (2, 1, 2, 2)
        ok = add_orders(m, ms.alternating_orders(half, 1, 2), 1)
        try:
            _, _, _, (xptr, xorg, xcnt), _ = ok.arrays()
            assert ok.shape() == (2, 2, 2, 4) and xorg.tolist() == [0, 1, 0, 1] and xcnt.tolist() == [half] * 4
        finally:
            ok.close()
        with pytest.raises(NemGpuError, match="2\\^24"):
            add_orders(m, ms.alternating_orders(half + 1, 1, 2), 1)
        assert m.shape() == (2, 1, 2, 2)
    finally:
        m.close()


# ---- what reads a grown master
def test_consumers_of_the_grown_scan_master(gpu_lib):
    """Master.projection and Master.evolution on the scan fixture appended to and on its one build: the same arrays, the
    same rows, the generator left in the same state"""
    base, upd = ms.scan_parts()
    o = ms.scan_orders("more")                                # (what is projected: more kept genes than a scan pass)
    a, b = from_orders(base), from_orders(ms.scan_orders())
    g = add_orders(a, upd, ms.SCAN_ORGANISMS - ms.SCAN_BASE)
    try:
        assert np.array_equal(g.order, b.order)
        part = scan_part()
        orders = (o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"])
        pg, pb = g.projection(part, orders=orders), b.projection(part, orders=orders)
        arrays = lambda p: (p.gene_family, p.gene_copies, p.nei_counts, p.org_counts)
        same_projection(arrays(pg), arrays(pb), "appended and built")
        same_projection(arrays(pg), projection_arrays(ms.scan_master(), ms.scan_master()[4], part, *orders), "the statement")
        assert pg.columns == pb.columns == list(range(ms.SCAN_ORGANISMS)) and pg.means() == pb.means()
        ep = dict(ratio=0.1, rmin=1, rmax=30, step=4, limit=16, chunk_size=10, tie="libc", batch=8, seed=3)
        r1, r2 = random.Random(64), random.Random(64)
        rows_g, rows_b = g.evolution(r1, **ep), b.evolution(r2, **ep)
        assert np.array_equal(rows_g, rows_b) and r1.getstate() == r2.getstate()
        assert sorted(rows_g[:, 0].tolist()) == [4, 8, 12, 16] and (rows_g[:, 1:].sum(axis=1) > 0).all()
    finally:
        for m in (a, b, g):
            m.close()
