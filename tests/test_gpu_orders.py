"""The master built on the device from the organisms' gene orders (nemgpu_master_create_orders, csrc/nem_orders.hip)
against its numpy statement chunks.master_arrays_from_orders -- which tests/test_orders_host.py holds against the
reference's own graphs -- on the recorded fixtures, on random annotation sets and at the shapes of
tests/master_shapes.py; the read-back (nemgpu_master_fetch) of masters made from arrays; partition() on a master from
orders and on the master from the graph of the same annotations."""
import ctypes as C
import random
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master, _bind_master, master_arrays_from_graph, master_arrays_from_orders, pack_rows
from tests import master_shapes as ms
from tests.orders_util import (FIXTURES, RecordedGraph, annotations_of, fixture_orders, load, orders_args, random_genomes, same_master,
                               synthetic_orders)
from tests.test_orders_host import neighborhood_graph

pytestmark = pytest.mark.gpu


def device_equals_host(o, directed, what):
    want = master_arrays_from_orders(**orders_args(o, directed))
    m = Master.from_orders(**orders_args(o, directed))
    try:
        got = m.arrays()
        assert m.shape() == (want[0].shape[0], want[0].shape[1], len(want[1][1]), len(want[3][1])), what
        assert np.array_equal(got[4], want[4]) and np.array_equal(m.order, want[4]), what + ": family order"
        same_master(got, want, what)
    finally:
        m.close()
    return want


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
@pytest.mark.parametrize("directed", [False, True])
def test_fixtures(gpu_lib, path, directed):
    rec = load(path)
    device_equals_host(fixture_orders(rec), directed, rec["name"])
    m = Master.from_annotations(annotations_of(rec), rec["organisms"], rec["circular"], rec["repeated"], directed=directed)
    assert m.names == [f for f, _ in rec["directed" if directed else "undirected"]["nodes"]] and m.organism_names == rec["organisms"]
    m.close()


def test_random_annotations(gpu_lib):
    from pangenomenem_amd.chunks import orders_from_annotations
    rng = np.random.default_rng(20261017)
    done = multi = 0
    for case in range(120):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 40)), int(rng.integers(1, 70)), max_len=30)
        o = orders_from_annotations(ann, orgs, circular, repeated)
        if not len(o["genes"]) or o["repeated"][o["genes"]].all():
            continue
        for directed in (False, True):
            want = device_equals_host(o, directed, "case %d directed %d" % (case, directed))
            multi += len(want[3][1])
        done += 1
    assert done > 100 and multi > 1000


@pytest.mark.parametrize("n,d", ms.BOUNDARY_SHAPES)
def test_boundary_shapes(gpu_lib, n, d):
    """n around one 64-family word, d around one 32-organism word (tests/master_shapes.py)"""
    o = synthetic_orders(n, d, 70 + n + d, p_repeat=0.0)
    for directed in (False, True):
        want = device_equals_host(o, directed, "%d x %d directed %d" % (n, d, directed))
        assert want[0].shape == (n, d)


def test_cloud_shape(gpu_lib):
    """cloud_master's shape (20 000 x 300), sparse: most families in a few organisms"""
    n, d = ms.cloud_master()[0].shape
    want = device_equals_host(synthetic_orders(n, d, 41, density=0.03), False, "cloud")
    assert want[0].shape[1] == d and want[0].shape[0] > 0.9 * n and len(want[3][1]) > 0


def test_wide_shape(gpu_lib):
    """wide_master's shape: more than 131 072 families x 300 organisms, a directed graph"""
    n, d = ms.wide_master()[0].shape
    o = synthetic_orders(n, d, 42, density=0.1, p_repeat=0.0)
    assert ms.scan_passes(len(o["genes"])) > 2 and ms.scan_passes(ms.orders_records(o)) > 4     # (k_scan_partials carries in every scan)
    want = device_equals_host(o, True, "wide")
    assert want[0].shape == (n, d) and n > 131072


def test_fetch_returns_what_went_in(gpu_lib):
    for rec in map(load, FIXTURES):
        for directed in (False, True):
            g = RecordedGraph(rec["directed" if directed else "undirected"], directed)
            want = master_arrays_from_graph(g, rec["organisms"])
            m = Master.from_graph(g, rec["organisms"])
            got = m.arrays()
            same_master(got, want, rec["name"])
            assert np.array_equal(got[4], np.arange(len(want[4])))
            m.close()
    x, (ptr, idx), eb = ms.boundary_master(65, 33)
    m = Master(x, ptr, idx, eb)                               # bits only: no extras
    rows, (p, i), e, (xp, xo, xc), order = m.arrays()
    assert m.shape() == (65, 33, len(idx), 0)
    assert np.array_equal(rows, pack_rows(x)) and np.array_equal(p, ptr) and np.array_equal(i, idx) and np.array_equal(e, eb)
    assert not xp.any() and len(xo) == 0 and len(xc) == 0 and np.array_equal(order, np.arange(65))
    m.close()


def test_partition_equals_from_graph(gpu_lib):
    o = synthetic_orders(300, 30, 7, density=0.5, p_repeat=0.03)
    fams, orgs = ["fam%d" % i for i in range(300)], ["org%d" % i for i in range(30)]
    ann = OrderedDict()
    circular = set()
    for j, org in enumerate(o["contig_org"]):
        contig = "c%d" % j
        ann.setdefault(orgs[org], OrderedDict())[contig] = OrderedDict(
            ("g%d" % p, ["CDS", fams[o["genes"][p]]]) for p in range(o["contig_ptr"][j], o["contig_ptr"][j + 1]))
        if o["contig_circular"][j]:
            circular.add(contig)
    repeated = [fams[i] for i in np.flatnonzero(o["repeated"])]
    for directed in (False, True):
        g, _ = neighborhood_graph(ann, circular, set(repeated), directed)
        a = Master.from_graph(g, orgs)
        b = Master.from_annotations(ann, orgs, circular, repeated, directed=directed)
        assert a.names == b.names
        same_master(b.arrays(), a.arrays(), "directed %d" % directed)
        ra = a.partition(chunk_size=10, rng=random.Random(5), batch=8, tie="libc", seed=3)
        rb = b.partition(chunk_size=10, rng=random.Random(5), batch=8, tie="libc", seed=3)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2] and ra[2] > 0
        sa = a.partition(organisms=np.arange(8), just_stats=True, tie="libc", seed=3)       # (core_exact reads the packed rows)
        sb = b.partition(organisms=np.arange(8), just_stats=True, tie="libc", seed=3)
        assert dict(sa[0]) == dict(sb[0]) and np.array_equal(sa[1], sb[1])
        a.close()
        b.close()


def test_malformed_orders_are_refused(gpu_lib):
    lib = _bind_master(gpu_lib)

    def create(genes, ptr, org, circ, d, f, rep=None):
        arrs = [np.ascontiguousarray(genes, np.int32), np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(org, np.int32),
                np.ascontiguousarray(circ, np.uint8)]
        rep = None if rep is None else np.ascontiguousarray(rep, np.uint8)
        h = C.c_void_p()
        rc = lib.nemgpu_master_create_orders(C.byref(h), 0, d, f, 0, arrs[0].ctypes.data, len(arrs[0]), arrs[1].ctypes.data, arrs[2].ctypes.data,
                                             arrs[3].ctypes.data, len(arrs[2]), None if rep is None else rep.ctypes.data)
        assert not h.value
        return rc, lib.nemgpu_last_error().decode()

    for args, word in ((([0, 1, 3], [0, 3], [0], [0], 1, 3), "family id"), (([0, -1, 2], [0, 3], [0], [0], 1, 3), "family id"),
                       (([0, 1, 2], [0, 2, 1, 3], [0, 0, 0], [0, 0, 0], 1, 3), "monotone"), (([0, 1, 2], [0, 2], [0], [0], 1, 3), "contig_ptr"),
                       (([0, 1, 2], [0, 3], [1], [0], 1, 3), "organism"), (([0, 1, 2], [0, 3], [-1], [0], 1, 3), "organism"),
                       (([0, 1, 1], [0, 3], [0], [0], 1, 2, [1, 1]), "no gene is kept")):
        rc, msg = create(*args)
        assert rc == 3 and word in msg, (args, rc, msg)
    with pytest.raises(ValueError):
        Master.from_orders([0, 1, 5], [0, 3], [0], [0], 1, f=3)
