"""The master from the organisms' gene orders, on the host: chunks.master_arrays_from_orders (the numpy statement of
csrc/nem_orders.hip) against chunks.master_arrays_from_graph applied to the graph that the reference's own
__neighborhood_computation built (tests/golden/orders/, made by tests/golden/make_orders.py), and, on seeded random
annotation sets, to the networkx graph built by a transcription of ppanggolin.py:432-530 kept below."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import (master_arrays_from_graph, master_arrays_from_orders, orders_from_annotations)
from tests.orders_util import (FIXTURES, RecordedGraph, annotations_of, fixture_orders, load, orders_args, random_genomes, same_master)



def neighborhood_graph(annotations, circular, repeated, directed):
    """ppanggolin.py:463-530 with __add_gene (:414) and __add_link (:432-459), the parts a master reads: node -> {organism:
    genes}, edge -> {organism: count}.  Returns the graph and (self-loop links, genes bridged over)."""
    import networkx
    g = networkx.DiGraph() if directed else networkx.Graph()
    loops = bridged = 0

    def add_gene(fam, org, gene):
        g.add_node(fam)
        g.nodes[fam].setdefault(org, set()).add(gene)

    def add_link(fam, nei, org):
        if not g.has_edge(fam, nei):
            g.add_edge(fam, nei)
        g[fam][nei][org] = g[fam][nei].get(org, 0) + 1

    for org, contigs in annotations.items():
        for contig, annot in contigs.items():
            items = list(annot.items())
            while items and items[0][1][1] in repeated:       # :485-488
                items.pop(0)
            if not items:
                continue                                      # :489-490
            gene_start, info_start = items[0]
            add_gene(info_start[1], org, gene_start)
            nei = info_start[1]
            pending = 0
            for gene, info in items[1:]:
                if info[1] not in repeated:                   # :505
                    add_gene(info[1], org, gene)
                    add_link(info[1], nei, org)               # :513
                    loops += info[1] == nei
                    bridged += pending
                    pending = 0
                    nei = info[1]
                else:
                    pending += 1
            if contig in circular:
                add_link(info_start[1], nei, org)             # :518-519
                loops += info_start[1] == nei
    return g, (loops, bridged)


def from_orders(ann, orgs, circular, repeated, directed):
    o = orders_from_annotations(ann, orgs, circular, repeated)
    return o, master_arrays_from_orders(**orders_args(o, directed))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
@pytest.mark.parametrize("directed", [False, True])
def test_fixture_equals_recorded_graph(path, directed):
    rec = load(path)
    want = master_arrays_from_graph(RecordedGraph(rec["directed" if directed else "undirected"], directed), rec["organisms"])
    o, got = from_orders(annotations_of(rec), rec["organisms"], rec["circular"], rec["repeated"], directed)
    assert [o["families"][i] for i in got[4]] == list(want[4]), "family order"
    same_master(got, want, rec["name"])


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_transcription_equals_recorded_graph(path):
    """the transcription the random test relies on makes the reference's graph of every fixture"""
    rec = load(path)
    for directed in (False, True):
        g, _ = neighborhood_graph(annotations_of(rec), set(rec["circular"]), set(rec["repeated"]), directed)
        want = master_arrays_from_graph(RecordedGraph(rec["directed" if directed else "undirected"], directed), rec["organisms"])
        got = master_arrays_from_graph(g, rec["organisms"])
        assert list(got[4]) == list(want[4])
        same_master(got, want, rec["name"])


def test_fixtures_cover_the_cases():
    assert len(FIXTURES) >= 4
    recs = {r["name"]: r for r in map(load, FIXTURES)}
    assert any(b == a for a, nbrs in recs["duplicates"]["undirected"]["adj"] for b, _ in nbrs), "a self-loop"
    assert any(v >= 2 for _, nbrs in recs["duplicates"]["undirected"]["adj"] for _, data in nbrs for v in data.values())
    late = recs["late"]["undirected"]
    order = [f for f, _ in late["nodes"]]
    assert any([order.index(b) for b, _ in nbrs] != sorted(order.index(b) for b, _ in nbrs) for _, nbrs in late["adj"])


def test_orders_from_annotations_round_trips():
    for rec in map(load, FIXTURES):
        o = fixture_orders(rec)
        col = {name: c for c, name in enumerate(rec["organisms"])}
        j = 0
        for org, contigs in rec["annotations"]:
            for contig, genes in contigs:
                lo, hi = o["contig_ptr"][j], o["contig_ptr"][j + 1]
                assert [o["families"][f] for f in o["genes"][lo:hi]] == [fam for _, fam in genes]
                assert o["contig_org"][j] == col[org] and o["contig_circular"][j] == (contig in rec["circular"])
                j += 1
        assert j == len(o["contig_org"]) and o["contig_ptr"][-1] == len(o["genes"])
        assert sorted(o["families"][f] for f in np.flatnonzero(o["repeated"])) == sorted(set(rec["repeated"]) & set(o["families"]))


def test_random_annotations_equal_the_transcribed_graph():
    rng = np.random.default_rng(20261016)
    loops = bridged = multi = circ_small = late = 0
    for case in range(300):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 9)), int(rng.integers(1, 7)))
        for directed in (False, True):
            g, (lp, br) = neighborhood_graph(ann, set(circular), set(repeated), directed)
            o, got = from_orders(ann, orgs, circular, repeated, directed)
            if g.number_of_nodes() == 0:
                assert len(got[4]) == 0 and got[0].shape == (0, len(orgs)) and len(got[1][1]) == 0
                continue
            want = master_arrays_from_graph(g, orgs)
            assert [o["families"][i] for i in got[4]] == list(want[4]), (case, directed)
            same_master(got, want, "case %d directed %d" % (case, directed))
            loops += lp
            bridged += br
            multi += int((want[3][2] >= 2).sum())
            late += any(list(np.sort(got[1][1][a:b])) != list(got[1][1][a:b]) for a, b in zip(got[1][0][:-1], got[1][0][1:]))
    assert loops > 100 and bridged > 100 and multi > 100 and late > 100, (loops, bridged, multi, late)


def good():
    return dict(genes=[0, 1, 2, 1], contig_ptr=[0, 3, 4], contig_org=[0, 1], contig_circular=[1, 0], d=2, repeated=[0, 0, 1])


@pytest.mark.parametrize("field,value", [("genes", [0, 1, 3, 1]), ("genes", [0, -1, 2, 1]), ("contig_ptr", [0, 5, 4]), ("contig_ptr", [1, 3, 4]),
                                         ("contig_ptr", [0, 3, 3]), ("contig_org", [0, 2]), ("contig_org", [-1, 0]), ("contig_circular", [1]),
                                         ("repeated", [0, 0]), ("d", 0)])
def test_malformed_orders_raise(field, value):
    master_arrays_from_orders(**good())
    with pytest.raises(ValueError):
        master_arrays_from_orders(**dict(good(), **{field: value}))


def test_library_checks_orders_before_any_device_call():
    """nemgpu_master_create_orders refuses malformed orders on the host (NEMGPU_E_ARG and a message): no device is needed
    to see it"""
    from pangenomenem_amd import build
    from pangenomenem_amd.chunks import _bind_master
    from pangenomenem_amd.engine import load_library
    build.build()
    lib = _bind_master(load_library())

    def create(genes, ptr, org, circ, d, f, g=None, null=()):
        arrs = [np.ascontiguousarray(genes, np.int32), np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(org, np.int32),
                np.ascontiguousarray(circ, np.uint8)]
        at = [None if i in null else a.ctypes.data for i, a in enumerate(arrs)]
        h = C.c_void_p(1)
        rc = lib.nemgpu_master_create_orders(C.byref(h), 0, d, f, 0, at[0], len(arrs[0]) if g is None else g, at[1], at[2], at[3], len(arrs[2]), None)
        assert not h.value                                    # (refused: the handle is null, whatever it held)
        return rc, lib.nemgpu_last_error().decode()

    for args, word in ((([0, 1, 3], [0, 3], [0], [0], 1, 3), "family id"), (([0, 1, -1], [0, 3], [0], [0], 1, 3), "family id"),
                       (([0, 1, 2], [0, 2, 1, 3], [0, 0, 0], [0, 0, 0], 1, 3), "monotone"),
                       (([0, 1, 2], [0, 2], [0], [0], 1, 3), "contig_ptr"), (([0, 1, 2], [1, 3], [0], [0], 1, 3), "contig_ptr"),
                       (([0, 1, 2], [0, 3], [1], [0], 1, 3), "organism"), (([0, 1, 2], [0, 3], [-1], [0], 1, 3), "organism"),
                       (([0, 1, 2], [0, 3], [0], [0], 131072 * 32 + 1, 3), "131 072")):
        rc, msg = create(*args)
        assert rc == 3 and word in msg, (args, rc, msg)
    rc, msg = create([0, 1, 2], [0, 3], [0], [0], 1, 3, g=1 << 30)     # (refused by the sizes alone: no array is read)
    assert rc == 3 and "2^30" in msg, (rc, msg)
    # what is missing: NEMGPU_E_FUNCARG
    for kw in (dict(d=0), dict(f=0), dict(g=0), dict(null=(0,)), dict(null=(1,)), dict(null=(2,)), dict(null=(3,))):
        args = dict(genes=[0, 1, 2], ptr=[0, 3], org=[0], circ=[0], d=1, f=3)
        args.update(kw)
        rc, msg = create(**args)
        assert rc == 8 and "needed" in msg, (kw, rc, msg)
    rc, msg = create([0, 1, 2], [0], [], [], 1, 3)             # (no contig)
    assert rc == 8 and "needed" in msg, (rc, msg)
    assert lib.nemgpu_master_create_orders(None, 0, 1, 3, 0, None, 0, None, None, None, 0, None) == 8
