"""The GEXF export and the U-shaped plot's series in numpy (pangenomenem_amd/gexf.py: edge_table_arrays, attvalues_host,
HostEdgeTable, write_gexf, ushape_counts) against what the reference's own export_to_GEXF() and networkx's write_gexf
wrote and what ushaped_plot's own lines counted (tests/golden/gexf/), byte for byte except <meta> and the values the
reference joins from a set; the statement against a plain per-link walk over the transcribed graph build on random
annotation sets; and what the statement refuses."""
import gzip
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.gexf import attvalues_host, edge_table_arrays, gexf_orders, ushape_counts, write_gexf
from tests.append_util import build_host
from tests.gexf_util import GEXF_FIXTURES, contigs_orders, host_tables, path_contigs, same_gexf_text
from tests.orders_util import load, orders_from_annotations, random_genomes


def exports(rec, tmp_path, **kw):
    ft, et, ann = host_tables(rec)
    write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, **kw)
    write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, **kw)
    return ft, et


@pytest.mark.parametrize("path", GEXF_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixture_exports(path, tmp_path):
    rec = load(path)
    everyone = rec["organisms"] + rec["new_organisms"]
    ft, _ = exports(rec, tmp_path)
    same_gexf_text(open(str(tmp_path / "full.gexf"), newline="", encoding="utf-8").read(), rec["gexf"], everyone, rec["name"] + " full")
    same_gexf_text(open(str(tmp_path / "light.gexf"), newline="", encoding="utf-8").read(), rec["gexf_light"], everyone, rec["name"] + " light")
    assert ushape_counts(rec["labels"], ft).T.tolist() == rec["ushape"]


def test_fixtures_cover_the_cases():
    recs = {r["name"]: r for r in map(load, GEXF_FIXTURES)}
    assert set(recs) == {"repeated", "circular", "duplicates", "late", "repeated_late", "copies", "links"}
    rec = recs["links"]
    assert len(rec["organisms"]) <= 6 and len(rec["labels"]) <= 8
    _, et, _ = host_tables(rec)
    loops = et.src == et.dst
    assert loops.sum() == 2                                   # a circular contig of one kept gene, a tandem pair
    assert (et.len_min < 0).any()                             # overlapping genes
    even = (et.len_distinct % 2 == 0) & ((et.len_mid_lo + et.len_mid_hi) % 2 == 1)
    assert even.any() and 'value="357.5"' in rec["gexf"]     # the same pair twice on a circular contig of two kept genes
    assert et.org_first_edge.tolist() == [1, 0, 1]            # organism 0 is first met on a later edge than organism 1
    attr_id, _ = et.attribute_ids(12)
    assert attr_id[1] < attr_id[0]
    assert "&amp;&lt;&quot;" in rec["gexf"] and '"R"' not in rec["gexf"]
    assert recs["repeated_late"]["new_organisms"]
    assert any(any(row) for row in recs["copies"]["ushape"])


def test_compressed_and_batched_exports_are_the_same_bytes(tmp_path):
    rec = load([p for p in GEXF_FIXTURES if p.endswith("duplicates.json")][0])
    exports(rec, tmp_path)
    plain = open(str(tmp_path / "full.gexf"), "rb").read()
    ft, et, ann = host_tables(rec)
    write_gexf(str(tmp_path / "z"), rec["labels"], ft, et, ann, compressed=True)
    assert gzip.open(str(tmp_path / "z.gexf.gz"), "rb").read() == plain
    write_gexf(str(tmp_path / "b"), rec["labels"], ft, et, ann, budget=1)         # a batch per edge
    assert open(str(tmp_path / "b.gexf"), "rb").read() == plain
    assert list(et._batches(1)) == [(e, 1) for e in range(et.n_edges)] and list(et._batches(1 << 30)) == [(0, et.n_edges)]


def link_walk(ann, orgs, repeated, sizes):
    """the graph the way __neighborhood_computation, __add_gene and __add_link make it (ppanggolin.py:414-520), per gene
    and per link, into dictionaries: the nodes in order of first kept gene, every node's adjacency in insertion order,
    per edge {organism: count} and the set of its lengths; per node the set of its gene lengths"""
    nodes, adj, data = OrderedDict(), {}, {}

    def add_gene(fam, length):
        nodes.setdefault(fam, set()).add(length)
        adj.setdefault(fam, OrderedDict())

    def add_link(a, b, org, length):
        if b not in adj[a]:
            adj[a][b] = adj[b][a] = data[frozenset((a, b))] = dict(orgs=OrderedDict(), lengths=set())
        e = adj[a][b]
        e["orgs"][org] = e["orgs"].get(org, 0) + 1
        e["lengths"].add(length)

    for org, contigs in ann.items():
        for contig, annot in contigs.items():
            kept = [info for info in annot.values() if info[1] not in repeated]
            if not kept:
                continue
            first = kept[0]
            add_gene(first[1], first[3] - first[2])
            nei, end_nei = first[1], first[3]
            for info in kept[1:]:
                add_gene(info[1], info[3] - info[2])
                add_link(info[1], nei, orgs.index(org), info[2] - end_nei)
                nei, end_nei = info[1], info[3]
            if contig in sizes:
                add_link(first[1], nei, orgs.index(org), (sizes[contig] - end_nei) + first[2])
    edges, seen = [], set()
    for u in nodes:                                           # nx.Graph.edges()
        for v, e in adj[u].items():
            if v not in seen:
                edges.append((u, v, e))
        seen.add(u)
    return nodes, edges


def middles(values):
    v = sorted(values)
    return v[(len(v) - 1) // 2], v[len(v) // 2]


def test_random_annotations_equal_the_link_walk():
    rng = np.random.default_rng(20270301)
    done = multi = loops = 0
    for case in range(30):
        ann, _, circular, repeated = random_genomes(rng, int(rng.integers(2, 30)), int(rng.integers(1, 40)), max_len=25)
        orgs = list(ann)                                      # (the columns in walk order)
        for contigs in ann.values():
            for annot in contigs.values():
                at = 0
                for info in annot.values():
                    start = at + int(rng.integers(-3, 4)) * 20
                    at = start + int(rng.integers(1, 4)) * 150
                    info += [start, at, "+", "n", "p"]
        sizes = {contig: int(rng.integers(5000, 5004)) for contig in circular}
        o = orders_from_annotations(ann, orgs, circular, repeated)
        if not len(o["genes"]) or o["repeated"][o["genes"]].all():
            continue
        host = build_host(o)
        names = [o["families"][i] for i in host[4]]
        t = gexf_orders(ann, orgs, o["families"], repeated, sizes)
        got = edge_table_arrays(host[1], host[2], host[3], host[4], t["genes"], t["starts"], t["ends"], t["contig_ptr"], t["contig_org"],
                                t["contig_sizes"], t["repeated"], d=len(orgs))
        nodes, edges = link_walk(ann, orgs, set(repeated), sizes)
        assert list(nodes) == names and len(edges) == len(got["src"]), case
        attr_id = np.arange(len(orgs)) * 7 + 3
        text, ends = attvalues_host(host[1], host[2], host[3], attr_id, len(orgs)) if edges else (np.zeros(0, np.uint8), np.zeros(0))
        first = {}
        for e, (u, v, data) in enumerate(edges):
            lo, hi = middles(data["lengths"])
            assert (names[got["src"][e]], names[got["dst"][e]], got["weight"][e]) == (u, v, len(data["orgs"])), (case, e)
            assert (got["len_min"][e], got["len_max"][e], got["len_distinct"][e], got["len_sum"][e], got["len_mid_lo"][e], got["len_mid_hi"][e]) == \
                (min(data["lengths"]), max(data["lengths"]), len(data["lengths"]), sum(data["lengths"]), lo, hi), (case, e)
            assert list(data["orgs"]) == sorted(data["orgs"])     # (walked in column order: first met in column order)
            want = "".join('          <attvalue for="%d" value="%d" />\n' % (attr_id[org], cnt) for org, cnt in data["orgs"].items())
            assert bytes(text[(ends[e - 1] if e else 0):ends[e]]).decode() == want, (case, e)
            for org in data["orgs"]:
                first.setdefault(org, e)
            multi += max(data["orgs"].values()) > 1
            loops += u == v
        assert got["org_first_edge"].tolist() == [first.get(c, len(edges)) for c in range(len(orgs))], case
        for i, name in enumerate(names):
            assert (got["fam_mid_lo"][i], got["fam_mid_hi"][i]) == middles(nodes[name]), (case, name)
        done += 1
    assert done >= 20 and multi >= 10 and loops >= 10


def statement(host, o, **kw):
    return edge_table_arrays(host[1], host[2], host[3], host[4], kw.get("genes", o["genes"]), kw.get("starts", o["starts"]), o["ends"],
                             o["contig_ptr"], kw.get("contig_org", o["contig_org"]), o["contig_sizes"], d=o["d"], f=kw.get("f"),
                             bits_only=kw.get("bits_only", False))


def test_the_statement_refuses_what_is_not_the_masters():
    rng = np.random.default_rng(3)
    o = contigs_orders(path_contigs(rng, 12, 5) + [(4, [3, 3], -1), (4, [7], 10)], 5, rng)
    host = build_host(o)
    got = statement(host, o)
    assert len(got["src"]) == 14 and (got["src"] == got["dst"]).sum() == 2
    changed = o["genes"].copy()
    changed[5] = 9                                            # (organism 0's path now runs 4 - 9 - 6: edges the master lacks)
    with pytest.raises(ValueError, match="not this master's"):
        statement(host, o, genes=changed)
    with pytest.raises(ValueError, match="not in the master"):
        statement(host, o, genes=np.where(np.arange(len(o["genes"])) == 5, 13, o["genes"]), f=14)
    # one adjacency duplicated: the same edges and organisms, one count differs; a bits-only master cannot tell
    twice = contigs_orders(path_contigs(np.random.default_rng(3), 12, 5) + [(4, [3, 3], -1), (4, [7], 10), (0, [0, 1], -1)], 5,
                           np.random.default_rng(3))
    with pytest.raises(ValueError, match="number of links is not the master's count"):
        statement(host, twice)
    assert np.array_equal(statement(host, twice, bits_only=True)["weight"], got["weight"])
    with pytest.raises(ValueError, match="non-decreasing"):
        statement(host, o, contig_org=o["contig_org"][::-1].copy())
    far = o["starts"].copy()
    far[1], o["ends"][0] = 2 ** 31 - 1, -5
    with pytest.raises(ValueError, match="outside int32"):
        statement(host, o, starts=far)
    with pytest.raises(ValueError, match="rows outside"):
        attvalues_host(host[1], host[2], host[3], np.zeros(5, np.int32), 5, 3, 12)
    with pytest.raises(ValueError, match="attr_id"):
        attvalues_host(host[1], host[2], host[3], np.asarray([0, 1, -1, 2, 3]), 5)


def test_the_synthetic_pangenome_goes_through_the_whole_host_path(tmp_path):
    import xml.etree.ElementTree as ET

    from pangenomenem_amd.gexf import HostEdgeTable
    from pangenomenem_amd.matrix import HostFamilyTable, table_orders
    from pangenomenem_amd.synth import annotated_pangenome
    ann, orgs, circular = annotated_pangenome(60, 7, 3)
    o = orders_from_annotations(ann, orgs, circular, ())
    host = build_host(o)
    names = [o["families"][i] for i in host[4]]
    t = table_orders(ann, orgs, o["families"], ())
    ft = HostFamilyTable(host[0], host[4], t["genes"], t["lengths"], t["contig_ptr"], t["contig_org"], t["repeated"], names=names,
                         organism_names=orgs)
    t = gexf_orders(ann, orgs, o["families"], (), circular)
    et = HostEdgeTable(host[1], host[2], host[3], host[4], t["genes"], t["starts"], t["ends"], t["contig_ptr"], t["contig_org"], t["contig_sizes"],
                       t["repeated"], d=len(orgs))
    assert ft.n == 60 and et.n_edges > 60 and (et.len_min < 0).any() and (et.src == et.dst).any() and circular
    write_gexf(str(tmp_path / "g"), {name: "PSC"[i % 3] for i, name in enumerate(names)}, ft, et, ann)
    ns = "{http://www.gexf.net/1.2draft}"
    graph = ET.parse(str(tmp_path / "g.gexf")).getroot().find(ns + "graph")
    assert len(graph.find(ns + "nodes")) == 60 and len(graph.find(ns + "edges")) == et.n_edges
    lines = sum(len(edge.find(ns + "attvalues")) for edge in graph.find(ns + "edges"))
    assert lines == int(et.weight.sum()) + 4 * et.n_edges
