"""The GEXF nodes without the nested annotations, in plain Python (pangenomenem_amd/gexf.py: node_text_host,
node_attribute_ids, HostNodeTable, write_gexf(node_table=)): the file written through a node table against the file written
through the annotations, byte for byte, on every recorded GEXF export and on every loadable loader fixture; against the
reference's recorded text; what the statement refuses; and the reach of the built cases the device tests run."""
import numpy as np
import pytest

from pangenomenem_amd import loader
from pangenomenem_amd.gexf import HostEdgeTable, HostNodeTable, escape, escape_bytes, node_attribute_ids, node_text_host, write_gexf
from pangenomenem_amd.matrix import HostFamilyTable
from tests import gexf_nodes_util as nu
from tests.append_util import build_host
from tests.gexf_metadata_util import METADATA_FIXTURES, metadata_of, read_text
from tests.gexf_util import GEXF_FIXTURES, host_tables, same_gexf_text
from tests.loader_util import CASES, case_id, paths, recorded
from tests.matrix_util import repeated_by_organism
from tests.orders_util import load
from tests.projection_util import annotations_of, fixture_master_host

GOOD = [p for p in CASES if recorded(p)["raises"] is None]


def both_ways(tmp_path, labels, ft, et, ann, nt, what, **kw):
    """the file through the annotations and through the node table: the same bytes"""
    write_gexf(str(tmp_path / "a"), labels, ft, et, ann, **kw)
    write_gexf(str(tmp_path / "t"), labels, ft, et, None, node_table=nt, **kw)
    ext = ".gexf.gz" if kw.get("compressed") else ".gexf"
    nu.same_file(str(tmp_path / ("t" + ext)), str(tmp_path / ("a" + ext)), what)
    return str(tmp_path / "t.gexf")


def fixture_tables(rec):
    ft, et, ann = host_tables(rec)
    m, ids, _ = fixture_master_host(rec)
    everyone = rec["organisms"] + rec["new_organisms"]
    o, text, spans = nu.flat_of_annotations(ann, everyone, ids, repeated_by_organism(rec))
    return ft, et, ann, nu.host_node_table(m[0], m[4], o, text, spans), everyone


@pytest.mark.parametrize("path", GEXF_FIXTURES + METADATA_FIXTURES, ids=lambda p: "/".join(p.split("/")[-2:])[:-5])
def test_fixture_exports_without_annotations(path, tmp_path):
    rec = load(path)
    ft, et, ann, nt, everyone = fixture_tables(rec)
    meta = metadata_of(rec) if "metadata" in rec else None
    got = both_ways(tmp_path, rec["labels"], ft, et, ann, nt, rec["name"] + " full", metadata=meta)
    same_gexf_text(read_text(got), rec["gexf"], everyone, rec["name"] + " full")
    got = both_ways(tmp_path, rec["labels"], ft, et, ann, nt, rec["name"] + " light", metadata=meta, all_node_attributes=False,
                    all_edge_attributes=False)
    same_gexf_text(read_text(got), rec["gexf_light"], everyone, rec["name"] + " light")
    rng = np.random.default_rng(5)
    sub = ("subpartition_shell", {name: "S%d<&" % (i % 3) for i, name in enumerate(ft.names)})
    everything = dict(positions=rng.random((ft.n, 2)), subpartition=sub,
                      metadata=meta or {org: {"where": "site %d" % (k % 2), "who": "x"} for k, org in enumerate(everyone)})
    both_ways(tmp_path, rec["labels"], ft, et, ann, nt, rec["name"] + " positions, subpartition, metadata", **everything)
    both_ways(tmp_path, rec["labels"], ft, et, ann, nt, rec["name"] + " the same, light", all_node_attributes=False, all_edge_attributes=False,
              **everything)
    both_ways(tmp_path, rec["labels"], ft, et, ann, nt, rec["name"] + " a node per batch, compressed", budget=1, compressed=True)


def loaded_tables(ld):
    o = ld.orders
    host = build_host(o)
    names = [o["families"][i] for i in host[4]]
    ft = HostFamilyTable(host[0], host[4], o["genes"], o["lengths"], o["contig_ptr"], o["contig_org"], o["repeated"], names=names,
                         organism_names=list(ld.organisms), repeated_names=ld.families_repeted)
    et = HostEdgeTable(host[1], host[2], host[3], host[4], o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"], o["contig_sizes"],
                       o["repeated"], d=o["d"])
    nt = HostNodeTable(host[0], host[4], o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"], b"\n".join(ld._files),
                       (ld.span_off[:3], ld.span_len[:3]), d=o["d"])
    return ft, et, nt, names


@pytest.mark.parametrize("path", GOOD, ids=case_id)
def test_loader_fixtures_from_the_flat_load(path, tmp_path):
    rec = recorded(path)
    ld = loader.load_arrays_host(*paths(path), **rec["args"])
    ft, et, nt, names = loaded_tables(ld)
    labels = {name: "PSCU"[i % 4] for i, name in enumerate(names)}
    both_ways(tmp_path, labels, ft, et, ld.annotations(), nt, rec["name"] + " full")
    both_ways(tmp_path, labels, ft, et, ld.annotations(), nt, rec["name"] + " light", all_node_attributes=False, all_edge_attributes=False)


def test_escape_bytes_is_escape():
    for text in ("plain", '&<>"\r\n\t', "a&amp;b", "é<中>", ""):
        assert escape_bytes(text.encode()) == escape(text).encode()
    assert escape_bytes(b"\xff&\x80") == b"\xff&amp;\x80"


def test_the_ids_are_numbered_where_first_met():
    # 4 organisms, 3 nodes: organisms 2 and 0 at node 0, organism 3 at node 2, organism 1 nowhere
    org_id, name_id, (light, full) = node_attribute_ids([0, 3, 0, 2], 3, tail=2)
    assert full == ["nb_genes", 0, "name", "product", 2, ("tail", 0), ("tail", 1), 3] and org_id.tolist() == [1, -1, 4, 7] and name_id == (1, 2)
    assert light == ["nb_genes", "name", "product", ("tail", 0), ("tail", 1)]
    org_id, name_id, (_, full) = node_attribute_ids([1, 1], 2, tail=1)          # node 0 has no organism
    assert full == ["nb_genes", "name", "product", ("tail", 0), 0, 1] and name_id == (1, 1)
    assert node_attribute_ids([0, 0], 0)[2] == ([], [])


def test_the_statement_refuses_what_is_not_the_masters():
    case = nu.flagged_case()
    host, table = nu.host_of(case)
    args = lambda **kw: [kw.get(k, v) for k, v in (("x", host[0]), ("order", host[4]), ("genes", case["genes"]), ("contig_ptr", case["contig_ptr"]),
                                                  ("contig_org", case["contig_org"]), ("repeated", case["repeated"]), ("text", case["text"]),
                                                  ("spans", case["spans"]))]
    assert node_text_host(*args(), d=3)["nb_genes"].tolist() == table.nb_genes.tolist() == [2, 2, 1]
    with pytest.raises(ValueError, match="per organism"):
        node_text_host(*args(repeated={"o0": frozenset(), "o1": frozenset(["f1"]), "o2": frozenset(["f1"])}), d=3)
    other = nu.built([(0, [nu.gene(0, 0), nu.gene(2, 0)]), (1, [nu.gene(2, 1)]), (2, [nu.gene(2, 2), nu.gene(0, 2), nu.gene(4, 2)])], 3, n_ids=5)
    with pytest.raises(ValueError, match="not this master's"):                 # organism 1 has a kept gene the master does not know of
        node_text_host(*args(genes=other["genes"], contig_ptr=other["contig_ptr"], contig_org=other["contig_org"], repeated=other["repeated"],
                             text=other["text"], spans=other["spans"]), d=3)
    moved = case["genes"].copy()
    moved[0] = 4                                              # organism 0 loses family 0 and gains family 4
    with pytest.raises(ValueError, match="not this master's"):
        node_text_host(*args(genes=moved), d=3)
    with pytest.raises(ValueError, match="not in the master"):
        node_text_host(*args(genes=np.where(np.arange(len(moved)) == 0, 5, case["genes"]), repeated=np.zeros(6, np.uint8)), d=3)
    past = (case["spans"][0].copy(), case["spans"][1].copy())
    past[1][2, -1] += 1                                       # the last product ends one byte past the text
    with pytest.raises(ValueError, match="past the end"):
        node_text_host(*args(spans=past), d=3)
    with pytest.raises(ValueError, match="non-decreasing"):
        node_text_host(*args(contig_org=case["contig_org"][::-1].copy()), d=3)
    ft, et, ann, nt, _ = fixture_tables(load([p for p in GEXF_FIXTURES if p.endswith("links.json")][0]))
    with pytest.raises(ValueError, match="node table is not of"):
        write_gexf("unused", {}, ft, et, None, node_table=table)
    with pytest.raises(ValueError, match="annotations, or a node_table"):
        write_gexf("unused", {}, ft, et)
    with pytest.raises(ValueError, match="rows outside"):
        nt.lines(0, nt.n + 1)


def test_flagged_genes_add_nothing():
    table = nu.reach(nu.flagged_case())["table"]
    text = table.lines()[0].tobytes()
    assert table.first.tolist() == [0, 3, 0] and table.ids()[0].tolist() == [1, -1, 4]
    assert b"gone" not in text and b"lost" not in text and b"g1_" not in text and b"g3_" not in text and b"g4_2" in text


def test_no_family_and_one_gene():
    case = nu.built([(0, [nu.gene(0, 0)])], 1, flagged=(0,))                   # every gene flagged: no family, n = 0
    table = HostNodeTable(np.zeros((0, 1), np.uint8), np.zeros(0, np.int32), case["genes"], case["contig_ptr"], case["contig_org"],
                          case["repeated"], case["text"], case["spans"])
    assert (table.n, table.d) == (0, 1) and table.titles() == [] and table.titles(False) == [] and list(table._batches(10)) == []
    assert table.ids()[0].tolist() == [-1]
    table = nu.reach(nu.built([(0, [nu.gene(0, 0, b"", b"")])], 1))["table"]
    assert table.lines()[0].tobytes() == (b'          <attvalue for="1" value="g0_0" />\n          <attvalue for="2" value="" />\n'
                                          b'          <attvalue for="3" value="" />\n')
    assert table.titles() == ["nb_genes", 0, "name", "product"] + [("tail", j) for j in range(6)]


def test_the_built_cases_reach_what_they_are_for():
    for d in (1, 63, 64, 65, 2049):
        got = nu.reach(nu.one_family_in(d))
        assert (got["n"], got["organisms"], got["copies"]) == (1, d, 1)
        assert got["table"].lines()[0].tobytes().count(b"\n") == d + 2
    for k in (1, 2, 65, 4097):
        got = nu.reach(nu.copies_on_one_line(k))
        assert (got["n"], got["organisms"], got["copies"]) == (1, 1, k)
        assert got["table"].lines()[0].tobytes().split(b"\n")[0].count(b"|") == k - 1
    got = nu.reach(nu.hub_beside_singles())
    starts = np.concatenate([[0], np.cumsum(got["table"].nb_genes)])
    assert got["copies"] == 1500 and got["n"] > 600 and (got["table"].nb_genes[1:] == 1).all()
    assert starts[1] % 256 != 0 and starts[1] > 256 * 10 and got["kept"] > starts[1] + 256        # the hub ends, the singles run on, inside blocks
    for which, names in (("equal", b"same"), ("distinct", b"a|b|c|d|e|f"), ("empty_first", b"|x|y"), ("empty_middle", b"x||y|z"), ("empty_only", b"")):
        table = nu.reach(nu.names_case(which))["table"]
        assert table.lines(full=False)[0].tobytes().split(b"\n")[0] == b'          <attvalue for="1" value="' + names + b'" />', which
    table = nu.reach(nu.names_case("two_families"))["table"]
    light = table.lines(full=False)[0].tobytes().split(b"\n")
    assert table.n == 2 and light[0] == light[2] and b'value="x|y|z"' in light[0]
    got = nu.reach(nu.many_products(3000))
    assert got["table"].lines(full=False)[0].tobytes().split(b"\n")[1].count(b"|") == 2999
    # with the hash cut to 2 bits a key's home slot is one of 4, whatever the hash: of 3000 distinct classes at most 4 find
    # their home empty, every other first probe meets another class
    classes, homes = 3000, 2 ** 2
    assert got["kept"] == classes and classes - homes >= 2996
    text = nu.reach(nu.escapes_case())["table"].lines()[0].tobytes()
    values = b"".join(line[line.index(b'value="') + 7:-4] for line in text.split(b"\n")[:-1])
    for ch, word in zip(nu.SPECIAL, (b"&amp;", b"&lt;", b"&gt;", b"&quot;", b"&#13;", b"&#10;", b"&#09;")):
        assert values.count(word) >= 5 and (ch == ord("&") or bytes((ch,)) not in values)
    assert b"&amp;&lt;&gt;&quot;&#13;&#10;&#09;|" in text and "géne\u0085".encode() in text and b"\xc3\xa9&amp;\xc3\xa9" in text
    case = nu.escapes_case()
    inside = np.zeros(len(case["text"]), bool)
    for off, length in zip(case["spans"][0].ravel(), case["spans"][1].ravel()):
        inside[off:off + length] = True
    special = np.flatnonzero(inside & np.isin(np.frombuffer(case["text"], np.uint8), list(nu.SPECIAL)))
    assert set((special % 8).tolist()) == set(range(8))      # escaped bytes start at each of the 8 alignments of the text
    got = nu.reach(nu.late_organisms(1100))
    ids = got["table"].ids()[0]
    assert got["n"] == 1100 and {len(str(k)) for k in ids.tolist()} == {1, 2, 3, 4} and ids[1099] < ids[5] and ids.max() == 1100 + 8
    assert got["table"].first.tolist()[:6] == [0, 0, 0, 0, 0, 5] and got["table"].first[1099] == 1
