"""The GEXF node text on the device (nemgpu_node_table_*, csrc/nem_nodes.hip) against the host statement
gexf.node_text_host / HostNodeTable -- which tests/test_gexf_nodes_host.py holds against write_gexf's annotations path and the
reference's recorded exports -- byte for byte: the slices, the node ends, the titles and the ids.  The recorded fixtures;
the loader fixtures end to end from the files (Master.from_files -> node_table -> write_gexf(node_table=)), once with the
string hash cut to 2 bits; and the built cases of tests/gexf_nodes_util.py, each at the smallest shape where a kernel takes
another path; what is refused, before the text kernels run."""
import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.gexf import write_gexf
from tests import gexf_nodes_util as nu
from tests.gexf_metadata_util import METADATA_FIXTURES, metadata_of
from tests.gexf_util import GEXF_FIXTURES, sizes_of
from tests.loader_util import CASES, case_id, paths, recorded
from tests.matrix_util import repeated_by_organism
from tests.orders_util import load, same_master
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

GOOD = [p for p in CASES if recorded(p)["raises"] is None]


def from_orders(o):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])


def orders_of(o):
    return o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]


def statement_on(m, o, text, spans):
    """the host statement on the device master's own matrix and order"""
    rows, _, _, _, order = m.arrays()
    return nu.host_node_table(rows, order, o, text, spans, d=m.d)


def device_equals_statement(case, what, **kw):
    """a built case: its master and node table on the device against the statement; returns (host table, device text)"""
    m = from_orders(case)
    try:
        before = m.arrays()
        want = statement_on(m, case, case["text"], case["spans"])
        t = m.node_table(orders=orders_of(case), text=case["text"], spans=case["spans"], **kw)
        try:
            nu.same_node_tables(t, want, what)
            text = t.lines()[0].tobytes()
        finally:
            t.close()
        same_master(m.arrays(), before, what)
        return want, text
    finally:
        m.close()


@pytest.mark.parametrize("path", GEXF_FIXTURES + METADATA_FIXTURES, ids=lambda p: "/".join(p.split("/")[-2:])[:-5])
def test_fixtures(gpu_lib, path, tmp_path):
    rec = load(path)
    ann = annotations_of(rec)
    everyone = rec["organisms"] + rec["new_organisms"]
    m = Master.from_annotations(annotations_of(rec, rec["organisms"]), rec["organisms"], rec["circular"], rec["repeated"])
    try:
        if rec["new_organisms"]:
            grown = m.add_annotations(annotations_of(rec, rec["new_organisms"]), rec["new_organisms"],
                                      set(rec["circular"]) | set(rec["update_circular"]), set(rec["repeated"]) | set(rec["update_repeated"]))
            m.close()
            m = grown
        o, text, spans = nu.flat_of_annotations(ann, everyone, m.id_names, repeated_by_organism(rec))
        repeated = set(rec["repeated"]) | set(rec["update_repeated"])
        ft, et = m.family_table(ann, repeated), m.edge_table(ann, repeated, sizes_of(rec))
        nt = m.node_table(orders=orders_of(o), text=text, spans=spans)
        try:
            nu.same_node_tables(nt, statement_on(m, o, text, spans), rec["name"])
            meta = metadata_of(rec) if "metadata" in rec else None
            sub = ("subpartition_shell", {name: "S%d" % (i % 3) for i, name in enumerate(ft.names)})
            for k, kw in enumerate((dict(), dict(all_node_attributes=False, all_edge_attributes=False), dict(budget=1),
                                    dict(subpartition=sub, positions=np.random.default_rng(1).random((ft.n, 2))))):
                write_gexf(str(tmp_path / ("a%d" % k)), rec["labels"], ft, et, ann, metadata=meta, **kw)
                write_gexf(str(tmp_path / ("t%d" % k)), rec["labels"], ft, et, None, node_table=nt, metadata=meta, **kw)
                nu.same_file(str(tmp_path / ("t%d.gexf" % k)), str(tmp_path / ("a%d.gexf" % k)), "%s %r" % (rec["name"], sorted(kw)))
        finally:
            for table in (ft, et, nt):
                table.close()
    finally:
        m.close()


@pytest.mark.parametrize("path", GOOD, ids=case_id)
def test_from_the_files_to_the_graph(gpu_lib, path, tmp_path):
    rec = recorded(path)
    m = Master.from_files(*paths(path), **rec["args"])
    try:
        ld, o = m.loaded, m.loaded.orders
        text, spans = b"\n".join(ld._files), (ld.span_off[:3], ld.span_len[:3])
        want = statement_on(m, o, text, spans)
        tables = [m.node_table(), m.node_table(batch_bytes=1, _hash_bits=2), m.node_table(orders=orders_of(o), text=text, spans=spans, batch_bytes=64)]
        ann = ld.annotations()
        ft, et = m.family_table(ann), m.edge_table(ann, circular_contig_size=ld.circular_contig_size)
        try:
            for k, nt in enumerate(tables):
                nu.same_node_tables(nt, want, "%s table %d" % (rec["name"], k))
            labels = {name: "PSCU"[i % 4] for i, name in enumerate(m.names)}
            for k, kw in enumerate((dict(), dict(all_node_attributes=False, all_edge_attributes=False))):
                write_gexf(str(tmp_path / ("a%d" % k)), labels, ft, et, ann, **kw)
                write_gexf(str(tmp_path / ("t%d" % k)), labels, ft, et, node_table=tables[1], **kw)
                nu.same_file(str(tmp_path / ("t%d.gexf" % k)), str(tmp_path / ("a%d.gexf" % k)), rec["name"])
        finally:
            for table in tables + [ft, et]:
                table.close()
    finally:
        m.close()


@pytest.mark.parametrize("d", [1, 63, 64, 65, 2049])
def test_one_family_in_d_organisms(gpu_lib, d):
    want, text = device_equals_statement(nu.one_family_in(d), "d %d" % d)
    assert text.count(b"\n") == d + 2


@pytest.mark.parametrize("k", [1, 2, 65, 4097])
def test_copies_on_one_line(gpu_lib, k):
    _, text = device_equals_statement(nu.copies_on_one_line(k), "copies %d" % k)
    assert text.split(b"\n")[0].count(b"|") == k - 1


def test_a_hub_beside_single_gene_families(gpu_lib):
    want, _ = device_equals_statement(nu.hub_beside_singles(), "hub")
    assert want.nb_genes[0] == 4500 and want.n > 600


@pytest.mark.parametrize("which", ["equal", "distinct", "empty_first", "empty_middle", "empty_only", "two_families"])
def test_names(gpu_lib, which):
    for bits in (0, 1):
        device_equals_statement(nu.names_case(which), which, _hash_bits=bits)


def test_thousands_of_products_with_colliding_probes(gpu_lib):
    _, text = device_equals_statement(nu.many_products(3000), "products", _hash_bits=2)
    assert text.split(b"\n")[2].count(b"|") == 2999


def test_escaped_bytes(gpu_lib):
    _, text = device_equals_statement(nu.escapes_case(), "escapes")
    assert b"&amp;&lt;&gt;&quot;&#13;&#10;&#09;|" in text and b"\xc3\xa9&amp;\xc3\xa9" in text


def test_ids_of_one_to_four_digits(gpu_lib):
    want, _ = device_equals_statement(nu.late_organisms(1100), "late")
    assert {len(str(k)) for k in want.ids()[0].tolist()} == {1, 2, 3, 4}


def test_flagged_families(gpu_lib):
    want, text = device_equals_statement(nu.flagged_case(), "flagged")
    assert want.ids()[0].tolist() == [1, -1, 4] and b"gone" not in text and b"g3_" not in text


def test_text_batches_cut_a_familys_genes(gpu_lib):
    case = nu.hub_beside_singles(copies=300, singles=40)
    m = from_orders(case)
    try:
        want = statement_on(m, case, case["text"], case["spans"])
        for batch_bytes in (1, 100, 5000):                    # a gene per batch; a few genes; a few hundred
            t = m.node_table(orders=orders_of(case), text=case["text"], spans=case["spans"], batch_bytes=batch_bytes)
            try:
                nu.same_node_tables(t, want, "batch_bytes %d" % batch_bytes, tails=(6,))
            finally:
                t.close()
    finally:
        m.close()


def test_text_budgets(gpu_lib):
    case = nu.hub_beside_singles(copies=300, singles=40)
    m = from_orders(case)
    try:
        want = statement_on(m, case, case["text"], case["spans"])
        t = m.node_table(orders=orders_of(case), text=case["text"], spans=case["spans"])
        try:
            whole, ends = want.lines()
            assert list(t._batches(1)) == [(i, 1) for i in range(t.n)] == list(want._batches(1))          # the hub, above the budget, comes alone
            small = int(np.diff(ends)[1:].max())
            cut = list(t._batches(3 * small))
            assert cut[0] == (0, 1) and max(rows for _, rows in cut) >= 3 and cut == list(want._batches(3 * small))
            for full in (True, False):
                whole, ends = want.lines(full=full)
                parts = []
                for row0, rows in t._batches(3 * small, full):
                    part, part_ends = t.lines(row0, rows, full)
                    assert np.array_equal(part_ends, ends[row0:row0 + rows] - (ends[row0 - 1] if row0 else 0)), (row0, full)
                    parts.append(part.tobytes())
                assert b"".join(parts) == whole.tobytes()
            needed = t.lines_size(0, 2)
            out = np.full(needed - 1, 7, np.uint8)
            with pytest.raises(NemGpuError, match="the batch needs %d" % needed) as err:
                t.lines(0, 2, out=out)
            assert err.value.needed == needed and (out == 7).all()
            out = np.full(needed + 3, 7, np.uint8)
            text, _ = t.lines(0, 2, out=out)
            assert text.tobytes() == whole_full(want, 2) and (out[needed:] == 7).all()
            for row0, rows in ((-1, 1), (0, 0), (t.n, 1), (0, t.n + 1)):
                with pytest.raises((NemGpuError, ValueError), match="rows outside"):
                    t.lines(row0, rows)
        finally:
            t.close()
    finally:
        m.close()


def whole_full(table, rows):
    return table.lines(0, rows)[0].tobytes()


def test_the_smallest_masters(gpu_lib):
    want, text = device_equals_statement(nu.built([(0, [nu.gene(0, 0, b"", b"")])], 1), "one gene")
    assert want.n == 1 and text.count(b"\n") == 3
    with pytest.raises(NemGpuError, match="no gene is kept"):                  # n = 0: there is no such master to make a table of
        from_orders(nu.built([(0, [nu.gene(0, 0)])], 1, flagged=(0,)))


def test_what_is_refused(gpu_lib):
    case = nu.flagged_case()
    m = from_orders(case)
    try:
        before = m.arrays()
        moved = dict(case, genes=case["genes"].copy())
        moved["genes"][0] = 4                                 # organism 0 loses family 0 and gains family 4
        with pytest.raises(NemGpuError, match="not this master's"):
            m.node_table(orders=orders_of(moved), text=case["text"], spans=case["spans"])
        fewer = dict(case, genes=case["genes"].copy(), repeated=case["repeated"].copy())
        fewer["repeated"][4] = 1                              # family 4's only gene is not kept: the master has a bit without a gene
        with pytest.raises(NemGpuError, match="not this master's"):
            m.node_table(orders=orders_of(fewer), text=case["text"], spans=case["spans"])
        past = (case["spans"][0].copy(), case["spans"][1].copy())
        past[1][2, -1] += 1                                   # the last product ends one byte past the text
        with pytest.raises(NemGpuError, match="past the end"):
            m.node_table(orders=orders_of(case), text=case["text"], spans=past)
        with pytest.raises(NemGpuError, match="non-decreasing"):
            m.node_table(orders=(case["genes"], case["contig_ptr"], case["contig_org"][::-1].copy(), case["repeated"]), text=case["text"],
                         spans=case["spans"])
        m.repeated_by_organism = {"a": frozenset(), "b": frozenset(["x"])}
        with pytest.raises(ValueError, match="differ between organisms"):
            m.node_table(type("L", (), {})())
        same_master(m.arrays(), before, "refusals")
    finally:
        m.close()
