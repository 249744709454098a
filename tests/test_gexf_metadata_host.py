"""export_to_GEXF's metadata= in numpy (pangenomenem_amd/gexf.py: rank_metadata, edge_metadata_arrays, metavalues_host,
HostEdgeTable.metavalues, write_gexf(metadata=)) against what the reference's own export_to_GEXF(path, False, metadata[,
False, False]) and networkx's write_gexf wrote (tests/golden/gexf_metadata/), compared as the exports without metadata
are; the CLI's parse of its metadata file; the first column as partition_shell's init; what is refused; and the export
without metadata, byte for byte what it was."""
from collections import OrderedDict, defaultdict

import numpy as np
import pytest

from pangenomenem_amd.gexf import (edge_metadata_arrays, metavalues_host, rank_metadata, read_metadata, shell_init_from_metadata,
                                   write_gexf)
from tests.gexf_metadata_util import METADATA_FIXTURES, metadata_of, read_text
from tests.gexf_util import GEXF_FIXTURES, host_tables, same_gexf_text
from tests.orders_util import load


@pytest.mark.parametrize("path", METADATA_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixture_exports_with_metadata(path, tmp_path):
    rec = load(path)
    everyone = rec["organisms"] + rec["new_organisms"]
    ft, et, ann = host_tables(rec)
    write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, metadata=metadata_of(rec))
    write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, metadata=metadata_of(rec))
    same_gexf_text(read_text(str(tmp_path / "full.gexf")), rec["gexf"], everyone, rec["name"] + " full")
    same_gexf_text(read_text(str(tmp_path / "light.gexf")), rec["gexf_light"], everyone, rec["name"] + " light")
    write_gexf(str(tmp_path / "cut"), rec["labels"], ft, et, ann, metadata=metadata_of(rec), budget=1)        # a batch per edge
    assert open(str(tmp_path / "cut.gexf"), "rb").read() == open(str(tmp_path / "full.gexf"), "rb").read()


def test_fixtures_cover_the_cases():
    recs = {r["name"]: r for r in map(load, METADATA_FIXTURES)}
    assert set(recs) == {"links", "repeated_late", "circular"}
    links = metadata_of(recs["links"])
    assert [list(v) for v in links.values()] == [["country", "host"]] * 3
    values = [v for row in links.values() for v in row.values()]
    assert 'pig&"x"' in values and "" in values and "Åb|c" in values and values.count("fr") == 2
    full, light = recs["links"]["gexf"], recs["links"]["gexf_light"]
    for title, a, b in (("country", 17, 13), ("host", 18, 14)):                       # behind length_max, before o1 and o3
        assert '<attribute id="%d" title="%s" type="string" />' % (a, title) in full
        assert '<attribute id="%d" title="%s" type="string" />' % (b, title) in light
    assert '<attribute id="19" title="o1" type="long" />' in full and 'title="o1"' not in light
    assert 'value="cow|pig&amp;&quot;x&quot;"' in full and '<attvalue for="17" value="" />' in full and 'value="Åb|c"' in light
    assert recs["repeated_late"]["new_organisms"]
    one = metadata_of(recs["circular"])
    assert all(list(v.items()) == [("kingdom", "Bacteria")] for v in one.values())


def test_the_statements_on_the_links_case():
    rec = load([p for p in METADATA_FIXTURES if p.endswith("links.json")][0])
    _, et, _ = host_tables(rec)
    meta = rank_metadata(metadata_of(rec), rec["organisms"])
    assert meta["titles"] == ["country", "host"] and meta["n_values"].tolist() == [2, 3]
    assert meta["value_rank"].tolist() == [[1, 0, 1], [1, 2, 0]]                      # "" < "fr"; "cow" < 'pig&"x"' < "Åb|c"
    blob = meta["value_text"].tobytes()
    assert [blob[a:b].decode() for a, b in zip(meta["value_ptr"][:-1], meta["value_ptr"][1:])] == ["", "fr", "cow", "pig&amp;&quot;x&quot;", "Åb|c"]
    graph, bits, _ = et._master
    masks = edge_metadata_arrays(graph, bits, meta["value_rank"], meta["n_values"], 3)
    assert masks.dtype == np.uint32 and masks.tolist() == [[1, 4], [2, 3], [1, 4], [2, 1], [2, 1]]
    text, ends = metavalues_host(graph, bits, [7, 12345], meta["value_rank"], meta["n_values"], meta["value_ptr"], meta["value_text"], 3, 1, 2)
    want = ['          <attvalue for="7" value="fr" />\n          <attvalue for="12345" value="cow|pig&amp;&quot;x&quot;" />\n',
            '          <attvalue for="7" value="" />\n          <attvalue for="12345" value="Åb|c" />\n']
    assert text.tobytes().decode() == "".join(want) and ends.tolist() == [len(want[0].encode()), len("".join(want).encode())]
    et.set_metadata([7, 12345], meta["value_rank"], meta["n_values"], meta["value_ptr"], meta["value_text"])
    assert et.metavalues_size(1, 2) == len(text) and np.array_equal(et.metamasks(1, 2), masks[1:3])
    attr_id, titles = et.attribute_ids(12, n_attr=2)
    assert [k for k, what in titles if isinstance(what, tuple)] == [17, 18] and attr_id.tolist() == [19, 12, 20]
    assert [k for k, what in et.attribute_ids(9, organisms=False, n_attr=2)[1]] == [9, 10, 11, 12, 13, 14]
    with pytest.raises(ValueError, match="rows outside"):
        metavalues_host(graph, bits, [7, 8], meta["value_rank"], meta["n_values"], meta["value_ptr"], meta["value_text"], 3, 4, 2)
    for bad, word in ((dict(attr_id=[7, -1]), "negative"), (dict(value_rank=np.asarray([[1, 0, 2], [1, 2, 0]])), "rank"),
                      (dict(value_ptr=np.asarray([0, 0, 2, 1, 21, 26])), "value_ptr"), (dict(n_values=np.asarray([2, 0])), "values")):
        args = dict(attr_id=[7, 8], value_rank=meta["value_rank"], n_values=meta["n_values"], value_ptr=meta["value_ptr"], value_text=meta["value_text"])
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            metavalues_host(graph, bits, d=3, **args)


def cli_parse(lines, organisms):
    """command_line.py:439-447 and 487, transcribed"""
    metadata = list()
    attribute_names = list()
    for num, line in enumerate(lines):
        elements = [el.strip() for el in line.split("\t")]
        if num == 0:
            attribute_names = elements
        else:
            metadata.append(dict(zip(attribute_names, elements)))
    return OrderedDict(zip(list(organisms), metadata))


def test_read_metadata_is_the_clis_parse(tmp_path):
    text = "country\thost \t note\nfr\tpig\t x y \n\t cow\t\nde\tÅb|c\n"
    organisms = ["o1", "o2", "o3"]
    path = tmp_path / "meta.tsv"
    path.write_text(text, encoding="utf-8")
    want = cli_parse(text.splitlines(True), organisms)
    got = read_metadata(str(path), organisms)
    assert got == want and [list(v.items()) for v in got.values()] == [list(v.items()) for v in want.values()] and list(got) == organisms
    assert got["o1"] == {"country": "fr", "host": "pig", "note": "x y"} and got["o2"] == {"country": "", "host": "cow", "note": ""}
    assert list(got["o3"].items()) == [("country", "de"), ("host", "Åb|c")]          # (zip cuts a short line: write_gexf refuses it)
    assert read_metadata(text.splitlines(True), organisms) == want
    assert list(read_metadata(text.splitlines(True), ["o1", "o2"])) == ["o1", "o2"] and list(read_metadata(text.splitlines(True), organisms + ["o4"])) == organisms


def test_the_first_column_as_partition_shells_init():
    metadata = read_metadata(["country\thost\n", "fr\tpig\n", "de\tpig\n", "fr\tcow\n"], ["o1", "o2", "o3"])
    want = defaultdict(set)
    for org, row in metadata.items():
        want[list(row.values())[0]].add(org)                  # "use the first column of metadata"
    assert shell_init_from_metadata(metadata) == dict(want) == {"fr": {"o1", "o3"}, "de": {"o2"}}
    assert shell_init_from_metadata(metadata, "host") == {"pig": {"o1", "o2"}, "cow": {"o3"}}
    with pytest.raises(ValueError):
        shell_init_from_metadata(metadata, "nothing")
    with pytest.raises(ValueError):
        shell_init_from_metadata({"o1": {}})


def test_what_write_gexf_refuses(tmp_path):
    rec = load([p for p in METADATA_FIXTURES if p.endswith("links.json")][0])
    ft, et, ann = host_tables(rec)
    good = metadata_of(rec)

    def changed(**rows):
        return dict(good, **rows)

    missing = dict(good)
    del missing["o2"]
    for bad, word in ((missing, "missing"),
                      (changed(o2={"country": "x", "host": 3}), "not a str"),
                      (changed(o2={"country": "x", "host": None}), "not a str"),
                      (changed(o3={"host": "cow", "country": "fr"}), "has attributes"),
                      (changed(o3={"country": "fr"}), "has attributes"),
                      (changed(o3={"country": "fr", "host": "cow", "more": "x"}), "has attributes"),
                      ({org: {"o2": "x"} for org in good}, "named like"),
                      ({org: {"weight": "x"} for org in good}, "named like"),
                      ({org: {"ok": "x", "length_med": "x"} for org in good}, "named like")):
        for light in (False, True):
            with pytest.raises(ValueError, match=word):
                write_gexf(str(tmp_path / "bad"), rec["labels"], ft, et, ann, all_node_attributes=not light, all_edge_attributes=not light, metadata=bad)


@pytest.mark.parametrize("path", GEXF_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_without_metadata_the_export_is_what_it_was(path, tmp_path):
    rec = load(path)
    everyone = rec["organisms"] + rec["new_organisms"]
    ft, et, ann = host_tables(rec)
    for name, kw in (("none", dict(metadata=None)), ("empty", dict(metadata={})), ("plain", {})):
        write_gexf(str(tmp_path / name), rec["labels"], ft, et, ann, **kw)
        write_gexf(str(tmp_path / (name + "_light")), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, **kw)
    same_gexf_text(read_text(str(tmp_path / "none.gexf")), rec["gexf"], everyone, rec["name"] + " full")
    same_gexf_text(read_text(str(tmp_path / "none_light.gexf")), rec["gexf_light"], everyone, rec["name"] + " light")
    for name in ("empty", "plain"):
        assert open(str(tmp_path / (name + ".gexf")), "rb").read() == open(str(tmp_path / "none.gexf"), "rb").read()
        assert open(str(tmp_path / (name + "_light.gexf")), "rb").read() == open(str(tmp_path / "none_light.gexf"), "rb").read()
