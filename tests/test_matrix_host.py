"""The pangenome matrix, the partition lists and the summary in numpy (pangenomenem_amd/matrix.py: family_table_arrays,
rtab_cells_host, HostFamilyTable, write_partitions, summary) against what the reference's own write_matrix(), the CLI's
partition-list lines and __str__ wrote (tests/golden/matrix/), byte for byte except the fields the reference joins from
a set; and the statement against a plain per-gene walk on random annotation sets."""
from collections import OrderedDict, defaultdict

import numpy as np
import pytest

from pangenomenem_amd.matrix import HostFamilyTable, copy_counts, family_table_arrays, rtab_cells_host, table_orders
from tests.append_util import build_host
from tests.matrix_util import MATRIX_FIXTURES, counts_orders, files_equal_fixture, random_counts, repeated_by_organism
from tests.orders_util import load, orders_from_annotations, random_genomes
from tests.projection_util import annotations_of, fixture_master_host


def host_table(rec):
    m, ids, names = fixture_master_host(rec)
    everyone = rec["organisms"] + rec["new_organisms"]
    ann = annotations_of(rec)
    by_org = repeated_by_organism(rec)
    o = table_orders(ann, everyone, ids, by_org)
    return HostFamilyTable(m[0], m[4], o["genes"], o["lengths"], o["contig_ptr"], o["contig_org"], o["repeated"], names=names,
                           organism_names=everyone, repeated_names=by_org), ann


@pytest.mark.parametrize("path", MATRIX_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixture_files(path, tmp_path):
    rec = load(path)
    table, ann = host_table(rec)
    files_equal_fixture(table, rec, ann, tmp_path)


def test_fixtures_cover_the_cases():
    recs = {r["name"]: r for r in map(load, MATRIX_FIXTURES)}
    assert set(recs) == {"repeated", "circular", "duplicates", "late", "repeated_late", "copies"}
    rtab = recs["copies"]["files"]["matrix.Rtab"].split("\n")
    assert any("\t12\t" in line for line in rtab) and any("\t250\t250\t250.0\t" in line for line in rtab)
    assert recs["copies"]["files"]["partitions/persistent.txt"] == "\n"                  # an empty list is one newline
    assert recs["repeated_late"]["new_organisms"] and '"R"' in recs["repeated_late"]["files"]["matrix.Rtab"]


def test_header_less_and_single_files(tmp_path):
    rec = load([p for p in MATRIX_FIXTURES if p.endswith("copies.json")][0])
    table, ann = host_table(rec)
    table.write_matrix(str(tmp_path / "m"), rec["labels"], ann, header=False, csv=False)
    assert not (tmp_path / "m.csv").exists()
    assert open(str(tmp_path / "m.Rtab"), newline="").read().split("\n")[0].endswith("\t2\t1\t1")
    # a budget of one line's text: a batch per family, the same bytes
    table.write_matrix(str(tmp_path / "b"), rec["labels"], ann, header=False, csv=False, budget=1)
    assert open(str(tmp_path / "b.Rtab"), "rb").read() == open(str(tmp_path / "m.Rtab"), "rb").read()


def gene_walk(ann, orgs, names, repeated):
    """the table the way __add_gene makes it: per gene, into dictionaries"""
    node = OrderedDict((name, dict(nb=0, lengths=set(), cells=defaultdict(int))) for name in names)
    for org, contigs in ann.items():
        for annot in contigs.values():
            for info in annot.values():
                if info[1] in repeated:
                    continue
                v = node[info[1]]
                v["nb"] += 1
                v["lengths"].add(info[3] - info[2])
                v["cells"][orgs.index(org)] += 1
    return node


def test_random_annotations_equal_the_gene_walk():
    rng = np.random.default_rng(20270118)
    done = multi = 0
    for case in range(30):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 30)), int(rng.integers(1, 40)), max_len=25)
        for contigs in ann.values():
            for annot in contigs.values():
                for info in annot.values():
                    start = int(rng.integers(0, 5000))
                    info += [start, start + int(rng.integers(-2, 4)) * 150, "+", "n", "p"]
        o = orders_from_annotations(ann, orgs, circular, repeated)
        if not len(o["genes"]) or o["repeated"][o["genes"]].all():
            continue
        host = build_host(o)
        names = [o["families"][i] for i in host[4]]
        t = table_orders(ann, orgs, o["families"], repeated)
        got = family_table_arrays(host[0], host[4], t["genes"], t["lengths"], t["contig_ptr"], t["contig_org"], t["repeated"])
        node = gene_walk(ann, orgs, names, set(repeated))
        counts = copy_counts(np.asarray(host[0]) != 0, got["multi_ptr"], got["multi_org"], got["multi_cnt"])
        for i, name in enumerate(names):
            v = node[name]
            assert (got["nb_genes"][i], got["nb_org"][i]) == (v["nb"], len(v["cells"])), (case, name)
            assert (got["len_min"][i], got["len_max"][i], got["len_distinct"][i], got["len_sum"][i]) == \
                (min(v["lengths"]), max(v["lengths"]), len(v["lengths"]), sum(v["lengths"])), (case, name)
            assert counts[i].tolist() == [v["cells"].get(c, 0) for c in range(len(orgs))], (case, name)
            text, ends = rtab_cells_host(host[0], got["multi_ptr"], got["multi_org"], got["multi_cnt"], i, 1)
            assert bytes(text).decode() == "\t".join(str(v["cells"].get(c, 0)) for c in range(len(orgs))) + "\n" and ends.tolist() == [len(text)]
        assert (np.diff(got["multi_ptr"]) >= 0).all() and (got["multi_cnt"] >= 2).all()
        done += 1
        multi += len(got["multi_cnt"]) > 0
    assert done >= 20 and multi >= 10


def test_statement_refuses_orders_of_another_master_and_formats_wide_counts():
    rng = np.random.default_rng(5)
    counts = random_counts(rng, 9, 7)
    counts[3, :5] = [9, 10, 99, 100, 1000]
    o = counts_orders(counts, rng)
    x = (counts > 0).astype(np.uint8)
    got = family_table_arrays(x, np.arange(9), o["genes"], o["gene_len"], o["contig_ptr"], o["contig_org"])
    assert np.array_equal(copy_counts(x != 0, got["multi_ptr"], got["multi_org"], got["multi_cnt"]), counts)
    text, ends = rtab_cells_host(x, got["multi_ptr"], got["multi_org"], got["multi_cnt"])
    assert bytes(text).decode() == "".join("\t".join(map(str, row)) + "\n" for row in counts.tolist()) and ends[-1] == len(text)
    flipped = x.copy()
    flipped[0, 0] ^= 1
    for bad_x, genes in ((flipped, o["genes"]), (x, np.where(np.arange(len(o["genes"])) == 0, 9, o["genes"]))):
        with pytest.raises(ValueError, match="not this master's"):
            family_table_arrays(bad_x, np.arange(9), genes, o["gene_len"], o["contig_ptr"], o["contig_org"], f=10)
