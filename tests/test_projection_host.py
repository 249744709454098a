"""A partition projected onto the organisms, on the host: projection.projection_arrays (the numpy statement of
csrc/nem_project.hip) and Projection.write / means against what the reference's own projection() wrote and returned
(tests/golden/projection/, made by tests/golden/make_projection.py), and, on seeded random annotation sets, against a
per-gene dictionary walk (ppanggolin.py:1713-1743 in the terms of a dict) over the networkx graph that the transcription
of the graph build in tests/test_orders_host.py makes."""
from collections import OrderedDict, defaultdict

import numpy as np
import pytest

from pangenomenem_amd.chunks import master_arrays_from_orders, orders_from_annotations
from pangenomenem_amd.projection import LONG, projection_arrays, shell_q_auto
from tests.orders_util import load, random_genomes
from tests.projection_util import PROJECTION_FIXTURES, fixture_projection_host, random_part, written
from tests.test_orders_host import neighborhood_graph

ids = lambda p: p.split("/")[-1][:-5]


@pytest.mark.parametrize("path", PROJECTION_FIXTURES, ids=ids)
def test_fixture_files_and_means(path, tmp_path):
    rec = load(path)
    proj, ann = fixture_projection_host(rec)
    got = written(proj, ann, tmp_path)
    assert sorted(got) == sorted(rec["files"])
    for name in rec["files"]:
        assert got[name] == rec["files"][name], name
    assert list(proj.means()) == rec["means"]
    assert proj.organisms == rec["project"]


def test_fixtures_cover_the_cases():
    recs = {r["name"]: r for r in map(load, PROJECTION_FIXTURES)}
    assert set(recs) >= {"repeated", "circular", "duplicates", "late", "repeated_late", "subset", "dnaa"}
    assert all("U" in r["labels"].values() for r in recs.values())
    assert recs["repeated_late"]["new_organisms"] and recs["repeated_late"]["update_repeated"]
    assert recs["subset"]["project"] == ["o3", "o1"] and len(recs["subset"]["organisms"]) == 3
    lines = [line.split(",") for name, text in recs["dnaa"]["files"].items() if name != "nb_genes.csv" for line in text.splitlines()[1:]]
    assert {line[5] for line in lines} == {"T", "F"}
    assert any(int(line.split(",")[7]) >= 3 for text in recs["duplicates"]["files"].values() for line in text.splitlines()[1:] if "," in line)


def dictionary_walk(g, ann, project, repeated, labels, n_organisms):
    """projection()'s loop over the graph's dicts: per organism its counters, per gene None (skipped) or its line's
    (family, copies, partition, persistent, shell, cloud neighbours)"""
    import networkx
    per_org, per_gene = OrderedDict(), []
    for org in project:
        counts = defaultdict(int)
        for contig, annot in ann[org].items():
            for gene, info in annot.items():
                fam = info[1]
                if fam in repeated:
                    per_gene.append(None)
                    continue
                node = g.nodes[fam]
                exact = "core_exact" if sum(1 for key in node) == n_organisms else "accessory"     # (the nodes hold organisms only)
                counts[labels[fam]] += 1
                counts[exact] += 1
                counts["pangenome"] += 1
                nei = [labels[b] for b in networkx.all_neighbors(g, fam)]
                per_gene.append((fam, len(node[org]), labels[fam], nei.count("persistent"), nei.count("shell"), nei.count("cloud")))
        per_org[org] = counts
    return per_org, per_gene


def test_random_annotations_equal_the_dictionary_walk():
    rng = np.random.default_rng(20261201)
    done = skipped = copies = loops = subsets = undefined = 0
    for case in range(32):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 12)), int(rng.integers(1, 9)))
        g, (lp, _) = neighborhood_graph(ann, set(circular), set(repeated), False)
        if g.number_of_nodes() == 0:
            continue
        o = orders_from_annotations(ann, orgs, circular, repeated)
        m = master_arrays_from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])
        names = [o["families"][i] for i in m[4]]
        assert names == list(g.nodes())
        part = random_part(rng, len(names))
        labels = {name: LONG[k] for name, k in zip(names, part)}
        project = list(ann)                                   # (walk order, which is not column order)
        if case % 2:
            project = [project[i] for i in rng.permutation(len(project))[:max(1, len(project) // 2)]]
            subsets += 1
        sub = OrderedDict((name, ann[name]) for name in project)
        p = orders_from_annotations(sub, orgs, (), repeated, families=o["families"])
        fam, cop, nei, org = projection_arrays(m, m[4], part, p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"])
        per_org, per_gene = dictionary_walk(g, ann, project, set(repeated), labels, len(orgs))
        assert len(per_gene) == len(fam)
        for q, line in enumerate(per_gene):
            if line is None:
                assert fam[q] == -1 and cop[q] == 0, (case, q)
                skipped += 1
            else:
                i = int(fam[q])
                assert (names[i], int(cop[q]), LONG[part[i]], int(nei[i][0]), int(nei[i][1]), int(nei[i][2])) == line, (case, q)
                copies += line[1] >= 2
        col = {name: c for c, name in enumerate(orgs)}
        want = np.zeros((len(orgs), 7), np.int32)
        for name, counts in per_org.items():
            want[col[name]] = [counts[k] for k in ("persistent", "shell", "cloud", "undefined", "core_exact", "accessory", "pangenome")]
        assert np.array_equal(org, want), case
        done += 1
        loops += lp
        undefined += int(want[:, 3].sum())
    assert done >= 28 and skipped > 50 and copies > 50 and loops > 10 and subsets >= 10 and undefined > 50, (done, skipped, copies, loops, subsets, undefined)


def small():
    """two organisms; family ids 0, 1, 2 kept, 3 repeated, 4 unknown to the master (it has no kept gene in the build)"""
    genes, cptr, corg = [0, 1, 2, 1, 3, 0], [0, 3, 6], [0, 1]
    m = master_arrays_from_orders(genes, cptr, corg, [0, 0], 2, repeated=[0, 0, 0, 1, 0])
    return m, dict(genes=genes, contig_ptr=cptr, contig_org=corg, repeated=[0, 0, 0, 1, 0])


def test_unknown_ids_and_packed_rows():
    from pangenomenem_amd.chunks import pack_rows
    m, o = small()
    part = np.asarray([0, 1, 3], np.uint8)
    fam, cop, nei, org = projection_arrays(m, m[4], part, [0, 4, 3, 1, 4], [0, 2, 2, 5], [1, 0, 0], repeated=o["repeated"])
    assert fam.tolist() == [0, -2, -1, 1, -2] and cop.tolist() == [1, 0, 0, 1, 0]
    assert org.tolist() == [[0, 1, 0, 0, 1, 0, 1], [1, 0, 0, 0, 1, 0, 1]]
    assert nei.tolist() == [[0, 1, 0], [1, 0, 0], [0, 1, 0]]     # rows 0: (1) -- one entry, both organisms carry it; 1: (0, 2); 2: (1)
    packed = (pack_rows(m[0]),) + tuple(m[1:])
    again = projection_arrays(packed, m[4], part, [0, 4, 3, 1, 4], [0, 2, 2, 5], [1, 0, 0], repeated=o["repeated"], d=2)
    assert all(np.array_equal(a, b) for a, b in zip(again, (fam, cop, nei, org)))
    with pytest.raises(ValueError):
        projection_arrays(packed, m[4], part, [0], [0, 1], [0], repeated=o["repeated"])


@pytest.mark.parametrize("field,value", [("genes", [0, 1, 5, 1, 3, 0]), ("genes", [0, -1, 2, 1, 3, 0]), ("contig_ptr", [0, 7, 6]), ("contig_ptr", [1, 3, 6]),
                                         ("contig_ptr", [0, 3, 5]), ("contig_org", [0, 2]), ("contig_org", [-1, 0]), ("repeated", [0, 0]),
                                         ("part", [0, 4, 1]), ("part", [0, 255, 1]), ("part", [0, 1])])
def test_malformed_projection_raises(field, value):
    m, o = small()
    args = dict(o, part=[0, 1, 2])
    projection_arrays(m, m[4], **args)
    with pytest.raises(ValueError):
        projection_arrays(m, m[4], **dict(args, **{field: value}))


def test_shell_q_auto():
    for n_shell, mean_shell in ((0, 3.5), (10, 4.0), (7, 2.0), (5, 2.0), (1234, 81.25), (3, 7.0)):
        assert shell_q_auto(n_shell, mean_shell) == int(round(float(n_shell) / mean_shell, 0)) + 1
    assert shell_q_auto(10, 4.0) == 3 and shell_q_auto(7, 2.0) == 5 and shell_q_auto(5, 2.0) == 3 and shell_q_auto(0, 1.0) == 1


def test_library_refuses_a_null_master_without_a_device():
    from pangenomenem_amd import build
    from pangenomenem_amd.chunks import _bind_master
    from pangenomenem_amd.engine import load_library
    build.build()
    lib = _bind_master(load_library())
    part, ptr = np.zeros(1, np.uint8), np.zeros(1, np.int32)
    assert lib.nemgpu_master_project(None, part.ctypes.data, 1, None, 0, ptr.ctypes.data, None, 0, None, None, None, None, None) == 8


def test_the_two_rule_sets_differ_where_they_did():
    """the projection's orders check and the build's are one function now: what only one of them refuses stays so"""
    from pangenomenem_amd.chunks import _check_orders
    from pangenomenem_amd.projection import check_projection_orders
    # no gene at all: the projection takes it, with and without a contig; the build wants a contig
    genes, ptr, org, rep = check_projection_orders([], [0], [], None, 2, 3)
    assert (genes.dtype, ptr.dtype, org.dtype, rep) == (np.int32, np.int32, np.int32, None) and len(genes) == 0 and list(ptr) == [0]
    assert list(check_projection_orders([], [0, 0], [1], None, 2, 3)[1]) == [0, 0]
    with pytest.raises(ValueError, match="contig_ptr"):
        _check_orders([], [0], [], [], None, 2, 3)
    assert _check_orders([], [0, 0], [1], [0], None, 2, 3)[6] == 3        # (an empty contig is the build's too)
    # the build infers f, the projection is told it; the build returns contig_circular, d and f as well
    out = _check_orders([0, 4, 2], [0, 2, 3], [0, 1], [1, 0], None, 2, None)
    assert len(out) == 7 and out[3].dtype == np.uint8 and out[5:] == (2, 5)
    assert _check_orders([0, 1], [0, 2], [0], [0], [0, 0, 1, 0], 1, None)[6] == 4
    with pytest.raises(ValueError, match="contig_circular"):
        _check_orders([0, 1], [0, 2], [0], [0, 1], None, 1, 2)
    with pytest.raises(ValueError, match=r"contig_org \[C\]$"):
        check_projection_orders([0, 1], [0, 2, 2], [0], None, 1, 2)
    # each one's words for a size that is not positive
    with pytest.raises(ValueError, match="D and F"):
        _check_orders([0], [0, 1], [0], [0], None, 0, 1)
    with pytest.raises(ValueError, match="F must be positive"):
        check_projection_orders([], [0], [], None, 2, 0)
    # both refuse these alike
    for bad in (dict(genes=[0, 3]), dict(genes=[-1, 0]), dict(ptr=[0, 3]), dict(ptr=[1, 2]), dict(org=[2]), dict(org=[-1]), dict(rep=[0, 0])):
        a = dict(genes=[0, 1], ptr=[0, 2], org=[0], rep=None)
        a.update(bad)
        with pytest.raises(ValueError):
            check_projection_orders(a["genes"], a["ptr"], a["org"], a["rep"], 2, 3)
        with pytest.raises(ValueError):
            _check_orders(a["genes"], a["ptr"], a["org"], [0], a["rep"], 2, 3)
