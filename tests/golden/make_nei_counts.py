#!/usr/bin/env python3
"""Generate tests/golden/nei_counts/: what the REAL `__write_nem_input_files` (ppanggolin/ppanggolin.py:821-930) writes
for a few small pangenome graphs built through the REAL `__add_link` (:435-459), in which adjacencies occur more than
once per organism: tandem self-loops, an adjacency repeated within one organism, an edge carried in both directions,
as a networkx Graph and as a DiGraph.

Runs only in the build container (where the reference tree and networkx exist); nothing of the reference travels:
what is stored is data -- per case the graph (node data keys, per-edge {organism: count}, directedness), the ordered
samples and, per sample, the `.index`, `.dat` and `.nei` text the reference wrote.  tests/test_nei_counts.py reads it.

How the reference is run here, as make_pypins.py does it: the third-party modules ppanggolin.py imports but the writer
never uses (bidict, fa2, highcharts, nem) are empty stand-ins in sys.modules, and `ordered_set.OrderedSet` is the small
list-backed ordered set below; sys.dont_write_bytecode keeps the read-only reference tree untouched.  A PPanGGOLiN
object is made without its __init__ and given an empty neighbors_graph; node data is set through graph.nodes[f][org]
(the reference's __add_gene uses the networkx 1.x `graph.node` API).

    python tests/golden/make_nei_counts.py
"""
import json
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nei_counts")


class OrderedSet:
    """the few operations of ordered_set.OrderedSet that __write_nem_input_files uses, over a list"""

    def __init__(self, items=()):
        self._items = []
        self._set = set()
        for it in items:
            self.add(it)

    def add(self, it):
        if it not in self._set:
            self._set.add(it)
            self._items.append(it)

    def __contains__(self, it):
        return it in self._set

    def __iter__(self):
        return iter(self._items)

    def __len__(self):
        return len(self._items)

    def isdisjoint(self, other):
        return all(it not in self._set for it in other)


def reference_writer():
    for name, attr in (("bidict", "bidict"), ("fa2", "ForceAtlas2"), ("highcharts", "Highchart")):
        stub = types.ModuleType(name)
        setattr(stub, attr, type(attr, (), {}))
        sys.modules[name] = stub
    osm = types.ModuleType("ordered_set")
    osm.OrderedSet = OrderedSet
    sys.modules["ordered_set"] = osm
    nem = types.ModuleType("nem")
    nem.__all__ = []
    sys.modules["nem"] = nem
    sys.dont_write_bytecode = True
    sys.path.insert(0, "/root/reference")
    from ppanggolin.ppanggolin import PPanGGOLiN
    return PPanGGOLiN


def build(PPanGGOLiN, directed, families, genomes):
    """genomes: {organism: [contig, ...]}, a contig = the families of its genes in order; a circular contig's last gene
    is linked to its first.  Every consecutive pair goes through __add_link, as __neighborhood_computation does."""
    import networkx as nx
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    g = nx.DiGraph() if directed else nx.Graph()
    obj.neighbors_graph = g
    for f in families:
        g.add_node(f)
    gene = 0
    for org, contigs in genomes.items():
        for contig, circular in contigs:
            for f in contig:
                gene += 1
                node = g.nodes[f]
                node.setdefault(org, set()).add("g%d" % gene)
                node["nb_genes"] = node.get("nb_genes", 0) + 1
                for attr, val in (("name", f.lower()), ("length", 300 + gene % 7), ("product", "p_" + f)):
                    node.setdefault(attr, set()).add(val)
            pairs = list(zip(contig[:-1], contig[1:])) + ([(contig[-1], contig[0])] if circular else [])
            for k, (a, b) in enumerate(pairs):
                obj._PPanGGOLiN__add_link(a, b, org, 10 + k)
    return obj


def cases():
    fam = ["A", "B", "C", "D", "E", "F"]
    g1 = {                                                  # tandem A A, A-B twice in one organism, B-A carried backwards
        "org1": [(["A", "A", "B", "C"], False), (["C", "B", "A"], False)],
        "org2": [(["A", "B", "C", "D"], True)],
        "org3": [(["B", "A", "A", "A", "B"], False), (["E", "F"], False)],
        "org4": [(["D", "E", "F", "D", "E"], False)],
        "org5": [(["C", "C", "D"], False), (["A", "B"], False)],
        "org6": [(["F", "E", "E", "D"], False)],
    }
    three = {"o1": [(["A", "B", "A", "B", "C", "C"], False)], "o2": [(["B", "A", "C"], False)], "o3": [(["C", "A", "A"], True)]}
    orgs = list(g1)
    samples = [orgs, ["org3", "org1", "org5"], ["org6", "org2", "org4", "org1"], ["org4"], ["org2", "org3"]]
    return [dict(name="graph6", directed=False, families=fam, genomes=g1, samples=samples),
            dict(name="digraph6", directed=True, families=fam, genomes=g1, samples=samples),
            dict(name="graph3", directed=False, families=fam[:3], genomes=three, samples=[list(three), ["o3", "o1"]]),
            dict(name="digraph3", directed=True, families=fam[:3], genomes=three, samples=[list(three), ["o2", "o3"]])]


def jsonable(v):
    return sorted(v) if isinstance(v, set) else v


def main():
    PPanGGOLiN = reference_writer()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for cs in cases():
        obj = build(PPanGGOLiN, cs["directed"], cs["families"], cs["genomes"])
        g = obj.neighbors_graph
        rec = dict(name=cs["name"], directed=cs["directed"],
                   nodes=[[f, {k: jsonable(v) for k, v in data.items()}] for f, data in g.nodes(data=True)],
                   edges=[[a, b, {k: jsonable(v) for k, v in data.items()}] for a, b, data in g.edges(data=True)],
                   samples=[])
        for sample in cs["samples"]:
            tmp = tempfile.mkdtemp(prefix="neicounts_")
            obj._PPanGGOLiN__write_nem_input_files(tmp, OrderedSet(sample))
            files = {}
            for ext in ("index", "dat", "nei"):
                with open(os.path.join(tmp, "nem_file." + ext)) as f:
                    files[ext] = f.read()
            rec["samples"].append(dict(organisms=sample, **files))
            shutil.rmtree(tmp)
        with open(os.path.join(OUT, cs["name"] + ".json"), "w") as f:
            json.dump(rec, f, indent=0, sort_keys=False)
            f.write("\n")
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
