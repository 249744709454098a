#!/usr/bin/env python3
"""Generate tests/golden/orders/: the graph the REAL `__neighborhood_computation` (ppanggolin/ppanggolin.py:463-530, with
its own `__add_gene` and `__add_link`) makes of a few small annotation sets, as a networkx Graph and as a DiGraph.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case the annotations as lists (organism, contig, (gene, family) in order), the circular contigs, the repeated families
and, for the undirected and the directed run, the graph: the nodes in order with their organism keys, every node's
adjacency in order with the per-edge {organism: count}, and for the DiGraph every node's predecessors in order.
tests/test_orders_host.py and tests/test_gpu_orders.py read it.

The reference is run as make_nei_counts.py runs it (stand-in modules for the third-party imports the graph build never
uses, the small OrderedSet); a PPanGGOLiN object is made without its __init__ and given what the method reads:
annotations, families_repeted, circular_contig_size, index and an empty neighbors_graph whose networkx 1.x attribute
`node` points at `nodes`.

    python tests/golden/make_orders.py
"""
import json
import os
import shutil
import sys
import types
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "orders")
RESERVED = {"id", "label", "name", "weight", "partition", "partition_exact", "length", "length_min", "length_max", "length_avg",
            "length_med", "product", "nb_genes", "subpartition_shell", "viz"}


class OrderedSet(list):
    """stands in for ordered_set.OrderedSet (the graph build does not use it)"""


def reference_class():
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


def annotations_of(genomes):
    """genomes: [(organism, [(contig, [family, ...]), ...]), ...] -> PPanGGOLiN's annotations; a gene's info is
    [TYPE, FAMILY, START, END, STRAND, NAME, PRODUCT] (ppanggolin.py:25)"""
    ann = OrderedDict()
    k = 0
    for org, contigs in genomes:
        ann[org] = OrderedDict()
        for contig, fams in contigs:
            ann[org][contig] = OrderedDict()
            for j, fam in enumerate(fams):
                k += 1
                ann[org][contig]["g%d" % k] = ["CDS", fam, 100 * j, 100 * j + 90, "+", fam.lower(), "p_" + fam]
    return ann


def run(PPanGGOLiN, genomes, circular, repeated, directed):
    import networkx as nx
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations = annotations_of(genomes)
    obj.families_repeted = set(repeated)
    obj.circular_contig_size = {c: 100000 for c in circular}
    obj.index = {}
    g = nx.DiGraph() if directed else nx.Graph()
    g.node = g.nodes
    obj.neighbors_graph = g
    obj._PPanGGOLiN__neighborhood_computation(directed=directed)
    counts = lambda data: {k: v for k, v in data.items() if k not in RESERVED}
    rec = dict(nodes=[[f, [k for k in data if k not in RESERVED]] for f, data in g.nodes(data=True)],
               adj=[[a, [[b, counts(g[a][b])] for b in g[a]]] for a in g.nodes()])
    if directed:
        rec["pred"] = [[a, list(g.pred[a])] for a in g.nodes()]
    return rec


def cases():
    out = []
    # a repeated family in the middle, at the start and as a whole contig; several contigs per organism
    out.append(dict(name="repeated", circular=["o2c1"], repeated=["R", "Q"], genomes=[
        ("o1", [("o1c1", ["A", "R", "B", "C"]), ("o1c2", ["R", "Q", "D", "A"]), ("o1c3", ["R", "R"])]),
        ("o2", [("o2c1", ["Q", "B", "R", "R", "A", "D"]), ("o2c2", ["Q"]), ("o2c3", ["C", "R"])]),
        ("o3", [("o3c1", ["D", "C", "Q", "B", "A", "R"])])]))
    # circular contigs of one, two and many kept genes (one of them with a repeated gene at either end)
    out.append(dict(name="circular", circular=["one", "two", "many", "ends", "none"], repeated=["R"], genomes=[
        ("o1", [("one", ["A"]), ("two", ["B", "C"]), ("many", ["A", "B", "C", "D", "E"])]),
        ("o2", [("ends", ["R", "D", "E", "A", "R"]), ("none", ["R"]), ("lin", ["E", "D"])]),
        ("o3", [("one", ["R", "C", "R"]), ("two", ["D", "D"])])]))
    # a tandem duplicate (self-loop), an adjacency occurring twice in one organism and in both orientations
    out.append(dict(name="duplicates", circular=["o3c1"], repeated=[], genomes=[
        ("o1", [("o1c1", ["A", "A", "B", "C", "A", "B"]), ("o1c2", ["B", "A", "C", "C", "C"])]),
        ("o2", [("o2c1", ["B", "A", "B", "A"])]),
        ("o3", [("o3c1", ["C", "A", "A"]), ("o3c2", ["A", "B"])])]))
    # a family first seen late (Z) whose edge predates its neighbour's other edges: B's neighbours are Z, C, A, not A, C, Z
    out.append(dict(name="late", circular=[], repeated=["R"], genomes=[
        ("o1", [("o1c1", ["A"]), ("o1c2", ["B"]), ("o1c3", ["C", "R", "D"])]),
        ("o2", [("o2c1", ["B", "Z", "D"]), ("o2c2", ["C", "B", "A"])]),
        ("o3", [("o3c1", ["A", "C"]), ("o3c2", ["Z", "A", "Z", "B"])])]))
    return out


def main():
    PPanGGOLiN = reference_class()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for cs in cases():
        rec = dict(name=cs["name"], organisms=[org for org, _ in cs["genomes"]],
                   annotations=[[org, [[contig, [[gene, info[1]] for gene, info in annot.items()]] for contig, annot in contigs.items()]]
                                for org, contigs in annotations_of(cs["genomes"]).items()],
                   circular=cs["circular"], repeated=cs["repeated"],
                   undirected=run(PPanGGOLiN, cs["genomes"], cs["circular"], cs["repeated"], False),
                   directed=run(PPanGGOLiN, cs["genomes"], cs["circular"], cs["repeated"], True))
        with open(os.path.join(OUT, cs["name"] + ".json"), "w") as f:
            json.dump(rec, f, indent=0, sort_keys=False)
            f.write("\n")
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
