#!/usr/bin/env python3
"""Generate tests/golden/orders_update/: the nx.Graph the REAL `add_organism` (ppanggolin/ppanggolin.py:342-358) leaves
after a base graph built by `__neighborhood_computation` (:463-530) is grown by new organisms -- the graph kept,
families_repeted united, `__neighborhood_computation(False, update=new_orgs)` walking the new organisms alone.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case the base annotations and the update's (organism, contig, (gene, family) in order), both sets of circular contigs,
the base's repeated families and the ones the update adds, and the final graph in the format of tests/golden/orders/
(nodes in order with their organism keys, every node's adjacency in order with the per-edge {organism: count}).
tests/test_master_append_host.py and tests/test_gpu_master_append.py read it.

The reference is run as make_orders.py runs it (its stand-in modules, an object made without __init__); `add_organism`
itself is called: `bidict` stands in as a dict (it only receives the gene index), families_repeted is a list (the
method concatenates it) and nem_intermediate_files is None.

    python tests/golden/make_orders_update.py
"""
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_orders import RESERVED, annotations_of, reference_class  # noqa: E402

OUT = os.path.join(HERE, "orders_update")


def run(PPanGGOLiN, cs):
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    both = annotations_of(cs["genomes"] + cs["update"])       # (one gene numbering over base and update)
    base_orgs, new_orgs = [o for o, _ in cs["genomes"]], [o for o, _ in cs["update"]]
    obj.annotations = type(both)((o, both[o]) for o in base_orgs)
    obj.organisms = list(base_orgs)
    obj.families_repeted = list(cs["repeated"])
    obj.circular_contig_size = {c: 100000 for c in cs["circular"]}
    obj.index = {}
    obj.nem_intermediate_files = None
    g = nx.Graph()
    g.node = g.nodes
    obj.neighbors_graph = g
    obj._PPanGGOLiN__neighborhood_computation()
    base_nodes = g.number_of_nodes()
    obj.add_organism(list(new_orgs), type(both)((o, both[o]) for o in new_orgs), {c: 100000 for c in cs["update_circular"]},
                     list(cs["update_repeated"]))
    assert obj.neighbors_graph is g and obj.organisms == base_orgs + new_orgs
    counts = lambda data: {k: v for k, v in data.items() if k not in RESERVED}
    graph = dict(nodes=[[f, [k for k in data if k not in RESERVED]] for f, data in g.nodes(data=True)],
                 adj=[[a, [[b, counts(g[a][b])] for b in g[a]]] for a in g.nodes()])
    lists = lambda orgs: [[org, [[contig, [[gene, info[1]] for gene, info in annot.items()]] for contig, annot in both[org].items()]]
                          for org in orgs]
    return dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs, annotations=lists(base_orgs),
                update_annotations=lists(new_orgs), circular=cs["circular"], update_circular=cs["update_circular"],
                repeated=cs["repeated"], update_repeated=cs["update_repeated"], base_nodes=base_nodes, undirected=graph)


def cases():
    out = []
    # new counts on old edges (A-B, B-C), new edges at row ends, new families (X, Y); D's row ends C, E, A and A's ends
    # ..., Y, X (Y is numbered after X): neighbour order not sorted
    out.append(dict(name="grow", circular=[], repeated=[], update_circular=[], update_repeated=[], genomes=[
        ("o1", [("o1c1", ["A", "B", "C", "D", "E"])]),
        ("o2", [("o2c1", ["A", "C", "B"]), ("o2c2", ["E", "D"])])],
        update=[
        ("o3", [("o3c1", ["X", "B", "A", "B", "C"]), ("o3c2", ["Y", "A", "X"]), ("o3c3", ["D", "A"])]),
        ("o4", [("o4c1", ["C", "B", "A", "Y"]), ("o4c2", ["E", "X", "E"])])]))
    # R is kept in the base and repeated from the update on: its node and edges stay, its new genes are bridged over
    out.append(dict(name="repeated_late", circular=["o2c1"], repeated=[], update_circular=["o3c2"], update_repeated=["R"], genomes=[
        ("o1", [("o1c1", ["A", "R", "B"])]),
        ("o2", [("o2c1", ["B", "R", "C"])])],
        update=[
        ("o3", [("o3c1", ["A", "R", "C", "R", "R", "B"]), ("o3c2", ["R", "C", "A", "R"]), ("o3c3", ["R"])])]))
    # Z and W absent from the base and kept in the update; Q repeated in both: it never exists; S has genes only in the
    # update, which also declares it repeated: it never exists either
    out.append(dict(name="unseen", circular=[], repeated=["Q"], update_circular=["o3c1"], update_repeated=["S"], genomes=[
        ("o1", [("o1c1", ["A", "Q", "B"]), ("o1c2", ["Q", "Q"])]),
        ("o2", [("o2c1", ["B", "A", "Q"])])],
        update=[
        ("o3", [("o3c1", ["Q", "Z", "A", "Q", "S", "B", "W"]), ("o3c2", ["S", "Q"]), ("o3c3", ["W", "Q", "Z"])])]))
    # circular contigs of one and two kept genes, a tandem self-loop, and A-B three times in the new organism on an edge
    # that has an extra already (twice in o1)
    out.append(dict(name="circular_dup", circular=["ring"], repeated=["R"], update_circular=["one", "two", "ring"], update_repeated=[], genomes=[
        ("o1", [("o1c1", ["A", "A", "B"]), ("o1c2", ["B", "A", "C"]), ("ring", ["C", "C"])]),
        ("o2", [("o2c1", ["C", "A"])])],
        update=[
        ("o3", [("one", ["R", "A", "R"]), ("two", ["B", "C"]), ("o3c3", ["A", "A", "B", "A", "B"]), ("ring", ["D", "A", "A"])]),
        ("o4", [("two", ["D", "D"]), ("o4c2", ["B", "A"])])]))
    return out


def main():
    PPanGGOLiN = reference_class()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for cs in cases():
        with open(os.path.join(OUT, cs["name"] + ".json"), "w") as f:
            json.dump(run(PPanGGOLiN, cs), f, indent=0, sort_keys=False)
            f.write("\n")
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
