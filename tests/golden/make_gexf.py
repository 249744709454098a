#!/usr/bin/env python3
"""Generate tests/golden/gexf/: what the REAL `export_to_GEXF()` (ppanggolin/ppanggolin.py:1294-1362) and networkx's
write_gexf write, full and light, and the three series of `ushaped_plot` (:1486-1523), for a few small annotation sets
whose graph the real `__neighborhood_computation` (:463-530) built -- for one case a base grown through the real
`add_organism` (:342-358) -- and whose nodes carry a labelling written in the case as partition() writes it (:1131-1157),
`viz` included.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case the annotations as lists (organism, contig, (gene, [type, family, start, end, strand, name, product]) in order),
the organisms in column order, the circular contigs' sizes, the repeated families, for the grown case what the update
brought, the labelling {family: P | S | C | U}, the text of the two files and the three series.
tests/test_gexf_host.py and tests/test_gpu_gexf.py read it.

The reference is run as make_matrix.py runs it (the stand-in modules, an object made without __init__).  The graph is a
subclass of nx.Graph with the networkx 1.x attribute `node` as a property, so that it survives the copy()
export_to_GEXF makes.  Lines 1494-1507 of ushaped_plot are read from the reference's file and executed as they stand.

    python tests/golden/make_gexf.py
"""
import json
import os
import shutil
import sys
import tempfile
import textwrap
from collections import OrderedDict, defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_matrix  # noqa: E402
from make_orders import RESERVED, reference_class  # noqa: E402

OUT = os.path.join(HERE, "gexf")
LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
SIZE = 100000                                                 # a circular contig's size where the case gives none


def explicit_annotations(genomes):
    """genomes: [(organism, [(contig, [(family, start, end), ...]), ...]), ...] -> PPanGGOLiN's annotations"""
    ann = OrderedDict()
    k = 0
    for org, contigs in genomes:
        ann[org] = OrderedDict()
        for contig, genes in contigs:
            ann[org][contig] = OrderedDict()
            for fam, start, end in genes:
                k += 1
                ann[org][contig]["g%d" % k] = ["CDS", fam, start, end, "+-"[k % 2], "n" + fam.lower(), "product %d of %s" % (k % 2, fam)]
    return ann


def run(PPanGGOLiN, cs):
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict

    class NodeGraph(nx.Graph):
        node = property(lambda self: self.nodes)

    update = cs.get("update", [])
    make = explicit_annotations if cs.get("explicit") else make_matrix.annotations_of
    both = make(cs["genomes"] + update)                       # (one gene numbering over base and update)
    base_orgs, new_orgs = [o for o, _ in cs["genomes"]], [o for o, _ in update]
    sizes = dict({c: SIZE for c in cs["circular"]}, **cs.get("sizes", {}))
    update_sizes = {c: SIZE for c in cs.get("update_circular", [])}
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations = OrderedDict((o, both[o]) for o in base_orgs)
    obj.organisms = list(base_orgs)
    obj.nb_organisms = len(base_orgs)
    obj.families_repeted = list(cs["repeated"])
    obj.circular_contig_size = dict(sizes)
    obj.index = {}
    obj.nem_intermediate_files = None
    g = NodeGraph()
    obj.neighbors_graph = g
    obj._PPanGGOLiN__neighborhood_computation()
    if update:
        obj.add_organism(list(new_orgs), OrderedDict((o, both[o]) for o in new_orgs), dict(update_sizes), list(cs.get("update_repeated", [])))
    organisms = base_orgs + new_orgs
    assert list(obj.organisms) == organisms and obj.nb_organisms == len(organisms)
    assert set(cs["labels"]) == set(g.nodes()), (cs["name"], sorted(g.nodes()))
    for fam, data in g.nodes(data=True):                      # partition(), :1131-1157
        nb_orgs = sum(1 for key in data if key not in RESERVED)
        data["partition"] = LONG[cs["labels"][fam]]
        data["partition_exact"] = "core_exact" if nb_orgs == len(organisms) else "accessory"
        data["viz"] = {}
        data["viz"]["color"] = module.COLORS_RGB[data["partition"] if cs["labels"][fam] != "U" else data["partition_exact"]]
        data["viz"]["size"] = nb_orgs
    obj.is_partitionned = True
    with open(module.__file__) as f:
        lines = f.read().splitlines()[1493:1507]
    assert "count = defaultdict" in lines[0] and "cloud_values.append" in lines[-1]
    scope = dict(self=obj, defaultdict=defaultdict)
    exec(textwrap.dedent("\n".join(lines)), scope)
    tmp = tempfile.mkdtemp()
    try:
        obj.export_to_GEXF(tmp + "/full")
        obj.export_to_GEXF(tmp + "/light", all_node_attributes=False, all_edge_attributes=False)
        full = open(tmp + "/full.gexf", newline="", encoding="utf-8").read()
        light = open(tmp + "/light.gexf", newline="", encoding="utf-8").read()
    finally:
        shutil.rmtree(tmp)
    lists = [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in both[org].items()]] for org in organisms]
    return dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs, annotations=lists, circular=sizes, update_circular=update_sizes,
                repeated=cs["repeated"], update_repeated=cs.get("update_repeated", []), labels=cs["labels"], gexf=full, gexf_light=light,
                ushape=[scope["persistent_values"], scope["shell_values"], scope["cloud_values"]])


def cases():
    out = make_matrix.cases()
    # one small case with every kind of link.  o1's first contig is one gene of A on a linear contig: A's first link,
    # the graph's first edge, comes with o2, and o1 is first met on a later edge (C, D) -- the edge attribute ids are not
    # in column order.  o1's C and D overlap (length -50).  o2's R is repeated and bridged over (A - B).  ring2 is
    # circular with two kept genes: B - C twice, lengths 10 and 705, median 357.5.  ring1 is circular with one kept
    # gene: a self-loop of E, whose name and product need escaping.  o3 has C - D twice more (the edge has three distinct
    # lengths) and a tandem pair of B (the other kind of self-loop).
    nasty = 'E&<"q>'
    out.append(dict(name="links", explicit=True, circular=["ring1", "ring2"], sizes=dict(ring1=5000, ring2=1000), repeated=["R"],
                    labels={"A": "P", "B": "S", "C": "C", "D": "U", nasty: "P"}, genomes=[
        ("o1", [("c1", [("A", 0, 100)]), ("c2", [("C", 0, 300), ("D", 250, 500)])]),
        ("o2", [("c1", [("A", 10, 110), ("R", 200, 300), ("B", 400, 500)]), ("ring2", [("B", 105, 200), ("C", 210, 400)])]),
        ("o3", [("ring1", [(nasty, 100, 400)]), ("c2", [("D", 0, 90), ("C", 100, 200), ("D", 300, 390)]), ("c3", [("B", 0, 10), ("B", 20, 30)])])]))
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
