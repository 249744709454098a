#!/usr/bin/env python3
"""Generate tests/golden/gexf_metadata/: what the REAL `export_to_GEXF(path, False, metadata[, False, False])`
(ppanggolin/ppanggolin.py:1294-1362, the metadata lines :1339-1354) and networkx's write_gexf write, full and light, for
a few of the cases of make_gexf.py / make_matrix.py with a metadata dict as the CLI makes it from its -mt file
(command_line.py:439-447, 487): {organism: ordered {attribute: str}}.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case what make_gexf.py stores (without the U-shaped plot's series), the metadata as a list (organism, [(attribute,
value), ...]) in order, and the text of the two files.  tests/test_gexf_metadata_host.py and
tests/test_gpu_gexf_metadata.py read it.

The graph is built and labelled as make_gexf.py builds and labels it (its case builders are imported, not changed).

    python tests/golden/make_gexf_metadata.py
"""
import json
import os
import shutil
import sys
import tempfile
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_gexf  # noqa: E402
import make_matrix  # noqa: E402
from make_orders import RESERVED, reference_class  # noqa: E402

OUT = os.path.join(HERE, "gexf_metadata")


def run(PPanGGOLiN, cs):
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict

    class NodeGraph(nx.Graph):
        node = property(lambda self: self.nodes)

    update = cs.get("update", [])
    make = make_gexf.explicit_annotations if cs.get("explicit") else make_matrix.annotations_of
    both = make(cs["genomes"] + update)
    base_orgs, new_orgs = [o for o, _ in cs["genomes"]], [o for o, _ in update]
    sizes = dict({c: make_gexf.SIZE for c in cs["circular"]}, **cs.get("sizes", {}))
    update_sizes = {c: make_gexf.SIZE for c in cs.get("update_circular", [])}
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
    assert list(obj.organisms) == organisms
    for fam, data in g.nodes(data=True):                      # partition(), :1131-1157
        nb_orgs = sum(1 for key in data if key not in RESERVED)
        data["partition"] = make_gexf.LONG[cs["labels"][fam]]
        data["partition_exact"] = "core_exact" if nb_orgs == len(organisms) else "accessory"
        data["viz"] = {}
        data["viz"]["color"] = module.COLORS_RGB[data["partition"] if cs["labels"][fam] != "U" else data["partition_exact"]]
        data["viz"]["size"] = nb_orgs
    obj.is_partitionned = True
    rows = cs["metadata"]
    assert [org for org, _ in rows] == organisms
    metadata = OrderedDict((org, OrderedDict(pairs)) for org, pairs in rows)      # command_line.py:447, 487
    tmp = tempfile.mkdtemp()
    try:
        obj.export_to_GEXF(tmp + "/full", False, metadata)
        obj.export_to_GEXF(tmp + "/light", False, metadata, False, False)
        full = open(tmp + "/full.gexf", newline="", encoding="utf-8").read()
        light = open(tmp + "/light.gexf", newline="", encoding="utf-8").read()
    finally:
        shutil.rmtree(tmp)
    lists = [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in both[org].items()]] for org in organisms]
    return dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs, annotations=lists, circular=sizes, update_circular=update_sizes,
                repeated=cs["repeated"], update_repeated=cs.get("update_repeated", []), labels=cs["labels"],
                metadata=[[org, [list(pair) for pair in pairs]] for org, pairs in rows], gexf=full, gexf_light=light)


def cases():
    by_name = {cs["name"]: cs for cs in make_gexf.cases()}
    # two attributes: a value shared by two organisms and an empty one; a value that needs escaping and a multi-byte
    # one that holds the separator itself
    links = dict(by_name["links"], metadata=[("o1", [("country", "fr"), ("host", 'pig&"x"')]),
                                             ("o2", [("country", ""), ("host", "Åb|c")]),
                                             ("o3", [("country", "fr"), ("host", "cow")])])
    # a base grown through add_organism: every organism another value, and one of two
    grown = dict(by_name["repeated_late"], metadata=[("o1", [("site", "soil"), ("clade", "b")]),
                                                     ("o2", [("site", "gut <1>"), ("clade", "a")]),
                                                     ("o3", [("site", "air"), ("clade", "b")])])
    # one attribute with one value for all
    one = dict(by_name["circular"], metadata=[(org, [("kingdom", "Bacteria")]) for org in ("o1", "o2", "o3")])
    return [links, grown, one]


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
