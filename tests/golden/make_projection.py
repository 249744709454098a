#!/usr/bin/env python3
"""Generate tests/golden/projection/: what the REAL `projection()` (ppanggolin/ppanggolin.py:1698-1755) writes and
returns for a few small annotation sets whose graph the real `__neighborhood_computation` (:463-530) built -- for one
case a base grown through the real `add_organism` (:342-358) -- and whose nodes carry a labelling written in the case.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case the annotations as lists (organism, contig, (gene, [type, family, start, end, strand, name, product]) in order),
the organisms in column order, the circular contigs, the repeated families, for the grown case which organisms, circular
contigs and repeated families the update brought, the labelling {family: P | S | C | U}, the organisms projected in the
order given, the text of nb_genes.csv and of every organism's file, and the returned means.
tests/test_projection_host.py and tests/test_gpu_projection.py read it.

The reference is run as make_orders.py and make_orders_update.py run it (their stand-in modules, an object made
without __init__).  `partition` comes from the case's labelling; `partition_exact` is set as partition() sets it
(:1133-1148): core_exact for a node that has every organism among its keys, else accessory.

    python tests/golden/make_projection.py
"""
import json
import os
import shutil
import sys
import tempfile
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_orders  # noqa: E402
import make_orders_update  # noqa: E402
from make_orders import RESERVED, reference_class  # noqa: E402

OUT = os.path.join(HERE, "projection")
LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}


def annotations_of(genomes):
    """genomes: [(organism, [(contig, [family | (family, name, product), ...]), ...]), ...] -> PPanGGOLiN's annotations;
    coordinates, strand, name and product differ from gene to gene so that every column of a line is checked"""
    ann = OrderedDict()
    k = 0
    for org, contigs in genomes:
        ann[org] = OrderedDict()
        for contig, fams in contigs:
            ann[org][contig] = OrderedDict()
            for j, fam in enumerate(fams):
                fam, name, product = fam if isinstance(fam, tuple) else (fam, "n" + fam.lower(), "product of " + fam)
                k += 1
                ann[org][contig]["g%d" % k] = ["CDS", fam, 1 + 1000 * j + 7 * k, 900 + 1000 * j + 11 * k, "+-"[(k // 2) % 2], name, product]
    return ann


def run(PPanGGOLiN, cs):
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict
    update = cs.get("update", [])
    both = annotations_of(cs["genomes"] + update)             # (one gene numbering over base and update)
    base_orgs, new_orgs = [o for o, _ in cs["genomes"]], [o for o, _ in update]
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations = OrderedDict((o, both[o]) for o in base_orgs)
    obj.organisms = list(base_orgs)
    obj.families_repeted = list(cs["repeated"])
    obj.circular_contig_size = {c: 100000 for c in cs["circular"]}
    obj.index = {}
    obj.nem_intermediate_files = None
    g = nx.Graph()
    g.node = g.nodes
    obj.neighbors_graph = g
    obj._PPanGGOLiN__neighborhood_computation()
    if update:
        obj.add_organism(list(new_orgs), OrderedDict((o, both[o]) for o in new_orgs), {c: 100000 for c in cs.get("update_circular", [])},
                         list(cs.get("update_repeated", [])))
    organisms = base_orgs + new_orgs
    assert set(cs["labels"]) == set(g.nodes()), (cs["name"], sorted(g.nodes()))
    assert "U" in cs["labels"].values()
    for fam, data in g.nodes(data=True):
        data["partition"] = LONG[cs["labels"][fam]]
        data["partition_exact"] = "core_exact" if sum(1 for key in data if key not in RESERVED) == len(organisms) else "accessory"
    obj.is_partitionned = True
    obj.partitions_by_organism = dict()
    project = cs.get("project", organisms)
    tmp = tempfile.mkdtemp()
    try:
        means = obj.projection(tmp, list(project))
        files = {name: open(os.path.join(tmp, name), newline="").read() for name in sorted(os.listdir(tmp))}
    finally:
        shutil.rmtree(tmp)
    assert sorted(files) == sorted(["nb_genes.csv"] + [o + ".csv" for o in project])
    lists = [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in both[org].items()]] for org in organisms]
    return dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs, annotations=lists, circular=cs["circular"],
                update_circular=cs.get("update_circular", []), repeated=cs["repeated"], update_repeated=cs.get("update_repeated", []),
                labels=cs["labels"], project=list(project), files=files, means=list(means))


def cases():
    out = []
    sets = {cs["name"]: cs for cs in make_orders.cases()}
    labels = dict(repeated=dict(A="P", B="S", C="C", D="U"),
                  circular=dict(A="P", B="P", C="S", D="U", E="C"),
                  duplicates=dict(A="S", B="U", C="P"),
                  late=dict(A="C", B="P", C="S", D="U", Z="S"))
    for name in ("repeated", "circular", "duplicates", "late"):
        out.append(dict(sets[name], labels=labels[name]))
    # R is kept in the base and repeated from the update on: its node and edges stay (a neighbour that still counts), its
    # genes are skipped in every organism, the old ones too
    upd = {cs["name"]: cs for cs in make_orders_update.cases()}["repeated_late"]
    out.append(dict(upd, labels=dict(A="P", R="S", B="U", C="C")))
    # a subset of the organisms, not in column order
    out.append(dict(sets["late"], name="subset", labels=dict(A="P", B="C", C="U", D="S", Z="P"), project=["o3", "o1"]))
    # the `ori` column: a gene named dnaA, one whose product is DnaA, neither
    out.append(dict(name="dnaa", circular=["chr"], repeated=["R"], labels=dict(A="P", B="S", C="U"), genomes=[
        ("o1", [("chr", [("A", "dnaA", "chromosomal replication initiator"), "B", "R", ("C", "x", "DnaA")])]),
        ("o2", [("chr", [("A", "dnaa", "p"), ("B", "dnaA2", "dnaA-like"), "A"]), ("p1", ["C", ("R", "dnaA", "repeated")])])]))
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
