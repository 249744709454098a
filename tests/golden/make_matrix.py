#!/usr/bin/env python3
"""Generate tests/golden/matrix/: what the REAL `write_matrix()` (ppanggolin/ppanggolin.py:1400-1452), the CLI's
partition-list lines (command_line.py:549-555) and `__str__` (:319-340) write for a few small annotation sets whose graph
the real `__neighborhood_computation` (:463-530) built -- for one case a base grown through the real `add_organism`
(:342-358) -- and whose nodes carry a labelling written in the case.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data -- per
case the annotations as lists (organism, contig, (gene, [type, family, start, end, strand, name, product]) in order),
the organisms in column order, the circular contigs, the repeated families, for the grown case what the update brought,
the labelling {family: P | S | C | U}, and the text of matrix.csv, matrix.Rtab, the six partitions/<name>.txt,
pangenome.txt and the summary.  tests/test_matrix_host.py and tests/test_gpu_matrix.py read it.

The reference is run as make_projection.py runs it (the stand-in modules, an object made without __init__).  `partition`
comes from the case's labelling; pan.partitions is filled as partition() fills it (:1131-1148), walking the nodes; the
CLI's lines that write the lists are read from its file and executed as they stand.

    python tests/golden/make_matrix.py
"""
import json
import os
import shutil
import sys
import tempfile
import textwrap
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_orders  # noqa: E402
import make_orders_update  # noqa: E402
from make_orders import RESERVED, reference_class  # noqa: E402

OUT = os.path.join(HERE, "matrix")
LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
LISTS = ("undefined", "persistent", "shell", "cloud", "core_exact", "accessory")


def annotations_of(genomes):
    """genomes: [(organism, [(contig, [family | (family, length), ...]), ...]), ...] -> PPanGGOLiN's annotations.  A
    gene's length END - START repeats every fourth gene unless the case gives it, so that a family's set of lengths is
    smaller than its genes now and then; products repeat too"""
    ann = OrderedDict()
    k = 0
    for org, contigs in genomes:
        ann[org] = OrderedDict()
        for contig, fams in contigs:
            ann[org][contig] = OrderedDict()
            for j, fam in enumerate(fams):
                k += 1
                fam, length = fam if isinstance(fam, tuple) else (fam, 300 + 33 * (k % 4))
                start = 1 + 1000 * j + 7 * k
                ann[org][contig]["g%d" % k] = ["CDS", fam, start, start + length, "+-"[(k // 2) % 2], "n" + fam.lower(),
                                               "product %d of %s" % (k % 3, fam)]
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
    obj.nb_organisms = len(base_orgs)
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
    assert list(obj.organisms) == organisms and obj.nb_organisms == len(organisms)
    obj.pan_size = g.number_of_nodes()
    assert set(cs["labels"]) == set(g.nodes()), (cs["name"], sorted(g.nodes()))
    obj.partitions = OrderedDict((name, []) for name in LISTS)
    for fam, data in g.nodes(data=True):
        data["partition"] = LONG[cs["labels"][fam]]
        obj.partitions[data["partition"]].append(fam)
        exact = "core_exact" if sum(1 for key in data if key not in RESERVED) == len(organisms) else "accessory"
        data["partition_exact"] = exact
        obj.partitions[exact].append(fam)
    obj.is_partitionned = True
    with open(os.path.join(os.path.dirname(module.__file__), "command_line.py")) as f:
        cli = f.read().splitlines()[548:555]
    assert "pangenome.txt" in cli[0] and "file.close()" in cli[-1]
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(tmp, "partitions"))
        exec(textwrap.dedent("\n".join(cli)), dict(OUTPUTDIR=tmp, PARTITION_DIR="/partitions/", pan=obj))
        obj.write_matrix(tmp + "/matrix")
        files = {}
        for root, _, names in os.walk(tmp):
            for name in names:
                path = os.path.join(root, name)
                files[os.path.relpath(path, tmp)] = open(path, newline="").read()
    finally:
        shutil.rmtree(tmp)
    assert sorted(files) == sorted(["matrix.csv", "matrix.Rtab", "pangenome.txt"] + ["partitions/%s.txt" % name for name in LISTS])
    lists = [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in both[org].items()]] for org in organisms]
    return dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs, annotations=lists, circular=cs["circular"],
                update_circular=cs.get("update_circular", []), repeated=cs["repeated"], update_repeated=cs.get("update_repeated", []),
                labels=cs["labels"], files=files, summary=str(obj))


def cases():
    out = []
    sets = {cs["name"]: cs for cs in make_orders.cases()}
    labels = dict(repeated=dict(A="P", B="S", C="C", D="U"),
                  circular=dict(A="P", B="P", C="S", D="U", E="C"),
                  duplicates=dict(A="S", B="U", C="P"),
                  late=dict(A="C", B="P", C="S", D="U", Z="S"))
    for name in ("repeated", "circular", "duplicates", "late"):
        out.append(dict(sets[name], labels=labels[name]))
    # R is kept in the base and repeated from the update on: its node keeps the genes of the base
    upd = {cs["name"]: cs for cs in make_orders_update.cases()}["repeated_late"]
    out.append(dict(upd, labels=dict(A="P", R="S", B="U", C="C")))
    # a cell of 12 copies next to cells of 1 and 2; E's genes all have one length; a negative and a zero length; no family
    # is persistent (an empty list), A and E are in every organism
    out.append(dict(name="copies", circular=["ring"], repeated=["R"], labels=dict(A="S", B="C", E="S", N="U"), genomes=[
        ("o1", [("c1", ["A"] + ["B"] * 12 + ["A", ("E", 250)]), ("ring", [("E", 250), "R", ("N", -40)])]),
        ("o2", [("c1", ["B", "A", "B", ("E", 250), ("N", 0)])]),
        ("o3", [("c1", ["A", "R", ("E", 250), ("E", 250)]), ("c2", ["R"])])]))
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
