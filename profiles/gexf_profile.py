#!/usr/bin/env python3
"""Times for profiles/gexf.md: the GEXF export of one synthetic pangenome (synth.annotated_pangenome), either by the
reference (--reference: the real __neighborhood_computation builds the graph, the real export_to_GEXF writes it; needs
the reference tree and networkx, as the generators under tests/golden/ do) or from the resident master (--device:
Master.from_annotations, family_table, edge_table, write_gexf; needs the GPU).  Both label a family persistent above
0.9 d organisms, cloud below 0.1 d, shell between.  --metadata: three metadata attributes of 2, 20 and 200 distinct
values (export_to_GEXF's metadata=, write_gexf's metadata=) -- the exports are timed with and, on the device, also
without them, and the device's metadata lines of all the edges on their own.  --nodes: the export from the loader's flat
form (needs the GPU), through Loaded.annotations() and through Master.node_table.  Prints one JSON line.

    python profiles/gexf_profile.py --n 2000 --d 200 --seed 11 --device --runs 3
    python profiles/gexf_profile.py --n 2000 --d 200 --seed 11 --nodes --runs 5
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from pangenomenem_amd.synth import annotated_pangenome  # noqa: E402


def label(nb_org, d):
    return "P" if nb_org > 0.9 * d else "C" if nb_org < 0.1 * d else "S"


def metadata_of(orgs):
    """{organism: {attribute: value}}: 2, 20 and 200 distinct values (as far as there are organisms)"""
    return {org: {"clade": "clade%d" % (i % 2), "country": "country %d" % (i % 20), "isolate": "isolate-%03d" % (i % 200)} for i, org in enumerate(orgs)}


def timed(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def reference(ann, orgs, circular, runs, tmp, metadata=False):
    sys.path.insert(0, os.path.join(HERE, "..", "tests", "golden"))
    from make_orders import RESERVED, reference_class
    PPanGGOLiN = reference_class()
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict
    module.tqdm = lambda it, **kw: type("quiet", (), dict(__iter__=lambda s: iter(it), set_description=lambda s, t: None, refresh=lambda s: None))()

    class NodeGraph(nx.Graph):
        node = property(lambda self: self.nodes)

    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations, obj.organisms, obj.nb_organisms = ann, list(orgs), len(orgs)
    obj.families_repeted, obj.circular_contig_size, obj.index, obj.nem_intermediate_files = [], dict(circular), {}, None
    obj.neighbors_graph = g = NodeGraph()
    t0 = time.perf_counter()
    obj._PPanGGOLiN__neighborhood_computation()
    build = time.perf_counter() - t0
    long = {"P": "persistent", "S": "shell", "C": "cloud"}
    for fam, data in g.nodes(data=True):
        nb = sum(1 for key in data if key not in RESERVED)
        data["partition"] = long[label(nb, len(orgs))]
        data["partition_exact"] = "core_exact" if nb == len(orgs) else "accessory"
        data["viz"] = dict(color=module.COLORS_RGB[data["partition"]], size=nb)
    obj.is_partitionned = True
    meta = metadata_of(orgs) if metadata else None
    full = timed(lambda: obj.export_to_GEXF(tmp + "/ref", False, meta), runs)
    light = timed(lambda: obj.export_to_GEXF(tmp + "/ref_light", False, meta, all_node_attributes=False, all_edge_attributes=False), runs)
    return dict(who="reference", metadata=bool(metadata), families=g.number_of_nodes(), edges=g.number_of_edges(), graph_build_s=build, export_full_s=full, export_light_s=light,
                full_bytes=os.path.getsize(tmp + "/ref.gexf"), light_bytes=os.path.getsize(tmp + "/ref_light.gexf"))


def device(ann, orgs, circular, runs, tmp, metadata=False):
    from pangenomenem_amd.chunks import Master
    from pangenomenem_amd.gexf import LENGTH_TITLES, gexf_orders, rank_metadata, write_gexf
    m = Master.from_annotations(ann, orgs, list(circular))
    ft = m.family_table(ann)
    labels = {name: label(int(nb), len(orgs)) for name, nb in zip(m.names, ft.nb_org)}
    m.edge_table(ann, (), circular).close()                   # (warm-up)
    tables = []
    table = timed(lambda: tables.append(m.edge_table(ann, (), circular)), runs)
    et = tables[-1]
    for t in tables[:-1]:
        t.close()
    o = gexf_orders(ann, orgs, m.id_names, {org: frozenset() for org in orgs}, circular)
    tables = []
    flat = timed(lambda: tables.append(m.edge_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]), starts=o["starts"],
                                                    ends=o["ends"], contig_sizes=o["contig_sizes"])), runs)
    for t in tables:
        t.close()
    attr_id, _ = et.attribute_ids(100)

    def text():
        return sum(len(et.attvalues(attr_id, row0, rows)[0]) for row0, rows in et._batches(64 << 20))

    text_bytes = text()
    lines = timed(text, runs)
    full = timed(lambda: write_gexf(tmp + "/dev", labels, ft, et, ann), runs)
    light = timed(lambda: write_gexf(tmp + "/dev_light", labels, ft, et, ann, all_node_attributes=False, all_edge_attributes=False), runs)
    out = dict(who="device", families=m.n, edges=et.n_edges, edge_table_from_annotations_s=table, edge_table_from_flat_orders_s=flat,
               attvalue_text_bytes=text_bytes, attvalue_text_s=lines, write_full_s=full, write_light_s=light,
               full_bytes=os.path.getsize(tmp + "/dev.gexf"), light_bytes=os.path.getsize(tmp + "/dev_light.gexf"))
    if metadata:
        meta = metadata_of(orgs)
        write_gexf(tmp + "/dev_meta", labels, ft, et, ann, metadata=meta)             # (warm-up: the three kernels' code)
        out["write_full_metadata_s"] = timed(lambda: write_gexf(tmp + "/dev_meta", labels, ft, et, ann, metadata=meta), runs)
        out["write_light_metadata_s"] = timed(lambda: write_gexf(tmp + "/dev_meta_light", labels, ft, et, ann, all_node_attributes=False,
                                                                 all_edge_attributes=False, metadata=meta), runs)
        out["write_full_again_s"] = timed(lambda: write_gexf(tmp + "/dev", labels, ft, et, ann), runs)          # (alternated with the above)
        out["write_light_again_s"] = timed(lambda: write_gexf(tmp + "/dev_light", labels, ft, et, ann, all_node_attributes=False,
                                                              all_edge_attributes=False), runs)
        out["rank_metadata_s"] = timed(lambda: rank_metadata(meta, orgs, ("weight",) + LENGTH_TITLES), runs)
        out["metavalue_text_bytes"] = len(et.metavalues()[0])
        out["metavalue_text_s"] = timed(lambda: et.metavalues(), runs)                # (one call, all edges; the text comes down)
        out["metamasks_s"] = timed(lambda: et.metamasks(), runs)
        out.update(full_metadata_bytes=os.path.getsize(tmp + "/dev_meta.gexf"), light_metadata_bytes=os.path.getsize(tmp + "/dev_meta_light.gexf"))
    et.close()
    ft.close()
    m.close()
    return out


def flat_load(ann, orgs, families, circular):
    """the annotations in the loader's flat form: a loader.Loaded with one text per organism that holds, per gene, its id,
    name, product, strand and contig name, and the spans into it -- what Master.from_files keeps, without the GFF columns"""
    import numpy as np
    from pangenomenem_amd.gexf import gexf_orders
    from pangenomenem_amd.loader import Loaded
    o = gexf_orders(ann, orgs, families, {org: frozenset() for org in orgs}, circular)
    files, base, off, length, coff, clen, at = [], [], [[], [], [], []], [[], [], [], []], [], [], 0
    for contigs in ann.values():
        parts, here = [], 0
        for contig, annot in contigs.items():
            coff.append(at + here)
            clen.append(len(contig.encode()))
            parts.append(contig.encode() + b"\t")
            here += clen[-1] + 1
            for gene, info in annot.items():
                for j, piece in enumerate((gene, info[5], info[6], info[4])):
                    piece = piece.encode()
                    off[j].append(at + here)
                    length[j].append(len(piece))
                    parts.append(piece + b"\t")
                    here += len(piece) + 1
        files.append(b"".join(parts)[:-1] if parts else b"")
        base.append(at)
        at += len(files[-1]) + 1
    o.update(families=list(families), organisms=list(orgs), d=len(orgs), lengths=(o["ends"].astype(np.int64) - o["starts"]).astype(np.int32))
    return Loaded(list(orgs), files, np.asarray(base, np.int64), o, list(families), set(), dict(circular),
                  (np.asarray(off, np.int64), np.asarray(length, np.int32)), (np.asarray(coff, np.int64), np.asarray(clen, np.int32)))


def nodes(ann, orgs, circular, runs, tmp, metadata=False):
    """write_gexf from the loader's flat form, through Loaded.annotations() (the walk that builds the nested dict is counted)
    and through Master.node_table (the second upload and the table's creation are counted); then node_table() alone and
    lines() over all nodes.  The family and edge tables are made from the flat orders once, for both."""
    from pangenomenem_amd.chunks import Master
    from pangenomenem_amd.gexf import write_gexf
    m = Master.from_annotations(ann, orgs, list(circular))
    ld = flat_load(ann, orgs, m.id_names, circular)
    o = ld.orders
    orders = (o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"])
    ft = m.family_table(orders=orders, lengths=o["lengths"])
    et = m.edge_table(orders=orders, starts=o["starts"], ends=o["ends"], contig_sizes=o["contig_sizes"])
    labels = {name: label(int(nb), len(orgs)) for name, nb in zip(m.names, ft.nb_org)}
    light = dict(all_node_attributes=False, all_edge_attributes=False)

    def old(path, **kw):
        write_gexf(path, labels, ft, et, ld.annotations(), **kw)

    def new(path, **kw):
        nt = m.node_table(ld)
        write_gexf(path, labels, ft, et, node_table=nt, **kw)
        nt.close()

    old(tmp + "/old")                                         # (warm-up of both paths, and the two files to compare)
    new(tmp + "/new")
    same = open(tmp + "/old.gexf", "rb").read() == open(tmp + "/new.gexf", "rb").read()
    out = dict(who="nodes", families=m.n, edges=et.n_edges, text_bytes=sum(len(f) + 1 for f in ld._files), same_bytes=same,
               full_bytes=os.path.getsize(tmp + "/new.gexf"))
    for _ in range(2):                                        # (alternated)
        for name, fn, kw in (("annotations_full_s", old, {}), ("node_table_full_s", new, {}), ("annotations_light_s", old, light),
                             ("node_table_light_s", new, light)):
            out.setdefault(name, []).extend(timed(lambda: fn(tmp + "/" + name, **kw), runs))
    out["annotations_walk_s"] = timed(ld.annotations, runs)
    tables = []
    out["node_table_s"] = timed(lambda: tables.append(m.node_table(ld)), runs)
    nt = tables[-1]
    nt.titles()
    out["node_text_bytes"] = nt.lines_size()
    out["lines_all_nodes_s"] = timed(lambda: [nt.lines(row0, rows) for row0, rows in nt._batches(64 << 20)], runs)
    out["lines_all_nodes_light_s"] = timed(lambda: [nt.lines(row0, rows, False) for row0, rows in nt._batches(64 << 20, False)], runs)
    for t in tables + [ft, et]:
        t.close()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--d", type=int, default=200)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--metadata", action="store_true")
    ap.add_argument("--nodes", action="store_true")
    args = ap.parse_args()
    ann, orgs, circular = annotated_pangenome(args.n, args.d, args.seed)
    genes = sum(len(annot) for contigs in ann.values() for annot in contigs.values())
    tmp = tempfile.mkdtemp()
    for who, fn in (("reference", reference), ("device", device), ("nodes", nodes)):
        if getattr(args, who):
            res = fn(ann, orgs, circular, args.runs, tmp, args.metadata)
            res.update(n=args.n, d=args.d, seed=args.seed, genes=genes, date=time.strftime("%Y-%m-%d"))
            print(json.dumps(res), flush=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
