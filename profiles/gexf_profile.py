#!/usr/bin/env python3
"""Times for profiles/gexf.md: the GEXF export of one synthetic pangenome (synth.annotated_pangenome), either by the
reference (--reference: the real __neighborhood_computation builds the graph, the real export_to_GEXF writes it; needs
the reference tree and networkx, as the generators under tests/golden/ do) or from the resident master (--device:
Master.from_annotations, family_table, edge_table, write_gexf; needs the GPU).  Both label a family persistent above
0.9 d organisms, cloud below 0.1 d, shell between.  --metadata: three metadata attributes of 2, 20 and 200 distinct
values (export_to_GEXF's metadata=, write_gexf's metadata=) -- the exports are timed with and, on the device, also
without them, and the device's metadata lines of all the edges on their own.  Prints one JSON line.

    python profiles/gexf_profile.py --n 2000 --d 200 --seed 11 --device --runs 3
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--d", type=int, default=200)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--metadata", action="store_true")
    args = ap.parse_args()
    ann, orgs, circular = annotated_pangenome(args.n, args.d, args.seed)
    genes = sum(len(annot) for contigs in ann.values() for annot in contigs.values())
    tmp = tempfile.mkdtemp()
    for who, fn in (("reference", reference), ("device", device)):
        if getattr(args, who):
            res = fn(ann, orgs, circular, args.runs, tmp, args.metadata)
            res.update(n=args.n, d=args.d, seed=args.seed, genes=genes, date=time.strftime("%Y-%m-%d"))
            print(json.dumps(res), flush=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
