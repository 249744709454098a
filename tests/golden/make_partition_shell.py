#!/usr/bin/env python3
"""Generate tests/golden/partition_shell/: what the REAL `partition_shell()` (ppanggolin/ppanggolin.py:1175-1248) and the
REAL `__write_nem_input_files(..., filter_by_partition="shell")` (:821-930) do on a few small pangenomes whose graph the
real `__neighborhood_computation` (:463-530) built -- for one case a base grown through the real `add_organism`
(:342-358) -- and whose nodes carry a labelling written in the case.

Runs only where the reference tree and networkx exist; nothing of the reference travels: what is stored is data.  Per
case <name>.json.gz (gzip of compact JSON) holds
  * the annotations as lists, the organisms in column order, the circular contigs' sizes, what an update brought, the
    labelling {family: P | S | C | U} (the keys tests/golden/gexf/ uses), the projection's means;
  * `writer`: the `.index`, `.dat`, `.nei` and `.str` text the filtered writer wrote for all organisms, or the exception
    it raised and its argument; `induced`: what the same writer wrote, unfiltered, for
    `neighbors_graph.subgraph(shell).copy()`;
  * `m_dict`, `m_list` (two cases): the `.m` text for a dict init of 3 groups and for a list init, with the inits;
  * `runs`: the whole of the real partition_shell with `run_partitioning` replaced by a stand-in that returns a listed
    result (recorded) and, where the writer raises, the writer replaced by a no-op: Q = "auto", an int, a dict and a
    list init, mean(eps) on both sides of exclusity_th -- the three attributes it fills, the node attribute and its
    return value;
  * `gexf`, `gexf_light` (one case): what the real export_to_GEXF wrote after that.
<name>.npz holds the compiled reference's INIT_RANDOM run (oracle/_ref: ClassifyByNem after srandom(seed), 50 starts,
ncem, sk_, beta 0.5) on the induced problem as pangenomenem_amd.shell.form_subproblem_host forms it from the numpy
master, for Q = 2, 4 and 7: status, best_start, c, center, disp, prop.
tests/test_partition_shell_host.py and tests/test_gpu_partition_shell.py read both.

The reference is run as make_gexf.py runs it (the stand-in modules, an object made without __init__, a graph class with
the networkx 1.x attribute `node`); `organisms` is the small ordered set of make_nei_counts.py.

    python tests/golden/make_partition_shell.py
"""
import contextlib
import gzip
import io
import json
import os
import random
import shutil
import sys
import tempfile
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_projection  # noqa: E402
from make_nei_counts import OrderedSet  # noqa: E402
from make_orders import RESERVED, reference_class  # noqa: E402

OUT = os.path.join(HERE, "partition_shell")
LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
SIZE = 100000
REF_SEED = 20271019
REF_QS = (2, 4, 7)


def genomes_of(d, seed, n_shell=20, mode="closed", first=1):
    """d organisms: a chromosome of persistent families with a few cloud ones and, mode "open", the shell families among
    them; mode "closed": the shell families on contigs of their own (the shell is closed under adjacency)"""
    rng = random.Random(seed)
    P, S, Cl = ["P%d" % i for i in range(10)], ["S%d" % i for i in range(n_shell)], ["C%d" % i for i in range(6)]
    genomes = []
    for o in range(d):
        org = "o%d" % (first + o)
        chrom = [p for p in P if rng.random() < 0.95]
        for c in Cl:
            if rng.random() < 1.5 / d:
                chrom.insert(rng.randrange(len(chrom) + 1), c)
        contigs = []
        if mode == "open":
            for s in S:
                if rng.random() < 0.5:
                    chrom.insert(rng.randrange(len(chrom) + 1), s)
        elif S:
            for j in range(rng.randint(1, 3)):
                a = rng.randrange(len(S))
                run = S[a:a + rng.randint(1, 7)]
                contigs.append(("%s_i%d" % (org, j), run[::-1] if rng.random() < 0.4 else run))
        genomes.append((org, [(org + "_chr", chrom)] + contigs))
    seen = set(f for _, contigs in genomes for _, fams in contigs for f in fams)
    missing = [f for f in P + S + Cl if f not in seen]
    if missing:                                               # (every family exists: the first organism carries the rest)
        org, contigs = genomes[0]
        if mode == "open":
            contigs[0] = (contigs[0][0], contigs[0][1] + missing)
        else:
            contigs[0] = (contigs[0][0], contigs[0][1] + [f for f in missing if f[0] != "S"])
            if any(f[0] == "S" for f in missing):
                contigs.append((org + "_rest", [f for f in missing if f[0] == "S"]))
    return genomes


def add_contigs(genomes, extra):
    """extra: [(organism index, contig name, [families])]"""
    for o, contig, fams in extra:
        genomes[o][1].append((contig, list(fams)))
    return genomes


def labels_of(genomes, special=()):
    lab = OrderedDict()
    for _, contigs in genomes:
        for _, fams in contigs:
            for f in fams:
                lab.setdefault(f, f[0])
    lab.update(special)
    return dict(lab)


def cases():
    out = []
    g = genomes_of(8, 1)
    out.append(dict(name="closed", genomes=g, circular={}, labels=labels_of(g), m_inits=True, gexf=True))
    g = genomes_of(10, 2, mode="open")
    out.append(dict(name="open", genomes=g, circular={}, labels=labels_of(g, {"C0": "U"})))
    # X is a shell family whose neighbours are all persistent: degree 0 in the induced graph
    g = genomes_of(7, 3, mode="open")
    for o in (0, 2, 3, 6):
        chrom = g[o][1][0][1]
        chrom.insert(max(1, len(chrom) // 2), "SX")
    lab = labels_of(g)
    for o in (0, 2, 3, 6):                                    # (its neighbours there, whatever they are, are not shell)
        chrom = g[o][1][0][1]
        at = chrom.index("SX")
        for nb in (chrom[at - 1], chrom[at + 1] if at + 1 < len(chrom) else chrom[at - 1]):
            if lab[nb] == "S":
                lab[nb] = "P"
    out.append(dict(name="outside_only", genomes=g, circular={}, labels=lab))
    g = add_contigs(genomes_of(6, 4), [(1, "o2_tandem", ["S2", "S2", "S3"]), (4, "o5_tandem", ["S3", "S2", "S2", "S2"])])
    out.append(dict(name="selfloop", genomes=g, circular={}, labels=labels_of(g)))
    g = add_contigs(genomes_of(6, 5), [(2, "o3_twice", ["S1", "S2", "S5", "S1", "S2", "S1"])])
    out.append(dict(name="twice", genomes=g, circular={}, labels=labels_of(g)))
    g = add_contigs(genomes_of(9, 6), [(o, "pl%d" % o, ["S10", "S11", "S12"]) for o in (0, 3, 4, 7)] + [(5, "pl5", ["S13"]), (8, "pl8", ["S14", "S15"])])
    out.append(dict(name="circular", genomes=g, circular={"pl%d" % o: 5000 + o for o in (0, 3, 4, 5, 7, 8)}, labels=labels_of(g), m_inits=True))
    g = genomes_of(9, 7)
    out.append(dict(name="grown", genomes=g[:6], update=g[6:], circular={}, labels=labels_of(g)))
    g = genomes_of(6, 8, n_shell=0)
    out.append(dict(name="noshell", genomes=g, circular={}, labels=labels_of(g)))
    return out


def listed_result(families, organisms, Q, rng):
    """the stand-in's answer: classes dealt round the families, parameters with mean(eps) on both sides of 0.1 (class 2:
    eight times 0.1, whose float mean is just below it)"""
    classes = OrderedDict((f, (3 + 7 * i) % Q) for i, f in enumerate(families))
    params = OrderedDict()
    for k in range(Q):
        mu = [rng.random() < 0.5 for _ in organisms]
        if k == 2:
            eps = [0.1] * len(organisms)
        elif k % 2 == 0:
            eps = [round(rng.uniform(0.01, 0.09), 4) for _ in organisms]
        else:
            eps = [round(rng.uniform(0.15, 0.45), 4) for _ in organisms]
        params[k] = (mu, eps, round(1.0 / Q + (k - (Q - 1) / 2.0) * 0.01, 3))
    return classes, params


def read_files(tmp):
    return {ext: open(os.path.join(tmp, "nem_file." + ext)).read() for ext in ("index", "dat", "nei", "str")}


def build(PPanGGOLiN, cs):
    import networkx as nx
    import ppanggolin.ppanggolin as module
    module.bidict = dict

    class NodeGraph(nx.Graph):
        node = property(lambda self: self.nodes)

    update = cs.get("update", [])
    both = make_projection.annotations_of(cs["genomes"] + update)
    base_orgs, new_orgs = [o for o, _ in cs["genomes"]], [o for o, _ in update]
    obj = PPanGGOLiN.__new__(PPanGGOLiN)
    obj.annotations = OrderedDict((o, both[o]) for o in base_orgs)
    obj.organisms = list(base_orgs)
    obj.nb_organisms = len(base_orgs)
    obj.families_repeted = []
    obj.circular_contig_size = {c: s for c, s in cs["circular"].items() if any(c in both[o] for o in base_orgs)}
    obj.index = {}
    obj.nem_intermediate_files = None
    obj.neighbors_graph = NodeGraph()
    obj._PPanGGOLiN__neighborhood_computation()
    update_circular = {c: s for c, s in cs["circular"].items() if c not in obj.circular_contig_size}
    if update:
        obj.add_organism(list(new_orgs), OrderedDict((o, both[o]) for o in new_orgs), dict(update_circular), [])
    organisms = base_orgs + new_orgs
    g = obj.neighbors_graph
    assert set(cs["labels"]) == set(g.nodes()), (cs["name"], sorted(set(cs["labels"]) ^ set(g.nodes())))
    obj.partitions = {long: [] for long in list(LONG.values()) + ["core_exact", "accessory"]}
    for fam, data in g.nodes(data=True):                      # partition(), :1131-1157
        nb_orgs = sum(1 for key in data if key not in RESERVED)
        data["partition"] = LONG[cs["labels"][fam]]
        data["partition_exact"] = "core_exact" if nb_orgs == len(organisms) else "accessory"
        data["viz"] = {"color": module.COLORS_RGB[data["partition"] if cs["labels"][fam] != "U" else data["partition_exact"]], "size": nb_orgs}
        obj.partitions[data["partition"]].append(fam)
        obj.partitions[data["partition_exact"]].append(fam)
    obj.is_partitionned = True
    obj.partitions_by_organism = dict()
    obj.organisms = OrderedSet(organisms)
    obj.nb_organisms = len(organisms)
    return obj, module, both, base_orgs, new_orgs, update_circular


def run(PPanGGOLiN, cs):
    obj, module, both, base_orgs, new_orgs, update_circular = build(PPanGGOLiN, cs)
    g = obj.neighbors_graph
    organisms = base_orgs + new_orgs
    shell = [f for f in g.nodes() if cs["labels"][f] == "S"]
    rec = dict(name=cs["name"], organisms=base_orgs, new_organisms=new_orgs,
               annotations=[[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in both[org].items()]]
                            for org in organisms],
               circular={c: s for c, s in cs["circular"].items() if c not in update_circular}, update_circular=update_circular,
               repeated=[], update_repeated=[], labels=cs["labels"], project=list(organisms))
    quiet = io.StringIO()
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(tmp + "/proj")
        os.makedirs(tmp + "/ps")
        with contextlib.redirect_stdout(quiet):
            rec["means"] = list(obj.projection(tmp + "/proj", list(organisms)))
            # (a) the writer as written, and unfiltered on the induced subgraph
            try:
                obj._PPanGGOLiN__write_nem_input_files(tmp + "/w/", obj.organisms, init=None, filter_by_partition="shell")
                rec["writer"] = dict(files=read_files(tmp + "/w"))
                assert open(tmp + "/w/nem_file.m").read() == ""
            except Exception as e:                           # noqa: BLE001 (whatever it raises is the record)
                rec["writer"] = dict(error=[type(e).__name__, list(e.args)])
            sub = PPanGGOLiN.__new__(PPanGGOLiN)
            sub.neighbors_graph = g.subgraph(shell).copy()
            sub._PPanGGOLiN__write_nem_input_files(tmp + "/s/", obj.organisms, init=None)
            rec["induced"] = dict(files=read_files(tmp + "/s"))
            third = max(1, len(organisms) // 3)
            init_dict = OrderedDict([("g1", set(organisms[:third])), ("g2", set(organisms[third:2 * third])), ("g3", set(organisms[2 * third:-1]))])
            init_list = [set(organisms[:third]), set(organisms[third:2 * third])]
            if cs.get("m_inits"):
                for key, init in (("m_dict", init_dict), ("m_list", init_list)):
                    obj._PPanGGOLiN__write_nem_input_files(tmp + "/" + key + "/", obj.organisms, init=init, filter_by_partition="shell")
                    rec[key] = open(tmp + "/" + key + "/nem_file.m").read()
                rec["m_inits"] = dict(dict=[[k, sorted(v)] for k, v in init_dict.items()], list=[sorted(v) for v in init_list])
            # (b) the real partition_shell around a listed run_partitioning
            if "error" in rec["writer"]:
                obj._PPanGGOLiN__write_nem_input_files = lambda *a, **k: None
            rec["runs"] = []
            rng = random.Random(len(shell))
            settings = [dict(Q="auto", init=None, exclusity_th=0.1), dict(Q=3, init=None, exclusity_th=0.3), dict(Q="auto", init=init_dict, exclusity_th=0.1),
                        dict(Q="auto", init=init_list, exclusity_th=0.05), dict(Q=1, init=None, exclusity_th=0.1)]
            for st in settings:
                calls = []

                def stand_in(nem_dir_path, nb_org, beta, free_dispersion, Q=3, init="param_file_default"):
                    fams, params = listed_result(shell, organisms, Q, rng)
                    calls.append(dict(Q=Q, init=init, nb_org=nb_org, classes=[[f, k] for f, k in fams.items()],
                                      parameters=[[k, list(p[0]), list(p[1]), p[2]] for k, p in params.items()]))
                    return (dict(fams), dict(params))

                module.run_partitioning = stand_in
                for data in g.nodes.values():
                    data.pop("subpartition_shell", None)
                one = dict(Q=st["Q"], exclusity_th=st["exclusity_th"],
                           init=None if st["init"] is None else dict(dict=[[k, sorted(v)] for k, v in st["init"].items()]) if isinstance(st["init"], dict)
                           else dict(list=[sorted(v) for v in st["init"]]))
                try:
                    ret = obj.partition_shell(tmp + "/ps", Q=st["Q"], exclusity_th=st["exclusity_th"], init_using_qual=st["init"])
                except Exception as e:                       # noqa: BLE001
                    one["error"] = [type(e).__name__, [str(a) for a in e.args]]
                    rec["runs"].append(one)
                    continue
                one["returned"] = ret if not isinstance(ret, tuple) else list(ret)
                one["calls"] = calls
                if calls:
                    one["parameters"] = [[label, list(v[0]), v[1], v[2]] for label, v in obj.subpartitions_shell_parameters.items()]
                    one["organisms"] = {org: sorted(v) for org, v in obj.organisms_subpartitions_shell.items()}
                    one["families"] = {label: list(v) for label, v in obj.subpartition_shell.items()}
                    one["node_attribute"] = {f: data.get("subpartition_shell") for f, data in g.nodes(data=True)}
                rec["runs"].append(one)
            if cs.get("gexf"):                                # the export after an int-Q run
                for data in g.nodes.values():
                    data.pop("subpartition_shell", None)
                rng = random.Random(99)
                module.run_partitioning = lambda *a, Q=3, init=None: tuple(map(dict, listed_result(shell, organisms, Q, rng)))
                assert obj.partition_shell(tmp + "/ps", Q=4) == 4
                rec["gexf_node_attribute"] = {f: data["subpartition_shell"] for f, data in g.nodes(data=True)}
                obj.export_to_GEXF(tmp + "/full")
                obj.export_to_GEXF(tmp + "/light", all_node_attributes=False, all_edge_attributes=False)
                rec["gexf"] = open(tmp + "/full.gexf", newline="", encoding="utf-8").read()
                rec["gexf_light"] = open(tmp + "/light.gexf", newline="", encoding="utf-8").read()
    finally:
        shutil.rmtree(tmp)
    return rec


def reference_runs(rec):
    """(c) the compiled reference's random starts on the induced problem"""
    from oracle import pyoracle
    from pangenomenem_amd.shell import form_subproblem_host
    from tests.projection_util import fixture_master_host
    m, _, names = fixture_master_host(rec)
    select = np.asarray([rec["labels"][f] == "S" for f in names], bool)
    if not select.any():
        return None
    x, nei, _ = form_subproblem_host(m[0], m[1][0], m[1][1], m[2], np.arange(m[0].shape[1]), select, m[3], "induced")
    ref = pyoracle.Reference()
    out = {}
    for Q in REF_QS:
        r = ref.classify_random(x, nei, Q, n_starts=50, rng_seed=REF_SEED, algo="ncem", disper="sk_", beta=0.5, it_max=100)
        out["status_%d" % Q] = np.int32(r["status"])
        out["best_start_%d" % Q] = np.int32(r["best_start"])
        for key in ("c", "center", "disp", "prop"):
            out["%s_%d" % (key, Q)] = r[key]
    return out


def main():
    from oracle import pyoracle
    pyoracle.build(ref=True)
    if not pyoracle.have_reference():
        raise SystemExit("the compiled reference (oracle/_ref) is needed")
    PPanGGOLiN = reference_class()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for cs in cases():
        rec = run(PPanGGOLiN, cs)
        with open(os.path.join(OUT, cs["name"] + ".json.gz"), "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:
            f.write(json.dumps(rec, separators=(",", ":")).encode())
        runs = reference_runs(rec)
        if runs is not None:
            np.savez_compressed(os.path.join(OUT, cs["name"] + ".npz"), **runs)
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
