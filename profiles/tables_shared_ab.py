"""A/B of two built checkouts of this package on the calls that read the resident master: the projection (profiles/projection.md),
the family table and its .Rtab cells at both sizes of profiles/matrix.md, the edge table and its <attvalue> text
(profiles/gexf.md).  Wall clock around the Python call, host-device copies included.

    python profiles/tables_shared_ab.py --parent /path/to/the/parent's/checkout [--rounds 6] [--runs 2]

The inputs are made once and kept in a temporary directory.  Then the two builds alternate, the parent first in one round and the candidate first
in the next: every round starts one fresh process per build, which imports that checkout's package and library, makes its masters, calls every call
once to warm up and then times it --runs times.  Every run goes into profiles/tables_shared_ab.json; no threshold is set here.
"""
import argparse
import json
import os
import pickle
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = dict(projection=(20000, 2000), matrix_small=(2000, 500), matrix_large=(20000, 5000))
TEXT_BATCH = 64 << 20


def make_inputs(tmp):
    sys.path.insert(0, ROOT)
    from pangenomenem_amd.synth import annotated_pangenome
    from tests.orders_util import synthetic_orders
    for name, (n_fam, d) in SIZES.items():
        o = synthetic_orders(n_fam, d, 11, p_repeat=0.01, contigs_per_org=2) if name == "projection" else synthetic_orders(n_fam, d, 1)
        o["gene_len"] = np.random.default_rng(3).integers(0, 39, len(o["genes"])).astype(np.int32) * 30 + 90
        np.savez(os.path.join(tmp, name + ".npz"), **{k: np.asarray(v) for k, v in o.items()})
    ann, orgs, circular = annotated_pangenome(2000, 200, 11)
    with open(os.path.join(tmp, "gexf.pickle"), "wb") as f:
        pickle.dump((ann, orgs, circular), f)


def timed(call, runs):
    call()                                                    # warm-up
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return out


def worker(root, tmp, runs):
    sys.path.insert(0, root)
    from pangenomenem_amd.chunks import Master
    from pangenomenem_amd.gexf import gexf_orders
    res = {}

    def master_of(name):
        o = dict(np.load(os.path.join(tmp, name + ".npz")))
        return o, Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], int(o["d"]), repeated=o["repeated"])

    o, m = master_of("projection")
    part = np.random.default_rng(1).integers(0, 4, m.n).astype(np.uint8)
    res["project_orders 20000x2000"] = timed(lambda: m.project_orders(part, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]), runs)
    m.close()
    for name in ("matrix_small", "matrix_large"):
        o, m = master_of(name)
        size = "%dx%d" % (m.n, m.d)
        tables = []
        res["family_table " + size] = timed(lambda: tables.append(m.family_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]),
                                                                                  lengths=o["gene_len"])), runs)
        t = tables.pop()
        for other in tables:
            other.close()
        res["rtab_cells " + size] = timed(lambda: sum(len(t.rtab_cells(row0, rows)[0]) for row0, rows in t._batches(TEXT_BATCH)), runs)
        t.close()
        m.close()
    with open(os.path.join(tmp, "gexf.pickle"), "rb") as f:
        ann, orgs, circular = pickle.load(f)
    m = Master.from_annotations(ann, orgs, list(circular))
    g = gexf_orders(ann, orgs, m.id_names, {org: frozenset() for org in orgs}, circular)
    tables = []
    res["edge_table(annotations) 2000x200"] = timed(lambda: tables.append(m.edge_table(ann, (), circular)), runs)
    res["edge_table(orders) 2000x200"] = timed(lambda: tables.append(m.edge_table(orders=(g["genes"], g["contig_ptr"], g["contig_org"], g["repeated"]),
                                                                                  starts=g["starts"], ends=g["ends"], contig_sizes=g["contig_sizes"])), runs)
    et = tables.pop()
    for other in tables:
        other.close()
    attr_id, _ = et.attribute_ids(100)
    res["attvalues 2000x200"] = timed(lambda: sum(len(et.attvalues(attr_id, row0, rows)[0]) for row0, rows in et._batches(TEXT_BATCH)), runs)
    et.close()
    m.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent's checkout, built")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--worker", nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(*args.worker, args.runs)
    roots = dict(parent=os.path.abspath(args.parent), candidate=ROOT)
    tmp = tempfile.mkdtemp()
    try:
        make_inputs(tmp)
        runs = {who: {} for who in roots}
        for r in range(args.rounds):
            for who, root in list(roots.items())[::1 if r % 2 == 0 else -1]:      # (parent first, then candidate first, ...)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, tmp, "--runs", str(args.runs)], check=True,
                                     stdout=subprocess.PIPE, text=True, timeout=600).stdout
                for call, times in json.loads(out.strip().splitlines()[-1]).items():
                    runs[who].setdefault(call, []).extend(times)
                print(who, "done", flush=True)
    finally:
        shutil.rmtree(tmp)
    calls = {}
    for call in runs["parent"]:
        p, c = runs["parent"][call], runs["candidate"][call]
        calls[call] = dict(parent_s=p, candidate_s=c, parent_median_s=statistics.median(p), parent_slowest_s=max(p), candidate_median_s=statistics.median(c),
                           candidate_median_above_parent_slowest=statistics.median(c) > max(p))
        print("%-36s parent %.5f (%.5f - %.5f)  candidate %.5f (%.5f - %.5f)%s" % (call, statistics.median(p), min(p), max(p), statistics.median(c), min(c),
                                                                               max(c), "  ABOVE" if calls[call]["candidate_median_above_parent_slowest"] else ""), flush=True)
    with open(os.path.join(ROOT, "profiles", "tables_shared_ab.json"), "w") as f:
        json.dump(dict(device="MI355X (gfx950), one GPU", date=time.strftime("%Y-%m-%d"), rounds=args.rounds, runs_per_round=args.runs,
                       what="wall clock around the Python call, host-device copies included; the builds alternate (the first of a round changes too), a fresh process per build and "
                            "round, one warm-up call of each call per process", calls=calls), f, indent=1)


if __name__ == "__main__":
    main()
