#!/usr/bin/env python3
"""Projecting a partition onto the organisms (Master.project_orders, nemgpu_master_project) against the two things a
user could do instead: projection.projection_arrays (numpy, from the master's arrays on the host) and a plain Python
walk over every gene, written here with dicts as the reference's projection() loop is (ppanggolin.py:1713-1743).
20 000 families x 2 000 organisms (tests/orders_util.synthetic_orders), every organism projected, random classes; per
figure the median of 5 calls in one process after one warm-up call; the walk: one call over the first 200 organisms
(a tenth of the genes: its dicts for all of them would not fit a modest host), its time also scaled to all genes.  Writes
profiles/projection.json; profiles/projection.md carries the table.  No threshold anywhere: this measures.

    python profiles/projection.py                 # the table
    python profiles/projection.py 5000 500        # other sizes (families, organisms)
    python profiles/projection.py --trace         # three library calls: the program of a kernel trace
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangenomenem_amd.chunks import Master  # noqa: E402
from pangenomenem_amd.projection import projection_arrays  # noqa: E402
from tests.orders_util import synthetic_orders  # noqa: E402
from tests.projection_util import ARRAYS, same_projection  # noqa: E402

REPEATS = 5


def timed(call, repeats=REPEATS):
    call()                                                    # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


WALK_ORGANISMS = 200


def python_walk(arrays, order, part, o, d, n_org):
    """over the contigs of organisms < n_org: the reference's loop with dicts in place of the graph: per organism its
    counters, per kept gene its line's numbers (copies, the family's three neighbour counts from a walk of its adjacency)"""
    rows, (ptr, idx) = arrays[0], arrays[1]
    n = len(order)
    fam_of = {int(order[i]): i for i in range(n)}
    adj = [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(n)]
    present = [int(v) for v in np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1).sum(axis=1)]
    label = part.tolist()
    repeated = set(np.flatnonzero(o["repeated"]).tolist())
    genes, cptr, corg = o["genes"].tolist(), o["contig_ptr"].tolist(), o["contig_org"].tolist()
    node = {}                                                 # (family, organism) -> its genes, as node[family][organism]
    for j, org in enumerate(corg):
        for p in range(cptr[j], cptr[j + 1] if org < n_org else cptr[j]):
            if genes[p] not in repeated:
                node.setdefault((fam_of[genes[p]], org), []).append(p)
    counts = [[0] * 7 for _ in range(d)]
    lines = 0
    for j, org in enumerate(corg):
        for p in range(cptr[j], cptr[j + 1] if org < n_org else cptr[j]):
            if genes[p] in repeated:
                continue
            fam = fam_of[genes[p]]
            counts[org][label[fam]] += 1
            counts[org][4 if present[fam] == d else 5] += 1
            counts[org][6] += 1
            nei = [label[b] for b in adj[fam]]
            line = (len(node[(fam, org)]), nei.count(0), nei.count(1), nei.count(2))
            lines += 1 if line else 0
    return np.asarray(counts, np.int32), lines


def main():
    trace = "--trace" in sys.argv
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n_fam, d = sizes if len(sizes) == 2 else (20000, 2000)
    o = synthetic_orders(n_fam, d, 11, p_repeat=0.01, contigs_per_org=2)
    t0 = time.perf_counter()
    m = Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], d, repeated=o["repeated"])
    t_build = time.perf_counter() - t0
    print("master of %d genes built in %.2f s" % (len(o["genes"]), t_build), flush=True)
    part = np.random.default_rng(1).integers(0, 4, m.n).astype(np.uint8)
    device = lambda: m.project_orders(part, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"])
    if trace:
        for _ in range(3):
            device()
        m.close()
        return
    arrays = m.arrays()
    host = lambda: projection_arrays(arrays, arrays[4], part, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"], d=d)
    got, want = device(), host()
    same_projection(got, want, "device against numpy")
    print("device equals numpy", flush=True)
    t0 = time.perf_counter()
    n_walk = min(WALK_ORGANISMS, d)
    walk_counts, lines = python_walk(arrays, arrays[4], part, o, d, n_walk)
    t_walk = time.perf_counter() - t0
    walked = int(np.repeat(o["contig_org"] < n_walk, np.diff(o["contig_ptr"])).sum())
    assert np.array_equal(walk_counts[:n_walk], want[3][:n_walk]) and lines == int(want[3][:n_walk, 6].sum())
    t_walk_all = t_walk * len(o["genes"]) / max(walked, 1)
    t_dev, all_dev = timed(device)
    t_host, all_host = timed(host)
    t0 = time.perf_counter()
    m.arrays()
    t_fetch = time.perf_counter() - t0
    row = dict(families=n_fam, organisms=d, genes=int(len(o["genes"])), contigs=int(len(o["contig_org"])),
               master=dict(zip(("n", "d", "nnz", "extras"), m.shape())), outputs=list(ARRAYS), repeats=REPEATS,
               device_s=t_dev, numpy_s=t_host, python_walk_organisms=n_walk, python_walk_genes=walked, python_walk_s=t_walk,
               python_walk_scaled_to_all_genes_s=t_walk_all, numpy_over_device=t_host / t_dev, walk_scaled_over_device=t_walk_all / t_dev,
               master_build_s=t_build, master_fetch_s=t_fetch, device_all=all_dev, numpy_all=all_host)
    print("%d families x %d organisms, %d genes: device %.4f s, numpy %.4f s (x%.1f), python walk %.2f s for %d genes (scaled to all: %.1f s, x%.0f); master fetch for numpy %.3f s"
          % (n_fam, d, row["genes"], t_dev, t_host, t_host / t_dev, t_walk, walked, t_walk_all, t_walk_all / t_dev, t_fetch), flush=True)
    m.close()
    with open(os.path.join(ROOT, "profiles", "projection.json"), "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
