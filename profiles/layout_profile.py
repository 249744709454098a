#!/usr/bin/env python3
"""Times for profiles/layout.md: the ForceAtlas2 layout of one synthetic pangenome's family graph on the device
(synth.annotated_pangenome -> Master.from_annotations -> Master.layout; needs the GPU).  Per n: a warm-up run, then a
host clock around run(k) that ends in a synchronise (state() waits for the stream), k chosen from a short probe so that
the window is about a second.  Pair interactions and FLOP are counted from the shapes: n^2 ordered pairs per iteration,
12 float64 operations a pair (2 differences, the squared distance 3, the masses' product 1, the division 1, the two
terms 2 and their additions 2, the test for a coincident pair 1), the division counted as one.  Prints one JSON line per
n.  --trace: a fixed, small number of iterations and no clock, for a run under `rocprofv3 --kernel-trace --stats`.
--repulsion: exact (the default), barnes_hut, or both, one line each per n from the same master and start, so that the
Barnes-Hut sum is compared with the exact one of the same session; a barnes_hut line also carries the walk's counters
(Layout.tree() after the timed iterations: the cells accepted and the leaf bodies visited per family, mean and maximum)
and the tree's cells.  Its pairs / FLOP columns are left out: it does not visit n^2 pairs.

    python profiles/layout_profile.py --n 2000 20000 200000 --d 10 --seed 11 --repulsion both
"""
import argparse
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from pangenomenem_amd.synth import annotated_pangenome  # noqa: E402

FLOP_PER_PAIR = 12


def clocked(lay, k):
    t0 = time.perf_counter()
    lay.run(k)
    lay.state()
    return time.perf_counter() - t0


def measure(m, build, d, seed, window, trace, repulsion, theta):
    from pangenomenem_amd.layout import slices_of
    _, _, nnz, _ = m.shape()
    bh = repulsion == "barnes_hut"
    lay = m.layout(0, rng=random.Random(seed), repulsion=repulsion, theta=theta)
    out = dict(n=m.n, d=d, seed=seed, csr_entries=nnz, repulsion=repulsion, slices=1 if bh else slices_of(m.n), master_from_annotations_s=build)
    if bh:
        out.update(theta=theta)
    if trace:
        lay.run(trace)
        out.update(iterations=lay.state()["iterations"])
    else:
        clocked(lay, 2)                                       # (warm-up)
        probe = clocked(lay, 3) / 3
        k = max(3, min(50000, int(window / probe)))
        wall = clocked(lay, k)
        per = wall / k
        pairs = float(m.n) * m.n
        out.update(iterations_timed=k, window_s=wall, ms_per_iteration=1e3 * per, seconds_for_500_iterations=500 * per, state=lay.state())
        if not bh:
            out.update(pairs_per_s=pairs / per, flop_per_s=FLOP_PER_PAIR * pairs / per)
    if bh:
        t = lay.tree()
        out.update(cells=t["cells"], cell_bound=t["bound"], accepted_mean=float(t["accepted"].mean()), accepted_max=int(t["accepted"].max()),
                   visited_mean=float(t["visited"].mean()), visited_max=int(t["visited"].max()))
    lay.close()
    out["date"] = time.strftime("%Y-%m-%d")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 20000, 200000])
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--repulsion", choices=("exact", "barnes_hut", "both"), default="exact")
    ap.add_argument("--theta", type=float, default=1.2)
    args = ap.parse_args()
    from pangenomenem_amd.chunks import Master
    for n in args.n:
        ann, orgs, circular = annotated_pangenome(n, args.d, args.seed)
        t0 = time.perf_counter()
        m = Master.from_annotations(ann, orgs, list(circular))
        build = time.perf_counter() - t0
        for repulsion in (("exact", "barnes_hut") if args.repulsion == "both" else (args.repulsion,)):
            print(json.dumps(measure(m, build, args.d, args.seed, args.window, args.trace, repulsion, args.theta)), flush=True)
        m.close()


if __name__ == "__main__":
    main()
