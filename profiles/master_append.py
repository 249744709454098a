#!/usr/bin/env python3
"""Appending organisms to a resident master (Master.add_orders, nemgpu_master_append_orders) against what a user had to
do before: Master.from_orders on the concatenated orders.  20 000 families (tests/orders_util.synthetic_orders), bases
of 1 000 and 5 000 organisms, updates of 1, 10 and 100; per figure the median of 5 calls in one process after one
warm-up call.  Writes profiles/master_append.json; profiles/master_build.md carries the table.

    python profiles/master_append.py                  # the table
    python profiles/master_append.py --trace 5000 10  # one base, one update, three appends: the program of a kernel trace
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
from tests.append_util import slice_orders  # noqa: E402
from tests.orders_util import same_master, synthetic_orders  # noqa: E402

N_FAM, REPEATS = 20000, 5


def build(o, d):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], d, repeated=o["repeated"])


def timed(call):
    call().close()                                            # warm-up
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        m = call()
        times.append(time.perf_counter() - t0)
        m.close()
    return statistics.median(times), times


def main():
    trace = "--trace" in sys.argv
    bases = [int(sys.argv[2])] if trace else [1000, 5000]
    adds = [int(sys.argv[3])] if trace else [1, 10, 100]
    rows = []
    for d0 in bases:
        whole = synthetic_orders(N_FAM, d0 + max(adds), 11, p_repeat=0.01, contigs_per_org=2)
        base = slice_orders(whole, 0, d0)
        m = build(base, d0)
        for k in adds:
            upd = slice_orders(whole, d0, d0 + k)
            both = slice_orders(whole, 0, d0 + k)
            append = lambda: m.add_orders(upd["genes"], upd["contig_ptr"], upd["contig_org"], upd["contig_circular"], k, repeated=upd["repeated"])
            if trace:
                for _ in range(3):
                    append().close()
                continue
            g, r = append(), build(both, d0 + k)
            same_master(g.arrays(), r.arrays(), "%d + %d" % (d0, k))
            assert np.array_equal(g.order, r.order)
            shape = g.shape()
            g.close()
            r.close()
            t_app, all_app = timed(append)
            t_reb, all_reb = timed(lambda: build(both, d0 + k))
            rows.append(dict(families=N_FAM, base_organisms=d0, added=k, update_genes=int(len(upd["genes"])), all_genes=int(len(both["genes"])),
                             master=dict(zip(("n", "d", "nnz", "extras"), shape)), append_s=t_app, rebuild_s=t_reb, ratio=t_reb / t_app,
                             append_all=all_app, rebuild_all=all_reb))
            print("%5d + %3d organisms: append %.4f s, rebuild %.4f s, x%.1f" % (d0, k, t_app, t_reb, t_reb / t_app), flush=True)
        m.close()
    if not trace:
        with open(os.path.join(ROOT, "profiles", "master_append.json"), "w") as f:
            json.dump(dict(repeats=REPEATS, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
