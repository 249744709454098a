#!/usr/bin/env python3
"""Merging two resident masters (Master.merge, nemgpu_master_merge) against the two things a user had before:
Master.from_orders on the concatenated orders, and Master.add_orders of B's orders (which needs B's orders, not B's
master).  The shapes of profiles/master_append.py: 20 000 families (tests/orders_util.synthetic_orders), A of 1 000 and
5 000 organisms, B of 1, 10 and 100; B's master is resident before the clock starts; per figure the median of 15 calls in
one process after one warm-up call (the spread of the merge's calls is in the table: the machine is shared).  The bytes
moved per call are computed from the shapes (what each entry point copies between host and device).  Writes master_merge.json and master_merge.md into --out (default: this directory).

    python profiles/master_merge.py                         # the table
    python profiles/master_merge.py --trace DIR             # the table, then one A and one B merged four times under
                                                            # `rocprofv3 --kernel-trace --stats` in a child process: the
                                                            # fill kernels' times against the bytes they read and write
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangenomenem_amd.chunks import Master  # noqa: E402
from tests.append_util import slice_orders  # noqa: E402
from tests.orders_util import same_master, synthetic_orders  # noqa: E402

N_FAM, REPEATS = 20000, 15
HBM_PEAK = 8e12                                               # bytes / s (the MI355X's specified peak)
TRACED = (5000, 100)                                          # the traced run's A and B organisms
FILL_KERNELS = ("k_merge_bits", "k_merge_xt_a", "k_merge_xt_b", "k_merge_a_entries", "k_merge_b_entries")


def build(o, d):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], d, repeated=o["repeated"])


def alone(o, lo, hi):
    return dict(o, contig_org=(o["contig_org"] - lo).astype(np.int32)), hi - lo


def timed(call):
    call().close()                                            # warm-up
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        m = call()
        times.append(time.perf_counter() - t0)
        m.close()
    return statistics.median(times), times


def orders_bytes(o):
    return int(4 * len(o["genes"]) + 4 * len(o["contig_ptr"]) + 5 * len(o["contig_org"]) + len(o["repeated"]))


def fill_bytes(a, b, m):
    """bytes read + written by the fill kernels, from the three masters' shapes (n, d, nnz, extras); the searches of the
    row pointers, which stay in cache, are not counted"""
    wf, nw = lambda s: (s[1] + 31) // 32, lambda s: (s[0] + 63) // 64
    return dict(k_merge_bits=8 * m[2] + 4 * (a[2] * wf(a) + b[2] * wf(b)) + 4 * m[2] * wf(m),
                k_merge_xt_a=8 * a[1] * nw(a) + 8 * a[1] * nw(m),
                k_merge_xt_b=8 * b[1] * nw(b) + 4 * m[0] + 8 * b[1] * nw(m),
                k_merge_a_entries=4 * a[2] + 12 * a[2],
                k_merge_b_entries=12 * b[2] + 12 * b[2])


def case(whole, d0, k):
    base, upd, both = slice_orders(whole, 0, d0), slice_orders(whole, d0, d0 + k), slice_orders(whole, 0, d0 + k)
    (b_alone, _) = alone(upd, d0, d0 + k)
    return base, upd, both, b_alone


def table(bases, adds):
    rows = []
    for d0 in bases:
        whole = synthetic_orders(N_FAM, d0 + max(adds), 11, p_repeat=0.01, contigs_per_org=2)
        ma = build(slice_orders(whole, 0, d0), d0)
        for k in adds:
            base, upd, both, b_alone = case(whole, d0, k)
            mb = build(b_alone, k)
            merge = lambda: ma.merge(mb)
            append = lambda: ma.add_orders(upd["genes"], upd["contig_ptr"], upd["contig_org"], upd["contig_circular"], k, repeated=upd["repeated"])
            g, r = merge(), build(both, d0 + k)
            same_master(g.arrays(), r.arrays(), "%d + %d" % (d0, k))
            assert np.array_equal(g.order, r.order)
            shape = g.shape()
            g.close()
            r.close()
            t_mrg, all_mrg = timed(merge)
            t_app, all_app = timed(append)
            t_reb, all_reb = timed(lambda: build(both, d0 + k))
            n_a, n_b, n = ma.n, mb.n, shape[0]
            rows.append(dict(families=N_FAM, a_organisms=d0, b_organisms=k, b_genes=int(len(upd["genes"])), all_genes=int(len(both["genes"])),
                             a=dict(zip(("n", "d", "nnz", "extras"), ma.shape())), b=dict(zip(("n", "d", "nnz", "extras"), mb.shape())),
                             master=dict(zip(("n", "d", "nnz", "extras"), shape)), merge_s=t_mrg, append_s=t_app, rebuild_s=t_reb,
                             rebuild_over_merge=t_reb / t_mrg, append_over_merge=t_app / t_mrg,
                             merge_bytes=dict(up=4 * n_a + 4 * n_b, down=4 * (n - n_a) + 12),
                             append_bytes=dict(up=orders_bytes(upd) + 4 * n_a, down=4 * (n - n_a) + 16),
                             rebuild_bytes=dict(up=orders_bytes(both), down=4 * n + 16),
                             merge_all=all_mrg, append_all=all_app, rebuild_all=all_reb))
            print("%5d + %3d organisms: merge %.4f s, append %.4f s, rebuild %.4f s (x%.1f)" % (d0, k, t_mrg, t_app, t_reb, t_reb / t_mrg), flush=True)
            mb.close()
        ma.close()
    return rows


def traced_child(d0, k, out):
    """one A, one B, a warm-up merge and three more: the program of the kernel trace; the shapes go to `out`"""
    whole = synthetic_orders(N_FAM, d0 + k, 11, p_repeat=0.01, contigs_per_org=2)
    base, upd, both, b_alone = case(whole, d0, k)
    ma, mb = build(base, d0), build(b_alone, k)
    shapes = None
    for _ in range(4):
        m = ma.merge(mb)
        shapes = dict(a=ma.shape(), b=mb.shape(), merged=m.shape())
        m.close()
    with open(out, "w") as f:
        json.dump(shapes, f)


def trace(outdir):
    os.makedirs(outdir, exist_ok=True)
    shapes_file = os.path.join(outdir, "traced_shapes.json")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "master_merge", "--",
           sys.executable, os.path.abspath(__file__), "--traced-child", shapes_file]
    with open(os.path.join(outdir, "rocprofv3_stderr.txt"), "w") as err:
        subprocess.run(cmd, check=True, timeout=900, stderr=err)
    files = sorted(glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        raise RuntimeError("no kernel_stats.csv under " + outdir)
    with open(shapes_file) as f:
        shapes = json.load(f)
    need = fill_bytes(shapes["a"], shapes["b"], shapes["merged"])
    per, merge_ns = {}, 0.0
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            if "k_merge_" not in row["Name"]:
                continue
            merge_ns += float(row["TotalDurationNs"])
            for name in FILL_KERNELS:
                if name in row["Name"]:
                    mean_s = float(row["AverageNs"]) * 1e-9
                    per[name] = dict(calls=int(row["Calls"]), mean_us=mean_s * 1e6, bytes=int(need[name]), bytes_per_s=need[name] / mean_s,
                                     hbm_peak_fraction=need[name] / mean_s / HBM_PEAK)
    return dict(a_organisms=TRACED[0], b_organisms=TRACED[1], shapes=shapes, merges=4, merge_kernels_total_us=merge_ns * 1e-3, kernels=per)


def report(res):
    lines = ["# Merging two resident masters", "",
             "`profiles/master_merge.py`: `Master.merge` (B's master resident) against `Master.from_orders` of the concatenated orders",
             "(\"rebuild\") and `Master.add_orders` of B's orders (\"append\"), %d families, the median of %d calls after a warm-up call;" % (N_FAM, res["repeats"]),
             "bytes: what one call copies host to device / device to host, from the shapes.", "",
             "| A organisms | B organisms | merge s | merge min - max s | append s | rebuild s | rebuild / merge | append / merge | merge bytes up / down | append bytes up / down | rebuild bytes up / down |",
             "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in res["rows"]:
        b = lambda k: "%d / %d" % (r[k]["up"], r[k]["down"])
        lines.append("| %d | %d | %.4f | %.4f - %.4f | %.4f | %.4f | %.1f | %.1f | %s | %s | %s |" % (
            r["a_organisms"], r["b_organisms"], r["merge_s"], min(r["merge_all"]), max(r["merge_all"]), r["append_s"], r["rebuild_s"],
            r["rebuild_over_merge"], r["append_over_merge"],
            b("merge_bytes"), b("append_bytes"), b("rebuild_bytes")))
    slower = [r for r in res["rows"] if r["rebuild_over_merge"] < 1.0]
    lines += ["", "The merge is slower than the rebuild at: " + ", ".join("%d + %d" % (r["a_organisms"], r["b_organisms"]) for r in slower) + "."
              if slower else "The merge is faster than the rebuild from orders at every shape of this run."]
    t = res.get("trace")
    if t:
        lines += ["", "## The fill kernels against the HBM peak", "",
                  "A run of its own under `rocprofv3 --kernel-trace --stats`: A of %d organisms, B of %d, %d merges; a kernel's bytes are the" % (
                      t["a_organisms"], t["b_organisms"], t["merges"]),
                  "bytes it must read plus the bytes it writes, from the shapes (the searches of the row pointers are not counted); the",
                  "peak is the specified %.0f TB/s.  All `k_merge_*` kernels of the run: %.0f us." % (HBM_PEAK * 1e-12, t["merge_kernels_total_us"]), "",
                  "| kernel | mean us | bytes | GB/s | of HBM peak |", "|---|---:|---:|---:|---:|"]
        for name, k in t["kernels"].items():
            lines.append("| `%s` | %.1f | %d | %.0f | %.1f %% |" % (name, k["mean_us"], k["bytes"], k["bytes_per_s"] * 1e-9, 100 * k["hbm_peak_fraction"]))
        lines += ["", "`k_merge_bits` moves nearly all of the bytes, one 4-byte word per lane.  Not done: 16-byte accesses where the strides",
                  "allow them.  The kernels are a small part of a call: the rest is the call's allocations, its stream and its three waits."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace", default=None, help="directory for a rocprofv3 run of its own")
    ap.add_argument("--traced-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.traced_child:
        traced_child(TRACED[0], TRACED[1], a.traced_child)
        return
    os.makedirs(a.out, exist_ok=True)
    res = dict(repeats=REPEATS, rows=table([1000, 5000], [1, 10, 100]))

    def write():
        with open(os.path.join(a.out, "master_merge.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        with open(os.path.join(a.out, "master_merge.md"), "w") as f:
            f.write(report(res))

    write()                                                   # (what was measured stays, whatever the traced run does)
    if a.trace:
        res["trace"] = trace(a.trace)
        write()


if __name__ == "__main__":
    main()
