#!/usr/bin/env python3
"""Master.partition on a 20 000 x 5 000 pangenome with occurrence counts (nemgpu_master_create_counts) against the same
graph as a bits-only master: time per call, samples voted, and with --trace the kernel time of k_chunk_cov per launch,
bits-only (k_chunk_cov<false>) against counts (k_chunk_cov<true>), from `rocprofv3 --kernel-trace --stats` runs of their
own (child processes).  Masters (synth.master_pangenome_counts):
  * plain   -- synth.master_pangenome, the workload of profiles/partition_chunked.py;
  * bits    -- the counts generator's graph (the plain one plus ~200 tandem self-loops) without its counts;
  * counts  -- the same with its counts: ~2 % of the carried (edge, organism) pairs multi-copy, and 4 dense self-loops
               on the families present in the most organisms (each ~5 000 extras: walked by the whole wave).
Prints one JSON object; --out writes it to a file too.

    python profiles/partition_counts.py [--reps 5] [--trace DIR] [--out FILE]
"""
import argparse
import csv
import glob
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangenomenem_amd import synth  # noqa: E402
from pangenomenem_amd.chunks import Master  # noqa: E402

N, D, CHUNK = 20000, 5000, 500
VARIANTS = ("plain", "bits", "counts")


def master(variant):
    if variant == "plain":
        x, (ptr, idx), eb = synth.master_pangenome(N, D, 1)
        return Master(x, ptr, idx, eb), dict(nnz=len(idx))
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(N, D, 1, multi_frac=0.015, dense_loops=4)
    carried = int(np.unpackbits(eb.view(np.uint8), axis=1).sum())
    info = dict(nnz=len(idx), carried_pairs=carried, multi_copy_pairs=int(counts[0][-1]),
                multi_copy_share=int(counts[0][-1]) / carried, max_extras_per_edge=int(np.diff(counts[0]).max()))
    return Master(x, ptr, idx, eb, edge_counts=counts if variant == "counts" else None), info


def run(variants, reps, batch):
    out = []
    for v in variants:
        m, info = master(v)
        _, _, warm = m.partition(chunk_size=CHUNK, rng=random.Random(100), batch=batch)      # (warm-up)
        times, samples = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            _, _, s = m.partition(chunk_size=CHUNK, rng=random.Random(r), batch=batch)
            times.append(time.perf_counter() - t0)
            samples.append(s)
        m.close()
        out.append(dict(variant=v, families=N, organisms=D, chunk_size=CHUNK, batch=batch, warmup_samples=warm, seconds_per_call=times,
                        samples_voted=samples, ms_per_sample=[1e3 * t / s for t, s in zip(times, samples)], **info))
    return out


def trace(outdir, batch):
    res = {}
    for v in ("bits", "counts"):
        d = os.path.join(outdir, v)
        os.makedirs(d, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "partition", "--",
               sys.executable, os.path.abspath(__file__), "--variants", v, "--reps", "1", "--batch", str(batch)]
        subprocess.run(cmd, check=True, timeout=900)
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
        if not files:
            raise RuntimeError("no kernel_stats.csv under " + d)
        total, kernels = 0.0, {}
        with open(files[-1]) as f:
            for row in csv.DictReader(f):
                total += float(row["TotalDurationNs"])
                if "k_chunk_" in row["Name"]:
                    kernels[row["Name"].split("(")[0]] = dict(calls=int(row["Calls"]), total_us=float(row["TotalDurationNs"]) * 1e-3,
                                                              mean_us=float(row["AverageNs"]) * 1e-3, min_us=float(row["MinNs"]) * 1e-3,
                                                              max_us=float(row["MaxNs"]) * 1e-3)
        res[v] = dict(stats_file=os.path.relpath(files[-1], outdir), kernel_time_ms=total * 1e-6, chunk_kernels=kernels)
    res["note"] = "traced runs: one warm-up and one call (seed 0) per master; k_chunk_cov launches once per batch of 64 samples"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--trace", default=None, help="directory for rocprofv3 runs of their own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(workload="Master.partition, synth.master_pangenome_counts %d x %d, chunk_size %d" % (N, D, CHUNK),
               calls=run(a.variants.split(","), a.reps, a.batch))
    if a.trace:
        res["trace"] = trace(a.trace, a.batch)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
