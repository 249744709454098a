#!/usr/bin/env python3
"""Master.partition on large pangenomes (partition()'s loop over 500-organism samples with the vote on the device):
time per call, samples voted, samples/s; with --trace, the same calls once more under
`rocprofv3 --kernel-trace --stats` (a run of its own, in a child process) and the vote kernels' share of the kernel time.
Prints one JSON object; --out writes it to a file too.

    python profiles/partition_chunked.py [--reps 3] [--trace DIR] [--out FILE]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangenomenem_amd import synth  # noqa: E402
from pangenomenem_amd.chunks import Master  # noqa: E402

SHAPES = [(20000, 5000, 500), (20000, 1000, 500)]
VOTE_KERNELS = ("k_vote_classmap", "k_vote_scatter", "k_vote_scan", "k_vote_commit", "k_vote_init")


def run(reps, batch):
    out = []
    for n, d, chunk in SHAPES:
        x, (ptr, idx), eb = synth.master_pangenome(n, d, 1)
        m = Master(x, ptr, idx, eb)
        _, _, warm = m.partition(chunk_size=chunk, rng=random.Random(100), batch=batch)      # (warm-up: every shape of the loop)
        times, samples = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            _, _, s = m.partition(chunk_size=chunk, rng=random.Random(r), batch=batch)
            times.append(time.perf_counter() - t0)
            samples.append(s)
        m.close()
        out.append(dict(families=n, organisms=d, chunk_size=chunk, batch=batch, warmup_samples=warm, seconds_per_call=times, samples_voted=samples,
                        samples_per_second=[s / t for s, t in zip(samples, times)],
                        batches_per_call=[-(-s // batch) for s in samples]))
    return out


def trace(outdir, batch):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "partition", "--",
           sys.executable, os.path.abspath(__file__), "--reps", "1", "--batch", str(batch), "--out", os.path.join(outdir, "traced.json")]
    subprocess.run(cmd, check=True, timeout=1200)
    with open(os.path.join(outdir, "traced.json")) as f:
        traced = json.load(f)["calls"]
    batches = sum(-(-c["warmup_samples"] // batch) + -(-c["samples_voted"][0] // batch) for c in traced)
    files = sorted(glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        raise RuntimeError("no kernel_stats.csv under " + outdir)
    total, vote, per = 0.0, 0.0, {}
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            name = row["Name"]
            for k in VOTE_KERNELS:
                if k in name:
                    vote += ns
                    per[k] = dict(calls=int(row["Calls"]), total_us=ns * 1e-3, mean_us=float(row["AverageNs"]) * 1e-3)
    per_batch = sum(v["total_us"] for k, v in per.items() if k != "k_vote_init") / batches
    return dict(stats_file=os.path.relpath(files[-1], outdir), kernel_time_ms=total * 1e-6, vote_kernel_time_ms=vote * 1e-6,
                vote_share=vote / total if total else None, vote_kernels=per, batches=batches, vote_us_per_batch=per_batch,
                note="traced run: per shape one warm-up and one call (seed 0), every batch of both counted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--trace", default=None, help="directory for a rocprofv3 run of its own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(workload="Master.partition, synth.master_pangenome", calls=run(a.reps, a.batch))
    if a.trace:
        res["trace"] = trace(a.trace, a.batch)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
