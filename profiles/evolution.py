#!/usr/bin/env python3
"""Master.evolution -- the CLI's --evolution curve from one master -- against a loop of Master.partition(just_stats=True)
over the same resamples in the same process: seconds per curve, resamples per second, and whether both give the same
rows and leave the generator in the same state.  With --trace, the curves alone once more under
`rocprofv3 --kernel-trace --stats` (a run of its own, in a child process) and the time of the two resample kernels.
Prints one JSON object; --out writes it to a file too.

    python profiles/evolution.py [--reps 2] [--case NAME ...] [--no-loop] [--trace DIR] [--out FILE]
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
from pangenomenem_amd.evolution import STATS, evolution_resamples  # noqa: E402

# name, families, organisms, chunk_size, -ep (ratio, min, max, step, limit), vote batch of the large resamples
CASES = [("all_small_20000x200", 20000, 200, 500, (0.1, 10, 30, 1, None), 64),
         ("mixed_5000x600", 5000, 600, 500, (0.1, 2, 30, 1, None), 8)]
KERNELS = ("k_resample_core", "k_resample_tally", "k_vote_classmap")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def loop(m, rng, chunk, ep, batch):
    """the reference's --cpu 1 worker: one Master.partition(just_stats=True) per resample, in shuffled order"""
    rows = []
    for r in evolution_resamples(m.d, *ep, rng=rng):
        st = m.partition(organisms=r, chunk_size=chunk, rng=rng, batch=batch, just_stats=True)[0]
        rows.append([len(r)] + [st[s] for s in STATS])
    return np.array(rows, np.int64)


def run(reps, with_loop, cases):
    out = []
    for name, n, d, chunk, ep, batch in CASES:
        if cases and name not in cases:
            continue
        x, (ptr, idx), eb = synth.master_pangenome(n, d, 1)
        m = Master(x, ptr, idx, eb)
        m.evolution(random.Random(100), *ep, chunk_size=chunk, batch=batch)          # (warm-up)
        times = []
        for r in range(reps):
            rng = random.Random(r)
            t0 = time.perf_counter()
            rows = m.evolution(rng, *ep, chunk_size=chunk, batch=batch)
            times.append(time.perf_counter() - t0)
            log(name, "curve", r, "%.3f s" % times[-1])
        state = rng.getstate()
        count = len(rows)
        res = dict(case=name, families=n, organisms=d, chunk_size=chunk, ep=list(ep), vote_batch=batch, resamples=count,
                   large_resamples=int(np.count_nonzero(rows[:, 0] > chunk)), seconds_per_curve=times,
                   resamples_per_second=[count / t for t in times],
                   rows_with_undefined=int(np.count_nonzero(rows[:, 4])))
        if with_loop:
            rng = random.Random(reps - 1)
            t0 = time.perf_counter()
            want = loop(m, rng, chunk, ep, batch)
            t = time.perf_counter() - t0
            log(name, "loop", "%.3f s" % t)
            res.update(loop_seconds=t, loop_resamples_per_second=count / t, speedup=t / min(times),
                       rows_equal_loop=bool(np.array_equal(rows, want)), rng_state_equal_loop=rng.getstate() == state)
        m.close()
        out.append(res)
    return out


def trace(outdir, reps, cases):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "evolution", "--",
           sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--no-loop", "--out", os.path.join(outdir, "traced.json")]
    for c in cases:
        cmd += ["--case", c]
    with open(os.path.join(outdir, "rocprofv3_stderr.txt"), "w") as err:
        subprocess.run(cmd, check=True, timeout=1200, stderr=err)
    files = sorted(glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not files:
        raise RuntimeError("no kernel_stats.csv under " + outdir)
    total, per = 0.0, {}
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            for k in KERNELS:
                if k in row["Name"]:
                    per[k] = dict(calls=int(row["Calls"]), total_us=ns * 1e-3, mean_us=float(row["AverageNs"]) * 1e-3)
    mine = sum(per[k]["total_us"] for k in ("k_resample_core", "k_resample_tally") if k in per)
    return dict(stats_file=os.path.relpath(files[-1], outdir), kernel_time_ms=total * 1e-6, kernels=per,
                resample_kernel_share=mine * 1e3 / total if total else None,
                note="traced run: per case one warm-up and %d curve(s), no per-resample loop; k_vote_classmap also runs in "
                     "the large resamples' vote loops" % reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-loop", action="store_true", help="skip the per-resample Master.partition loop")
    ap.add_argument("--case", action="append", default=[], help="run only these cases (default: all)")
    ap.add_argument("--trace", default=None, help="directory for a rocprofv3 run of its own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def write(res):
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    res = dict(workload="Master.evolution vs a Master.partition(just_stats=True) loop, synth.master_pangenome",
               cases=run(a.reps, not a.no_loop, a.case))
    write(res)                                                # (what was measured stays, whatever the traced run does)
    if a.trace:
        res["trace"] = trace(a.trace, 1, a.case)
        write(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
