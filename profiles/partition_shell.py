#!/usr/bin/env python3
"""Forming partition_shell's sub-problem on the device (nemgpu_master_subproblem) against the host route it replaces
(Master.arrays(), shell.form_subproblem_host, then NemEngine + set_matrix + set_graph), and the 50-start run for scale.
A counts master of 20 000 families x 500 organisms (synth.master_pangenome_counts); the selection: the third of the
families whose presence is nearest to half the organisms (shell-like).  Both routes end in an engine that holds the
problem, and each timing ends in the same small read-back that waits for the engine's stream.  Per figure the median of
5 calls in one process after one warm-up call.  The two problems are compared bit for bit first.  Writes the figures as
JSON (default profiles/partition_shell.json); profiles/partition_shell.md carries the table.  No threshold anywhere.

    python profiles/partition_shell.py [families organisms] [--out PATH]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangenomenem_amd import synth  # noqa: E402
from pangenomenem_amd.chunks import Master, pack_rows  # noqa: E402
from pangenomenem_amd.engine import NemEngine  # noqa: E402
from pangenomenem_amd.shell import Subproblem, _bind, form_subproblem_host  # noqa: E402

REPEATS = 5
Q = 4
SEED = 7


def timed(call, repeats=REPEATS):
    call()                                                    # warm-up
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def wait(lib, eng, n):
    """ends a timing: the engine's row pointers read back, behind everything enqueued on its stream"""
    ptr = np.zeros(n + 1, np.int32)
    assert lib.nemgpu_subproblem_fetch(eng._h, None, ptr.ctypes.data, None, None) == 0
    return ptr


def main():
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n, d = sizes if len(sizes) == 2 else (20000, 500)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "partition_shell.json")
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(n, d, SEED)
    pc = x.sum(axis=1).astype(np.int64)
    select = np.zeros(n, bool)
    select[np.argsort(np.abs(2 * pc - d), kind="stable")[:n // 3]] = True
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    lib = _bind(m.lib)
    organisms = np.arange(d)
    res = dict(families=n, organisms=d, csr_entries=int(len(idx)), multi_copy_pairs=int(len(counts[1])), selected=int(select.sum()), Q=Q,
               repeats=REPEATS)

    def device():
        sub = Subproblem(m, select, Q)
        wait(lib, sub.engine, sub.n)
        return sub

    def host():
        rows, (mptr, midx), meb, mcounts, _ = m.arrays()
        mx = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :d]
        xs, nei, fam = form_subproblem_host(mx, mptr, midx, meb, organisms, select, mcounts)
        eng = NemEngine(len(fam), d, Q)
        eng.set_matrix(xs)
        eng.set_graph(nei)
        wait(lib, eng, len(fam))
        return eng, xs, nei, fam

    # the same problem first
    sub = device()
    eng, xs, (hp, hi, hw), fam = host()
    rows, (p, i, w) = sub.fetch()
    assert np.array_equal(sub.families, fam) and np.array_equal(rows, pack_rows(xs))
    assert np.array_equal(p, hp) and np.array_equal(i, hi) and np.array_equal(w.view(np.uint32), hw.view(np.uint32))
    res["sub_families"], res["sub_entries"] = int(sub.n), int(sub.nnz)
    eng.close()
    sub.close()

    def device_once():
        device().close()

    def host_once():
        host()[0].close()

    res["device_formation_s"], res["device_formation_all"] = timed(device_once)
    res["host_route_s"], res["host_route_all"] = timed(host_once)

    # the host route's parts, one after the other
    def part_fetch():
        return m.arrays()

    got = m.arrays()
    mx = np.unpackbits(got[0].view(np.uint8), axis=1, bitorder="little")[:, :d]

    def part_form():
        return form_subproblem_host(mx, got[1][0], got[1][1], got[2], organisms, select, got[3])

    def part_upload():
        e = NemEngine(len(fam), d, Q)
        e.set_matrix(xs)
        e.set_graph((hp, hi, hw))
        wait(lib, e, len(fam))
        e.close()

    res["host_fetch_s"] = timed(part_fetch)[0]
    res["host_form_s"] = timed(part_form)[0]
    res["host_upload_s"] = timed(part_upload)[0]

    # the 50-start run on the device-formed engine, for scale
    sub = device()
    sub.engine.configure(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, tie="libc", seed=SEED)
    status = []

    def run():
        status.append(sub.engine.run_random(50, SEED)["status"])

    res["run_50_starts_s"], res["run_50_starts_all"] = timed(run, 3)
    res["run_status"] = int(status[-1])
    sub.close()
    m.close()
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
