#!/usr/bin/env python3
"""Times for profiles/tileplot.md: the organisms of one random master clustered on the device (nemgpu_orgclust_*; needs
the GPU).  F families (default 200 000) of density one half, D organisms; the master is made from packed random words,
so no F x D byte matrix is ever built.  Per D three steps are timed, each in a process of its own that the parent starts
under `timeout` and chains (the first that fails ends the run):

    distances   nemgpu_orgclust_create: the popcounts and the distance kernel (and the allocation of the square); the
                least of three calls.  Word pairs = D (D + 1) / 2 x ceil(F / 64) (the tiles on and above the diagonal,
                whole tiles counted at their organisms); the kernel's HBM reads are about D^2 / (2 tile) rows of F / 8
                bytes, its stores 8 D^2 bytes.
    merges      nemgpu_orgclust_run: the copy of the square, the first nearest neighbours and the D - 1 merges.
    raster      nemgpu_orgclust_cells of a batch of `--rows` families in a random order, all organisms reversed; the
                least of three calls.

A host clock around each call, which ends in a synchronise.  Prints one JSON line per D and step.  --host: scipy's
pdist(..., "jaccard") and linkage(..., "complete") on the host instead, for orientation only (scipy is not the
reference), at every D where a probe at 128 organisms predicts a minute or less.

    python profiles/tileplot.py --d 2048 4096 20000
    python profiles/tileplot.py --host --d 2048 4096 20000
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

STEPS = ("distances", "merges", "raster")
LIMIT = {"distances": 240, "merges": 420, "raster": 240}       # seconds a step's process may take, master included


def random_master(f, d, seed):
    """a bits-only master of f x d random bits without a graph, from packed rows"""
    from pangenomenem_amd.chunks import Master, _bind_master
    from pangenomenem_amd.engine import NemGpuError, load_library
    rng = np.random.default_rng(seed)
    wf = (d + 31) // 32
    rows = rng.integers(0, 1 << 32, (f, wf), dtype=np.uint32)
    if d % 32:
        rows[:, -1] &= np.uint32((1 << (d % 32)) - 1)
    m = Master.__new__(Master)
    m.lib, m._h = _bind_master(load_library()), C.c_void_p()
    ptr = np.zeros(f + 1, np.int32)
    rc = m.lib.nemgpu_master_create(C.byref(m._h), 0, f, d, rows.ctypes.data, ptr.ctypes.data, None, None)
    if rc != 0:
        raise NemGpuError("nemgpu_master_create failed (status %d): %s" % (rc, m.lib.nemgpu_last_error().decode()))
    m.n, m.d, m.wf, m._rows_host = f, d, wf, rows
    m.order, m.directed, m.f = np.arange(f, dtype=np.int32), False, f
    return m


def clocked(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def step(name, f, d, rows, seed):
    from pangenomenem_amd import tileplot as tp
    m = random_master(f, d, seed)
    lib = tp._bind_orgclust(m.lib)
    tile, chunk, _ = tp.tile_info(lib)
    out = dict(step=name, families=f, organisms=d, tile=tile, chunk_words=chunk)

    def create():
        h = C.c_void_p()
        rc = lib.nemgpu_orgclust_create(C.byref(h), m._h)
        assert rc == 0, lib.nemgpu_last_error().decode()
        return h

    if name == "distances":
        times = []
        for _ in range(3):
            t, h = clocked(create)
            times.append(t)
            lib.nemgpu_orgclust_destroy(h)
        nw = (f + 63) // 64
        pairs = d * (d + 1) // 2 * nw
        tiles = (d + tile - 1) // tile
        read = tiles * (tiles + 1) // 2 * 2 * min(tile, d) * nw * 8
        out.update(seconds=min(times), all_seconds=times, word_pairs=pairs, word_pairs_per_s=pairs / min(times),
                   hbm_read_bytes=read, hbm_write_bytes=8 * d * d, hbm_bytes_per_s=(read + 8 * d * d) / min(times))
    else:
        h = create()
        if name == "merges":
            i2, j2, height = np.zeros(d - 1, np.int32), np.zeros(d - 1, np.int32), np.zeros(d - 1)
            t, rc = clocked(lambda: lib.nemgpu_orgclust_run(h, i2.ctypes.data, j2.ctypes.data, height.ctypes.data))
            assert rc == 0, lib.nemgpu_last_error().decode()
            assert (np.diff(height) >= 0).all() and (i2 < j2).all()
            out.update(seconds=t, merges=d - 1, microseconds_per_merge=1e6 * t / (d - 1), last_height=float(height[-1]))
        else:
            rng = np.random.default_rng(seed + 1)
            fam, org = rng.permutation(f).astype(np.int32), np.arange(d - 1, -1, -1, dtype=np.int32)
            rows = min(rows, f)
            cells = np.zeros((rows, d), np.uint8)
            times = []
            for _ in range(3):
                t, rc = clocked(lambda: lib.nemgpu_orgclust_cells(h, fam.ctypes.data, org.ctypes.data, 0, rows, cells.ctypes.data))
                assert rc == 0, lib.nemgpu_last_error().decode()
                times.append(t)
            out.update(seconds=min(times), all_seconds=times, rows=rows, cells=rows * d, cells_per_s=rows * d / min(times), ones=int(cells.sum()))
        lib.nemgpu_orgclust_destroy(h)
    m.close()
    print(json.dumps(out), flush=True)


def host(f, sizes, seed):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    rng = np.random.default_rng(seed)
    probe_d = 128
    x = rng.random((probe_d, f)) < 0.5
    probe, _ = clocked(lambda: pdist(x, "jaccard"))
    for d in sizes:
        predicted = probe * (d / probe_d) ** 2
        out = dict(step="scipy", families=f, organisms=d, predicted_pdist_seconds=predicted)
        if predicted <= 60:
            x = rng.random((d, f)) < 0.5
            out["pdist_seconds"], cond = clocked(lambda: pdist(x, "jaccard"))
            out["linkage_seconds"], _ = clocked(lambda: linkage(cond, "complete"))
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, nargs="+", default=[2048, 4096, 20000])
    ap.add_argument("--f", type=int, default=200000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.host:
        return host(a.f, a.d, a.seed)
    if a.step:
        return step(a.step, a.f, a.d[0], a.rows, a.seed)
    for d in a.d:
        for name in STEPS:
            cmd = ["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--d", str(d),
                   "--f", str(a.f), "--rows", str(a.rows), "--seed", str(a.seed)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print("step %s at %d organisms ended with status %d: nothing more is started" % (name, d, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
