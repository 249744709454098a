#!/usr/bin/env python3
"""Where the prologue of the fused density launch spends its time, stamp by stamp (development probe; a sibling of
entry_loads_phases.py with the finer stamps of round 13): a library built with -DNEM_PHASE_PROF stamps the 100 MHz wall
clock in the first block's first thread around the class constants (log(pk) on its own), the arrival of the entry loads,
the centres, epsilon, the class's logs, ff_build, the tables' barrier and word 0 of the chain.  The script builds that
library itself into a scratch directory (never into pangenomenem_amd/lib) and runs configs[1]'s engine loop on it, graphs
off, one restart cycle at a time, reading the stamps after each cycle.

    python3 profiles/density_prologue_phases.py [--dir DIR] [--build-only] [--cycles 20] [--out FILE.json]

--dir: where the instrumented library is built and kept (default: a temporary directory); a library already there is used
as it is, so that it can be built where there is no GPU and run where there is one.
The stamps are those of the LAST density launch that got past its stop test (the seventh iteration's k_density_verify).
A stamp behind a value waits for that value (an empty asm that reads it); "entry loads in" waits for every load the thread
has asked for, which the build without stamps does a few instructions later, where the centres read the counts.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAMPS = [(16, "entry (tile known, loads asked for)"), (17, "past the stop test"), (13, "proportion stored, ahead of log(pk)"),
          (14, "log(pk)"), (18, "class constants, zeroing loops"), (15, "entry loads in"),
          (19, "centres and masks (behind their barrier)"), (20, "epsilon"), (25, "the class's log call (before round 13: the first of two)"),
          (26, "the class's logs (l1 and l0)"), (27, "ff_build (own table entry stored)"), (21, "ff tables (behind their barrier)"),
          (28, "word 0 stepped"), (22, "chain"), (23, "stored")]


def build_instrumented(where):
    from pangenomenem_amd import build as b
    lib = os.path.join(where, "libnem_mi355x.so")
    if os.path.isfile(lib):
        return lib
    b.LIB, b.OBJ = lib, os.path.join(where, "obj")
    os.environ["NEM_EXTRA_HIPCC_FLAGS"] = (os.environ.get("NEM_EXTRA_HIPCC_FLAGS", "") + " -DNEM_PHASE_PROF").strip()
    b.build(force=True)
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    where = args.dir or tempfile.mkdtemp(prefix="nem_phase_prof_")
    os.makedirs(where, exist_ok=True)
    lib_path = build_instrumented(where)
    print("instrumented library:", lib_path, file=sys.stderr)
    if args.build_only:
        return 0
    os.environ["NEM_MI355X_LIB"] = lib_path           # (read when pangenomenem_amd.engine is imported)
    os.environ["NEM_MI355X_GRAPHS"] = "0"
    import bench
    from pangenomenem_amd.engine import load_library
    lib = load_library()
    lib.nemgpu_debug_phases.argtypes = [C.POINTER(C.c_ulonglong)]
    x, nei, prop, center, disp, disper, _ = bench.make_workload(20000, 500, 3, "ushape", 2)
    run = bench.EngineRun(x, nei, 3, prop, center, disp, "ncem", 0.5, "sk_", tie="hash")
    run.prime(run.cycle * 4, run.cycle)
    rows = []
    for _ in range(args.cycles):
        run.run_steps(run.cycle)
        d = (C.c_ulonglong * 32)()
        if lib.nemgpu_debug_phases(d) != 0:
            return 1
        rows.append([(int(d[i]) - int(d[16])) / 100.0 for i, _ in STAMPS])
    run.eng.close()
    out = {"unit": "us since the block's entry, block 0 / thread 0, median over %d restart cycles (100 MHz clock: 0.01 us steps)" % args.cycles,
           "density_fused_body": {name: statistics.median(v[j] for v in rows) for j, (_, name) in enumerate(STAMPS)}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
