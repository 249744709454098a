#!/usr/bin/env python3
"""Where the tail of a relaxation round spends its time (development probe, sibling of entry_loads_phases.py): a library
built with -DNEM_PHASE_PROF stamps the 100 MHz wall clock in the first block's first thread at sweep_body's phase
boundaries -- slots 0-4 the head (entry_loads_phases.py), 5 behind the first tail barrier, 6 behind the flag publication,
7 behind the last count add issued (the block's last instruction ahead of the ticket).  The counting instance stamps a
copy of its own (nemgpu_debug_sweep_phases_count), so a cycle's last plain round does not overwrite it.

    python3 profiles/sweep_tail_phases.py [--dir DIR | --lib FILE.so] [--build-only] [--cycles 20] [--out FILE.json]

configs[1]'s engine loop, graphs off.  The counting round is read after restarts of 1, 2 and 3 iterations: the last
counting round that got past its stop test is then the one of iteration 1, 2 or 3, where labels still move and both
flags are reported.  The plain round is read after a whole cycle: the last round the cycle launched on its own.
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

PHASES = [(1, "past the stop and previous-round tests"), (2, "head barrier"), (3, "first four neighbours (counting: rows asked for when late)"),
          (4, "block-local steps done, labels stored"), (5, "behind the first tail barrier"), (6, "flags published"),
          (7, "last count add issued")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--lib", default=None, help="an instrumented library built elsewhere")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lib:
        lib_path = args.lib
    else:
        from profiles.entry_loads_phases import build_instrumented
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
    for f in (lib.nemgpu_debug_sweep_phases, lib.nemgpu_debug_sweep_phases_count):
        f.argtypes = [C.POINTER(C.c_ulonglong)]

    def read(f):
        s = (C.c_ulonglong * 8)()
        if f(s) != 0:
            raise SystemExit("reading the stamps failed")
        # (a round that leaves behind its entry tests stamps slots 0 and 1 only: the rest is then an earlier launch's)
        v = [(int(s[i]) - int(s[0])) / 100.0 for i, _ in PHASES]
        return v if all(0.0 <= t <= 100.0 for t in v) else None

    x, nei, prop, center, disp, disper, _ = bench.make_workload(20000, 500, 3, "ushape", 2)
    run = bench.EngineRun(x, nei, 3, prop, center, disp, "ncem", 0.5, "sk_", tie="hash")
    run.prime(run.cycle * 4, run.cycle)
    plain, count = [], {1: [], 2: [], 3: []}
    for _ in range(args.cycles):
        for m in (1, 2, 3):
            run.eng.restart_iterate(m)
            count[m].append(read(lib.nemgpu_debug_sweep_phases_count))
        run.run_steps(run.cycle)
        plain.append(read(lib.nemgpu_debug_sweep_phases))
    run.eng.close()

    def table(rows):
        kept = [v for v in rows if v is not None]
        t = {name: statistics.median(v[j] for v in kept) for j, (_, name) in enumerate(PHASES)} if kept else {}
        t["samples"] = len(kept)
        return t

    out = {"unit": "us since block 0's entry, thread 0, median over %d restart cycles (100 MHz clock: 0.01 us steps)" % args.cycles,
           "counting_round": {"iteration %d" % m: table(count[m]) for m in (1, 2, 3)},
           "counting_round_iterations_1_to_3": table(count[1] + count[2] + count[3]),
           "plain_round": table(plain)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
