#!/usr/bin/env python3
"""Step 0 of the batched fast-forward (development probe): in a library built with -DNEM_PHASE_PROF every wave of the
density launch's block 0 (tile 0, class 0) stamps the 100 MHz wall clock where its chain ends, and counts the lane steps
of chain_ff_batched and the crossing passes of either chain (nemgpu_debug_ff_waves), beside thread 0's phase stamps of
profiles/entry_loads_phases.py.  configs[1]'s engine loop, graphs off, one restart cycle at a time.

    python3 profiles/ff_batch_phases.py [--dir DIR] [--build-only] [--cycles 20] [--out FILE.json]

NEM_MI355X_FF_BATCH=0 in the environment measures the word-synchronous chain with the same library.  The counters add
up over a cycle's density launches that reach the chain (the start and seven iterations: 8); the counting itself costs
an atomic per step and pass, so the clocks of an instrumented library run a little behind a plain one's.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LAUNCHES = 8


def main():
    from entry_loads_phases import DENSITY, build_instrumented
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
    lib.nemgpu_debug_ff_waves.argtypes = [C.POINTER(C.c_ulonglong)]
    x, nei, prop, center, disp, disper, _ = bench.make_workload(20000, 500, 3, "ushape", 2)
    run = bench.EngineRun(x, nei, 3, prop, center, disp, "ncem", 0.5, "sk_", tie="hash")
    run.prime(run.cycle * 4, run.cycle)

    def waves():
        v = (C.c_ulonglong * 12)()
        if lib.nemgpu_debug_ff_waves(v) != 0:
            raise RuntimeError("nemgpu_debug_ff_waves")
        return [int(t) for t in v]
    dens, ends, steps, passes = [], [], [], []
    before = waves()
    for _ in range(args.cycles):
        run.run_steps(run.cycle)
        d = (C.c_ulonglong * 32)()
        if lib.nemgpu_debug_phases(d) != 0:
            return 1
        now = waves()
        dens.append([(int(d[i]) - int(d[16])) / 100.0 for i, _ in DENSITY])
        ends.append([(now[j] - int(d[16])) / 100.0 for j in range(4)])
        steps.append([(now[4 + j] - before[4 + j]) / LAUNCHES for j in range(4)])
        passes.append([(now[8 + j] - before[8 + j]) / LAUNCHES for j in range(4)])
        before = now
    run.eng.close()

    def med(rows):
        return [statistics.median(r[j] for r in rows) for j in range(len(rows[0]))]
    phase = dict(zip((name for _, name in DENSITY), med(dens)))
    end = med(ends)
    out = {"unit": "us since block 0's entry, median over %d restart cycles (100 MHz clock: 0.01 us steps)" % args.cycles,
           "chain": "word-synchronous" if os.environ.get("NEM_MI355X_FF_BATCH", "1")[0] == "0" else "batched",
           "density_fused_body": phase,
           "chain_end_per_wave": end,
           "slowest_wave_chain_us": round(max(end) - phase["ff tables (behind their barrier)"], 2),
           "store_behind_slowest_wave_us": round(phase["stored"] - max(end), 2),
           "lane_steps_per_wave_and_launch": med(steps), "passes_per_wave_and_launch": med(passes)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
