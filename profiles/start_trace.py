"""configs[1] (the headline's matrix and graph) as bench.py's engine loop runs it, 40 restart cycles of 7 iterations, for
a kernel trace of a run's fixed cost: with NEM_MI355X_GRAPHS=0 every launch of a start shows under its own name
(k_finish + k_density, or k_density_start alone).  Host time per cycle goes to stderr."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
x, nei, prop, center, disp, disper, _ = bench.make_workload(20000, 500, 3, "ushape", 2)
run = bench.EngineRun(x, nei, 3, prop, center, disp, "ncem", 0.5, "sk_", tie="hash")
run.prime(run.cycle * 4, run.cycle)
t0 = time.perf_counter()
run.run_steps(run.cycle * 40)
dt = time.perf_counter() - t0
print("%.4f ms per step (%d iterations per cycle)" % (dt * 1e3 / (run.cycle * 40), run.cycle), file=sys.stderr)
run.eng.close()
