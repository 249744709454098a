#!/usr/bin/env python3
"""ms per EM iteration of a masked NCEM run (10 % of the cells missing) beside the unmasked run of the same matrix.

    python profiles/missing_profile.py [--families 20000] [--organisms 500] [--iters 20] [--repeats 7] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/missing_profile.py --masked-only

Both runs take a fixed number of iterations (convergence test off), from the same parameters; the time is the engine's
own clock around its loop (nemgpu_run's loop_seconds: a host clock around work that ends in a stream synchronise),
the median over the repeats behind one warm-up run.  The per-kernel times of k_density_masked, k_mstep_counts_masked and
k_finish_masked come from the rocprofv3 run (its --stats table), not from this script.  Results: profiles/missing.md.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pangenomenem_amd import synth  # noqa: E402
from pangenomenem_amd.engine import NemEngine  # noqa: E402


def timed(x, obs, nei, prop, center, disp, iters, repeats):
    n, d = x.shape
    eng = NemEngine(n, d, 3)
    try:
        eng.set_matrix(x)
        if obs is not None:
            eng.set_observed(obs)
        eng.set_graph(nei)
        eng.set_params(prop, center, disp)
        eng.configure(algo="ncem", beta=0.5, disper="sk_", cvtest="none", it_max=iters, tie="hash", seed=1)
        ms = []
        for rep in range(repeats + 1):
            r = eng.run()
            if r["iters"] != iters or r["status"] != 0:
                raise SystemExit("the run ended after %d of %d iterations with status %d: choose another shape"
                                 % (r["iters"], iters, r["status"]))
            if rep > 0:
                ms.append(1e3 * r["loop_seconds"] / iters)
        return dict(ms_per_iteration_median=float(np.median(ms)), ms_per_iteration_min=float(min(ms)),
                    ms_per_iteration_max=float(max(ms)), repeats=repeats, iterations=iters)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=20000)
    ap.add_argument("--organisms", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--missing", type=float, default=0.10)
    ap.add_argument("--masked-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d = a.families, a.organisms
    x, _ = synth.ushaped_pa_matrix(n, d, 3)
    nei = synth.contiguity_graph(n, 3)
    prop, center, disp = synth.default_init(d)
    obs = np.random.Generator(np.random.PCG64(4)).random((n, d)) >= a.missing
    out = dict(families=n, organisms=d, missing_fraction=float(1.0 - obs.mean()))
    if not a.masked_only:
        out["unmasked"] = timed(x, None, nei, prop, center, disp, a.iters, a.repeats)
    out["masked"] = timed(x, obs, nei, prop, center, disp, a.iters, a.repeats)
    text = json.dumps(out, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
