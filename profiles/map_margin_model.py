#!/usr/bin/env python3
"""What the rows of an NCEM sweep look like on the headline data (host model, no GPU): the CPU oracle's run of bench.py's
configs[1] workload is stopped after 0, 1, 2, 4 and 7 iterations; from its labels and parameters the rows
cinum[k] = pkf[k] * exp(beta * ctx[k]) of the next sweep are rebuilt (contexts from the labels the sweep starts from)
and looked at the way csrc/nem_map.hpp does:

  * the share of sites whose sum is at most EPSILON = 1e-20 (the five-division branch of ComputeLocalProba);
  * the waves (64 consecutive sites) that hold both kinds of site;
  * the rows that are NOT clear at the margin 2^-16 (near ties, zero sums, maxima below the floor), and the subnormal
    entries;
  * the block-local steps of round 0 of that sweep (256 sites per block, Jacobi steps on the block's own lower
    neighbours until nothing in the block moves, sweep_body's inner loop): slowest block and mean per block.

    python3 profiles/map_margin_model.py [--out profiles/r11_map_margin_model.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPSILON, MARGIN, FLOOR, BLOCK = 1e-20, 2.0 ** -16, 2.0 ** -1000, 256


def contexts(ptr, idx, w, lab, k):
    site = np.repeat(np.arange(len(lab)), np.diff(ptr))
    ctx = np.zeros((len(lab), k), np.float32)
    np.add.at(ctx, (site, lab[idx]), w)
    return ctx


def rows(pk, ctx, beta):
    with np.errstate(all="ignore"):
        return pk * np.exp(np.float64(np.float32(beta)) * ctx.astype(np.float64))


def block_steps(pk, ptr, idx, w, old, beta, k):
    """round 0 of a sweep from the partition `old`: passes of sweep_body's inner loop per block (the pass that moves
    nothing included)"""
    n = len(old)
    site = np.repeat(np.arange(n), np.diff(ptr))
    local = (idx < site) & (idx // BLOCK == site // BLOCK)          # a lower neighbour held by the site's own block
    cur = old.copy()
    steps = np.zeros((n + BLOCK - 1) // BLOCK, np.int64)
    live = np.ones(len(steps), bool)
    for _ in range(64):
        seen = np.where(local, cur[idx], old[idx])
        ctx = np.zeros((n, k), np.float32)
        np.add.at(ctx, (site, seen), w)
        nxt = rows(pk, ctx, beta).argmax(1)
        moved = np.add.reduceat((nxt != cur) & live[np.arange(n) // BLOCK], np.arange(0, n, BLOCK)) > 0
        steps += live
        cur = np.where(live[np.arange(n) // BLOCK], nxt, cur)
        live &= moved
        if not live.any():
            break
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_map_margin_model.json"))
    args = ap.parse_args()
    import bench
    from oracle.pyoracle import Oracle
    oracle = Oracle()
    n, d, k, beta = 20000, 500, 3, 0.5
    x, nei, prop, center, disp, disper, what = bench.make_workload(n, d, k, "ushape", 2)
    ptr, idx, w = (np.asarray(a) for a in nei)
    out = {"workload": what, "margin": "2^-16", "floor": "2^-1000", "sweeps": []}
    for m in (0, 1, 2, 4, 7):
        r = oracle.run(x, nei, k, prop, center, disp, algo="ncem", beta=beta, disper=disper, propor="pk", cvtest="none",
                       it_max=m, tie="hash", seed=1)
        lab = r["c"].argmax(1)
        pk = oracle.density(x, r["prop"], r["center"], r["disp"])[0]
        c = rows(pk, contexts(ptr, idx, w, lab, k), beta)
        cum = c.sum(1)
        s = np.sort(c, axis=1)
        v1, v2 = s[:, -1], s[:, -2]
        clear = (cum > 0) & np.isfinite(cum) & (v1 >= FLOOR) & (v2 <= v1 * (1.0 - MARGIN))
        small = cum <= EPSILON
        pad = (-n) % 64
        sm = np.concatenate([small, np.zeros(pad, bool)]).reshape(-1, 64)
        valid = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(-1, 64)
        mixed = ((sm & valid).any(1)) & ((~sm & valid).any(1))
        notclear = np.concatenate([~clear, np.zeros(pad, bool)]).reshape(-1, 64).any(1)
        steps = block_steps(pk, ptr, idx, w, lab, beta, k)
        tiny = np.finfo(np.float64).tiny
        out["sweeps"].append({
            "after_iterations": m,
            "share_of_sites_with_sum_at_most_epsilon": float(small.mean()),
            "waves": int(len(mixed)), "waves_with_both_kinds_of_site": int(mixed.sum()),
            "rows_not_clear": int((~clear).sum()), "waves_with_a_row_not_clear": int(notclear.sum()),
            "rows_with_zero_sum": int((~(cum > 0)).sum()),
            "rows_whose_two_largest_are_within_1_plus_2^-20": int(((v2 > 0) & (v1 <= v2 * (1.0 + 2.0 ** -20))).sum()),
            "subnormal_entries": int(((c > 0) & (c < tiny)).sum()),
            "subnormal_row_maxima": int(((v1 > 0) & (v1 < tiny)).sum()),
            "block_local_steps_round0": {"slowest_block": int(steps.max()), "mean_per_block": float(steps.mean())},
        })
        print(json.dumps(out["sweeps"][-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
