"""The shadow-verify schedule of the pipelined NCEM loop (a sweep's verifying round and the loop control run inside the
next iteration's density launch, nem_engine.hip shadow_batch_enqueue) against the schedule without it
(NEM_MI355X_SHADOW_VERIFY=0): the same labels, parameters, criteria, iteration counts and status, bit for bit -- across
batch boundaries, runs that stop mid-batch, host-finished sweeps, deep iterations, empty classes and many restarts of
one engine -- and the oracle's answer on the configs[1]-like workload."""
import os

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

SKIP_KEYS = {"loop_seconds"}


def make_engine(shadow, n, d, k, x, nei, prop, center, disp, env=None, **cfg):
    from pangenomenem_amd.engine import NemEngine
    saved = {}
    env = dict(env or {})
    env["NEM_MI355X_SHADOW_VERIFY"] = "1" if shadow else "0"
    for key, v in env.items():                    # (read when the engine is created)
        saved[key] = os.environ.get(key)
        os.environ[key] = v
    try:
        eng = NemEngine(n, d, k)
    finally:
        for key, v in saved.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    eng.set_matrix(x); eng.set_graph(nei); eng.set_params(prop, center, disp); eng.configure(**cfg)
    return eng


def assert_same(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        if key in SKIP_KEYS:
            continue
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.shape == v.shape and u.dtype == v.dtype, (what, key)
        assert u.tobytes() == v.tobytes(), (what, key, a[key], b[key])


def both(problem, steps, env=None, **cfg):
    """run `steps` (callables eng -> dict) on one engine per schedule; every step's outputs agree"""
    n, d, k, x, nei, prop, center, disp = problem
    outs = []
    for shadow in (False, True):
        eng = make_engine(shadow, n, d, k, x, nei, prop, center, disp, env=env, **cfg)
        try:
            res = []
            for step in steps:
                r = step(eng)
                r.update(eng.results())
                r["crit_now"] = eng.criteria()
                res.append(r)
        finally:
            eng.close()
        outs.append(res)
    for j, (a, b) in enumerate(zip(*outs)):
        assert_same(a, b, "step %d" % j)
    return outs[1]


def problem(n, d, k, weights="small", seed=3, grouped=False):
    if grouped:
        x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
        prop, center, disp = synth.kclass_init(x, k)
    else:
        x, _ = synth.ushaped_pa_matrix(n, d, seed)
        prop, center, disp = synth.default_init(d) if k == 3 else synth.kclass_init(x, k)
    nei = synth.contiguity_graph(n, seed, weights=weights, d=d)
    return n, d, k, x, nei, prop, center, disp


def restarts(*ms):
    return [lambda eng, m=m: eng.restart_iterate(m) for m in ms]


def run(eng):
    return eng.run()


def test_configs1_workload_and_restarts():
    """BASELINE configs[1]'s shape as bench.py runs it: a whole run, then restarts of 7 (one batch), 8 (across a batch
    boundary), 3 and 10 iterations (it_max reached mid-batch) on the same engine, then a whole run again"""
    p = problem(20000, 500, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, tie="hash", seed=1)
    out = both(p, [run] + restarts(7, 8, 3, 10, 7, 1, 2) + [run], **cfg)
    assert out[0]["iters"] >= 2


def test_many_restarts_one_engine():
    p = problem(20000, 500, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", cvtest="none", it_max=100, tie="hash", seed=1)
    both(p, restarts(*([7] * 12 + [5, 6, 9, 13, 14, 15, 7])), **cfg)


@pytest.mark.parametrize("weights", ["coverage", "adjacency"])
def test_host_finished_sweeps(weights):
    """heavy weights: sweeps that need more rounds than enqueued, so a speculative density is thrown away"""
    n, d = 20000, 200
    x, _ = synth.ushaped_pa_matrix(n, d, 4)
    nei = synth.contiguity_graph(n, 4, weights=weights, d=d, counts=x.sum(axis=1) if weights == "adjacency" else None)
    prop, center, disp = synth.default_init(d)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=2)
    both((n, d, 3, x, nei, prop, center, disp), [run] + restarts(7, 11, 4) + [run], **cfg)


def test_two_rounds_per_sweep_deep_mispredicts():
    p = problem(20000, 300, 3, weights="coverage", seed=6)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=3)
    both(p, [run] + restarts(7, 9) + [run], env={"NEM_MI355X_ROUNDS": "2"}, **cfg)


def test_without_graphs():
    p = problem(20000, 300, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=1)
    both(p, [run] + restarts(7, 8, 3), env={"NEM_MI355X_GRAPHS": "0"}, **cfg)


@pytest.mark.parametrize("k,tie", [(2, "hash"), (3, "first"), (4, "hash"), (5, "first"), (5, "hash")])
def test_k_and_tie_rules(k, tie):
    p = problem(9000, 64, k, grouped=True)
    cfg = dict(algo="ncem", beta=0.5, disper="skd", it_max=100, tie=tie, seed=4)
    both(p, [run] + restarts(7, 8, 1), **cfg)


def test_converges_at_once_and_at_batch_ends():
    """restarted from the converged parameters the run stops at its first iterations; it_max at 1, 7 and 8"""
    n, d, k, x, nei, prop, center, disp = problem(20000, 200, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=1)

    def from_fixed_point(eng):
        r = eng.run()
        eng.set_params(r["prop"], r["center"], r["disp"])
        return eng.run()

    def capped(m):
        def step(eng):
            eng.configure(**dict(cfg, it_max=m))
            return eng.run()
        return step
    out = both((n, d, k, x, nei, prop, center, disp), [from_fixed_point, capped(1), capped(7), capped(8), capped(100)], **cfg)
    assert out[0]["iters"] <= 3
    assert out[2]["iters"] == min(7, out[4]["iters"]) and out[3]["iters"] == min(8, out[4]["iters"])


def test_empty_class_runs():
    """K above the data's structure: runs that stop with an empty class (status, parameters and labels of that
    iteration) agree too"""
    statuses = []
    for k in (8, 9, 10):
        p = problem(6000, 48, k, grouped=True)
        cfg = dict(algo="ncem", beta=0.5, disper="skd", it_max=100, tie="hash", seed=1)
        out = both(p, [run] + restarts(7, 20), **cfg)
        statuses += [o["status"] for o in out]
    print("statuses", statuses)


def test_matches_oracle(gpu_lib, oracle):
    """the default (shadow-verify) schedule against the oracle, as the existing parity tests check the other"""
    n, d, k, x, nei, prop, center, disp = problem(20000, 60, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=12, tie="hash", seed=5)
    eng = make_engine(True, n, d, k, x, nei, prop, center, disp, **cfg)
    try:
        got = eng.run()
    finally:
        eng.close()
    want = oracle.run(x, nei, k, prop, center, disp, **cfg)
    assert want["iters"] == got["iters"] and np.array_equal(want["c"], got["c"])
    assert np.array_equal(want["center"], got["center"]) and maxdiff(want["disp"], got["disp"]) <= 1e-6
