"""M-step counts added up by the round that makes a held sweep's class masks (nem_engine.hip shadow_batch_enqueue,
NEM_MI355X_ROUND_COUNTS) against the counts launch per iteration (NEM_MI355X_ROUND_COUNTS=0), both under the
shadow-verify schedule: the same labels, parameters, criteria, iteration counts and status, bit for bit -- across batch
boundaries, runs that stop mid-batch, host-finished sweeps, deep and mispredicted sweeps, empty classes, graphs off,
K = 2..6 with every tie rule (TIE_LIBC keeps the old schedule), 1 000 organisms and many restarts of one engine -- and
the oracle's answer on the configs[1]-like workload.  (50 000 x 1 000 has too many partial counts for the counting
round: both settings run the counts launch there, see round_counts_on.)"""
import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.test_gpu_shadow_verify import assert_same, make_engine, problem, restarts, run
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]


def engine(counts, p, env=None, **cfg):
    n, d, k, x, nei, prop, center, disp = p
    env = dict(env or {})
    env["NEM_MI355X_ROUND_COUNTS"] = "1" if counts else "0"
    return make_engine(True, n, d, k, x, nei, prop, center, disp, env=env, **cfg)


def both(p, steps, env=None, **cfg):
    """run `steps` (callables eng -> dict) on one engine per setting; every step's outputs agree"""
    outs = []
    for counts in (False, True):
        eng = engine(counts, p, env=env, **cfg)
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


def test_configs1_workload_and_restarts():
    """BASELINE configs[1]'s shape as bench.py runs it, then restarts of one batch, across a batch boundary, and it_max
    reached mid-batch, on the same engine"""
    p = problem(20000, 500, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, tie="hash", seed=1)
    out = both(p, [run] + restarts(7, 8, 3, 10, 7, 1, 2) + [run], **cfg)
    assert out[0]["iters"] >= 2


def test_many_restarts_one_engine():
    p = problem(20000, 500, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", cvtest="none", it_max=100, tie="hash", seed=1)
    both(p, restarts(*([7] * 12 + [5, 6, 9, 13, 14, 15, 7])), **cfg)


def test_wide_rows():
    """1 000 organisms: four organism rows per thread in the counting round"""
    p = problem(8000, 1000, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=1)
    both(p, [run] + restarts(7, 9), **cfg)


@pytest.mark.parametrize("weights", ["coverage", "adjacency"])
def test_host_finished_sweeps(weights):
    """heavy weights: sweeps that need more rounds than enqueued -- the counts a mask round added up are thrown away
    with the speculative density, and the next batch starts with a counts launch"""
    n, d = 20000, 200
    x, _ = synth.ushaped_pa_matrix(n, d, 4)
    nei = synth.contiguity_graph(n, 4, weights=weights, d=d, counts=x.sum(axis=1) if weights == "adjacency" else None)
    prop, center, disp = synth.default_init(d)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=2)
    both((n, d, 3, x, nei, prop, center, disp), [run] + restarts(7, 11, 4) + [run], **cfg)


def test_deep_and_mispredicted_rounds():
    """two rounds per sweep (the mask round is round 0) until a sweep needs more, then three (round 1)"""
    p = problem(20000, 300, 3, weights="coverage", seed=6)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=3)
    both(p, [run] + restarts(7, 9) + [run], env={"NEM_MI355X_ROUNDS": "2"}, **cfg)
    both(p, [run] + restarts(7, 9) + [run], env={"NEM_MI355X_ROUNDS": "4"}, **cfg)


def test_without_graphs():
    p = problem(20000, 300, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="hash", seed=1)
    both(p, [run] + restarts(7, 8, 3), env={"NEM_MI355X_GRAPHS": "0"}, **cfg)


@pytest.mark.parametrize("k,tie", [(2, "hash"), (3, "first"), (4, "hash"), (5, "first"), (6, "hash"),
                                   (3, "libc"), (4, "libc")])
def test_k_and_tie_rules(k, tie):
    p = problem(9000, 64, k, grouped=True)
    cfg = dict(algo="ncem", beta=0.5, disper="skd", it_max=100, tie=tie, seed=4)
    both(p, [run] + restarts(7, 8, 1), **cfg)


def test_converges_at_once_and_at_batch_ends():
    """restarted from the converged parameters the run stops at its first iterations; it_max at 1, 2, 7 and 8"""
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
    out = both((n, d, k, x, nei, prop, center, disp),
               [from_fixed_point, capped(1), capped(2), capped(7), capped(8), capped(100)], **cfg)
    assert out[0]["iters"] <= 3
    assert out[3]["iters"] == min(7, out[5]["iters"]) and out[4]["iters"] == min(8, out[5]["iters"])


def test_empty_class_runs():
    """K above the data's structure: runs that stop with an empty class agree too"""
    for k in (8, 9, 10):
        p = problem(6000, 48, k, grouped=True)
        cfg = dict(algo="ncem", beta=0.5, disper="skd", it_max=100, tie="hash", seed=1)
        both(p, [run] + restarts(7, 20), **cfg)


def test_matches_oracle(gpu_lib, oracle):
    """the default (counting round) schedule against the oracle"""
    n, d, k, x, nei, prop, center, disp = p = problem(20000, 60, 3)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=12, tie="hash", seed=5)
    eng = engine(True, p, **cfg)
    try:
        got = eng.run()
    finally:
        eng.close()
    want = oracle.run(x, nei, k, prop, center, disp, **cfg)
    assert want["iters"] == got["iters"] and np.array_equal(want["c"], got["c"])
    assert np.array_equal(want["center"], got["center"]) and maxdiff(want["disp"], got["disp"]) <= 1e-6
