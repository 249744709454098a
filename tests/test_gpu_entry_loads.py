"""The loop kernels ask for their first loads at block entry, ahead of the stop word's and the previous round's tests
(density_fused_body in nem_kernels.hip, sweep_body in nem_sweep_dev.hpp).  A load issued too early reads outside a
buffer or uses a stale value at the shapes below, not at the workload's own: a part-empty last tile, organism counts
around the word / wave / group boundaries and at the fused kernel's cap, a class that empties, launches that enter with
the stop word set, engines whose graph pointers are not there, blocks beyond a batch member's grid.  Everything is held
to the CPU oracle: labels, centres, class sizes and the status words exact; posteriors, epsilon and pi within 1e-6."""
import os

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

TOL = 1e-6
# (no convergence test: small clean problems converge at once, and the fused density first reads the counts in iteration 2)
CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", it_max=4, tie="hash", seed=3)


def same_run(got, want):
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert got["iters"] == want["iters"], (got["iters"], want["iters"])
    assert got["converged"] == want["converged"]
    if want["status"] == 2:
        assert got["emptyk"] == want["emptyk"]
    assert np.array_equal(got["c"], want["c"])                       # NCEM: one-hot rows, the labels
    assert np.array_equal(got["center"], want["center"])
    assert np.array_equal(got["nbobs_k"], want["nbobs_k"])           # class sizes: integer counts
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= TOL, key


def make_engine(x, nei, k, start, env=None, **cfg):
    from pangenomenem_amd.engine import NemEngine
    env = dict(env or {})
    saved = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                            # (read when the engine is created)
    try:
        eng = NemEngine(x.shape[0], x.shape[1], k)
    finally:
        for key, v in saved.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    eng.set_matrix(x); eng.set_graph(nei); eng.set_params(*start); eng.configure(**cfg)
    return eng


def run_both(oracle, x, nei, k, start, env=None, **cfg):
    eng = make_engine(x, nei, k, start, env=env, **cfg)
    try:
        got = eng.run()
    finally:
        eng.close()
    want = oracle.run(x, nei, k, *start, **cfg)
    same_run(got, want)
    return got


@pytest.mark.parametrize("d", [1, 31, 33, 64, 65, 1024])
@pytest.mark.parametrize("n", [1, 255, 257, 300])
def test_part_empty_last_tile_and_ragged_organism_counts(oracle, n, d):
    """one tile and two, the last one part empty; D around a word, a wave and a four-word group, and at the fused cap"""
    x, _ = synth.bernoulli_pa_matrix(n, d, 1000 * n + d)
    nei = synth.contiguity_graph(n, 7) if n > 1 else None
    start = synth.default_init(d, low_disp=0.3 if d > 500 else 0.1)
    for disper in ("sk_", "skd"):
        run_both(oracle, x, nei, 3, start, **dict(CFG, disper=disper))


@pytest.mark.parametrize("disper", ["sk_", "skd"])
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_class_counts(oracle, k, disper):
    n, d = 300, 33
    x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
    run_both(oracle, x, synth.contiguity_graph(n, 4, d=d), k, synth.kclass_init(x, k), **dict(CFG, disper=disper, seed=4))


def fixed_point_problem(oracle):
    """bernoulli_pa_matrix, N = 600, D = 70, started from its own converged parameters: the run stops at its first
    iteration, and the batch's remaining kernels all enter with the stop word set"""
    n, d = 600, 70
    x, _ = synth.bernoulli_pa_matrix(n, d, 11)
    nei = synth.contiguity_graph(n, 11)
    cfg = dict(CFG, cvtest="clas", it_max=100)
    r = oracle.run(x, nei, 3, *synth.default_init(d), **cfg)
    assert r["converged"]
    return x, nei, (r["prop"], r["center"], r["disp"]), cfg


def emptying_problem():
    """every family everywhere: classes empty at the first M-step (status != 0), so the density that follows takes the
    center_in / disp_in path with N_k = 0"""
    n, d = 600, 70
    x = np.ones((n, d), np.uint8)
    return x, synth.contiguity_graph(n, 12), synth.default_init(d), dict(CFG, cvtest="clas", it_max=100)


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_run_that_converges_in_its_first_iteration(oracle, graphs):
    x, nei, start, cfg = fixed_point_problem(oracle)
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    got = run_both(oracle, x, nei, 3, start, env=env, **cfg)
    print("iterations", got["iters"])
    assert got["iters"] == 1 and got["converged"]


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
@pytest.mark.parametrize("disper", ["sk_", "skd"])
def test_class_that_empties(oracle, disper, graphs):
    x, nei, start, cfg = emptying_problem()
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    got = run_both(oracle, x, nei, 3, start, env=env, **dict(cfg, disper=disper))
    assert got["status"] != 0


@pytest.mark.parametrize("what", ["no_graph", "beta0"])
def test_engines_without_a_neighbourhood(oracle, what):
    """no graph at all, and a graph with beta = 0: the row bounds must not be asked for"""
    n, d = 300, 33
    x, _ = synth.bernoulli_pa_matrix(n, d, 21)
    nei = None if what == "no_graph" else synth.contiguity_graph(n, 21)
    run_both(oracle, x, nei, 3, synth.default_init(d), **dict(CFG, beta=0.5 if what == "no_graph" else 0.0))


def test_isolated_sites_and_rows_longer_than_four_neighbours(oracle):
    n, d = 700, 50
    x, _ = synth.ushaped_pa_matrix(n, d, 10)
    ptr, idx, w = (np.asarray(v) for v in synth.ring_graph(n, 3, 10, 1, 3))
    iso = np.zeros(n, bool); iso[::37] = True                        # drop these sites' rows and every mention of them
    row = np.repeat(np.arange(n), np.diff(ptr))
    keep = ~iso[row] & ~iso[idx]
    ptr2 = np.zeros(n + 1, np.int32); np.add.at(ptr2, row[keep] + 1, 1); ptr2 = np.cumsum(ptr2).astype(np.int32)
    nei = (ptr2, idx[keep].astype(np.int32), w[keep].astype(np.float32))
    assert int(np.diff(ptr2).max()) > 4 and int(np.diff(ptr2).min()) == 0 and ptr2[n] == ptr2[n - 1] + np.diff(ptr2)[-1]
    run_both(oracle, x, nei, 3, synth.default_init(d), **dict(CFG, beta=0.3))


@pytest.mark.parametrize("tie", ["libc", "first"])
def test_tie_rules(oracle, tie):
    """two classes with the same parameters: every site ties between them in the blind sweep (with "first" the second
    of them empties at once, so that rule also runs a problem without such ties)"""
    n, d = 300, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 8)
    nei = synth.contiguity_graph(n, 8)
    prop, center, disp = synth.default_init(d)
    if tie == "first":
        run_both(oracle, x, nei, 3, (prop, center, disp), **dict(CFG, tie=tie))
    prop = np.array([0.3, 0.3, 0.4], np.float32)
    center = center.copy(); disp = disp.copy()
    center[1] = center[0]; disp[1] = disp[0]
    run_both(oracle, x, nei, 3, (prop, center, disp), **dict(CFG, tie=tie))


def test_lock_step_batch_of_three_sizes(oracle):
    """nemgpu_run_many: the grid is the largest member's, so the smaller members see blocks beyond their own"""
    from pangenomenem_amd.engine import run_many
    engines, wants = [], []
    try:
        for n in (1, 300, 700):
            d = 33
            x, _ = synth.bernoulli_pa_matrix(n, d, 30 + n)
            nei = synth.contiguity_graph(n, 5) if n > 1 else None
            start = synth.default_init(d)
            engines.append(make_engine(x, nei, 3, start, **CFG))
            wants.append(oracle.run(x, nei, 3, *start, **CFG))
        for got, want in zip(run_many(engines), wants):
            same_run(got, want)
    finally:
        for e in engines:
            e.close()


def test_one_engine_through_five_restarts(oracle):
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    nei = synth.contiguity_graph(n, 13, d=d)
    start = synth.default_init(d)
    cfg = dict(CFG)
    eng = make_engine(x, nei, 3, start, **cfg)
    try:
        for m in (7, 1, 3, 2, 5):
            eng.configure(**dict(cfg, it_max=m))
            got = eng.restart_iterate(m)
            got.update(eng.results())
            want = oracle.run(x, nei, 3, *start, **dict(cfg, it_max=m))
            assert got["iters"] == want["iters"] == m
            assert np.array_equal(got["c"], want["c"]) and np.array_equal(got["center"], want["center"])
            assert np.array_equal(got["nbobs_k"], want["nbobs_k"])
            assert maxdiff(got["disp"], want["disp"]) <= TOL and maxdiff(got["prop"], want["prop"]) <= TOL
    finally:
        eng.close()
