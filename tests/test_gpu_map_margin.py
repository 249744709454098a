"""An NCEM round takes a site's label from the unnormalised row where the row's maximum is clear
(pangenomenem_amd/csrc/nem_map.hpp) and normalises only the other rows.  Held two ways: bit for bit against the same
library with NEM_MI355X_MAP_MARGIN=0 (every row normalised) -- labels, parameters, class sizes, the stored densities,
the criteria, the counters sweep_rounds and host_finished_sweeps, the tie draws -- and against the CPU oracle: labels,
centres, class sizes, logpkfki and the status words exact; epsilon and pi within 1e-6.  And on crafted rows the engine
cannot be made to meet (near ties at the margin, subnormal rows, sums next to EPSILON) the device's own arithmetic is
held to the host's through nemgpu_map_margin_device.

Shapes: one to three blocks, a last wave partly or wholly past the labels, a last block of one site; D = 1 (every
density far above EPSILON), 33 and 65 (sums on both sides of it), 500 (sums far below: the five-division branch)."""
import numpy as np
import pytest

from pangenomenem_amd import synth
from tests import map_margin_rows as mm
from tests.test_gpu_ff_batch import stored_density
from tests.test_gpu_shadow_verify import assert_same, make_engine, restarts, run
from tests.test_gpu_sweep_tail import same_as_oracle, tying_start, zero_density_problem
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

TOL = 1e-6
CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", it_max=4, tie="hash", seed=3)
FULL = {"NEM_MI355X_MAP_MARGIN": "0"}


def pair(x, nei, k, start, steps=(run,), env=None, **cfg):
    """`steps` (callables eng -> dict) on one engine with the shortcut and on one without: every step's outputs agree
    bit for bit.  Returns the outputs of the engine with the shortcut."""
    n, d = x.shape
    outs = []
    for twin_env in ({}, FULL):
        eng = make_engine(True, n, d, k, x, nei, *start, env=dict(env or {}, **twin_env), **cfg)
        try:
            res = []
            for step in steps:
                r = dict(step(eng))
                r.update(eng.results())
                r["crit_now"] = eng.criteria()
                r["pkfki"], r["logpkfki"] = stored_density(eng)
                r["host_finished_sweeps"] = eng.graph_counters()["host_finished_sweeps"]
                res.append(r)
        finally:
            eng.close()
        outs.append(res)
    for j, (a, b) in enumerate(zip(*outs)):
        assert_same(a, b, "step %d" % j)
    return outs[0]


def held(oracle, x, nei, k, start, env=None, **cfg):
    """a whole run: with and without the shortcut the same, and the oracle's answer"""
    got = pair(x, nei, k, start, env=env, **cfg)[0]
    want = oracle.run(x, nei, k, *start, **cfg)
    same_as_oracle(got, want, ncem=cfg.get("algo", "ncem") == "ncem")
    if want["status"] == 0:                               # (a run that ends on an empty class ends inside its M-step)
        assert got["logpkfki"].tobytes() == np.asarray(want["logpkfki"], np.float32).tobytes()
    return got, want


@pytest.mark.parametrize("n", [1, 63, 65, 255, 257, 300, 513])
def test_block_edges_and_density_ranges(oracle, n):
    for j, d in enumerate((1, 33, 65, 500)):
        x, _ = synth.bernoulli_pa_matrix(n, d, 1000 * n + d)
        nei = synth.contiguity_graph(n, 7) if n > 1 else None
        held(oracle, x, nei, 3, synth.default_init(d), **CFG)
        k = 2 + (j + n) % 4                               # K = 2 .. 5 over the shapes, from equal proportions
        held(oracle, x, nei, k, synth.kclass_init(x, k), **dict(CFG, seed=4))


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_class_counts(oracle, k):
    n, d = 300, 33
    x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
    for disper in ("sk_", "skd"):
        held(oracle, x, synth.contiguity_graph(n, 4, d=d), k, synth.kclass_init(x, k), **dict(CFG, disper=disper, seed=4))


def equal_classes(d, k):
    """k classes with the same parameters: every row ties between all of them, in every sweep"""
    prop = np.full(k, np.float32(round(1.0 / k, 4)), np.float32)
    return prop, np.full((k, d), 0.5, np.float32), np.full((k, d), 0.3, np.float32)


@pytest.mark.parametrize("tie", ["hash", "first", "libc"])
def test_tie_rules(oracle, tie):
    n, d = 300, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 8)
    nei = synth.contiguity_graph(n, 8)
    cfg = dict(CFG, tie=tie)
    for start in (synth.default_init(d), tying_start(d), equal_classes(d, 3)):
        got = pair(x, nei, 3, start, **cfg)[0]
        if tie == "libc":
            want, _ = oracle.trace_run(x, nei, 3, *start, **cfg)
            assert got["tie_draws"] == want["tie_draws"]
        else:
            want = oracle.run(x, nei, 3, *start, **cfg)
        same_as_oracle(got, want)
    if tie == "libc":
        assert got["tie_draws"] > 0                       # (the data do draw)


def test_zero_density_at_every_site(oracle):
    """every row is uniform (cum = 0): none is clear, the count and the first such site are the oracle's"""
    x, nei, start = zero_density_problem(300)
    got, want = held(oracle, x, nei, 2, start, **CFG)
    assert want["n_zero_density"] >= 300
    held(oracle, x, nei, 2, start, **dict(CFG, param_fix=True))


def test_weights_that_overflow_the_exponential(oracle):
    """weights of 1 500 at beta = 0.5: exp(beta * ctx) is inf wherever a class has a neighbour, rows hold inf and NaN
    (the regime of tests/golden/cov500_w1500_ncem)"""
    n, d = 300, 500
    x, _ = synth.ushaped_pa_matrix(n, d, 21)
    ptr, idx, w = synth.contiguity_graph(n, 21, d=d)
    nei = (ptr, idx, np.full_like(w, 1500.0))
    for beta in (0.5, 1.0):
        cfg = dict(CFG, beta=beta, it_max=3)
        got = pair(x, nei, 3, synth.default_init(d), **cfg)[0]
        want = oracle.run(x, nei, 3, *synth.default_init(d), **cfg)
        assert got["status"] == want["status"] and got["iters"] == want["iters"]
        assert got["n_zero_density"] == want["n_zero_density"]
        if want["status"] == 0:
            assert np.array_equal(got["c"], want["c"]) and np.array_equal(got["nbobs_k"], want["nbobs_k"])
            assert np.array_equal(np.nan_to_num(got["center"], nan=-7), np.nan_to_num(want["center"], nan=-7))
            for key in ("disp", "prop"):
                assert np.array_equal(np.isnan(got[key]), np.isnan(want[key]))
                assert maxdiff(np.nan_to_num(got[key]), np.nan_to_num(want[key])) <= TOL, key


def test_no_graph_and_beta_zero(oracle):
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    held(oracle, x, None, 3, synth.default_init(d), **CFG)
    held(oracle, x, synth.contiguity_graph(n, 13, d=d), 3, synth.default_init(d), **dict(CFG, beta=0.0))


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_start_plus_iterations_and_restarts(oracle, graphs):
    """a start alone (m = 0), a start plus iterations, five restarts on one engine; graph replay on and off"""
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    nei = synth.contiguity_graph(n, 13, d=d)
    start = synth.default_init(d)
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    ms = (0, 7, 1, 3, 2, 5)
    out = pair(x, nei, 3, start, steps=restarts(*ms), env=env, **CFG)
    for m, got in zip(ms[1:], out[1:]):
        want = oracle.run(x, nei, 3, *start, **dict(CFG, it_max=m))
        assert got["iters"] == want["iters"] == m
        assert np.array_equal(got["c"], want["c"]) and np.array_equal(got["center"], want["center"])
        assert np.array_equal(got["nbobs_k"], want["nbobs_k"])
        assert maxdiff(got["disp"], want["disp"]) <= TOL and maxdiff(got["prop"], want["prop"]) <= TOL
    got, _ = held(oracle, x, nei, 3, start, env=env, **dict(CFG, cvtest="clas", it_max=100))
    assert got["converged"]


def test_lock_step_batch_of_three_sizes(oracle):
    from pangenomenem_amd.engine import run_many
    outs = []
    for env in ({}, FULL):
        engines, wants = [], []
        try:
            for n in (1, 300, 700):
                d = 33
                x, _ = synth.bernoulli_pa_matrix(n, d, 30 + n)
                nei = synth.contiguity_graph(n, 5) if n > 1 else None
                start = synth.default_init(d)
                engines.append(make_engine(True, n, d, 3, x, nei, *start, env=env, **CFG))
                wants.append(oracle.run(x, nei, 3, *start, **CFG))
            res = run_many(engines)
            for got, want in zip(res, wants):
                same_as_oracle(got, want)
            outs.append(res)
        finally:
            for e in engines:
                e.close()
    for j, (a, b) in enumerate(zip(*outs)):
        assert_same(a, b, "member %d" % j)


def test_sharded_driver_on_one_rank(oracle, monkeypatch):
    """the sharded path's rounds run the same sweep_body; the switch reaches its worker through the environment.  With
    every row normalised the driver has the oracle's answer -- as it has with the shortcut, which is
    tests/test_gpu_sweep_tail.py::test_sharded_driver_on_one_rank (one worker process per test)"""
    from tests.test_gpu_distributed import _run
    n, d = 600, 15
    monkeypatch.setenv("NEM_MI355X_MAP_MARGIN", "0")
    (o,) = _run(1, "nccl", n, d, 0.5, bench_helpers=False)
    x, _ = synth.bernoulli_pa_matrix(n, d, 1)
    want = oracle.run(x, synth.contiguity_graph(n, 1), 3, *synth.default_init(d), algo="ncem", beta=0.5, tie="hash", seed=11)
    assert int(o["status"]) == want["status"] and int(o["iters"]) == want["iters"] and bool(o["converged"]) == want["converged"]
    assert np.array_equal(o["labels"], want["c"].argmax(1)) and np.array_equal(o["center"], want["center"])
    assert maxdiff(o["disp"], want["disp"]) <= TOL and maxdiff(o["prop"], want["prop"]) <= TOL


def test_fuzzy_run_is_untouched(oracle):
    n, d = 300, 33
    x, _ = synth.ushaped_pa_matrix(n, d, 9)
    held(oracle, x, synth.contiguity_graph(n, 9, d=d), 3, synth.default_init(d), **dict(CFG, algo="nem", it_max=3))


# ---- crafted rows through the device's arithmetic -------------------------------------------------------------------

def device_holds(lib, rows):
    """rows as densities, no graph (cinum = pkf): the device's four answers per row are the host's, and a clear row
    has the full path's label with nequal = 0"""
    got = mm.device_rows(lib, rows)
    want = mm.host_rows(lib, rows)
    bad = (got != want).any(axis=1)
    assert not bad.any(), (rows[bad][:5], got[bad][:5], want[bad][:5])
    clear = got[:, 3] != 0
    assert not (clear & ((got[:, 2] != got[:, 0]) | (got[:, 1] != 0))).any()
    return got


@pytest.mark.parametrize("K", [2, 3, 4, 5, 7, 8])
def test_crafted_rows_on_the_device(gpu_lib, K):
    lib = mm.declare(gpu_lib)
    rng = np.random.Generator(np.random.PCG64(1200 + K))                 # (the CPU test's rows)
    got = device_holds(lib, mm.near_tie_rows(rng, K))
    assert (got[:, 3] != 0).sum() > 300 and (got[:, 3] == 0).sum() > 300 and (got[:, 1] > 0).any()
    device_holds(lib, mm.special_rows(K))
    rng = np.random.Generator(np.random.PCG64(1300 + K))
    device_holds(lib, mm.epsilon_rows(rng, K, 20000))
    rng = np.random.Generator(np.random.PCG64(1100 + K))
    device_holds(lib, mm.whole_range_rows(rng, K, 40000))
    device_holds(lib, mm.narrow_rows(rng, K, 40000))


@pytest.mark.parametrize("K", [2, 3, 5])
def test_rows_with_the_device_exponential(gpu_lib, K):
    """cinum = pkf * exp(beta * ctx) with the device's exp (contexts that are small integers, contexts that are not,
    contexts that overflow it): the two device paths agree wherever the row is clear, and the shortcut does fire"""
    lib = mm.declare(gpu_lib)
    rng = np.random.Generator(np.random.PCG64(1400 + K))
    n = 40000
    pkf = np.ldexp(1.0 + rng.random((n, K)), rng.integers(-1074, -20, size=(n, 1)) + rng.integers(-2, 3, size=(n, K)))
    ctx = rng.integers(0, 40, size=(n, K)).astype(np.float32)
    ctx[n // 2:] += rng.random((n - n // 2, K)).astype(np.float32)
    ctx[-2000:] *= 100.0
    for beta in (0.5, 1.0):
        got = mm.device_rows(lib, pkf, ctx, beta)
        clear = got[:, 3] != 0
        assert clear.sum() > n // 2 and (~clear).sum() > 100
        assert not (clear & ((got[:, 2] != got[:, 0]) | (got[:, 1] != 0))).any()
