"""Differential fuzzing of the whole loop: seeded random problems (sizes, class counts, algorithms, dispersion and
proportion models, beta, graph density and weights, hand-made initial parameters with 0 / 0.5 / > 0.5 dispersions and
half centres, fixed parameters, tie rules) solved by the HIP engine and by the oracle; everything the reference
defines must agree (labels bit-exact, posteriors / epsilon / pi within 1e-6, centres, iteration count, status)."""
import os

import numpy as np
import pytest

from tests.fuzz_problems import random_problem
from tests.util import maxdiff

pytestmark = pytest.mark.gpu
TOL = 1e-6


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("NEM_FUZZ_SEEDS", "120")))))
def test_random_problem(gpu_lib, oracle, seed):
    from pangenomenem_amd.engine import solve
    x, nei, k, prop, center, disp, cfg = random_problem(seed)
    want = oracle.run(x, nei, k, prop, center, disp, **cfg)
    got = solve(x, nei, k, prop, center, disp, **cfg)
    ctx = (seed, x.shape, k, cfg)
    assert got["status"] == want["status"], ctx
    assert got["iters"] == want["iters"] and got["converged"] == want["converged"], ctx
    if want["status"] == 2:
        assert got["emptyk"] == want["emptyk"], ctx
    finite = np.isfinite(want["c"]).all()
    if finite:
        assert np.array_equal(got["c"].argmax(1), want["c"].argmax(1)), ctx
        if cfg["algo"] == "ncem":
            assert np.array_equal(got["c"], want["c"]), ctx
        assert maxdiff(got["c"], want["c"]) <= TOL, ctx
    else:                                                     # NaN posteriors (exp overflow): same places
        assert np.array_equal(np.isnan(got["c"]), np.isnan(want["c"])), ctx
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= TOL, (key, ctx)
    assert np.array_equal(np.nan_to_num(got["center"], nan=-7), np.nan_to_num(want["center"], nan=-7)), ctx
    assert got["n_zero_density"] == want["n_zero_density"], ctx


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("NEM_FUZZ_LARGE_SEEDS", "10")))))
def test_random_large_problem(gpu_lib, oracle, seed):
    """Sizes where the other code paths live: sums above 2^24 (sequential dispersion chains in k_finish), long
    chains (fast-forward over many binades), several density tiles per class, 1024-site sweep blocks."""
    from pangenomenem_amd import synth
    from pangenomenem_amd.engine import solve
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    n = int(rng.integers(18000, 80000))
    d = int(rng.choice([260, 500, 777, 1024, 1025, 1500, 2300]))
    k = int(rng.choice([2, 3, 3, 4]))
    x, _ = synth.grouped_pa_matrix(n, d, 1000 + seed, groups=max(k, 3), p_in=float(rng.uniform(0.7, 0.97)),
                                   p_out=float(rng.uniform(0.02, 0.3)))
    nei = synth.contiguity_graph(n, seed, chord_frac=float(rng.uniform(0.0, 0.3)))
    prop, center, disp = synth.kclass_init(x, k, eps=float(rng.uniform(0.05, 0.4)))
    cfg = dict(algo=str(rng.choice(["ncem", "ncem", "nem"])), beta=float(rng.choice([0.0, 0.5, 1.0])),
               disper=str(rng.choice(["sk_", "sk_", "skd", "s__", "s_d"])), propor="pk", it_max=3, tie="hash", seed=seed)
    want = oracle.run(x, nei, k, prop, center, disp, **cfg)
    got = solve(x, nei, k, prop, center, disp, **cfg)
    ctx = (seed, x.shape, k, cfg)
    assert got["status"] == want["status"] and got["iters"] == want["iters"], ctx
    assert np.array_equal(got["c"].argmax(1), want["c"].argmax(1)), ctx
    if cfg["algo"] == "ncem":
        assert np.array_equal(got["c"], want["c"]), ctx
    assert maxdiff(got["c"], want["c"]) <= TOL, ctx
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= TOL, (key, ctx)
    assert np.array_equal(got["center"], want["center"]), ctx


@pytest.mark.parametrize("n,d,tie", [(12000, 2800, "hash"), (66000, 2800, "hash"), (12000, 2800, "libc")])
def test_every_density_underflows(gpu_lib, oracle, n, d, tie):
    """Wide matrices drive every density to zero (exp(-dk) underflows): every site takes the uniform-posterior
    branch of nem_alg.c:2603-2613 and is counted.  Grids of 47 (256-site) and 65 (1024-site) blocks: the tally
    goes through the last-block counters from the second sweep on, and must still equal the reference's."""
    from pangenomenem_amd import synth
    from pangenomenem_amd.engine import solve
    x, _ = synth.bernoulli_pa_matrix(n, d, 5)
    nei = synth.contiguity_graph(n, 5)
    prop, center, disp = synth.default_init(d)
    # (tie = libc: every site of every sweep draws from the reference's stream -- the draw table slides batch by batch)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", it_max=3, tie=tie, seed=3)
    want = oracle.run(x, nei, 3, prop, center, disp, **cfg)
    got = solve(x, nei, 3, prop, center, disp, **cfg)
    assert want["n_zero_density"] > n // 2               # the regime this test is about
    assert got["n_zero_density"] == want["n_zero_density"]
    assert got["status"] == want["status"] and got["iters"] == want["iters"]
    assert np.array_equal(got["c"], want["c"])
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= TOL, key
