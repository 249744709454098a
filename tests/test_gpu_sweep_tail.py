"""The tail of a relaxation round (sweep_body in nem_sweep_dev.hpp, behind the block-local steps): the tally of
zero-density sites, the "changed" and "moved" flags -- published without a look at the flag first on grids of at most
128 blocks --, the class masks, the counting round's adds and the last-block ticket that reads the flags.  Held two
ways: bit for bit against the twins that do not run this tail in the same role (NEM_MI355X_ROUND_COUNTS=0: the mask
round does not count; NEM_MI355X_SHADOW_VERIFY=0: no round posts the iteration's bookkeeping from a held sweep), and
against the CPU oracle: labels, centres, class sizes and the status words exact; posteriors, epsilon and pi within 1e-6.
The shapes are the smallest at which the tail can go wrong: one to three blocks, a last wave partly or wholly past the
labels, a last block of one site, 33 blocks (the two-level ticket, and the tally riding on it), organism counts at every
row group of the counting round and at the last mask word."""
import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.test_gpu_shadow_verify import assert_same, make_engine, restarts, run
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

TOL = 1e-6
CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", it_max=4, tie="hash", seed=3)
# (shadow-verify schedule, environment): the default and the two twins
TWINS = [(True, {}), (True, {"NEM_MI355X_ROUND_COUNTS": "0"}), (False, {})]


def same_as_oracle(got, want, ncem=True):
    assert got["status"] == want["status"], (got["status"], want["status"])
    assert got["iters"] == want["iters"], (got["iters"], want["iters"])
    assert got["converged"] == want["converged"]
    if want["status"] == 2:
        assert got["emptyk"] == want["emptyk"]
    assert got["n_zero_density"] == want["n_zero_density"]
    if ncem:
        assert np.array_equal(got["c"], want["c"])                   # one-hot rows: the labels
        assert np.array_equal(got["nbobs_k"], want["nbobs_k"])       # class sizes: integer counts
    else:
        assert np.array_equal(got["c"].argmax(1), want["c"].argmax(1)) and maxdiff(got["c"], want["c"]) <= TOL
    assert np.array_equal(got["center"], want["center"])
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= TOL, key


def twins(x, nei, k, start, steps=(run,), env=None, **cfg):
    """`steps` (callables eng -> dict) on one engine per twin; every step's outputs agree bit for bit.  Returns the
    default schedule's outputs and its engine's graph counters."""
    n, d = x.shape
    outs, counters = [], None
    for shadow, twin_env in TWINS:
        eng = make_engine(shadow, n, d, k, x, nei, *start, env=dict(env or {}, **twin_env), **cfg)
        try:
            res = []
            for step in steps:
                r = step(eng)
                r.update(eng.results())
                res.append(r)
            if counters is None:
                counters = eng.graph_counters()
        finally:
            eng.close()
        outs.append(res)
    for other in outs[1:]:
        for j, (a, b) in enumerate(zip(outs[0], other)):
            assert_same(a, b, "step %d" % j)
    return outs[0], counters


def held(oracle, x, nei, k, start, env=None, **cfg):
    """a whole run: the three twins agree, and the default one has the oracle's answer"""
    out, counters = twins(x, nei, k, start, env=env, **cfg)
    want = oracle.run(x, nei, k, *start, **cfg)
    same_as_oracle(out[0], want, ncem=cfg.get("algo", "ncem") == "ncem")
    out[0]["counters"] = counters
    return out[0], want


D_ALL = [1, 31, 33, 64, 65, 257, 500, 1023, 1024]


@pytest.mark.parametrize("n", [1, 63, 65, 255, 256, 257, 300, 513])
def test_block_edges_and_row_groups(oracle, n):
    """N: one to three blocks, a last wave partly or wholly past the labels (its ballots store empty masks), a last block
    of one site.  D: the counting round's rows d = tid + 256 q at every q, and the last 64-bit mask word"""
    for d in D_ALL:
        x, _ = synth.bernoulli_pa_matrix(n, d, 1000 * n + d)
        nei = synth.contiguity_graph(n, 7) if n > 1 else None
        held(oracle, x, nei, 3, synth.default_init(d, low_disp=0.3 if d > 500 else 0.1), **CFG)


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_thirty_three_blocks(oracle, graphs):
    """N = 8 448: the last-block ticket's two levels"""
    n, d = 8448, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 5)
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    got, _ = held(oracle, x, synth.contiguity_graph(n, 5, d=d), 3, synth.default_init(d), env=env, **dict(CFG, it_max=9))
    assert got["iters"] == 9


@pytest.mark.parametrize("n", [32768, 32769])
def test_grids_at_the_look_threshold(oracle, n):
    """128 blocks: the last grid whose flags go out without a look; 129: the first that looks"""
    d = 33
    x, _ = synth.ushaped_pa_matrix(n, d, 7)
    held(oracle, x, synth.contiguity_graph(n, 7, d=d), 3, synth.default_init(d), **dict(CFG, cvtest="clas", it_max=100))


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_class_counts(oracle, k):
    n, d = 300, 33
    x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
    for disper in ("sk_", "skd"):
        held(oracle, x, synth.contiguity_graph(n, 4, d=d), k, synth.kclass_init(x, k), **dict(CFG, disper=disper, seed=4))


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_start_from_converged_parameters(oracle, graphs):
    """no label changes and none moves: both flags stay 0, and the run stops at its first iteration"""
    n, d = 600, 70
    x, _ = synth.bernoulli_pa_matrix(n, d, 11)
    nei = synth.contiguity_graph(n, 11)
    cfg = dict(CFG, cvtest="clas", it_max=100)
    r = oracle.run(x, nei, 3, *synth.default_init(d), **cfg)
    assert r["converged"]
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    got, _ = held(oracle, x, nei, 3, (r["prop"], r["center"], r["disp"]), env=env, **cfg)
    assert got["iters"] == 1 and got["converged"]


def test_every_block_changes_and_moves_labels(oracle):
    """the blind partition against a strong graph: the start's sweep changes labels in each of the three blocks, and the
    iterations behind it go on moving them"""
    n, d = 700, 40
    x, _ = synth.ushaped_pa_matrix(n, d, 6)
    nei = synth.contiguity_graph(n, 6, weights="coverage", d=d)
    start = synth.default_init(d)
    cfg = dict(CFG, beta=1.0, it_max=1)
    blind = oracle.run(x, None, 3, *start, **dict(cfg, beta=0.0))["c"].argmax(1)
    got, want = held(oracle, x, nei, 3, start, **cfg)
    differs = got["c"].argmax(1) != blind
    print("labels that differ from the graph-free run's, per block:", [int(differs[b:b + 256].sum()) for b in range(0, n, 256)])
    assert all(differs[b:b + 256].any() for b in range(0, n, 256))
    held(oracle, x, nei, 3, start, **dict(cfg, it_max=5))


def test_run_that_stops_mid_batch(oracle):
    """convergence inside a batch of seven, and it_max reached inside one"""
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    nei = synth.contiguity_graph(n, 13, d=d)
    start = synth.default_init(d)
    got, _ = held(oracle, x, nei, 3, start, **dict(CFG, cvtest="clas", it_max=100))
    print("iterations", got["iters"])
    assert got["converged"] and got["iters"] % 7 != 0
    held(oracle, x, nei, 3, start, **dict(CFG, it_max=3))


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_class_that_empties(oracle, graphs):
    n, d = 600, 70
    x = np.ones((n, d), np.uint8)
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    got, _ = held(oracle, x, synth.contiguity_graph(n, 12), 3, synth.default_init(d), env=env, **dict(CFG, cvtest="clas", it_max=100))
    assert got["status"] != 0


def zero_density_problem(n):
    """two classes with centres all-0 and all-1, every row half ones, D = 1024: both densities underflow at every site"""
    d = 1024
    rng = np.random.default_rng(n)
    x = np.zeros((n, d), np.uint8)
    for i in range(n):
        x[i, rng.permutation(d)[:d // 2]] = 1
    prop = np.array([0.5, 0.5], np.float32)
    center = np.stack([np.zeros(d, np.float32), np.ones(d, np.float32)])
    disp = np.full((2, d), 0.1, np.float32)
    return x, synth.contiguity_graph(n, 3), (prop, center, disp)


@pytest.mark.parametrize("n", [300, 8448])
def test_zero_density_sites(oracle, n):
    """the count and the first such site (the twins' outputs hold both); at 33 blocks with the parameters fixed every
    sweep is all zero densities, so from the second on the tally rides on the ticket"""
    x, nei, start = zero_density_problem(n)
    got, want = held(oracle, x, nei, 2, start, **CFG)
    print("zero-density sites", got["n_zero_density"], "first", got["first_zero_density_site"])
    assert want["n_zero_density"] >= n
    got, want = held(oracle, x, nei, 2, start, **dict(CFG, param_fix=True))
    print("parameters fixed: zero-density sites", got["n_zero_density"], "first", got["first_zero_density_site"])
    assert want["n_zero_density"] >= 3 * n


def domino_chains(n, seg, w):
    """chains of `seg` sites: every site but a chain's head has one neighbour, the site before it, at a weight that
    outvotes the data -- a sweep hands the head's label down the chain, and a round takes it kInnerCap = 64 sites far"""
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(np.arange(n) % seg != 0)
    idx = (np.arange(n, dtype=np.int32) - 1)[np.arange(n) % seg != 0]
    return ptr, idx, np.full(idx.size, w, np.float32)


@pytest.mark.parametrize("seg,seed", [(500, 3), (250, 5)])
def test_sweeps_the_host_finishes(oracle, seg, seed):
    """a sweep that needs more rounds than were enqueued (the heavy-weight workloads of test_gpu_round_counts do not at
    N = 2 000, domino chains do): the batch stops and the host finishes the sweep.  Chains of 500: the start's sweep,
    a whole run behind it; chains of 250: heads that change class in an iteration, until a class empties"""
    n, d = 2000, 200
    x, _ = synth.ushaped_pa_matrix(n, d, seed)
    got, want = held(oracle, x, domino_chains(n, seg, 1200.0), 3, synth.default_init(d), **dict(CFG, it_max=6))
    print("host-finished sweeps", got["counters"]["host_finished_sweeps"], "status", got["status"], "iterations", got["iters"])
    lab = want["c"].argmax(1)
    assert all((lab[s:s + seg] == lab[s]).all() for s in range(0, n, seg))
    assert got["counters"]["host_finished_sweeps"] > 0


def test_five_restarts_on_one_engine(oracle):
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    nei = synth.contiguity_graph(n, 13, d=d)
    start = synth.default_init(d)
    ms = (7, 1, 3, 2, 5)
    out, _ = twins(x, nei, 3, start, steps=restarts(*ms), **CFG)
    for m, got in zip(ms, out):
        want = oracle.run(x, nei, 3, *start, **dict(CFG, it_max=m))
        assert got["iters"] == want["iters"] == m
        assert np.array_equal(got["c"], want["c"]) and np.array_equal(got["center"], want["center"])
        assert np.array_equal(got["nbobs_k"], want["nbobs_k"])
        assert maxdiff(got["disp"], want["disp"]) <= TOL and maxdiff(got["prop"], want["prop"]) <= TOL


def tying_start(d):
    """two classes with the same parameters: every site ties between them in the blind sweep"""
    prop, center, disp = synth.default_init(d)
    center = center.copy(); disp = disp.copy()
    center[1] = center[0]; disp[1] = disp[0]
    return np.array([0.3, 0.3, 0.4], np.float32), center, disp


def test_libc_ties(oracle):
    """TIE_LIBC with ties: the blocks' draw counts are part of "changed", and the draws (FLAG_NTIES) are the oracle's"""
    n, d = 300, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 8)
    nei = synth.contiguity_graph(n, 8)
    cfg = dict(CFG, tie="libc")
    out, _ = twins(x, nei, 3, tying_start(d), **cfg)
    want, _ = oracle.trace_run(x, nei, 3, *tying_start(d), **cfg)
    same_as_oracle(out[0], want)
    print("draws", out[0]["tie_draws"])
    assert out[0]["tie_draws"] == want["tie_draws"] > 0


def test_tie_first(oracle):
    n, d = 300, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 8)
    nei = synth.contiguity_graph(n, 8)
    held(oracle, x, nei, 3, synth.default_init(d), **dict(CFG, tie="first"))
    held(oracle, x, nei, 3, tying_start(d), **dict(CFG, tie="first"))


def test_fuzzy_nem(oracle):
    """the fuzzy instance shares the tail: "changed" is a bit pattern that differs, nothing is posted or counted"""
    n, d = 300, 33
    x, _ = synth.ushaped_pa_matrix(n, d, 9)
    held(oracle, x, synth.contiguity_graph(n, 9, d=d), 3, synth.default_init(d), **dict(CFG, algo="nem", it_max=3))


def test_lock_step_batch_of_three_sizes(oracle):
    """nemgpu_run_many: the grid is the largest member's, the smaller members' tickets count their own blocks"""
    from pangenomenem_amd.engine import run_many
    engines, wants = [], []
    try:
        for n in (1, 300, 700):
            d = 33
            x, _ = synth.bernoulli_pa_matrix(n, d, 30 + n)
            nei = synth.contiguity_graph(n, 5) if n > 1 else None
            start = synth.default_init(d)
            engines.append(make_engine(True, n, d, 3, x, nei, *start, **CFG))
            wants.append(oracle.run(x, nei, 3, *start, **CFG))
        for got, want in zip(run_many(engines), wants):
            same_as_oracle(got, want)
    finally:
        for e in engines:
            e.close()


def test_sharded_driver_on_one_rank(oracle):
    """the sweep + counts launch of the sharded path: its ticket publishes the rank's "changed" and "moved" bytes"""
    from tests.test_gpu_distributed import _run
    n, d = 600, 15
    (o,) = _run(1, "nccl", n, d, 0.5, bench_helpers=False)
    x, _ = synth.bernoulli_pa_matrix(n, d, 1)
    want = oracle.run(x, synth.contiguity_graph(n, 1), 3, *synth.default_init(d), algo="ncem", beta=0.5, tie="hash", seed=11)
    assert int(o["status"]) == want["status"] and int(o["iters"]) == want["iters"] and bool(o["converged"]) == want["converged"]
    assert np.array_equal(o["labels"], want["c"].argmax(1))
    assert np.array_equal(o["center"], want["center"])
    assert maxdiff(o["disp"], want["disp"]) <= TOL and maxdiff(o["prop"], want["prop"]) <= TOL
