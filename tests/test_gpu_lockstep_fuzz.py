"""Differential fuzzing of the lock-step batches (nemgpu_run_many, nemgpu_solve_many, the random starts in lock step):
the `_b` twins of the loop kernels -- blockIdx.z = the member, a per-member grid width -- that launch_zipped
(nem_kernels.hip) and sweep_dispatch<true> (nem_sweep.hip) dispatch to.  Every member of every call is held to the
oracle by the rules of tests/test_gpu_fuzz.py::test_random_problem, and to its own solo run bit for bit
(include/nem_mi355x.h): a twin and its by-value kernel wrong alike would pass the second and fail the first.

The lock-step call comes first, on fresh engines, so that no solo run has left anything behind; then the solo runs on
the same engines; then the call again with the members in reverse order, so that another member leads.

What the member lists reach is asserted on the CPU by tests/test_lockstep_fuzz_host.py, with the library's own
arithmetic.  Two things no test can observe through the C interface, and these do not: how many sequence groups a step
formed, and whether a zip graph was replayed.  The grouping follows from the members by zip_and_launch's rule (the
recorded sequences of (kind, variant, block, gy, nbytes) are compared).  The replay follows from the number of calls:
a shape is captured at its fourth sighting by run_graphed, and the sightings are kept in the lead engine's own
context -- which is why test_random_groups calls six times in each order, not three."""
import time

import numpy as np
import pytest

from tests import lockstep_members as M
from tests.util import assert_crit_close, maxdiff

pytestmark = pytest.mark.gpu


def make_engines(members):
    from pangenomenem_amd.engine import NemEngine
    engines = []
    for x, nei, k, prop, center, disp, cfg in members:
        eng = NemEngine(x.shape[0], x.shape[1], k)
        eng.set_matrix(x); eng.set_graph(nei); eng.set_params(prop, center, disp); eng.configure(**cfg)
        engines.append(eng)
    return engines


def check_run_many(oracle, members, what, calls_per_order=1):
    """run_many on fresh engines == the oracle; == the solo runs, bit for bit; == run_many again, either order"""
    from pangenomenem_amd.engine import run_many
    t0 = time.perf_counter()
    want = [oracle.run(*m[:6], **m[6]) for m in members]
    t_oracle = time.perf_counter() - t0
    t0 = time.perf_counter()
    engines = make_engines(members)
    try:
        first = run_many(engines)
        for j, (m, got, w) in enumerate(zip(members, first, want)):
            M.assert_matches_oracle(got, w, m[6], (what, "member", j, m[0].shape, m[2], m[6]))
        solo = [eng.run() for eng in engines]
        for j, (m, got, s) in enumerate(zip(members, first, solo)):
            M.assert_same_run(got, s, (what, "solo", j, m[0].shape, m[2], m[6]))
        for rep in range(2 * calls_per_order - 1):
            again = run_many(engines[::-1])[::-1] if rep % 2 == 0 else run_many(engines)
            for j, (m, got, a) in enumerate(zip(members, first, again)):
                M.assert_same_run(a, got, (what, "call", rep + 2, "member", j, m[0].shape, m[2], m[6]))
                assert a["converged"] == got["converged"] and a["emptyk"] == got["emptyk"]
                assert a["n_zero_density"] == got["n_zero_density"]
    finally:
        for eng in engines:
            eng.close()
    print("%s: %d members, oracle %.2f s, engines %.2f s" % (what, len(members), t_oracle, time.perf_counter() - t0))
    return want, first


@pytest.mark.parametrize("g", list(range(M.FUZZ_GROUPS)))
def test_random_groups(gpu_lib, oracle, g):
    """(a) eight random problems, each with its own configuration, in ONE call: at least four class counts, mixed
    algorithms, models and tie rules, members of one family, without a graph, with it_max = 0, with fixed parameters,
    members that stop at their first M-step.  Twelve calls on the same engines, six in either order: the lead's context
    has seen its shapes four times by the fourth, the last ones replay what that one captured.  Every call's results
    are the first's."""
    check_run_many(oracle, M.fuzz_group(g), "random group %d" % g, calls_per_order=6)


@pytest.mark.parametrize("algo,tie", M.SWEEP_CASES)
def test_every_class_count_in_one_call(gpu_lib, oracle, algo, tie):
    """(b) K = 1..12, 17, 32 side by side, 2 to 6 sweep blocks each: all 33 of the 256-site k_sweep_b instances over
    the four cases, the fuzzy M-step, convergence and criteria twins at every K.  Every class count is a sequence
    group of its own (the sweep's variant is in the sequence); members leave at different iterations, converged, with
    an empty class, or at it_max."""
    want, _ = check_run_many(oracle, [M.build_member(s) for s in M.every_k_specs(algo, tie)], "every K %s %s" % (algo, tie))
    assert len({(w["status"], w["iters"]) for w in want}) >= 2


@pytest.mark.parametrize("algo,tie", M.BIG_CASES)
def test_big_sweep_twins(gpu_lib, oracle, algo, tie):
    """(c) the __launch_bounds__(1024) instances of k_sweep_b, K = 1..10: 65 536 families (the threshold itself: 256
    blocks of 256 sites) and 100 003 (224 blocks of 448, the last one of 99 sites), beside a member of 200 families -- one
    block of the 256-site instance in a group of its own."""
    check_run_many(oracle, [M.build_member(s) for s in M.big_specs(algo, tie)], "big %s %s" % (algo, tie))


@pytest.mark.parametrize("algo", M.DENSITY_CASES)
def test_every_density_and_update_path_in_one_call(gpu_lib, oracle, algo):
    """(d) 255 / 256 / 1024 / 1025 organisms x sk_ / skd / s__ / s_d, K = 3 and 4.  Recorded, every member updates its
    parameters in k_finish_b (one block per class for sk_ / skd, one block for s__ / s_d) and takes k_density_b, with
    the fast-forwarded chain from 256 organisms on, and k_mstep_counts_b<4> from 1023 on; alone, the NCEM members
    whose fused_update() holds run the fused density kernels instead -- and must give the same bits."""
    check_run_many(oracle, [M.build_member(s) for s in M.density_specs(algo)], "density paths %s" % algo)


@pytest.mark.parametrize("bits", [False, True], ids=["bytes", "bitrows"])
@pytest.mark.parametrize("call", list(range(5)))
def test_solve_many_over_the_random_problems(gpu_lib, oracle, call, bits):
    """(e) the problems of (a) under one configuration per call (lockstep_members.solve_many_calls), in groups of 1, 3
    and 32 with 1 and 4 workers, from byte matrices or bit rows.  One problem of every call holds a 2 (always as
    bytes: a bit row cannot): its rc is NEMGPU_E_ARG, so is the call's, and every other answer is the oracle's."""
    cfg, probs = M.solve_many_calls()[call]
    t0 = time.perf_counter()
    want = [oracle.run(*p, **cfg) for p in probs]
    t_oracle = time.perf_counter() - t0
    t0 = time.perf_counter()
    turn = 0
    for group in M.SOLVE_GROUPS:
        for workers in M.SOLVE_WORKERS:
            bad = (7 * turn + call) % len(probs)
            turn += 1
            given = [((M.as_bit_rows(p[0]) if bits else p[0]),) + tuple(p[1:]) for p in probs]
            wrong = probs[bad][0].copy()
            wrong[wrong.shape[0] // 2, wrong.shape[1] // 2] = 2
            given[bad] = (wrong,) + tuple(probs[bad][1:])
            rc, rcs, res = M.solve_many_raw(given, workers, group, **cfg)
            assert rc == 3 and rcs[bad] == 3, (rc, rcs, bad)                       # NEMGPU_E_ARG
            assert [r for j, r in enumerate(rcs) if j != bad] == [0] * (len(probs) - 1), (rcs, bad)
            for j, (p, got, w) in enumerate(zip(probs, res, want)):
                if j != bad:
                    M.assert_matches_oracle(got, w, cfg, ("solve_many", call, bits, group, workers, j, p[0].shape, p[2], cfg))
    print("solve_many call %d: %d problems, oracle %.2f s, six calls %.2f s" % (call, len(probs), t_oracle, time.perf_counter() - t0))


@pytest.mark.parametrize("k,d,algo", M.STARTS_CASES)
def test_lockstep_random_starts_at_other_class_counts(gpu_lib, oracle, monkeypatch, k, d, algo):
    """(f) RandNemAlgo's starts in lock step at K = 2, 6 and 11 (the generic instances), 20 and 300 organisms, NCEM
    everywhere and fuzzy NEM at 20 organisms (the oracle takes seconds for it at 300): the oracle's
    best start, labels and parameters by the rules of test_gpu_edges.test_random_starts_match_oracle, and the same call
    with the starts one after the other, bit for bit."""
    from pangenomenem_amd import synth
    from pangenomenem_amd.engine import NemEngine
    s = M.starts_spec(k, d)
    x, _ = synth.grouped_pa_matrix(s["n"], s["d"], s["seed"], groups=s["groups"])
    nei = synth.contiguity_graph(s["n"], s["seed"])
    cfg = dict(algo=algo, beta=0.5, disper="sk_", propor="pk", it_max=20, tie="hash", seed=s["seed"])
    want = oracle.run_random(x, nei, k, n_starts=M.STARTS, rng_seed=s["seed"], **cfg)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("NEM_MI355X_BATCH_STARTS", mode)
        eng = NemEngine(s["n"], d, k)
        eng.set_matrix(x); eng.set_graph(nei); eng.configure(**cfg)
        out[mode] = eng.run_random(n_starts=M.STARTS, rng_seed=s["seed"])
        assert (eng.random_start_counters()["in_lockstep"] > 0) == (mode == "1")
        eng.close()
    got = out["1"]
    assert got["status"] == want["status"] and got["best_start"] == want["best_start"]
    assert got["iters"] == want["iters"] and got["converged"] == want["converged"]
    assert np.array_equal(got["c"].argmax(1), want["c"].argmax(1))
    if algo == "ncem":
        assert np.array_equal(got["c"], want["c"])
    assert maxdiff(got["c"], want["c"]) <= M.TOL
    for key in ("disp", "prop"):
        assert maxdiff(got[key], want[key]) <= M.TOL, key
    assert np.array_equal(got["center"], want["center"])
    assert_crit_close(got["crit"], want["crit"], 1e-6)
    alone = out["0"]
    assert alone["best_start"] == got["best_start"] and alone["status"] == got["status"]
    assert alone["iters"] == got["iters"] and alone["tie_draws"] == got["tie_draws"]
    for key in ("c", "center", "disp", "prop", "crit"):
        assert np.array_equal(alone[key], got[key], equal_nan=True), key
