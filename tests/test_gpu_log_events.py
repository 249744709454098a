"""The logged runs -- nemgpu_run_logged, nemgpu_run_random_logged, nemgpu_iterate_logged, what nem(..., dolog=True)
goes through -- event by event against the oracle's trace (oracle/nem_oracle.h, anchored on the CPU by
tests/test_oracle_trace.py): all six criteria before and after every E-step sweep, the parameters and the class sizes of
every line at the tolerances the whole-run tests hold (1e-6), on problems that force each branch of the host code: the
batches of three and seven iterations cut by it_max or by convergence in every slot, a sweep the host has to finish, an
emptied class, the unbatched forms, random starts in lock step and one after the other.  Where a branch is forced, a
counter of the engine says that it ran."""
import functools
import math

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.golden_util import load_case
from tests.log_text_util import random_log_text
from tests.util import assert_crit_close, assert_same_nem_log, bits_equal, maxdiff

pytestmark = pytest.mark.gpu
TOL = 1e-6                                                    # test_gpu_fuzz's and test_gpu_golden's
ARRAYS = ("crit_before", "crit_after", "prop", "center", "disp", "nbobs_k")


# ---- the comparison ------------------------------------------------------------------------------------------
def same_sizes(got, want, algo, what):
    assert got is not None and want is not None, what
    if algo == "ncem":
        assert np.array_equal(got, want), (what, got, want)
    else:
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
        assert maxdiff(got, want) <= 1e-6 * max(1.0, float(np.nanmax(want))), (what, got, want)


def same_events(got, want, algo, empty_sizes=True):
    """The engine's events against the oracle's.  empty_sizes=False: nemgpu_run_logged's EMPTY event carries no sizes
    (only a start of nemgpu_run_random_logged hands them over, for the next start's line 0)."""
    head = lambda evs: [(ev["kind"], ev["start"], ev["iter"], ev["emptyk"]) for ev in evs]
    assert head(got) == head(want)
    for g, w in zip(got, want):
        what = (w["kind"], w["start"], w["iter"])
        if w["kind"] == "start":
            continue
        if w["kind"] == "empty":
            if empty_sizes:
                same_sizes(g["nbobs_k"], w["nbobs_k"], algo, what)
            else:
                assert g["nbobs_k"] is None, what
            continue
        assert np.array_equal(np.isnan(g["center"]), np.isnan(w["center"])), what
        assert bits_equal(np.nan_to_num(g["center"], nan=-7.0), np.nan_to_num(w["center"], nan=-7.0)), what
        for key in ("prop", "disp"):
            assert np.array_equal(np.isnan(g[key]), np.isnan(w[key])), (what, key)
            assert maxdiff(g[key], w[key]) <= TOL, (what, key, maxdiff(g[key], w[key]))
        if w["iter"] == 0:
            assert g["nbobs_k"] is None and w["nbobs_k"] is None, what
        else:
            same_sizes(g["nbobs_k"], w["nbobs_k"], algo, what)
        assert_crit_close(g["crit_before"], w["crit_before"], 1e-6, (what, "before"))
        assert_crit_close(g["crit_after"], w["crit_after"], 1e-6, (what, "after"))


def same_result(res, got, want_res, algo):
    """nemgpu_run_logged's result: the oracle's counts; crit = the last line's second criteria, bit for bit, or
    crit[0] = NaN where the header leaves them to the caller (no iteration ran, or the run ended on an emptied class)."""
    for key in ("iters", "status", "converged"):
        assert res[key] == want_res[key], (key, res[key], want_res[key])
    if want_res["status"] == 2:
        assert res["emptyk"] == want_res["emptyk"] > 0
    if want_res["iters"] == 0 or want_res["status"] == 2:
        assert math.isnan(res["crit"][0]), res["crit"]
    else:
        assert got[-1]["kind"] == "line" and bits_equal(res["crit"], got[-1]["crit_after"]), (res["crit"], got[-1]["crit_after"])
        if algo == "ncem":
            assert np.array_equal(res["c"], want_res["c"])


def identical_events(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u["kind"], u["start"], u["iter"], u["emptyk"]) == (v["kind"], v["start"], v["iter"], v["emptyk"])
        for key in ARRAYS:
            assert (u[key] is None) == (v[key] is None), (u["iter"], key)
            if u[key] is not None:
                assert bits_equal(u[key], v[key]), (u["iter"], key, u[key], v[key])


# ---- the problems: the smallest that still reach each path --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def p1(seed=2, gen="ushaped"):
    """601 x 12, K = 3: n % 4 = 1 (the last word of a set-aside partition is partly filled), three 256-site blocks"""
    n, d = 601, 12
    if gen == "ushaped":
        x, _ = synth.ushaped_pa_matrix(n, d, seed)
    else:                                                     # two sharp classes out of three: at its fixed point at once
        x, _ = synth.bernoulli_pa_matrix(n, d, seed, p=(0.97, 0.97, 0.03))
    return (x, synth.contiguity_graph(n, seed, chord_frac=0.3), 3) + synth.default_init(d)


@functools.lru_cache(maxsize=None)
def p2():
    """3 x 1, K = 2, no graph"""
    x = np.array([[1], [0], [1]], np.uint8)
    return (x, None, 2, np.array([0.5, 0.5], np.float32), np.array([[1.0], [0.0]], np.float32),
            np.array([[0.1], [0.2]], np.float32))


@functools.lru_cache(maxsize=None)
def p3():
    """1 025 x 65, K = 8, K-class start, weights that are no integers: the parameters span more than one 64-organism
    word; class 1 empties at iteration 5 under NCEM (asserted where it matters)"""
    n, d, k = 1025, 65, 8
    x, _ = synth.ushaped_pa_matrix(n, d, 24)
    ptr, idx, w = synth.contiguity_graph(n, 24, chord_frac=0.3)
    return (x, (ptr, idx, (w * np.float32(0.37)).astype(np.float32)), k) + synth.kclass_init(x, k, eps=0.3)


def engine_for(problem, **cfg):
    from pangenomenem_amd.engine import NemEngine
    x, nei, k, prop, center, disp = problem
    eng = NemEngine(x.shape[0], x.shape[1], k)
    eng.set_matrix(x)
    eng.set_graph(nei)
    eng.set_params(prop, center, disp)
    eng.configure(**cfg)
    return eng


def logged_both(oracle, problem, **cfg):
    """run_logged of a fresh engine and the oracle's trace of the same run, compared; returns both"""
    want_res, want = oracle.trace_run(*problem, **cfg)
    eng = engine_for(problem, **cfg)
    res, got = eng.run_logged()
    eng.close()
    same_events(got, want, cfg["algo"], empty_sizes=False)
    same_result(res, got, want_res, cfg["algo"])
    return res, got, want_res, want


NCEM = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", cvthres=1e-8, tie="hash", seed=2)


# ---- the it_max ladder: batches of 3, 3+1, 3+6, 3+7, 3+7+1, 3+7+7 ------------------------------------------------
@pytest.mark.parametrize("it_max", [0, 1, 2, 3, 4, 9, 10, 11, 17])
def test_batches_cut_by_it_max(gpu_lib, oracle, it_max):
    res, got, want_res, want = logged_both(oracle, p1(), **dict(NCEM, it_max=it_max))
    assert want_res["iters"] == it_max and len(want) == it_max + 1


def p1_twins():
    """P1 started with class 3 a copy of class 1: every family the twins win ties, and the tie rule decides"""
    x, nei, k, prop, center, disp = p1()
    center, disp = center.copy(), disp.copy()
    center[2], disp[2] = center[0], disp[0]
    return x, nei, k, np.full(3, np.float32(1.0 / 3), np.float32), center, disp


@pytest.mark.parametrize("it_max", [4, 10, 11])
@pytest.mark.parametrize("twins", [False, True])
def test_batches_on_the_tie_stream(gpu_lib, oracle, it_max, twins):
    """TIE_LIBC: P1 itself never ties (0 draws on either side); with twin classes the start draws 321 times."""
    problem = p1_twins() if twins else p1()
    res, got, want_res, want = logged_both(oracle, problem, **dict(NCEM, it_max=it_max, tie="libc"))
    assert want[-1]["draws"] == want_res["tie_draws"] == (321 if twins else 0)   # (the trace exposes the oracle's draws)
    assert res["tie_draws"] == want_res["tie_draws"]
    print("tie draws at it_max %d: %d" % (it_max, res["tie_draws"]))


@pytest.mark.parametrize("it_max", [3, 10])
@pytest.mark.parametrize("variant", [dict(param_fix=True), dict(disper="skd", propor="p_")])
def test_batches_with_fixed_parameters_and_with_free_dispersions(gpu_lib, oracle, it_max, variant):
    logged_both(oracle, p1(), **dict(NCEM, it_max=it_max, **variant))


# ---- convergence in every slot: the last and first of the first two batches, the middle of the second, the third
CONVERGES_AT = {1: ("two_sharp", 6), 2: ("ushaped", 192), 3: ("ushaped", 12), 4: ("ushaped", 3), 5: ("ushaped", 6),
                10: ("ushaped", 44), 11: ("ushaped", 2)}


@pytest.mark.parametrize("iters", sorted(CONVERGES_AT))
def test_convergence_in_every_slot_of_a_batch(gpu_lib, oracle, iters):
    gen, seed = CONVERGES_AT[iters]
    cfg = dict(NCEM, cvtest="clas", it_max=40, seed=seed)
    problem = p1(seed, gen)
    want_res = oracle.run(*problem, **cfg)
    assert want_res["iters"] == iters and want_res["converged"] and want_res["status"] == 0
    res, got, _, _ = logged_both(oracle, problem, **cfg)
    assert res["converged"] and res["iters"] == iters
    print("the oracle converges at iteration %d (seed %d)" % (want_res["iters"], seed))


# ---- the host finishes a sweep (tail_open) -------------------------------------------------------------------------
def test_a_sweep_the_host_has_to_finish(gpu_lib, oracle, monkeypatch):
    """Two relaxation rounds per sweep and no more (NEM_MI355X_ROUNDS = NEM_MI355X_ROUNDS_ITER = 2, read when the engine
    is created).  On this problem the sweeps of iterations 4 and 8 are not through in two rounds even if every 256-site
    block swept its own sites in sequence within a round (worked out on the CPU with orc_relax_round): a change in one
    block moves a site of another, which moves a site of a third.  Such an iteration ends its batch, the host adds the
    rounds, and its line takes the plain sequence of calls.  The start alone accounts for c1 - c0 finished sweeps (it
    runs first on the same engine, with nothing adaptive left at two rounds); the logged run must add more than that."""
    cfg = dict(NCEM, it_max=11)
    want_res, want = oracle.trace_run(*p1(), **cfg)
    plain = engine_for(p1(), **cfg)
    res0, got0 = plain.run_logged()
    plain.close()
    monkeypatch.setenv("NEM_MI355X_ROUNDS", "2")
    monkeypatch.setenv("NEM_MI355X_ROUNDS_ITER", "2")
    eng = engine_for(p1(), **cfg)
    c0 = eng.graph_counters()["host_finished_sweeps"]
    eng.iterate_logged(1)
    c1 = eng.graph_counters()["host_finished_sweeps"]
    res, got = eng.run_logged()
    c2 = eng.graph_counters()["host_finished_sweeps"]
    eng.close()
    print("host-finished sweeps: the start %d, the logged run %d" % (c1 - c0, c2 - c1))
    assert c2 - c1 > c1 - c0
    same_events(got, want, "ncem", empty_sizes=False)
    same_result(res, got, want_res, "ncem")
    identical_events(got, got0)
    assert bits_equal(res["crit"], res0["crit"])


# ---- an emptied class: at iteration 1, and inside the second batch -------------------------------------------------
@pytest.mark.parametrize("which,at", [("empty_class", 1), ("p3", 5)])
def test_an_emptied_class_ends_the_log(gpu_lib, oracle, which, at):
    if which == "p3":
        problem, cfg = p3(), dict(NCEM, cvtest="clas", it_max=30, seed=24)
    else:
        case = load_case(which)
        problem = (case["x"], case["nei"], case["k"], case["prop"], case["center"], case["disp"])
        cfg = dict(NCEM, cvtest="clas", it_max=100, seed=0)
    res, got, want_res, want = logged_both(oracle, problem, **cfg)
    assert want_res["status"] == 2 and want_res["iters"] == at
    assert [ev["kind"] for ev in want] == ["line"] * at + ["empty"] and want[-1]["iter"] == at
    assert got[-1]["kind"] == "empty" and got[-1]["iter"] == at and got[-1]["emptyk"] == want_res["emptyk"]


# ---- the unbatched forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cvtest", ["clas", "none"])
@pytest.mark.parametrize("which", ["p1", "p3"])
def test_the_fuzzy_algorithm_one_iteration_per_wait(gpu_lib, oracle, which, cvtest):
    problem = p1() if which == "p1" else p3()
    logged_both(oracle, problem, **dict(NCEM, algo="nem", cvtest=cvtest, it_max=6 if which == "p1" else 4))


@pytest.mark.parametrize("thres", [1e-4, 0.05])
def test_the_criterion_test_of_a_logging_run(gpu_lib, oracle, thres):
    res, got, want_res, want = logged_both(oracle, p1(), **dict(NCEM, cvtest="crit_logged", cvthres=thres, it_max=40))
    assert want_res["converged"] and 0 < want_res["iters"] < 40
    print("crit_logged %g: converged at iteration %d" % (thres, want_res["iters"]))


def test_one_logged_iteration_per_call_equals_the_batched_run(gpu_lib, oracle):
    """nemgpu_iterate_logged in a loop (the start, then iteration by iteration until converged) against nemgpu_run_logged
    (batches, twins, one lock-step criteria pass): every float of every line bit for bit -- the criteria are i-ordered
    sums of the same kernels whichever engine holds the partition -- and both equal to the oracle's trace."""
    cfg = dict(NCEM, cvtest="clas", it_max=40)
    want_res, want = oracle.trace_run(*p1(), **cfg)
    assert want_res["converged"] and want_res["iters"] == 11
    eng = engine_for(p1(), **cfg)
    res, stepwise = eng.iterate_logged(1)
    while res["status"] == 0 and not res["converged"] and res["iters"] < cfg["it_max"]:
        res, ev = eng.iterate_logged(0)
        stepwise += ev
    eng.close()
    eng = engine_for(p1(), **cfg)
    res_run, batched = eng.run_logged()
    eng.close()
    same_events(stepwise, want, "ncem", empty_sizes=False)
    same_events(batched, want, "ncem", empty_sizes=False)
    assert res["iters"] == res_run["iters"] == 11 and res["converged"] and res_run["converged"]
    identical_events(stepwise, batched)


# ---- the smallest problem, and no iteration at all --------------------------------------------------------------------
@pytest.mark.parametrize("it_max", [0, 2])
@pytest.mark.parametrize("algo", ["ncem", "nem"])
def test_three_families_one_organism(gpu_lib, oracle, algo, it_max):
    res, got, want_res, want = logged_both(oracle, p2(), **dict(NCEM, algo=algo, it_max=it_max))
    if it_max == 0:
        assert len(got) == 1 and got[0]["iter"] == 0 and got[0]["nbobs_k"] is None and math.isnan(res["crit"][0])


# ---- random starts ----------------------------------------------------------------------------------------------
def starts_that_draw_in_their_iterations(events):
    """(the oracle's trace) the starts whose sweeps drew from the tie stream behind their line 0"""
    at0, last = {}, {}
    for ev in events:
        if ev["kind"] == "line" and ev["iter"] == 0:
            at0[ev["start"]] = ev["draws"]
        if ev["kind"] != "start":
            last[ev["start"]] = ev["draws"]
    return [s for s in at0 if last[s] != at0[s]]


def random_both(oracle, x, nei, k, starts, rng_seed, **cfg):
    from pangenomenem_amd.engine import NemEngine
    okw = {key: v for key, v in cfg.items() if key not in ("seed", "param_fix")}
    want_res, want = oracle.trace_run_random(x, nei, k, n_starts=starts, rng_seed=rng_seed, seed=cfg["seed"], **okw)
    eng = NemEngine(x.shape[0], x.shape[1], k)
    eng.set_matrix(x)
    eng.set_graph(nei)
    eng.configure(**cfg)
    res, got = eng.run_random_logged(starts, rng_seed)
    how = eng.random_start_counters()
    eng.close()
    assert [ev["start"] for ev in got if ev["kind"] == "start"] == list(range(starts))   # each start once, in order
    same_events(got, want, cfg["algo"])
    assert res["best_start"] == want_res["best_start"] and res["status"] == want_res["status"]
    if want_res["best_start"] >= 0:
        assert res["iters"] == want_res["iters"] and res["converged"] == want_res["converged"]
        if cfg["algo"] == "ncem":
            assert np.array_equal(res["c"], want_res["c"])
        assert maxdiff(res["c"], want_res["c"]) <= TOL
        assert np.array_equal(res["center"], want_res["center"])
        for key in ("disp", "prop"):
            assert maxdiff(res[key], want_res[key]) <= TOL, key
        assert_crit_close(res["crit"], want_res["crit"], 1e-6)
    return res, got, how, want_res, want


RANDOM = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=12, tie="libc", seed=5)


@pytest.mark.parametrize("starts", [1, 3, 64, 65])
@pytest.mark.parametrize("n", [300, 2000])
def test_random_starts_in_lock_step_and_one_after_the_other(gpu_lib, oracle, n, starts):
    """Twelve organisms: hundreds of ties per start, all of them in the initial sweeps (asserted on the oracle's draw
    counts) -- up to 64 starts stay in lock step to the end, 65 take the one-after-the-other form, as does one."""
    x, _ = synth.bernoulli_pa_matrix(n, 12, 5, p=(0.9, 0.5, 0.1))
    nei = synth.contiguity_graph(n, 5)
    res, got, how, want_res, want = random_both(oracle, x, nei, 3, starts, 5, **RANDOM)
    assert starts_that_draw_in_their_iterations(want) == [] and want[-1]["draws"] > 0
    print("%d starts of %d families: %s" % (starts, n, how))
    if 1 < starts <= 64:
        assert how["in_lockstep"] == starts and how["alone"] == 0 and how["redone"] == 0 and how["rounds"] >= 1, how
    else:
        assert how["alone"] == starts and how["in_lockstep"] == 0 and how["redone"] == 0 and how["rounds"] == 0, how


def test_random_starts_that_empty_classes(gpu_lib, oracle):
    """P3, K = 8: start 3 empties a class at iteration 7; its EMPTY event carries EstimSizes' sizes, and the next
    start's line 0 prints them (nothing resets NbObs between starts)."""
    x, nei, k = p3()[:3]
    res, got, how, want_res, want = random_both(oracle, x, nei, k, 6, 4, **dict(RANDOM, seed=4))
    empties = [ev for ev in want if ev["kind"] == "empty"]
    assert [(ev["start"], ev["iter"]) for ev in empties] == [(3, 7)]
    print("six starts of P3: %s" % how)
    n, d = x.shape
    text = random_log_text(got, n, k, d, 0.5, res["best_start"], res["crit"][3])
    assert_same_nem_log(text, random_log_text(want, n, k, d, 0.5, want_res["best_start"], want_res["crit"][3]))
    line0 = text.split("Random initialization 5 :\n")[1].split("\n")[0]
    assert line0.endswith("".join((" %7.1f" % v) * d for v in empties[0]["nbobs_k"]))


def test_random_starts_that_draw_behind_their_initial_sweeps(gpu_lib, oracle):
    """300 x 1 069 half-and-half columns: some starts' iterations draw (asserted on the oracle's draw counts), the logged
    lock-step round loses its bet, hands nothing over and the call runs the starts one after the other: the counters
    say so, and every event arrives exactly once."""
    x, _ = synth.bernoulli_pa_matrix(300, 1069, 2, p=(0.5, 0.5, 0.5))
    nei = synth.contiguity_graph(300, 2)
    res, got, how, want_res, want = random_both(oracle, x, nei, 3, 8, 2, **dict(RANDOM, seed=2))
    assert starts_that_draw_in_their_iterations(want) != []
    print("eight starts of 300 x 1069: %s" % how)
    assert how["redone"] > 0 and how["alone"] == 8 and how["in_lockstep"] == 0, how
    assert len(got) == len(want)


@pytest.mark.parametrize("algo,tie", [("nem", "hash"), ("ncem", "hash")])
def test_random_starts_without_a_stream_to_bet_on(gpu_lib, oracle, algo, tie):
    x, _ = synth.bernoulli_pa_matrix(300, 12, 5, p=(0.9, 0.5, 0.1))
    nei = synth.contiguity_graph(300, 5)
    res, got, how, want_res, want = random_both(oracle, x, nei, 3, 5, 5, **dict(RANDOM, algo=algo, tie=tie, it_max=8))
    print("five starts, %s / %s: %s" % (algo, tie, how))
    assert how["in_lockstep"] == 5 and how["alone"] == 0 and how["redone"] == 0, how


# ---- the engine is left usable ---------------------------------------------------------------------------------------
def test_a_plain_run_after_the_logged_ones_equals_a_fresh_engine(gpu_lib):
    """The twins, the set-aside copies and the retargeted streams leave nothing behind: run() on an engine that has just
    done run_logged() and run_random_logged() is, bit for bit, run() on a fresh one."""
    cfg = dict(NCEM, cvtest="clas", it_max=40)
    x, nei, k, prop, center, disp = p1()
    fresh = engine_for(p1(), **cfg)
    want = fresh.run()
    fresh.close()
    eng = engine_for(p1(), **cfg)
    eng.run_logged()
    first = eng.run()
    eng.configure(**dict(cfg, tie="libc"))
    eng.run_random_logged(3, 7)
    eng.set_params(prop, center, disp)
    eng.configure(**cfg)
    second = eng.run()
    eng.close()
    for got in (first, second):
        assert got["iters"] == want["iters"] == 11 and got["converged"] and got["status"] == 0
        for key in ("c", "prop", "center", "disp", "nbobs_k", "crit"):
            assert bits_equal(got[key], want[key]), key
