"""The oracle's per-iteration trace (orc_set_trace, oracle/nem_oracle.h) anchored on the CPU, before any GPU test
relies on it: it changes no result, every line restates what a shorter run and the single steps give, and its text
-- put together by tests/log_text_util.py -- is the log the unmodified reference wrote."""
import gzip
import json
import os

import numpy as np
import pytest

from tests.log_text_util import random_log_text, run_log_text
from tests.test_gpu_fuzz import random_problem
from tests.test_gpu_golden import LOG_CASES, RANDOM_LOGS, log_case
from tests.util import assert_same_nem_log, bits_equal

SEEDS = list(range(120))
RESULT_KEYS = ("c", "prop", "center", "disp", "nbobs_k", "crit", "pkfki", "logpkfki")
SCALAR_KEYS = ("status", "iters", "converged", "emptyk", "n_zero_density")


def lines_of(events):
    return [ev for ev in events if ev["kind"] == "line"]


@pytest.mark.parametrize("seed", SEEDS)
def test_trace_changes_no_result(oracle, seed):
    x, nei, k, prop, center, disp, cfg = random_problem(seed)
    plain = oracle.run(x, nei, k, prop, center, disp, **cfg)
    traced, events = oracle.trace_run(x, nei, k, prop, center, disp, **cfg)
    again = oracle.run(x, nei, k, prop, center, disp, **cfg)          # (and it is off again afterwards)
    for other in (traced, again):
        for key in SCALAR_KEYS:
            assert plain[key] == other[key], (seed, key)
        for key in RESULT_KEYS:
            assert bits_equal(plain[key], other[key]), (seed, key)
    assert len(events) > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_line_t_is_the_run_cut_at_t(oracle, seed):
    """iters + 1 lines (an emptied class: the lines before it, then EMPTY, then nothing); line t carries the criteria,
    parameters and sizes of run(it_max=t), and its crit_before is orc_crit of run(it_max=t-1)'s partition on
    run(it_max=t)'s densities."""
    x, nei, k, prop, center, disp, cfg = random_problem(seed)
    res, events = oracle.trace_run(x, nei, k, prop, center, disp, **cfg)
    lines = lines_of(events)
    assert [ev["iter"] for ev in lines] == list(range(len(lines)))
    assert all(ev["start"] == 0 for ev in events) and lines[0]["nbobs_k"] is None
    if res["status"] == 2:
        assert events[-1]["kind"] == "empty" and len(events) == len(lines) + 1 == res["iters"] + 1
        assert events[-1]["iter"] == res["iters"] and events[-1]["emptyk"] == res["emptyk"] > 0
        assert bits_equal(events[-1]["nbobs_k"], res["nbobs_k"])
        n_lines = res["iters"] - 1
    else:
        assert len(events) == len(lines) == res["iters"] + 1
        n_lines = res["iters"]
    short = {t: oracle.run(x, nei, k, prop, center, disp, **dict(cfg, it_max=t)) for t in range(n_lines + 1)}
    for t in range(1, n_lines + 1):
        ev, cut = lines[t], short[t]
        assert cut["iters"] == t and cut["status"] == 0, (seed, t)
        for key, name in (("crit_after", "crit"), ("prop", "prop"), ("center", "center"), ("disp", "disp"),
                          ("nbobs_k", "nbobs_k")):
            assert bits_equal(ev[key], cut[name]), (seed, t, key)
        before = oracle.crit(short[t - 1]["c"], nei, cfg["beta"], cut["pkfki"], cut["logpkfki"])
        assert bits_equal(ev["crit_before"], before), (seed, t)


@pytest.mark.parametrize("tie", ["hash", "first"])
@pytest.mark.parametrize("seed", SEEDS[::3])
def test_line_0_is_the_start_step_by_step(oracle, seed, tie):
    x, nei, k, prop, center, disp, cfg = random_problem(seed)
    cfg = dict(cfg, tie=tie)
    _, events = oracle.trace_run(x, nei, k, prop, center, disp, **cfg)
    ev = events[0]
    assert ev["kind"] == "line" and ev["iter"] == 0
    ncem = cfg["algo"] == "ncem"
    pk, lp, _ = oracle.density(x, prop, center, disp)
    blind, _ = oracle.sweep(np.zeros((x.shape[0], k), np.float32), nei, 0.0, pk, ncem, tie=tie, seed=cfg["seed"], sweep_id=0)
    first, _ = oracle.sweep(blind, nei, cfg["beta"], pk, ncem, tie=tie, seed=cfg["seed"], sweep_id=1)
    assert bits_equal(ev["crit_before"], oracle.crit(blind, nei, cfg["beta"], pk, lp)), seed
    assert bits_equal(ev["crit_after"], oracle.crit(first, nei, cfg["beta"], pk, lp)), seed
    assert bits_equal(ev["prop"], np.asarray(prop, np.float32)) and bits_equal(ev["center"], center) and bits_equal(ev["disp"], disp)


def _random_log_cases():
    return sorted(c for c in os.listdir(RANDOM_LOGS) if os.path.isdir(os.path.join(RANDOM_LOGS, c)))


@pytest.mark.parametrize("case", _random_log_cases())
def test_trace_text_is_the_reference_random_start_log(oracle, case):
    """The four logs the unmodified reference wrote for INIT_RANDOM runs (tests/golden/make_random_logs.py), reproduced
    from the oracle's trace by the Python formatter: start blocks, NbObs carried from start to start, emptied classes."""
    here = os.path.join(RANDOM_LOGS, case)
    meta = json.load(open(os.path.join(here, "meta.json")))
    z = np.load(os.path.join(here, "inputs.npz"))
    n, d, k = int(z["n"]), int(z["d"]), int(z["k"])
    x = np.unpackbits(z["xbits"], axis=1, bitorder="little")[:, :d]
    nei = (z["nei_ptr"], z["nei_idx"], z["nei_w"])
    res, events = oracle.trace_run_random(x, nei, k, n_starts=meta["n_starts"], rng_seed=meta["seed"], algo=meta["algo"],
                                          beta=meta["beta"], disper=meta["disper"], propor="pk", cvtest="clas",
                                          cvthres=1e-8, it_max=100, tie="libc")
    assert res["best_start"] == meta["best_start"]
    assert [ev["start"] for ev in events if ev["kind"] == "start"] == list(range(meta["n_starts"]))
    assert sum(ev["kind"] == "empty" for ev in events) == meta["starts_with_empty_class"]
    got = random_log_text(events, n, k, d, meta["beta"], res["best_start"], res["crit"][3])
    want = gzip.open(os.path.join(here, "ref_log.txt.gz"), "rt").read()
    assert_same_nem_log(got, want)


@pytest.mark.parametrize("algo,disper,n,d", LOG_CASES)
def test_trace_text_is_the_reference_log(oracle, reference, tmp_path, algo, disper, n, d):
    """... and the reference's own <Fname>.log of the three INIT_PARAM_FILE runs of tests/test_gpu_golden.py."""
    from pangenomenem_amd import synth
    base, args = log_case(str(tmp_path), algo, disper, n, d)
    assert reference.nem(base, *args) == 0
    x, _ = synth.bernoulli_pa_matrix(n, d, n + d)
    nei = synth.contiguity_graph(n, n + d)
    prop, center, disp = synth.default_init(d)
    res, events = oracle.trace_run(x, nei, 3, prop, center, disp, algo=algo, beta=0.5, disper=disper, propor="pk",
                                   cvtest="clas", cvthres=1e-8, it_max=20, tie="libc", seed=1)
    assert res["tie_draws"] == 0                              # (no tie: the reference's time-seeded stream is not drawn from)
    got = run_log_text(events, n, 3, d, 0.5)
    assert_same_nem_log(got, open(base + ".log").read())


def test_the_event_comparison_notices(oracle):
    """same_events of tests/test_gpu_log_events.py on the oracle's own trace: it passes a copy, and fails one whose
    criterion D is off by 1e-5 relative on one line, whose crit_before is the line before's (the wrong buffer's
    partition), whose densities are the iteration before's (crit_after of the line before), whose sizes are off by one
    family, whose dispersion is off by 1e-5, or that lacks its last line."""
    import copy
    from tests.test_gpu_log_events import NCEM, p1, same_events
    _, want = oracle.trace_run(*p1(), **dict(NCEM, it_max=5))
    same_events(copy.deepcopy(want), want, "ncem")

    def off_d(evs): evs[3]["crit_before"][0] *= np.float32(1.00001)
    def wrong_partition(evs): evs[3]["crit_before"] = evs[2]["crit_before"]
    def stale_densities(evs): evs[4]["crit_after"] = evs[3]["crit_after"]
    def sizes(evs): evs[2]["nbobs_k"][1] += 1
    def disp(evs): evs[5]["disp"][0, 0] += np.float32(1e-5)
    def short(evs): evs.pop()
    def sizes_on_line_0(evs): evs[0]["nbobs_k"] = np.zeros(3, np.float32)

    for spoil in (off_d, wrong_partition, stale_densities, sizes, disp, short, sizes_on_line_0):
        got = copy.deepcopy(want)
        spoil(got)
        with pytest.raises(AssertionError):
            same_events(got, want, "ncem")
