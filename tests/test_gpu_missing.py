"""NCEM on matrices with missing cells, on the GPU: the masked kernels (k_density_masked, k_mstep_counts_masked,
k_finish_masked) and the host-stepped loop against the oracle where nothing is missing, against the numpy statement
(tests/missing_util.py) step by step, and the drop-in nem() against the recorded reference's files."""
import os

import numpy as np
import pytest

from tests import missing_util as mu
from tests.util import (assert_printed_g_close, assert_same_nem_log, bits_equal, maxdiff, random_hard_partition,
                        ulp_diff64)

pytestmark = pytest.mark.gpu
TOL = 1e-6
NAMES = mu.fixture_names()

_cases = {}


def case_of(name):
    if name not in _cases:
        _cases[name] = mu.load_fixture(name)
    return _cases[name]


def run_kw(cfg):
    return dict(algo=cfg["algo"], beta=cfg["beta"], disper=cfg["disper"], propor=cfg["propor"], cvtest=cfg["cvtest"],
                cvthres=cfg["cvthres"], it_max=cfg["it_max"])


def engine_for(case, observed, **cfg):
    from pangenomenem_amd.engine import NemEngine
    n, d = case["x"].shape
    eng = NemEngine(n, d, case["k"])
    eng.set_matrix(case["x"])
    if observed is not None:
        eng.set_observed(observed)
    eng.set_graph(case["nei"])
    eng.set_params(case["prop"], case["center"], case["disp"])
    eng.configure(**cfg)
    return eng


@pytest.mark.parametrize("name", NAMES)
def test_all_ones_mask_runs_masked_path_and_equals_oracle(gpu_lib, oracle, name):
    """A mask of all ones keeps the engine on the masked kernels and the stepwise loop (no batch of the pipelined loop is
    enqueued); on the fixture's matrix taken as complete the run equals the oracle's as an unmasked run does."""
    case = case_of(name)
    kw = run_kw(case["cfg"])
    eng = engine_for(case, np.ones(case["x"].shape, bool), tie="hash", seed=99, **kw)
    try:
        got = eng.run()
        counters = eng.graph_counters()
    finally:
        eng.close()
    assert counters["plain"] == 0 and counters["captured"] == 0 and counters["replayed"] == 0
    want = oracle.run(case["x"], case["nei"], case["k"], case["prop"], case["center"], case["disp"], tie="hash", seed=99,
                      **kw)
    assert got["iters"] == want["iters"] and got["status"] == want["status"]
    assert got["converged"] == want["converged"]
    assert np.array_equal(got["c"], want["c"])
    assert np.array_equal(got["center"], want["center"])
    assert maxdiff(got["disp"], want["disp"]) <= TOL and maxdiff(got["prop"], want["prop"]) <= TOL


@pytest.mark.parametrize("name", ["empty_class", "c1_path_ncem_fixed", "c1_path_ncem_itmax0", "c1_ushape_ncem_cvcrit"])
def test_stepwise_loop_branches_equal_oracle(gpu_lib, oracle, name):
    """The branches of the host-stepped loop that the masked fixtures do not take, on complete golden cases under an
    all-ones mask: a class that empties mid-run (the iteration counts, the E-step does not run), fixed parameters,
    no iteration at all (the closing M-step and density), and the criterion-driven convergence test."""
    from pangenomenem_amd.engine import NemEngine
    from tests.golden_util import load_case
    case = load_case(name)
    cfg = case["cfg"]
    kw = dict(algo=cfg["algo"], beta=cfg["beta"], disper=cfg["disper"], propor=cfg["propor"], cvtest=cfg["cvtest"],
              cvthres=cfg["cvthres"], it_max=cfg["it_max"], param_fix=cfg["param_fix"], tie="hash", seed=99)
    n, d = case["x"].shape
    eng = NemEngine(n, d, case["k"])
    try:
        eng.set_matrix(case["x"])
        eng.set_observed(np.ones((n, d), bool))
        eng.set_graph(case["nei"])
        eng.set_params(case["prop"], case["center"], case["disp"])
        eng.configure(**kw)
        got = eng.run()
        assert eng.graph_counters()["plain"] == 0 and eng.graph_counters()["replayed"] == 0
    finally:
        eng.close()
    want = oracle.run(case["x"], case["nei"], case["k"], case["prop"], case["center"], case["disp"], **kw)
    assert got["iters"] == want["iters"] and got["status"] == want["status"]
    if name == "empty_class":
        assert got["status"] == 2 and got["emptyk"] == want["emptyk"] > 0
        return
    assert got["converged"] == want["converged"]
    assert np.array_equal(got["c"], want["c"])
    assert np.array_equal(got["center"], want["center"])
    assert maxdiff(got["disp"], want["disp"]) <= TOL and maxdiff(got["prop"], want["prop"]) <= TOL


def test_set_matrix_without_nan_removes_the_mask_it_made(gpu_lib):
    case = case_of("m300x40_sk_")
    xf = np.where(case["obs"], case["x"], np.nan).astype(np.float32)
    eng = engine_for(case, None, tie="hash", seed=5, **run_kw(case["cfg"]))
    fresh = engine_for(case, None, tie="hash", seed=5, **run_kw(case["cfg"]))
    try:
        eng.set_matrix(xf)                                   # NaN cells: the mask comes with the matrix
        eng.run()
        assert eng.graph_counters()["plain"] == 0
        eng.set_matrix(case["x"])                            # a complete matrix: that mask goes with it
        got, want = eng.run(), fresh.run()
        assert eng.graph_counters()["plain"] + eng.graph_counters()["replayed"] >= 1
        assert got["iters"] == want["iters"] and np.array_equal(got["c"], want["c"])
    finally:
        eng.close()
        fresh.close()


@pytest.mark.parametrize("name", NAMES)
def test_masked_steps_equal_statement(gpu_lib, name):
    """density(): LogPkFki bit-equal to the statement, PkFki within 2 ulp (the device's exp).  mstep() on hard
    partitions: bit-equal -- a random one, one that leaves a (class, organism) without an observed member, one that
    empties a class."""
    case = case_of(name)
    cfg, k = case["cfg"], case["k"]
    x, obs = case["x"], case["obs"]
    n, d = x.shape
    eng = engine_for(case, obs, tie="first", **run_kw(cfg))
    try:
        pk, lp = eng.density()
        want_pk, want_lp, _ = mu.density_masked_host(x, obs, case["prop"], case["center"], case["disp"])
        assert bits_equal(lp, want_lp)
        assert ulp_diff64(pk, want_pk) <= 2
        whole = np.flatnonzero(~obs.any(axis=1))             # the family without an observed cell: LogFk = 0, fk = 1
        assert len(whole) >= 1
        assert np.array_equal(pk[whole[0]], case["prop"].astype(np.float64))

        parts = {"random": random_hard_partition(n, k, 41)}
        # class 1 = families that did not observe organism 2 (and no other family): NbObs_KD[1][2] = 0
        lab = random_hard_partition(n, k, 43).argmax(axis=1)
        hidden = ~obs[:, 2]
        assert hidden.sum() >= 3
        lab[lab == 1] = 0
        lab[hidden] = 1
        parts["unobserved"] = np.eye(k, dtype=np.float32)[lab]
        c = random_hard_partition(n, k, 47)
        c[c[:, k - 1] == 1] = np.eye(k, dtype=np.float32)[0]
        parts["empty"] = c
        for what, c in parts.items():
            eng.set_params(case["prop"], case["center"], case["disp"])
            eng.set_partition(c)
            rc, ek = eng.mstep()
            got = eng.params()
            want = mu.mstep_masked_host(x, obs, c, cfg["disper"], cfg["propor"], case["prop"], case["center"], case["disp"])
            assert ek == want["emptyk"] and rc == want["status"], what
            if what == "unobserved":
                assert want["nbobs_kd"][1, 2] == 0 and want["nbobs_k"][1] > 0
            if what == "empty":
                assert ek == k
            for key in ("prop", "center", "disp", "nbobs_k"):
                assert bits_equal(got[key], want[key]), (what, key)
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_dropin_nem_on_masked_files_writes_reference_files(gpu_lib, tmp_path, name):
    """nem() on the five files with nan cells: .uf byte for byte, .mf as test_dropin_nem_writes_reference_files holds it,
    .log line by line, the iteration count in .stderr."""
    import nem as nem_module
    case = case_of(name)
    cfg = case["cfg"]
    base = mu.write_masked_inputs(str(tmp_path), case["x"], case["obs"], case["nei"], case["prop"], case["center"],
                                  case["disp"])
    rc = nem_module.nem(Fname=base.encode(), nk=case["k"], algo=cfg["algo"].encode(), beta=cfg["beta"],
                        convergence=cfg["cvtest"].encode(), convergence_th=cfg["cvthres"], format=b"fuzzy",
                        it_max=cfg["it_max"], dolog=True, model_family=b"bern", proportion=cfg["propor"].encode(),
                        dispersion=cfg["disper"].encode(), init_mode=2)
    assert rc == case["meta"]["nem_rc"] == 0
    assert open(base + ".uf", "rb").read() == case["ref_uf"]
    got_mf = open(base + ".mf", "rb").read().split(b"\n")
    ref_mf = case["ref_mf"].split(b"\n")
    assert len(got_mf) == len(ref_mf)
    for i, (a, b) in enumerate(zip(got_mf, ref_mf)):
        if i == 2:                                           # "  U    D    L    M   error"
            ta, tb = a.split(), b.split()
            assert len(ta) == len(tb) == 5 and ta[4] == tb[4] == b"nan"
            for u, v in zip(ta[:4], tb[:4]):
                if v in (b"-inf", b"inf", b"nan", b"-nan"):
                    assert u == v, (a, b)
                else:
                    assert_printed_g_close(u.decode(), v.decode(), (a, b))
        else:
            assert a == b, (i, a, b)
    assert_same_nem_log(open(base + ".log").read(), case["ref_log"].decode())
    text = open(base + ".stderr").read()
    assert "%d missing values / %d" % (case["meta"]["n_missing"], case["x"].size) in text
    assert ("NEM converged after %d iterations" % case["meta"]["iters"] in text) == case["meta"]["converged"]


def test_dropin_refuses_fuzzy_and_random_starts_on_masked_files(gpu_lib, tmp_path):
    import nem as nem_module
    case = case_of("m300x40_sk_")
    cfg = case["cfg"]
    base = mu.write_masked_inputs(str(tmp_path), case["x"], case["obs"], case["nei"], case["prop"], case["center"],
                                  case["disp"])
    for algo, init_mode, word in ((b"nem", 2, "only algorithm ncem"), (b"ncem", 1, "random starts")):
        for ext in ("uf", "mf", "stderr"):
            if os.path.exists(base + "." + ext):
                os.remove(base + "." + ext)
        rc = nem_module.nem(Fname=base.encode(), nk=case["k"], algo=algo, beta=cfg["beta"], convergence=b"clas",
                            convergence_th=cfg["cvthres"], format=b"fuzzy", it_max=cfg["it_max"], dolog=True,
                            model_family=b"bern", proportion=b"pk", dispersion=b"sk_", init_mode=init_mode)
        assert rc == 2
        text = open(base + ".stderr").read()
        assert word in text and "bad arguments" in text
        assert not os.path.exists(base + ".uf") and not os.path.exists(base + ".mf")


def test_batch_entries_refuse_a_masked_engine(gpu_lib):
    from pangenomenem_amd.engine import NemGpuError, run_many
    case = case_of("m300x40_sk_")
    kw = run_kw(case["cfg"])
    masked = engine_for(case, case["obs"], tie="hash", seed=3, **kw)
    plain = engine_for(case, None, tie="hash", seed=3, **kw)
    try:
        with pytest.raises(NemGpuError, match="observed mask"):
            run_many([plain, masked])
        with pytest.raises(NemGpuError, match="observed mask"):
            masked.run_random(n_starts=2, rng_seed=1)
        with pytest.raises(NemGpuError, match="observed mask"):
            masked.restart_iterate(1)
        with pytest.raises(NemGpuError, match="observed mask"):
            masked.profile_density(reps=1)
        assert masked.graph_counters() == dict(plain=0, captured=0, replayed=0, host_finished_sweeps=0)
        masked.configure(**dict(kw, algo="nem"))
        with pytest.raises(NemGpuError, match="ncem"):
            masked.run()
        a = plain.run()                                      # a plain engine works afterwards
        b = run_many([plain])[0]
        assert a["iters"] == b["iters"] > 0 and np.array_equal(a["c"], b["c"])
    finally:
        masked.close()
        plain.close()


def test_removing_the_mask_leaves_no_trace(gpu_lib):
    """After set_observed(None) the engine's run is bit-equal to a fresh unmasked engine's, on the pipelined path."""
    case = case_of("m300x40_skd")
    kw = run_kw(case["cfg"])
    eng = engine_for(case, case["obs"], tie="hash", seed=5, **kw)
    fresh = engine_for(case, None, tie="hash", seed=5, **kw)
    try:
        masked = eng.run()
        assert eng.graph_counters()["plain"] == 0
        eng.set_observed(None)
        got = eng.run()
        want = fresh.run()
        assert eng.graph_counters()["plain"] + eng.graph_counters()["replayed"] >= 1
        assert got["iters"] == want["iters"] and got["status"] == want["status"]
        for key in ("c", "prop", "center", "disp", "nbobs_k", "crit"):
            assert bits_equal(got[key], want[key]), key
        assert masked["status"] == 0
    finally:
        eng.close()
        fresh.close()
