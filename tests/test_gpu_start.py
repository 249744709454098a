"""A run's fixed cost (nem_engine.hip enqueue_init): the restart head inside the start's density launch (k_density_start,
NEM_MI355X_START_FUSED, default on) against the path it replaces -- k_finish + k_density as two launches.
restart_iterate(m) for m = 0, 1, 3 with the switch on and off: labels, parameters, the stored densities pkfki /
logpkfki, class sizes and the result's counters equal bit for bit.  m = 0 leaves the start's own densities and parameter copy behind, so that case looks at
exactly what the new launch wrote.  Two cases also against the oracle, so that both paths wrong alike cannot pass."""
import ctypes as C
import os

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.engine import ALGO
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

SWITCHES = ("NEM_MI355X_START_FUSED",)
ALL_OFF, ALL_ON = (0,), (1,)
SETTINGS = (ALL_OFF, ALL_ON)
SKIP_KEYS = {"loop_seconds"}
CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, tie="hash", seed=1)


def make_engine(setting, n, d, k, x, nei, env=None):
    from pangenomenem_amd.engine import NemEngine
    env = dict(env or {})
    env.update({key: str(v) for key, v in zip(SWITCHES, setting)})
    saved = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                        # (read when the engine is created)
    try:
        eng = NemEngine(n, d, k)
    finally:
        for key, v in saved.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    eng.set_matrix(x); eng.set_graph(nei)
    return eng


def stored_density(eng):
    """the densities the last launch left (no recomputation: nemgpu_get_density only copies)"""
    pk = np.zeros((eng.n, eng.k), np.float64)
    lp = np.zeros((eng.n, eng.k), np.float32)
    eng._chk(eng.lib.nemgpu_get_density(eng._h, pk.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p)))
    return pk, lp


def snapshot(eng, r):
    out = dict(r)
    out.update(eng.results())
    if eng.cfg.algo == ALGO["ncem"]:              # (a fuzzy run has memberships only: results()["c"])
        out["labels"] = eng.labels()
    out["pkfki"], out["logpkfki"] = stored_density(eng)
    return out


def assert_same(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        if key in SKIP_KEYS:
            continue
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.shape == v.shape and u.dtype == v.dtype, (what, key)
        assert u.tobytes() == v.tobytes(), (what, key, a[key], b[key])


def run_starts(setting, n, d, k, x, nei, starts, ms=(0, 1, 3), env=None, **cfg):
    """one engine through every start in `starts` ((prop, center, disp) or (prop, center, disp, beta) each),
    restart_iterate(m) for every m"""
    eng = make_engine(setting, n, d, k, x, nei, env=env)
    out = []
    try:
        for prop, center, disp, *beta in starts:
            eng.set_params(prop, center, disp)
            eng.configure(**dict(CFG, **dict(cfg, **(dict(beta=beta[0]) if beta else {}))))
            for m in ms:
                out.append(snapshot(eng, eng.restart_iterate(m)))
        counters = eng.graph_counters()
    finally:
        eng.close()
    return out, counters


def all_settings(n, d, k, x, nei, starts, ms=(0, 1, 3), env=None, **cfg):
    ref, _ = run_starts(ALL_OFF, n, d, k, x, nei, starts, ms, env, **cfg)
    for setting in SETTINGS[1:]:
        got, _ = run_starts(setting, n, d, k, x, nei, starts, ms, env, **cfg)
        assert len(got) == len(ref)
        for j, (a, b) in enumerate(zip(ref, got)):
            assert_same(a, b, "switches %r, step %d" % (setting, j))
    return ref


def ushaped(n, d, k, seed=3, weights="small"):
    x, _ = synth.ushaped_pa_matrix(n, d, seed)
    prop, center, disp = synth.default_init(d) if k == 3 else synth.kclass_init(x, k)
    return x, synth.contiguity_graph(n, seed, weights=weights, d=d), (prop, center, disp)


def test_configs1_shape():
    """the bench's shape and start: PPanGGOLiN's default .m (a centre of 1/2 in class 1, uniform dispersions per class)"""
    n, d = 20000, 500
    x, nei, start = ushaped(n, d, 3)
    out = all_settings(n, d, 3, x, nei, [start], ms=(0, 1, 3, 7))
    assert out[3]["iters"] == 7


@pytest.mark.parametrize("disper", ["sk_", "skd"])
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_models_and_k(disper, k):
    """D not a multiple of 32 or 64, N not a multiple of 256"""
    n, d = 9001, 77
    x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
    start = synth.kclass_init(x, k)
    nei = synth.contiguity_graph(n, 4, d=d)
    all_settings(n, d, k, x, nei, [start], disper=disper, seed=4)


@pytest.mark.parametrize("d", [31, 257, 1000])
def test_organism_counts_around_the_fast_forward_switch(d):
    """d >= 256 takes the fast-forwarded uniform chain, below it the plain one; 1000 is close to the fused kernel's cap"""
    n = 5003
    x, nei, start = ushaped(n, d, 3, seed=7)
    all_settings(n, d, 3, x, nei, [start])


@pytest.mark.parametrize("disper", ["sk_", "skd"])
def test_given_dispersions_differ_inside_a_class(disper):
    """general chain from given parameters: one class with per-organism dispersions, one uniform, one with a single
    organism off by one unit in the last place"""
    n, d = 7000, 90
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=5)
    rng = np.random.default_rng(2)
    disp = disp.copy()
    disp[0] = rng.uniform(0.02, 0.4, d).astype(np.float32)
    disp[2, d - 1] = np.nextafter(disp[2, d - 1], np.float32(1))
    all_settings(n, d, 3, x, nei, [(prop, center, disp)], disper=disper)


def test_centres_outside_zero_half_one():
    """a centre that is none of 0, 1/2, 1 sends its class down the general chain (|(int)(x - mu)| of any float)"""
    n, d = 6000, 70
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=6)
    center = center.copy()
    center[0, 3] = 2.5; center[0, 4] = -1.25; center[2, 0] = 0.25
    all_settings(n, d, 3, x, nei, [(prop, center, disp)])


@pytest.mark.parametrize("tie", ["hash", "first"])
def test_two_classes_with_identical_parameters(tie):
    """every site ties between classes 0 and 1 in the blind sweep"""
    n, d = 8000, 64
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=8)
    prop = np.array([0.3, 0.3, 0.4], np.float32)
    center = center.copy(); disp = disp.copy()
    center[1] = center[0]; disp[1] = disp[0]
    all_settings(n, d, 3, x, nei, [(prop, center, disp)], tie=tie)


def test_zero_density_sites_in_the_blind_sweep():
    """dispersions at and below EPSILON (null densities, nem_mod.c:662-666) and small enough for exp to underflow; the
    middle class gets a 0/1 centre (with PPanGGOLiN's 1/2 nothing mismatches it and no site's densities are all zero)"""
    n, d = 6000, 300
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=9)
    center = center.copy()
    center[1] = (np.random.default_rng(9).random(d) < 0.5).astype(np.float32)
    tiny = np.full((3, d), 1e-30, np.float32)
    small = np.full((3, d), 1e-9, np.float32)
    zero_one = disp.copy(); zero_one[0, :5] = 0.0
    out = all_settings(n, d, 3, x, nei, [(prop, center, tiny), (prop, center, small), (prop, center, zero_one)], ms=(0, 1))
    assert any(o["n_zero_density"] > 0 for o in out)


def test_long_rows_isolated_sites_and_far_neighbours():
    """rows of more than four neighbours, isolated sites, neighbours in other blocks on both sides"""
    n, d = 5000, 50
    x, _ = synth.ushaped_pa_matrix(n, d, 10)
    start = synth.default_init(d)
    ptr, idx, w = synth.ring_graph(n, 3, 10, 1, 3)
    ptr = np.asarray(ptr); idx = np.asarray(idx); w = np.asarray(w)
    # isolate every 97th site: drop its row and every mention of it
    iso = np.zeros(n, bool); iso[::97] = True
    row = np.repeat(np.arange(n), np.diff(ptr))
    keep = ~iso[row] & ~iso[idx]
    # ... and add far chords i <-> (i + n/2) % n for every 5th site that is not isolated
    src = np.arange(0, n, 5); src = src[~iso[src] & ~iso[(src + n // 2) % n]]
    far_r = np.concatenate([src, (src + n // 2) % n]); far_c = np.concatenate([(src + n // 2) % n, src])
    rows = np.concatenate([row[keep], far_r]); cols = np.concatenate([idx[keep], far_c])
    ws = np.concatenate([w[keep], np.full(far_r.size, 2.0, np.float32)]).astype(np.float32)
    order = np.argsort(rows, kind="stable")
    ptr2 = np.zeros(n + 1, np.int32); np.add.at(ptr2, rows + 1, 1); ptr2 = np.cumsum(ptr2).astype(np.int32)
    nei = (ptr2, cols[order].astype(np.int32), ws[order])
    assert int(np.diff(ptr2).max()) > 4 and int(np.diff(ptr2).min()) == 0
    all_settings(n, d, 3, x, nei, [start], beta=0.3)


def test_start_whose_beta_sweep_needs_a_third_round():
    """poor parameters and a strong field (tests/test_gpu_edges.py's hard starts): the host finishes the start's sweep"""
    n, d = 6000, 40
    x, _ = synth.bernoulli_pa_matrix(n, d, 5)
    nei = synth.contiguity_graph(n, 5)
    prop, center, disp = synth.default_init(d)
    rng = np.random.default_rng(1)
    starts = [(prop, center, disp)] * 5
    for rep in range(6):
        starts.append((prop, (rng.random((3, d)) < 0.5).astype(np.float32), np.full((3, d), 0.45, np.float32), float(1.0 + rep)))
    ref = None
    for setting in SETTINGS:
        got, counters = run_starts(setting, n, d, 3, x, nei, starts, ms=(0, 2), seed=3)
        assert counters["host_finished_sweeps"] > 0
        if ref is None:
            ref = got
        for j, (a, b) in enumerate(zip(ref, got)):
            assert_same(a, b, "switches %r, step %d" % (setting, j))


def test_one_engine_through_many_different_starts():
    n, d = 10000, 120
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=11)
    rng = np.random.default_rng(4)
    starts = []
    for rep in range(12):
        c = center.copy(); e = disp.copy(); p = prop.copy()
        if rep % 3 == 1:
            c = (rng.random((3, d)) < 0.5).astype(np.float32)
        if rep % 3 == 2:
            e = rng.uniform(0.05, 0.45, (3, d)).astype(np.float32)           # general chain
        if rep % 4 == 3:
            e = np.repeat(rng.uniform(0.05, 0.45, (3, 1)), d, axis=1).astype(np.float32)
            p = np.array([0.2, 0.5, 0.3], np.float32)
        starts.append((p, c, e))
    all_settings(n, d, 3, x, nei, starts, ms=(1, 0, 7))


def test_without_graphs():
    n, d = 8000, 300
    x, nei, start = ushaped(n, d, 3)
    all_settings(n, d, 3, x, nei, [start], ms=(0, 1, 3, 7, 7), env={"NEM_MI355X_GRAPHS": "0"})


@pytest.mark.parametrize("what", ["libc", "fuzzy", "wide", "no_graph", "beta0"])
def test_engines_that_do_not_qualify_keep_the_old_start(what):
    """TIE_LIBC, fuzzy NEM, D above the fused kernel's cap, no neighbourhood, beta = 0: the switches change nothing"""
    n, d = (3000, 1100) if what == "wide" else (6000, 60)
    x, nei, start = ushaped(n, d, 3, seed=12)
    cfg = {}
    if what == "libc":
        cfg = dict(tie="libc")
    if what == "fuzzy":
        cfg = dict(algo="nem")
    if what == "beta0":
        cfg = dict(beta=0.0)
    if what == "no_graph":
        nei = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    all_settings(n, d, 3, x, nei, [start], **cfg)


@pytest.mark.parametrize("case", ["default", "general"])
def test_against_the_oracle(oracle, case):
    n, d = 9001, 77
    x, nei, (prop, center, disp) = ushaped(n, d, 3, seed=13)
    if case == "general":
        disp = np.random.default_rng(6).uniform(0.05, 0.45, (3, d)).astype(np.float32)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", it_max=3, tie="hash", seed=5)
    want = oracle.run(x, nei, 3, prop, center, disp, **cfg)
    eng = make_engine(ALL_ON, n, d, 3, x, nei)
    try:
        eng.set_params(prop, center, disp)
        eng.configure(**cfg)
        got = eng.restart_iterate(3)
        got.update(eng.results())
    finally:
        eng.close()
    assert want["iters"] == got["iters"] and np.array_equal(want["c"], got["c"])
    assert np.array_equal(want["center"], got["center"])
    assert maxdiff(want["disp"], got["disp"]) <= 1e-6 and maxdiff(want["prop"], got["prop"]) <= 1e-6
    assert want["n_zero_density"] == got["n_zero_density"]
