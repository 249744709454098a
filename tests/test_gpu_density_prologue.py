"""The prologue of the fused density launch (density_fused_body, nem_kernels.hip): a class's two logs come out of one
call on alternating lanes, and the centres, the inertia and the mismatch masks of a non-empty NCEM class below 2^24
families out of integer comparisons (tests/test_centre_rule.py holds that rule to the float rule on the host).  Held here
through the C ABI, bit for bit, two ways: against the CPU oracle -- labels, centres, epsilon, pi, class sizes, logpkfki --
and against the paths the engine offers beside the default one: the start as k_finish + k_density and every verifying
round on its own (NEM_MI355X_START_FUSED=0, NEM_MI355X_SHADOW_VERIFY=0), the word-synchronous fast-forward
(NEM_MI355X_FF_BATCH=0) and the stepped chain (NEM_MI355X_FF=0).

Shapes: N = 1 ... 300 (one and two blocks of 256 families, a last wave partly past the rows) by D = 1 ... 1024 (one
organism, either side of a 32-organism mask word, of a 64-organism wave, of a thread's second and fourth row, the
kernel's cap); K = 2 ... 5; sk_ and skd.  Conditions: a class of one family, zero counts that tie N_k / 2 and miss it
by one on either side, a class that empties, given dispersions 0.5 (l1 = 0), 0.45, 1e-3 and 0.7 (l1 < 0: the stepped
chain), a dispersion at or below EPSILON, given centres outside {0, 1/2, 1}, a run of one iteration, graphs on and off,
five restarts of one engine, a lock-step batch of three sizes."""
import os

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests.test_gpu_ff_batch import stored_density

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", it_max=3, tie="hash", seed=3)
UNFUSED = {"NEM_MI355X_START_FUSED": "0", "NEM_MI355X_SHADOW_VERIFY": "0"}
WORD = {"NEM_MI355X_FF_BATCH": "0"}
STEPPED = {"NEM_MI355X_FF": "0"}
SKIP_KEYS = {"loop_seconds"}
NS = (1, 63, 65, 255, 257, 300)
DS = (1, 31, 32, 33, 64, 65, 257, 500, 1023, 1024)


def make_engine(n, d, k, x, nei, env):
    from pangenomenem_amd.engine import NemEngine
    saved = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                            # (read when the engine is created)
    try:
        eng = NemEngine(n, d, k)
    finally:
        for key, v in saved.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    eng.set_matrix(x)
    eng.set_graph(nei)
    return eng


def snapshot(eng, r):
    out = dict(r)
    out.update(eng.results())
    out["labels"] = eng.labels()
    out["pkfki"], out["logpkfki"] = stored_density(eng)
    return out


def run(eng):
    return eng.run()


def restarts(*ms):
    return [lambda eng, m=m: eng.restart_iterate(m) for m in ms]


def engine_steps(x, nei, k, starts, steps, env, **cfg):
    """one engine: every start in `starts`, every step in `steps` (callables eng -> result) on it"""
    n, d = x.shape
    eng = make_engine(n, d, k, x, nei, env)
    out = []
    try:
        for prop, center, disp in starts:
            eng.set_params(prop, center, disp)
            eng.configure(**cfg)
            for step in steps:
                out.append(snapshot(eng, step(eng)))
        counters = eng.graph_counters()
    finally:
        eng.close()
    return out, counters


def assert_same(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        if key in SKIP_KEYS:
            continue
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.shape == v.shape and u.dtype == v.dtype, (what, key)
        assert u.tobytes() == v.tobytes(), (what, key, a[key], b[key])


def paths_agree(x, nei, k, starts, steps=(run,), others=(UNFUSED,), env=None, **cfg):
    """the default path and every path in `others` give the same bits, step by step; returns the default path's"""
    got, counters = engine_steps(x, nei, k, starts, steps, dict(env or {}), **cfg)
    for other in others:
        ref, _ = engine_steps(x, nei, k, starts, steps, dict(env or {}, **other), **cfg)
        assert len(ref) == len(got)
        for j, (a, b) in enumerate(zip(ref, got)):
            assert_same(a, b, "%s step %d" % (sorted(other), j))
    return got, counters


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype).tobytes()


def same_as_oracle(got, want):
    """labels, centres, epsilon, pi, class sizes and logpkfki: the oracle's bits"""
    assert got["status"] == want["status"] and got["iters"] == want["iters"], (got["status"], want["status"], got["iters"], want["iters"])
    assert got["converged"] == want["converged"]
    if want["status"] == 2:
        assert got["emptyk"] == want["emptyk"]
    assert got["n_zero_density"] == want["n_zero_density"]
    assert np.array_equal(got["c"], want["c"])
    assert np.array_equal(got["labels"], want["c"].argmax(1))
    for key in ("center", "disp", "prop", "nbobs_k"):
        assert bits(got[key], np.float32) == bits(want[key], np.float32), (key, got[key], want[key])
    if want["status"] == 0:                           # (a run that ends on an empty class ends inside its M-step)
        assert bits(got["logpkfki"], np.float32) == bits(want["logpkfki"], np.float32)


def held(oracle, x, nei, k, start, others=(UNFUSED,), env=None, **cfg):
    """a whole run: every path the same, and the oracle's answer"""
    got = paths_agree(x, nei, k, [start], others=others, env=env, **cfg)[0][0]
    want = oracle.run(x, nei, k, *start, **cfg)
    same_as_oracle(got, want)
    return got, want


@pytest.mark.parametrize("d", DS)
def test_shapes(oracle, d):
    """every N by this D; K = 2 ... 5 and the two dispersion models go round over the shapes"""
    for j, n in enumerate(NS):
        x, _ = synth.grouped_pa_matrix(n, d, 1000 * n + d, groups=10)
        nei = synth.contiguity_graph(n, 7, d=d) if n > 1 else None
        k = 2 + (j + DS.index(d)) % 4
        disper = ("sk_", "skd")[(j + DS.index(d) // 4) % 2]
        held(oracle, x, nei, k, synth.kclass_init(x, k), **dict(CFG, disper=disper, seed=4))
        if n in (65, 300):
            held(oracle, x, nei, 3, synth.default_init(d), **CFG)


@pytest.mark.parametrize("k", [2, 3, 4, 5])
@pytest.mark.parametrize("disper", ["sk_", "skd"])
def test_class_counts_and_models(oracle, k, disper):
    """every K under both models at two shapes, against all three other paths"""
    for n, d in ((300, 33), (257, 500)):
        x, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
        held(oracle, x, synth.contiguity_graph(n, 4, d=d), k, synth.kclass_init(x, k), others=(UNFUSED, WORD, STEPPED),
             **dict(CFG, disper=disper, seed=4))


def two_camps(n0, n1, d, ones_in_camp0, seed):
    """n0 families that are mostly absent and n1 that are present everywhere; in camp 0 organism j is present in exactly
    ones_in_camp0[j] families (the other organisms in none).  Started from centres 0 / 1 the camps are the classes in
    every iteration: class 0 has n0 families and its zero count at organism j is n0 - ones_in_camp0[j]."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n0 + n1, d), np.uint8)
    x[n0:] = 1
    for j, c in ones_in_camp0.items():
        x[rng.permutation(n0)[:c], j] = 1
    order = rng.permutation(n0 + n1)
    x = x[order]
    camp0 = order < n0                                # family i lies in camp 0
    prop = np.array([0.5, 0.5], np.float32)
    center = np.stack([np.zeros(d, np.float32), np.ones(d, np.float32)])
    disp = np.full((2, d), 0.2, np.float32)
    return x, camp0, (prop, center, disp)


@pytest.mark.parametrize("disper", ["sk_", "skd"])
@pytest.mark.parametrize("n0,d", [(20, 40), (150, 300), (21, 40)])
def test_zero_counts_at_and_beside_the_tie(oracle, disper, n0, d):
    """class 0 has n0 families; organisms 0, 1, 2 (and 33, 34, 35 in the next mask word) are present in n0 / 2 - 1,
    n0 / 2 and n0 / 2 + 1 of them: with n0 even the middle one ties (centre 1/2, no mask bit), with n0 odd none does"""
    h = n0 // 2
    ones = {0: h - 1, 1: h, 2: h + 1, 33: h + 1, 34: h, 35: h - 1}
    x, camp0, start = two_camps(n0, 30, d, ones, n0 + d)
    nei = synth.contiguity_graph(n0 + 30, 5, d=d)
    got, want = held(oracle, x, nei, 2, start, others=(UNFUSED, WORD), **dict(CFG, disper=disper, beta=0.0))
    assert np.array_equal(want["c"].argmax(1) == 0, camp0) and want["nbobs_k"][0] == n0
    c0 = want["center"][0]
    if n0 % 2 == 0:
        assert c0[[0, 1, 2, 33, 34, 35]].tolist() == [0.0, 0.5, 1.0, 1.0, 0.5, 0.0]
    else:                                             # zero counts n0 - h + 1, n0 - h, n0 - h - 1 against n0 / 2 = h + 1/2
        assert c0[[0, 1, 2, 33, 34, 35]].tolist() == [0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    assert np.count_nonzero(c0) == (4 if n0 % 2 == 0 else 2)


@pytest.mark.parametrize("disper", ["sk_", "skd"])
def test_class_of_one_family(oracle, disper):
    """one family alone in its class: its inertia is zero, the class's dispersion is at or below EPSILON (null
    densities, the general chain)"""
    for n, d in ((65, 33), (300, 257)):
        x, camp0, start = two_camps(n - 1, 1, d, {0: (n - 1) // 3, d - 1: 2}, n)
        got, want = held(oracle, x, synth.contiguity_graph(n, 3, d=d), 2, start, others=(UNFUSED, WORD), **dict(CFG, disper=disper, beta=0.0))
        assert want["nbobs_k"].tolist() == [n - 1, 1]
        assert (want["disp"][1] == 0).all()


def test_class_that_empties(oracle):
    """three classes started on two camps: the class in between takes no family, keeps its centres and its
    per-organism dispersions, and the run ends as the oracle's does"""
    n0, d = 40, 65
    x, _, (_, center, _) = two_camps(n0, 30, d, {0: 3, 40: 5}, 9)
    prop = np.array([0.4, 0.2, 0.4], np.float32)
    rng = np.random.default_rng(9)
    center3 = np.stack([center[0], (rng.random(d) < 0.5).astype(np.float32), center[1]])
    disp3 = np.stack([np.full(d, 0.2, np.float32), rng.uniform(0.3, 0.45, d).astype(np.float32), np.full(d, 0.2, np.float32)])
    nei = synth.contiguity_graph(n0 + 30, 9, d=d)
    for disper in ("sk_", "skd"):
        got, want = held(oracle, x, nei, 3, (prop, center3, disp3), others=(UNFUSED, WORD), **dict(CFG, disper=disper))
        assert want["status"] == 2 and want["emptyk"] == 2 and want["nbobs_k"][1] == 0
        assert bits(got["center"][1], np.float32) == bits(center3[1], np.float32)
        assert bits(got["disp"][1], np.float32) == bits(disp3[1], np.float32)


@pytest.mark.parametrize("eps", [0.5, 0.45, 1e-3, 0.7])
def test_given_dispersions(oracle, eps):
    """the start's density from a given epsilon: 0.5 (l1 = 0), 0.45, 1e-3 (large l1), 0.7 (l1 < 0: the stepped chain) --
    the densities of the given parameters are the oracle's, then a run of one iteration and one of three"""
    for n, d in ((257, 65), (300, 500)):
        x, _ = synth.ushaped_pa_matrix(n, d, 11)
        nei = synth.contiguity_graph(n, 11, d=d)
        prop, center, _ = synth.default_init(d)
        start = (prop, center, np.full((3, d), eps, np.float32))
        first, _ = paths_agree(x, nei, 3, [start], steps=restarts(0), others=(UNFUSED, WORD), **CFG)
        _, lp, _ = oracle.density(x, *start)          # (pkfki goes through exp: the device's and the host's differ in a last bit)
        assert bits(first[0]["logpkfki"], np.float32) == bits(lp, np.float32)
        for it_max in (1, 3):
            held(oracle, x, nei, 3, start, others=(UNFUSED, WORD), **dict(CFG, it_max=it_max))


def test_dispersion_at_or_below_epsilon(oracle):
    """given dispersions of zero and of 1e-30 in some organisms of a class (the general chain, null densities)"""
    n, d = 300, 65
    x, _ = synth.ushaped_pa_matrix(n, d, 12)
    nei = synth.contiguity_graph(n, 12, d=d)
    prop, center, disp = synth.default_init(d)
    disp = disp.copy()
    disp[0, :5] = 0.0
    disp[2, 40] = 1e-30
    for disper in ("sk_", "skd"):
        held(oracle, x, nei, 3, (prop, center, disp), others=(UNFUSED, WORD), **dict(CFG, disper=disper))
    held(oracle, x, nei, 3, (prop, center, np.full((3, d), 1e-30, np.float32)), others=(UNFUSED,), **dict(CFG, it_max=1))


def test_given_centres_outside_zero_half_one(oracle):
    n, d = 257, 257
    x, _ = synth.ushaped_pa_matrix(n, d, 13)
    nei = synth.contiguity_graph(n, 13, d=d)
    prop, _, disp = synth.default_init(d)
    rng = np.random.default_rng(13)
    center = rng.uniform(0.0, 1.0, (3, d)).astype(np.float32)
    center[1, ::7] = 0.5
    center[2, 3] = 2.5                                # (abs((int)(x - mu)) above 1)
    for disper in ("sk_", "skd"):
        for it_max in (1, 3):
            held(oracle, x, nei, 3, (prop, center, disp), others=(UNFUSED, WORD), **dict(CFG, disper=disper, it_max=it_max))


def test_run_that_stops_at_its_first_iteration(oracle):
    """cvtest = clas on data whose labels do not move after the start, and it_max = 1"""
    x, camp0, start = two_camps(200, 100, 64, {0: 100, 1: 99, 2: 101}, 14)
    nei = synth.contiguity_graph(300, 14, d=64)
    got, want = held(oracle, x, nei, 2, start, others=(UNFUSED, WORD), **dict(CFG, cvtest="clas", cvthres=1e-8, it_max=100))
    assert want["converged"] and want["iters"] <= 2
    held(oracle, x, nei, 2, start, others=(UNFUSED, WORD), **dict(CFG, it_max=1))


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_five_restarts_on_one_engine(oracle, graphs):
    """five different starts on one engine, restart_iterate(1), (0) and (7) each; the whole runs of the first and the
    last start are the oracle's"""
    n, d = 300, 500
    x, _ = synth.ushaped_pa_matrix(n, d, 15)
    nei = synth.contiguity_graph(n, 15, d=d)
    prop, center, disp = synth.default_init(d)
    rng = np.random.default_rng(15)
    starts = [(prop, center, disp),
              (prop, (rng.random((3, d)) < 0.5).astype(np.float32), disp),
              (prop, center, rng.uniform(0.05, 0.45, (3, d)).astype(np.float32)),
              (np.array([0.2, 0.5, 0.3], np.float32), center, np.repeat(rng.uniform(0.05, 0.45, (3, 1)), d, axis=1).astype(np.float32)),
              (prop, rng.uniform(0, 1, (3, d)).astype(np.float32), disp)]
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else {}
    cfg = dict(CFG, cvtest="clas", cvthres=1e-8, it_max=100)
    _, counters = paths_agree(x, nei, 3, starts, steps=restarts(1, 0, 7), others=(UNFUSED,), env=env, **cfg)
    assert (counters["replayed"] > 0) == (graphs == "graphs")
    got, _ = engine_steps(x, nei, 3, starts, [run], env, **cfg)
    for j in (0, 4):
        same_as_oracle(got[j], oracle.run(x, nei, 3, *starts[j], **cfg))


def test_lock_step_batch_of_three_sizes(oracle):
    """three problems of different sizes solved in lock step: each the problem's own answer and the oracle's"""
    from pangenomenem_amd.batch import solve_many
    from pangenomenem_amd.engine import solve
    probs = []
    for p, (n, d) in enumerate(((300, 500), (257, 65), (63, 33))):
        x, _ = synth.grouped_pa_matrix(n, d, 16 + p, groups=10)
        probs.append((x, synth.contiguity_graph(n, 16 + p, d=d), 3) + tuple(synth.kclass_init(x, 3)))
    for disper in ("sk_", "skd"):
        cfg = dict(algo="ncem", beta=0.5, disper=disper, tie="hash", seed=6, it_max=5)
        batch = solve_many(probs, workers=1, group=3, **cfg)
        for got, p in zip(batch, probs):
            alone = solve(*p, **cfg)
            want = oracle.run(*p, **cfg)
            assert got["iters"] == alone["iters"] == want["iters"] and got["status"] == alone["status"] == want["status"]
            for key in ("c", "prop", "center", "disp", "nbobs_k"):
                assert bits(got[key], np.float32) == bits(alone[key], np.float32) == bits(want[key], np.float32), key
