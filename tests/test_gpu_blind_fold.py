"""The blind sweep inside the start's first relaxation round (nem_engine.hip enqueue_init, sweep_body's BLIND instances;
NEM_MI355X_BLIND_FOLD, default on) against the path it replaces -- the blind beta = 0 sweep as a launch of its own.
restart_iterate(m) for m = 0, 1, 3 with the switch on and off: labels, parameters, the stored densities, class sizes
and the result's counters (iterations, relaxation rounds, zero-density sites and the first of them, status) equal bit
for bit; blind_folds() says which path ran.  Three cases also against the oracle, so that both paths wrong alike cannot
pass.  Shapes: one to three blocks of 256 sites, neighbours on every side of a block edge, rows longer than the four a
lane keeps in registers, and both sides of the gate (128 blocks)."""
import ctypes as C
import os

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.engine import ALGO
from tests.util import maxdiff

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

SWITCH = "NEM_MI355X_BLIND_FOLD"
OFF, ON = 0, 1
SKIP_KEYS = {"loop_seconds"}
CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, tie="hash", seed=1)


def make_engine(setting, n, d, k, x, nei, env=None):
    from pangenomenem_amd.engine import NemEngine
    env = dict(env or {})
    env[SWITCH] = str(setting)
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
    eng.set_matrix(x)
    if nei is not None:
        eng.set_graph(nei)
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
    """one engine through every start in `starts` ((prop, center, disp) each), restart_iterate(m) for every m; returns
    the snapshots, the graph counters and the number of starts that went out with the fold"""
    eng = make_engine(setting, n, d, k, x, nei, env=env)
    out = []
    try:
        for prop, center, disp in starts:
            eng.set_params(prop, center, disp)
            eng.configure(**dict(CFG, **cfg))
            for m in ms:
                out.append(snapshot(eng, eng.restart_iterate(m)))
        counters = eng.graph_counters()
        folds = eng.blind_folds()
    finally:
        eng.close()
    return out, counters, folds


def on_against_off(n, d, k, x, nei, starts, ms=(0, 1, 3), env=None, folded=True, **cfg):
    """both settings agree bit for bit; the switch off never folds, the switch on folds every start (folded) or none"""
    ref, counters_off, folds_off = run_starts(OFF, n, d, k, x, nei, starts, ms, env, **cfg)
    got, counters, folds = run_starts(ON, n, d, k, x, nei, starts, ms, env, **cfg)
    assert folds_off == 0
    assert folds == (len(starts) * len(ms) if folded else 0), folds
    assert len(got) == len(ref)
    for j, (a, b) in enumerate(zip(ref, got)):
        assert_same(a, b, "step %d" % j)
    assert counters["host_finished_sweeps"] == counters_off["host_finished_sweeps"]
    return got, counters


def same_as_oracle(got, want):
    assert want["status"] == got["status"] and want["iters"] == got["iters"], (got["iters"], want["iters"])
    assert np.array_equal(want["c"], got["c"])
    assert np.array_equal(want["center"], got["center"])
    assert maxdiff(want["disp"], got["disp"]) <= 1e-6 and maxdiff(want["prop"], got["prop"]) <= 1e-6
    assert want["n_zero_density"] == got["n_zero_density"]


def csr(n, edges, seed):
    """undirected edges {(i, j, w)} listed from both endpoints; every row's order shuffled, so that the neighbours a lane
    keeps in registers (a row's first four) and those it walks from memory mix the three kinds"""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(n)]
    for i, j, w in sorted(edges):
        rows[i].append((j, w)); rows[j].append((i, w))
    ptr = np.zeros(n + 1, np.int32); idx = []; ws = []
    for i, row in enumerate(rows):
        for t in rng.permutation(len(row)):
            idx.append(row[t][0]); ws.append(row[t][1])
        ptr[i + 1] = len(idx)
    return ptr, np.asarray(idx, np.int32), np.asarray(ws, np.float32)


def fold_graph(n=600):
    """three blocks (256, 256, 88 sites): the path, chords to lower and to higher blocks, site 130 with neighbours in the
    other two blocks only, rows of 5 (site 280) and 9 (site 260) neighbours that lie below the site in its block, at or
    above it in its block and in both other blocks, and isolated sites (50, 333, 599)"""
    rng = np.random.default_rng(17)
    isolated = {50, 333, 599}
    edges = {}
    def link(i, j):
        if i != j and i not in isolated and j not in isolated:
            edges[(min(i, j), max(i, j))] = float(rng.integers(1, 4))
    for i in range(n - 1):
        if 130 not in (i, i + 1):
            link(i, i + 1)
    for i, j in [(10, 300), (270, 20), (520, 100), (255, 511), (0, 598), (256, 512), (511, 257), (200, 203), (400, 397)]:
        link(i, j)
    link(130, 400); link(130, 590)
    for j in (5, 100, 257, 258, 300, 301, 550):      # 260: + the path's 259 and 261 = 9
        link(260, j)
    for j in (3, 597, 270):                          # 280: + the path's 279 and 281 = 5
        link(280, j)
    nei = csr(n, {(i, j, w) for (i, j), w in edges.items()}, 18)
    deg = np.diff(nei[0])
    assert deg[260] == 9 and deg[280] == 5 and all(deg[i] == 0 for i in isolated)
    assert all(not 0 <= j < 256 for j in nei[1][nei[0][130]:nei[0][131]])
    return nei


@pytest.mark.parametrize("n", [1, 2, 63, 65, 255, 256, 257, 300, 513])
def test_block_edges(n):
    """N: one to three blocks, a last wave partly or wholly past the labels, a last block of one site; D on either side
    of a mask word.  (A problem without a graph -- N = 1 -- keeps the blind launch.)"""
    for d in (33, 64):
        x, _ = synth.grouped_pa_matrix(n, d, 1000 * n + d, groups=10)
        nei = synth.contiguity_graph(n, 7, d=d) if n > 1 else None
        for k in (2, 3, 4, 5):
            start = synth.kclass_init(x, k)
            for disper in ("sk_", "skd"):
                on_against_off(n, d, k, x, nei, [start], folded=n > 1, disper=disper, seed=4)


def test_graph_made_for_the_fold():
    n, d = 600, 40
    x, _ = synth.ushaped_pa_matrix(n, d, 6)
    nei = fold_graph(n)
    for beta in (0.5, 1.0):
        on_against_off(n, d, 3, x, nei, [synth.default_init(d)], beta=beta)
    xk, _ = synth.grouped_pa_matrix(n, d, 5, groups=10)
    for k in (2, 5, 7):
        on_against_off(n, d, k, xk, nei, [synth.kclass_init(xk, k)], beta=0.7)


@pytest.mark.parametrize("tie", ["hash", "first"])
def test_ties_in_the_blind_labels(tie):
    """two classes with identical parameters: every site ties between classes 0 and 1 in the blind sweep, on both sides
    of the block boundaries (the path links 255 - 256 and 511 - 512; chords link tied sites of different blocks)"""
    n, d = 600, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 8)
    prop, center, disp = synth.default_init(d)
    prop = np.array([0.3, 0.3, 0.4], np.float32)
    center = center.copy(); disp = disp.copy()
    center[1] = center[0]; disp[1] = disp[0]
    for nei in (synth.contiguity_graph(n, 8, d=d), fold_graph(n)):
        on_against_off(n, d, 3, x, nei, [(prop, center, disp)], tie=tie, seed=8)


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


def test_zero_densities_in_the_blind_sweep(oracle):
    """dispersions at and below EPSILON (null densities) and small enough for exp to underflow, as in
    tests/test_gpu_start.py; then a problem whose every site has zero density in every sweep, also against the oracle"""
    n, d = 700, 300
    x, _ = synth.ushaped_pa_matrix(n, d, 9)
    nei = synth.contiguity_graph(n, 9, d=d)
    prop, center, disp = synth.default_init(d)
    center = center.copy()
    center[1] = (np.random.default_rng(9).random(d) < 0.5).astype(np.float32)
    tiny = np.full((3, d), 1e-30, np.float32)
    small = np.full((3, d), 1e-9, np.float32)
    zero_one = disp.copy(); zero_one[0, :5] = 0.0
    out, _ = on_against_off(n, d, 3, x, nei, [(prop, center, tiny), (prop, center, small), (prop, center, zero_one)], ms=(0, 1))
    assert any(o["n_zero_density"] > 0 for o in out)
    n = 300
    x, nei, start = zero_density_problem(n)
    out, _ = on_against_off(n, 1024, 2, x, nei, [start], ms=(0, 2), cvtest="none")
    assert out[0]["n_zero_density"] == 2 * n and out[0]["first_zero_density_site"] == out[1]["first_zero_density_site"]
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", it_max=2, tie="hash", seed=1)
    want = oracle.run(x, nei, 2, *start, **cfg)
    same_as_oracle(out[1], want)


def domino_chains(n, seg, w):
    """chains of `seg` sites: every site but a chain's head has one neighbour, the site before it, at a weight that
    outvotes the data -- a sweep hands the head's label down the chain, and a round takes it 64 sites far"""
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(np.arange(n) % seg != 0)
    idx = (np.arange(n, dtype=np.int32) - 1)[np.arange(n) % seg != 0]
    return ptr, idx, np.full(idx.size, w, np.float32)


@pytest.mark.parametrize("seg,seed", [(500, 3), (250, 5)])
def test_start_whose_sweep_the_host_finishes(seg, seed):
    """the start's beta sweep needs more rounds than were enqueued: the host goes on from the blind labels in buffer 1,
    which the fused round wrote"""
    n, d = 2000, 200
    x, _ = synth.ushaped_pa_matrix(n, d, seed)
    _, counters = on_against_off(n, d, 3, x, domino_chains(n, seg, 1200.0), [synth.default_init(d)], cvtest="none", seed=3)
    assert counters["host_finished_sweeps"] > 0


def test_every_row_normalised():
    """NEM_MI355X_MAP_MARGIN=0: the blind labels, too, come from the normalised row"""
    n, d = 600, 64
    x, _ = synth.ushaped_pa_matrix(n, d, 21)
    on_against_off(n, d, 3, x, fold_graph(n), [synth.default_init(d)], env={"NEM_MI355X_MAP_MARGIN": "0"})


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_five_different_starts_on_one_engine(graphs):
    n, d = 1000, 120
    x, _ = synth.ushaped_pa_matrix(n, d, 11)
    nei = synth.contiguity_graph(n, 11, d=d)
    prop, center, disp = synth.default_init(d)
    rng = np.random.default_rng(4)
    starts = [(prop, center, disp),
              (prop, (rng.random((3, d)) < 0.5).astype(np.float32), disp),
              (prop, center, rng.uniform(0.05, 0.45, (3, d)).astype(np.float32)),
              (np.array([0.2, 0.5, 0.3], np.float32), center, np.repeat(rng.uniform(0.05, 0.45, (3, 1)), d, axis=1).astype(np.float32)),
              (prop, center, disp)]
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else None
    _, counters = on_against_off(n, d, 3, x, nei, starts, ms=(1, 0, 7), env=env)
    assert (counters["replayed"] > 0) == (graphs == "graphs")


@pytest.mark.parametrize("n", [32768, 32769])
def test_either_side_of_the_gate(n):
    """128 blocks: the last grid that folds; 129: the first that keeps the blind launch"""
    d = 33
    x, _ = synth.ushaped_pa_matrix(n, d, 7)
    on_against_off(n, d, 3, x, synth.contiguity_graph(n, 7, d=d), [synth.default_init(d)], folded=n <= 32768)


@pytest.mark.parametrize("what", ["libc", "fuzzy", "wide", "no_graph", "beta0", "k8"])
def test_engines_that_do_not_qualify_keep_the_blind_launch(what):
    """TIE_LIBC, fuzzy NEM, D above the fused density kernel's cap, no neighbourhood, beta = 0, K = 8: no start folds"""
    n, d, k = (600, 1056, 3) if what == "wide" else (1000, 60, 8 if what == "k8" else 3)
    x, _ = synth.grouped_pa_matrix(n, d, 12, groups=10)
    nei = synth.contiguity_graph(n, 12, d=d)
    start = synth.kclass_init(x, k) if what == "k8" else synth.default_init(d)
    cfg = {}
    if what == "libc":
        cfg = dict(tie="libc")
    if what == "fuzzy":
        cfg = dict(algo="nem")
    if what == "beta0":
        cfg = dict(beta=0.0)
    if what == "no_graph":
        nei = None
    on_against_off(n, d, k, x, nei, [start], folded=False, **cfg)


def test_configs1_shape():
    """the bench's shape and start"""
    n, d = 20000, 500
    x, _ = synth.ushaped_pa_matrix(n, d, 3)
    nei = synth.contiguity_graph(n, 3, d=d)
    out, _ = on_against_off(n, d, 3, x, nei, [synth.default_init(d)], ms=(0, 1, 7))
    assert out[2]["iters"] == 7


@pytest.mark.parametrize("case", ["fold_graph", "three_blocks"])
def test_against_the_oracle(oracle, case):
    if case == "fold_graph":
        n, d = 600, 40
        x, _ = synth.ushaped_pa_matrix(n, d, 6)
        nei = fold_graph(n)
    else:
        n, d = 513, 77
        x, _ = synth.ushaped_pa_matrix(n, d, 13)
        nei = synth.contiguity_graph(n, 13, d=d)
    prop, center, disp = synth.default_init(d)
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", it_max=3, tie="hash", seed=5)
    want = oracle.run(x, nei, 3, prop, center, disp, **cfg)
    eng = make_engine(ON, n, d, 3, x, nei)
    try:
        eng.set_params(prop, center, disp)
        eng.configure(**cfg)
        got = eng.restart_iterate(3)
        got.update(eng.results())
        assert eng.blind_folds() == 1
    finally:
        eng.close()
    same_as_oracle(got, want)
