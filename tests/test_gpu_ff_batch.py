"""The fused density kernels' fast-forwarded chain with the lanes decoupled from the wave's word (chain_ff_batched in
nem_kernels.hip, NEM_MI355X_FF_BATCH, default on) against the word-synchronous chain it replaces (switch off) and against
the CPU oracle: labels, parameters, class sizes and the stored log densities logpkfki equal bit for bit -- the walk changes
which lanes share a crossing pass, never a value.  (pkfki = pk * exp(logfk) in double goes through the device's exp,
which is not the host libm's to the last bit: it is compared between the two chains, not with the oracle.)  The
fast-forward is forced on (NEM_MI355X_FF=1: by itself it starts at 256 organisms).  Shapes: a part-empty wave, tile and second tile; a second word of one organism, partial last
words, more than the four groups the head holds, the LDS row at its largest; 32 and 1056 organisms and a grid of more
than three blocks per compute unit, where the chain is the old one.  Parameters: every lane crossing together (epsilon 1/2), rare and frequent crossings, epsilon above 1/2 (the
plain chain), centres at 1/2.  Matrices: one dense row among empty ones, all ones, all zeros."""
import ctypes as C
import os

import numpy as np
import pytest

from pangenomenem_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]

CFG = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="none", tie="hash", seed=3)
BATCHED = {"NEM_MI355X_FF": "1", "NEM_MI355X_FF_BATCH": "1"}
WORD = {"NEM_MI355X_FF": "1", "NEM_MI355X_FF_BATCH": "0"}
KEYS = ("status", "iters", "c", "center", "nbobs_k", "disp", "prop", "logpkfki", "pkfki")
ORACLE_KEYS = KEYS[:-1]


def make_engine(env, x, nei, k):
    from pangenomenem_amd.engine import NemEngine
    saved = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                            # (read when the engine is created)
    try:
        eng = NemEngine(x.shape[0], x.shape[1], k)
    finally:
        for key, v in saved.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    eng.set_matrix(x); eng.set_graph(nei)
    return eng


def stored_density(eng):
    """the densities the last launch left (nemgpu_get_density only copies)"""
    pk = np.zeros((eng.n, eng.k), np.float64)
    lp = np.zeros((eng.n, eng.k), np.float32)
    eng._chk(eng.lib.nemgpu_get_density(eng._h, pk.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p)))
    return pk, lp


def engine_runs(env, x, nei, k, start, ms, **cfg):
    """one engine, restart_iterate(m) for every m: m = 0 leaves the start's densities (k_density_start) behind, m > 0 an
    iteration's (k_density_verify / k_density_fused)"""
    eng = make_engine(env, x, nei, k)
    out = []
    try:
        eng.set_params(*start)
        for m in ms:
            eng.configure(**dict(CFG, it_max=max(m, 1), **cfg))
            got = dict(eng.restart_iterate(m))
            got.update(eng.results())
            got["pkfki"], got["logpkfki"] = stored_density(eng)
            out.append(got)
    finally:
        eng.close()
    return out


def same_bits(a, b, keys, what):
    for key in keys:
        u, v = np.asarray(a[key]), np.asarray(b[key])
        assert u.shape == v.shape, (what, key)
        if u.tobytes() != v.tobytes():
            bad = np.flatnonzero(u.ravel() != v.ravel())
            print(what, key, "differs at", bad[:8], u.ravel()[bad[:8]], v.ravel()[bad[:8]])
        assert u.astype(v.dtype).tobytes() == v.tobytes(), (what, key)


def check(oracle, x, nei, k, start, ms=(0, 2), env=None, **cfg):
    env = dict(env or {})
    new = engine_runs(dict(BATCHED, **env), x, nei, k, start, ms, **cfg)
    old = engine_runs(dict(WORD, **env), x, nei, k, start, ms, **cfg)
    for m, a, b in zip(ms, new, old):
        what = "n %d d %d k %d m %d" % (x.shape[0], x.shape[1], k, m)
        same_bits(a, b, KEYS, what + " batched / word-synchronous")
        if m == 0:                                    # the start: the densities of the given parameters
            pk, lp, _ = oracle.density(x, *start)
            same_bits(a, dict(logpkfki=lp), ("logpkfki",), what + " batched / oracle")
        else:
            want = oracle.run(x, nei, k, *start, **dict(CFG, it_max=m, **cfg))
            # (a run that ends on an empty class ends inside its M-step: the reference computes no density behind it, the
            #  engine's launch already has -- the densities left behind are then compared between the two chains only)
            same_bits(a, want, ORACLE_KEYS if want["status"] == 0 else ORACLE_KEYS[:-1], what + " batched / oracle")
    return new


def problem(n, d, seed, low_disp=None):
    x, _ = synth.ushaped_pa_matrix(n, d, seed)
    nei = synth.contiguity_graph(n, 7) if n > 1 else None
    return x, nei, synth.default_init(d, low_disp=low_disp or (0.3 if d > 500 else 0.1))


@pytest.mark.parametrize("d", [33, 64, 65, 257, 500, 1023, 1024])
def test_shapes(oracle, d):
    for n in (1, 63, 65, 255, 257, 300):
        x, nei, start = problem(n, d, 1000 * n + d)
        check(oracle, x, nei, 3, start)


@pytest.mark.parametrize("d", [32, 1056])
def test_shapes_the_walk_does_not_reach(oracle, d):
    """one word (nothing to walk) and more organisms than the fused kernels take: the word-synchronous chain"""
    for n in (65, 300):
        x, nei, start = problem(n, d, 1000 * n + d)
        check(oracle, x, nei, 3, start)


def test_grid_the_device_does_not_hold_at_once(oracle):
    """more density blocks than three per compute unit: the launch takes no LDS rows and the chain is the old one"""
    n, d = 66000, 65
    x, nei, start = problem(n, d, 29)
    check(oracle, x, nei, 3, start, ms=(0, 1))


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_class_counts(oracle, k):
    n, d = 300, 257
    x, _ = synth.ushaped_pa_matrix(n, d, 5)
    check(oracle, x, synth.contiguity_graph(n, 4), k, synth.kclass_init(x, k))


@pytest.mark.parametrize("eps", [0.5, 0.45, 1e-3, 0.7])
def test_given_dispersions(oracle, eps):
    """1/2: no increment depends on the organism, so all lanes of a wave cross together and the threshold fires;
    0.45 / 1e-3: small and large mismatch increments; 0.7: log((1 - eps) / eps) < 0, the block takes chain_plain"""
    n, d = 300, 500
    x, nei, (prop, center, _) = problem(n, d, 17)
    check(oracle, x, nei, 3, (prop, center, np.full((3, d), eps, np.float32)), ms=(0, 1))


def test_centres_at_one_half(oracle):
    n, d = 300, 500
    x, nei, (prop, center, disp) = problem(n, d, 19)
    center = np.full_like(center, 0.5)
    check(oracle, x, nei, 3, (prop, center, disp), ms=(0, 1))


@pytest.mark.parametrize("what", ["one_dense_row", "ones", "zeros"])
def test_matrices(oracle, what):
    """one dense row among empty ones: against the centre-1 class one lane never mismatches while 63 cross at every
    step, against the centre-0 class 63 run on while one waits"""
    n, d = 300, 500
    x = np.zeros((n, d), np.uint8)
    if what == "one_dense_row":
        x[5] = 1
    elif what == "ones":
        x[:] = 1
    check(oracle, x, synth.contiguity_graph(n, 12), 3, synth.default_init(d), ms=(0, 1))


@pytest.mark.parametrize("graphs", ["graphs", "no_graphs"])
def test_with_graphs_and_without(oracle, graphs):
    n, d = 300, 500
    x, nei, start = problem(n, d, 23)
    env = {"NEM_MI355X_GRAPHS": "0"} if graphs == "no_graphs" else {}
    check(oracle, x, nei, 3, start, ms=(3, 3, 0, 3), env=env)


def test_one_engine_through_five_restarts(oracle):
    n, d = 300, 500
    x, nei, start = problem(n, d, 13)
    check(oracle, x, nei, 3, start, ms=(7, 1, 3, 2, 5))
