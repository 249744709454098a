"""The member lists of the lock-step fuzz (tests/test_gpu_lockstep_fuzz.py), the library's launch arithmetic restated
for tests/test_lockstep_fuzz_host.py, and the two comparisons every member gets: against the oracle by the rules of
tests/test_gpu_fuzz.py::test_random_problem, and against its own solo run bit for bit (include/nem_mi355x.h).

A member is (x, nei, k, prop, center, disp, cfg), what tests/fuzz_problems.random_problem returns.  The lists (b) to (d)
exist as specs first -- sizes and configuration, no arrays -- so that the host test can do its arithmetic on them
without building a 100 003-family matrix."""
import ctypes as C

import numpy as np

from tests.fuzz_problems import random_problem
from tests.util import maxdiff

TOL = 1e-6                        # the project's bar (BASELINE.json), TOL of tests/test_gpu_fuzz.py
SOLO_KEYS = ("c", "center", "disp", "prop", "nbobs_k", "crit")

# ---- the library's arithmetic, restated ---------------------------------------------------------------------------
K_TEMPLATE_MAX = 10               # nem_sweep.hip, sweep_variant   K >= 1 && K <= 10 ? K : 0 (the generic instance)
BIG_SITES = 65536                 # nem_sweep.hip, sweep_block_sites   big = n_local >= 65536 && !generic
FUSED_MAX_D = 1024                # nem_kernels.hpp    kFusedMaxD
FF_MIN_D = 256                    # nem_engine.hip     use_ff(): ff_mode < 0 ? d >= 256
WIDE_COUNTS_D = 1023              # nem_kernels.hip    launch_mstep_counts: wide = D + 1 >= 1024
SWEEP_MODES = ("nem", "ncem", "ncem_libc")


def sweep_template_k(k):
    """nem_sweep.hip, sweep_variant: the K a round's kernel is compiled for, 0 = the generic instance"""
    return k if 1 <= k <= K_TEMPLATE_MAX else 0


def sweep_block_sites(n, k):
    """nem_sweep.hip, sweep_block_sites: (big, sites per block = threads per block)"""
    generic = not (1 <= k <= K_TEMPLATE_MAX)
    big = n >= BIG_SITES and not generic
    bs = 256
    if big:
        waves_of_blocks = (n + 256 * 1024 - 1) // (256 * 1024)
        per_block = (n + 256 * waves_of_blocks - 1) // (256 * waves_of_blocks)
        bs = min(1024, max(256, (per_block + 63) // 64 * 64))
    return big, bs


def sweep_mode(cfg):
    """nem_sweep.hip, sweep_variant: ncem, and libc only with ncem (the fuzzy round draws nothing)"""
    if cfg["algo"] != "ncem":
        return "nem"
    return "ncem_libc" if cfg["tie"] == "libc" else "ncem"


def sweep_instance(n, k, cfg):
    """(template K, mode, block class) of the k_sweep_b instance a member's rounds run: block class 1024 is the
    __launch_bounds__(1024) instance `big` selects (nem_sweep.hip, sweep_dispatch), launched with sweep_block_sites' threads"""
    big, _ = sweep_block_sites(n, k)
    return sweep_template_k(k), sweep_mode(cfg), 1024 if big else 256


def all_sweep_instances():
    """the instantiations of k_sweep_b that sweep_dispatch launches (nem_sweep.hip): K 0..10 x three modes at 256,
    K 1..10 x three at 1024 -- 63, the generic instance has no large-block form"""
    out = {(kt, m, 256) for kt in range(0, K_TEMPLATE_MAX + 1) for m in SWEEP_MODES}
    out |= {(kt, m, 1024) for kt in range(1, K_TEMPLATE_MAX + 1) for m in SWEEP_MODES}
    return out


def fused_update(d, disper):
    """nem_engine.hip, nemgpu_engine::fused_update()"""
    return d <= FUSED_MAX_D and disper in ("sk_", "skd")


def use_ff(d):
    """nem_engine.hip, nemgpu_engine::use_ff() in its automatic mode"""
    return d >= FF_MIN_D


def density_class(d, disper):
    if not fused_update(d, disper):
        return "non-fused"
    return "fused fast-forward" if use_ff(d) else "fused plain"


def finish_separable(disper):
    """nem_kernels.hip, launch_finish: OP_FINISH variant 1 (one block per class) for sk_ / skd, 0 for s__ / s_d"""
    return disper in ("sk_", "skd")


def wide_counts(d):
    """nem_kernels.hip, launch_mstep_counts: k_mstep_counts_b<4> against <1>"""
    return d >= WIDE_COUNTS_D


# ---- (a) random heterogeneous groups ------------------------------------------------------------------------------
FUZZ_GROUPS, FUZZ_GROUP_SIZE, FUZZ_SEED0 = 10, 8, 5000


def fuzz_group(g):
    return [random_problem(FUZZ_SEED0 + FUZZ_GROUP_SIZE * g + j) for j in range(FUZZ_GROUP_SIZE)]


# ---- (b) every class count in one call ----------------------------------------------------------------------------
EVERY_K = list(range(1, 13)) + [17, 32]
SWEEP_CASES = [("ncem", "hash"), ("ncem", "first"), ("ncem", "libc"), ("nem", "hash")]


def every_k_specs(algo, tie):
    """K = 1..12, 17, 32 on 20 latent groups, 300 to 1 496 families (2 to 6 blocks of 256 sites), 24 organisms"""
    return [dict(n=300 + 92 * j, d=24, k=k, groups=20, seed=100 + j,
                 cfg=dict(algo=algo, beta=0.5, disper=("sk_", "skd")[j % 2], propor="pk", it_max=4 if algo == "nem" else 6,
                          tie=tie, seed=7))
            for j, k in enumerate(EVERY_K)]


# ---- (c) the 1024-site twins --------------------------------------------------------------------------------------
BIG_CASES = [("ncem", "hash"), ("ncem", "libc"), ("nem", "hash")]
BIG_SMALL_MEMBER = 10             # its place in the list


def big_specs(algo, tie):
    """K = 1..10, odd K at 65 536 families (256 blocks of 256 sites), even K at 100 003 (224 blocks of 448, the last
    one 99 sites), and a member of 200 families (one block, the 256-site instance: a second sequence group)"""
    cfg = dict(algo=algo, beta=0.5, disper="sk_", propor="pk", it_max=2, tie=tie, seed=11)
    out = [dict(n=65536 if k % 2 else 100003, d=12, k=k, groups=10, seed=200 + k, cfg=dict(cfg)) for k in range(1, 11)]
    out.append(dict(n=200, d=12, k=3, groups=10, seed=211, cfg=dict(cfg)))
    return out


# ---- (d) every density and parameter-update path ------------------------------------------------------------------
DENSITY_D = (255, 256, 1024, 1025)
DENSITY_DISPER = ("sk_", "skd", "s__", "s_d")
DENSITY_CASES = ["ncem", "nem"]


def density_specs(algo):
    """d x dispersion model, K alternating so that every d and every model meets K = 3 and K = 4, 600 to 705 families"""
    out = []
    for a, d in enumerate(DENSITY_D):
        for b, disper in enumerate(DENSITY_DISPER):
            j = 4 * a + b
            out.append(dict(n=600 + 7 * j, d=d, k=3 + (a + b) % 2, groups=4, seed=300 + j,
                            cfg=dict(algo=algo, beta=0.5, disper=disper, propor="pk", it_max=4, tie="hash", seed=13)))
    return out


def build_member(spec):
    from pangenomenem_amd import synth
    x, _ = synth.grouped_pa_matrix(spec["n"], spec["d"], spec["seed"], groups=spec["groups"])
    nei = synth.contiguity_graph(spec["n"], spec["seed"])
    prop, center, disp = synth.kclass_init(x, spec["k"])
    return x, nei, spec["k"], prop, center, disp, dict(spec["cfg"])


# ---- (e) the problems of (a) through solve_many -------------------------------------------------------------------
CONFIG_KEY = ("algo", "disper", "propor", "tie")
SOLVE_GROUPS, SOLVE_WORKERS = (1, 3, 32), (1, 4)


def solve_many_calls():
    """The 80 problems of (a) dealt to four calls' worth of one configuration each.  A configuration is what selects
    kernels: (algo, disper, propor, tie).  The four that most problems were drawn with keep their problems; every other
    problem goes to one of the four in turn, its fields overridden.  beta, it_max, param_fix and seed are per call too
    (nemgpu_solve_many takes one configuration): those of the configuration's first problem that runs at least three
    iterations unfixed, so that no call is an it_max = 0 call.  (Equal counts: in the order of the key.)
    The four hold no NCEM configuration under the reference's tie stream, whose two initial sweeps are lock-step steps of
    their own (iterate_many, libc_init_a / _b / _c) and carry the builders' pending layouts.  So there is a fifth: the
    most frequent (ncem, libc) configuration, given every problem that was drawn with tie = libc, a second time.
    Returns [(cfg, [problem, ...]), ...], a problem being (x, nei, k, prop, center, disp)."""
    probs = [p for g in range(FUZZ_GROUPS) for p in fuzz_group(g)]
    key = lambda cfg: tuple(cfg[f] for f in CONFIG_KEY)
    count = {}
    for p in probs:
        count[key(p[6])] = count.get(key(p[6]), 0) + 1
    ranked = sorted(count, key=lambda c: (-count[c], c))
    top = ranked[:4]
    extra = next(c for c in ranked if c[0] == "ncem" and c[3] == "libc")
    calls = []
    for c in top + [extra]:
        own = [p[6] for p in probs if key(p[6]) == c]
        lead = next((f for f in own if f["it_max"] >= 3 and not f["param_fix"]), own[0])
        calls.append((dict(lead), []))
    turn = 0
    for p in probs:
        if key(p[6]) in top:
            slot = top.index(key(p[6]))
        else:
            slot = turn % 4
            turn += 1
        calls[slot][1].append(p[:6])
        if p[6]["tie"] == "libc":
            calls[4][1].append(p[:6])
    return calls


def as_bit_rows(x):
    b = np.packbits(x, axis=1, bitorder="little")
    b = np.pad(b, ((0, 0), (0, (-b.shape[1]) % 4)))
    return np.ascontiguousarray(b).view(np.uint32)


def solve_many_raw(problems, workers, group, **cfg):
    """nemgpu_solve_many as pangenomenem_amd.batch.solve_many calls it, but a failed call is not an exception here:
    returns (rc of the call, [rc of every problem], [results]).  That is the only way to see that the problems beside a
    wrong one were still answered."""
    from pangenomenem_amd.engine import ALGO, CVT, DISP, PROP, TIE, Config, Problem, load_library
    lib = load_library()
    full = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100, param_fix=False,
                tie="hash", seed=0)
    full.update(cfg)
    conf = Config(ALGO[full["algo"]], full["beta"], DISP[full["disper"]], PROP[full["propor"]], CVT[full["cvtest"]],
                  full["cvthres"], full["it_max"], int(full["param_fix"]), TIE[full["tie"]], full["seed"])
    arr = (Problem * len(problems))()
    keep, outs = [], []
    addr = lambda a: a.__array_interface__["data"][0]
    for q, (x, nei, k, prop, center, disp) in zip(arr, problems):
        bits = x.dtype == np.uint32
        x = np.ascontiguousarray(x, np.uint32 if bits else np.uint8)
        n = x.shape[0]
        d = np.asarray(center).size // int(k) if bits else x.shape[1]
        prop = np.ascontiguousarray(prop, np.float32)
        center = np.ascontiguousarray(center, np.float32).reshape(k, d)
        disp = np.ascontiguousarray(disp, np.float32).reshape(k, d)
        q.n, q.d, q.k = n, d, int(k)
        if bits:
            assert x.shape == (n, (d + 31) // 32)
            q.x_bits = addr(x)
        else:
            q.x_bytes = addr(x)
        keep += [x, prop, center, disp]
        if nei is not None:
            ptr, idx, w = (np.ascontiguousarray(nei[0], np.int32), np.ascontiguousarray(nei[1], np.int32),
                           np.ascontiguousarray(nei[2], np.float32))
            q.nei_ptr, q.nei_idx, q.nei_w = addr(ptr), addr(idx), addr(w)
            keep += [ptr, idx, w]
        q.prop, q.center, q.disp = addr(prop), addr(center), addr(disp)
        o = dict(prop=np.full(k, -9, np.float32), center=np.full((k, d), -9, np.float32), disp=np.full((k, d), -9, np.float32),
                 nbobs_k=np.full(k, -9, np.float32), c=np.full((n, k), -9, np.float32))
        q.out_prop, q.out_center, q.out_disp, q.out_nbobs_k, q.out_c = (addr(o[f]) for f in ("prop", "center", "disp", "nbobs_k", "c"))
        outs.append(o)
    rc = lib.nemgpu_solve_many(arr, len(problems), C.byref(conf), 0, int(workers), int(group))
    res = []
    for q, o in zip(arr, outs):
        r = q.result
        meta = dict(status=r.status, iters=r.iters, converged=bool(r.converged), emptyk=r.emptyk,
                    n_zero_density=r.zero_density_sites, crit=np.array(list(r.crit), np.float32), tie_draws=r.tie_draws)
        meta.update(o)
        res.append(meta)
    return rc, [int(q.rc) for q in arr], res


# ---- (f) random starts in lock step -------------------------------------------------------------------------------
STARTS_CASES = [(k, d, "ncem") for k in (2, 6, 11) for d in (20, 300)] + [(k, 20, "nem") for k in (2, 6, 11)]
STARTS = 6


def starts_spec(k, d):
    return dict(n=900 + k, d=d, k=k, groups=12, seed=400 + k)


# ---- the comparisons ----------------------------------------------------------------------------------------------
def assert_matches_oracle(got, want, cfg, ctx):
    """the rules of tests/test_gpu_fuzz.py::test_random_problem"""
    assert got["status"] == want["status"], ctx
    assert got["iters"] == want["iters"] and got["converged"] == want["converged"], ctx
    if want["status"] == 2:
        assert got["emptyk"] == want["emptyk"], ctx
    if np.isfinite(want["c"]).all():
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


def assert_same_run(got, solo, ctx):
    """the header's contract: a member's result is its solo nemgpu_run's, bit for bit"""
    for key in ("iters", "status", "tie_draws"):
        assert got[key] == solo[key], (key, got[key], solo[key], ctx)
    for key in SOLO_KEYS:
        assert np.array_equal(got[key], solo[key], equal_nan=True), (key, ctx)
