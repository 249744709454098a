"""The device chunk, vote and evolution paths (csrc/nem_chunks.hip, nem_vote.hip, nem_resample.hip and the lock-step
groups of solve_chunks_impl) at the shapes of real pangenomes, against the host recipe: a mostly-cloud master whose small
samples keep sparse families (k_chunk_rows' unstaged tiles), masters of 140 000 families (three k_chunk_index passes,
lock-step groups with members on both sides of 65 536 kept families, vote kernels over 547 blocks), masters at the
64-family and 32-organism word boundaries and one whose samples keep exactly 1, 255, 256 and 257 families.
tests/test_master_shapes_host.py asserts on the CPU that the fixtures (tests/master_shapes.py) reach those regimes."""
import random

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.evolution import STATS, evolution_resamples, resample_stats_host
from pangenomenem_amd.partitioning import CODES, vote_final, vote_host, vote_map, vote_state
from tests import master_shapes as ms
from tests.test_gpu_partition_chunked import stream
from tests.util import maxdiff

pytestmark = pytest.mark.gpu

CFG = dict(algo="ncem", beta=0.5, disper="sk_", it_max=30, seed=2)
BUILDERS = {"cloud": ms.cloud_master, "wide": ms.wide_master, "wide_counts": ms.wide_counts_master, "tile": ms.tile_master}
BUILDERS.update({"n%d_d%d" % s: (lambda s=s: ms.boundary_master(*s)) for s in ms.BOUNDARY_SHAPES})


@pytest.fixture(scope="module")
def masters(gpu_lib):
    """kind -> (Master, x, ptr, idx, edge_bits, edge_counts), built on first use.  The cloud and wide masters get one more
    organism that holds no family (a sample of it keeps nothing): the sampled tests never draw it by chance."""
    from pangenomenem_amd.chunks import Master
    made = {}

    def get(kind):
        if kind not in made:
            x, (ptr, idx), eb, *rest = BUILDERS[kind]()
            counts = rest[0] if rest else None
            if kind in ("cloud", "wide", "wide_counts"):
                x = np.concatenate([x, np.zeros((x.shape[0], 1), np.uint8)], axis=1)
                assert x.shape[1] <= 32 * eb.shape[1]
            made[kind] = (Master(x, ptr, idx, eb, edge_counts=counts), x, ptr, idx, eb, counts)
        return made[kind]

    yield get
    for m, *_ in made.values():
        m.close()


def samples_of(kind, d):
    if kind == "cloud":
        return ms.cloud_samples()
    if kind.startswith("wide"):
        return ms.wide_samples()
    if kind == "tile":
        return ms.tile_samples()
    return ms.boundary_samples(d)


def group_of(kind):
    return ms.WIDE_GROUP if kind.startswith("wide") else 3


def same_run(g, w, fam):
    assert np.array_equal(g["families"], fam)
    assert g["n"] == len(fam)
    assert g["status"] == w["status"] and g["iters"] == w["iters"] and g["converged"] == w["converged"]
    assert np.array_equal(g["labels"], w["c"].argmax(1))
    for key in ("prop", "center", "disp", "nbobs_k"):
        assert np.array_equal(g[key], w[key], equal_nan=True), key
    assert np.array_equal(g["crit"], w["crit"], equal_nan=True)


@pytest.mark.parametrize("tie", ["hash", "libc"])
@pytest.mark.parametrize("kind", list(BUILDERS))
def test_chunks_equal_host_formed_ones(masters, kind, tie):
    m, x, ptr, idx, eb, counts = masters(kind)
    subs = [s for s in samples_of(kind, x.shape[1]) if x[:, np.asarray(s, np.int64)].any()]
    assert subs
    cfg = dict(CFG, tie=tie)
    got = m.solve_chunks(subs, workers=4, group=group_of(kind), **cfg)
    host, want = ms.host_solve(x, ptr, idx, eb, counts, subs, **cfg)
    for g, w, (xc, nei, fam) in zip(got, want, host):
        same_run(g, w, fam)
        assert g["nnz"] == len(nei[1]) == int(nei[0][-1])
    if kind == "cloud":
        staged = [ms.tile_staged(fam) for _, _, fam in host]
        assert any(not all(t) for t in staged) and any(all(t) for t in staged)
    if kind.startswith("wide"):
        # every lock-step group straddles 65 536 kept families: each member also equals its own solo run
        from pangenomenem_amd.engine import solve
        assert all(min(len(h[2]) for h in host[g:g + ms.WIDE_GROUP]) < ms.FUSED_LIMIT <= max(len(h[2]) for h in host[g:g + ms.WIDE_GROUP])
                   for g in range(0, len(host), ms.WIDE_GROUP))
        for g, (xc, nei, fam) in zip(got, host):
            alone = solve(xc, nei, 3, *synth.default_init(xc.shape[1]), **cfg)
            same_run(g, alone, fam)


@pytest.mark.parametrize("kind", ["wide", "wide_counts"])
def test_a_chunk_above_65536_against_the_oracle(masters, oracle, kind):
    from pangenomenem_amd.chunks import form_chunk_host
    m, x, ptr, idx, eb, counts = masters(kind)
    sub = ms.wide_samples()[2]
    cfg = dict(CFG, tie="hash")
    got = m.solve_chunks([sub], workers=1, group=1, **cfg)[0]
    xc, nei, fam = form_chunk_host(x, ptr, idx, eb, sub, edge_counts=counts)
    assert len(fam) >= ms.FUSED_LIMIT
    want = oracle.run(xc, nei, 3, *synth.default_init(len(sub)), **cfg)
    assert np.array_equal(got["families"], fam)
    assert got["iters"] == want["iters"] and got["status"] == want["status"]
    assert np.array_equal(got["labels"], want["c"].argmax(1))
    assert np.array_equal(got["center"], want["center"])
    assert maxdiff(got["disp"], want["disp"]) <= 1e-6 and maxdiff(got["prop"], want["prop"]) <= 1e-6


@pytest.mark.parametrize("seed,chunk_size,batch,p_keep", [(1, 50, 64, 0.5), (2, 100, 7, 0.3)])
def test_votes_above_65536_families(masters, seed, chunk_size, batch, p_keep):
    """k_vote_init with more than 256 selected organisms (its thread-stride loop), k_vote_scan / k_vote_commit over
    more than 256 blocks"""
    from pangenomenem_amd.chunks import Votes
    m, x, *_ = masters("wide")
    rng = np.random.default_rng(seed)
    organisms = rng.permutation(300)[:int(rng.integers(260, 300))]
    pan = x[:, organisms].any(axis=1)
    assert m.n > ms.FUSED_LIMIT and len(organisms) > ms.VOTE_THREADS and ms.vote_blocks(m.n) > 256
    samples = stream(rng, pan, 400, p_keep)
    st = vote_state(m.n, pan)
    want_stop = vote_host(st, samples, len(organisms), chunk_size)
    assert want_stop > 0
    v = Votes(m, organisms, chunk_size, batch)
    got_stop = -1
    for b0 in range(0, len(samples), batch):
        s = v.add(samples[b0:b0 + batch])
        if s >= 0:
            got_stop = b0 + s
            break
    got = v.result()
    v.close()
    assert got_stop == want_stop
    assert got["samples"] == st["samples"] == want_stop + 1
    assert np.array_equal(got["cnt"], st["cnt"])
    assert np.array_equal(got["final"], vote_final(st))
    assert np.array_equal(got["first"], np.where(st["validated"], st["first"], -1))


def test_partition_above_65536_families(masters):
    """the whole loop on 140 000 families: 150 of 300 organisms per sample ends within a few dozen samples"""
    m, x, ptr, idx, eb, counts = masters("wide")
    organisms = np.arange(300)
    rng_h, rng_d = random.Random(5), random.Random(5)
    want = ms.host_partition(x, ptr, idx, eb, counts, organisms, 150, rng_h, "hash", 1, batch=16, max_samples=96)
    got, cnt, samples = m.partition(organisms=organisms, chunk_size=150, rng=rng_d, batch=16, tie="hash", seed=1, max_samples=96)
    fin = vote_final(want)
    assert samples == want["samples"] > 2
    assert np.array_equal(cnt, want["cnt"])
    assert got == {"fam%d" % (i + 1): CODES[fin[i]] for i in np.flatnonzero(want["pan"])}
    assert rng_d.getstate() == rng_h.getstate()


@pytest.mark.parametrize("kind,tie", [("cloud", "libc"), ("cloud", "hash"), ("wide", "libc"), ("wide_counts", "hash")])
def test_resample_stats_equal_host(masters, kind, tie):
    """k_resample_core over several y-blocks: single organisms, dc = 257, the full set and a sample that keeps nothing"""
    m, x, *_ = masters(kind)
    d = x.shape[1] - 1                                         # (organism d holds no family)
    assert ms.core_y_blocks(m.n) >= 2
    rng = np.random.default_rng(len(kind))
    samples = [[int(o)] for o in rng.permutation(d)[:4]] + [rng.permutation(d)[:257].tolist(), list(range(d)), [d],
                                                          rng.permutation(d)[:5].tolist(), [d, 7]]
    want = np.zeros((len(samples), 6), np.int64)
    solvable = [i for i, s in enumerate(samples) if x[:, s].any()]
    res = m.solve_chunks([samples[i] for i in solvable], tie=tie, beta=0.5, disper="sk_")
    for i, r in zip(solvable, res):
        want[i] = resample_stats_host(x, samples[i], r["labels"], vote_map(r["status"], r["center"], r["disp"]))
    got = m.resample_stats(samples, tie=tie, workers=4, group=3)
    assert np.array_equal(got, want)
    assert not got[samples.index([d])].any()
    assert np.array_equal(got[:, 4] + got[:, 5], [np.count_nonzero(x[:, s].any(axis=1)) for s in samples])


def test_evolution_above_4096_families(gpu_lib):
    """Master.evolution on 5 000 families (two core y-blocks) against partition(just_stats=True) in sequence"""
    from pangenomenem_amd.chunks import Master
    D = 40
    x, (ptr, idx), eb = synth.master_pangenome(5000, D, 9, a=0.05, b=1.0)
    assert ms.core_y_blocks(5000) == 2
    m = Master(x, ptr, idx, eb)
    try:
        chunk_size, ep = 24, dict(ratio=0.1, rmin=2, rmax=30, step=1, limit=None)
        seq_rng = random.Random(13)
        resamples = evolution_resamples(D, rng=seq_rng, **ep)
        want = []
        for r in resamples:
            st = m.partition(organisms=r, chunk_size=chunk_size, rng=seq_rng, batch=16, tie="libc", just_stats=True)[0]
            want.append([len(r)] + [st[s] for s in STATS])
        want = np.array(want, np.int64)
        assert (want[:, 0] > chunk_size).any() and (want[:, 0] <= chunk_size).any()
        rng = random.Random(13)
        rows = m.evolution(rng, chunk_size=chunk_size, tie="libc", batch=16, **ep)
        assert np.array_equal(rows, want)
        assert rng.getstate() == seq_rng.getstate()
    finally:
        m.close()
