"""Master.resample_stats / Master.evolution -- PPanGGOLiN's --evolution on the device (csrc/nem_resample.hip) --
against the host recipe: the same samples solved by Master.solve_chunks, their class maps by partitioning.vote_map and
their counts by evolution.resample_stats_host (CPU-tested against partition()'s just_stats branch in
tests/test_evolution_host.py); and the whole curve against a sequential loop of Master.partition(just_stats=True)."""
import random

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.evolution import STATS, evol_stats_text, evolution_resamples, resample_stats_host
from pangenomenem_amd.partitioning import vote_map

pytestmark = pytest.mark.gpu

N, D = 2000, 40


@pytest.fixture(scope="module")
def masters(gpu_lib):
    from pangenomenem_amd.chunks import Master
    out = {}
    x, (ptr, idx), eb = synth.master_pangenome(N, D, 3)
    x = np.concatenate([x, np.zeros((N, 1), np.uint8)], axis=1)      # organism D holds no family
    out["bits"] = (Master(x, ptr, idx, eb), x)
    xc, (pc, ic), ebc, cnts = synth.master_pangenome_counts(N, D, 5, multi_frac=0.1, loops=0.02)
    xc = np.concatenate([xc, np.zeros((N, 1), np.uint8)], axis=1)
    out["counts"] = (Master(xc, pc, ic, ebc, edge_counts=cnts), xc)
    yield out
    for m, _ in out.values():
        m.close()


def samples_of(seed, chunk_size):
    """sizes 1 .. chunk_size (several one-organism samples: their runs empty a class), plus the empty organism alone"""
    rng = np.random.default_rng(seed)
    out = []
    for size in list(range(1, chunk_size + 1)) + [1] * 6 + [2] * 4:
        out.append(rng.permutation(D)[:size].tolist())
    out.insert(len(out) // 2, [D])                            # keeps no family
    out.append([D, int(rng.integers(0, D))])
    return out


def host_stats(m, x, samples, tie, free_dispersion):
    want = np.zeros((len(samples), 6), np.int64)
    solvable = [i for i, s in enumerate(samples) if x[:, s].any()]
    res = m.solve_chunks([samples[i] for i in solvable], tie=tie, beta=0.5, disper="skd" if free_dispersion else "sk_")
    for i, r in zip(solvable, res):
        want[i] = resample_stats_host(x, samples[i], r["labels"], vote_map(r["status"], r["center"], r["disp"]))
    return want, res


@pytest.mark.parametrize("kind", ["bits", "counts"])
@pytest.mark.parametrize("tie,free_dispersion,workers,group", [("libc", False, 8, 32), ("hash", False, 3, 7), ("libc", True, 8, 64)])
def test_resample_stats_equal_host(masters, kind, tie, free_dispersion, workers, group):
    m, x = masters[kind]
    samples = samples_of(len(kind) * 10 + group, D)
    want, res = host_stats(m, x, samples, tie, free_dispersion)
    got = m.resample_stats(samples, tie=tie, free_dispersion=free_dispersion, workers=workers, group=group)
    assert got.dtype == np.int32 and got.shape == (len(samples), 6)
    assert np.array_equal(got, want)
    assert not got[samples.index([D])].any()                  # the sample that keeps no family: all 0
    assert any(r["status"] != 0 for r in res)                 # runs that emptied a class ...
    assert (got[:, 3] > 0).any() and (got[:, 3] == 0).any()   # ... count every family undefined, the others not
    assert np.array_equal(got[:, 4] + got[:, 5], [np.count_nonzero(x[:, s].any(axis=1)) for s in samples])


def test_resample_stats_refuses_bad_samples(masters):
    m, _ = masters["bits"]
    for bad in ([3, 5, 3], [0, D + 1], [-1]):
        with pytest.raises(NemGpuError) as e:
            m.resample_stats([[0, 1, 2], bad])
        assert e.value.status == 3                            # NEMGPU_E_ARG
    assert m.resample_stats([[0, 1, 2]]).shape == (1, 6)      # (the master is still usable)


@pytest.fixture(scope="module")
def plain_masters(gpu_lib):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb = synth.master_pangenome(1500, D, 7)
    xc, (pc, ic), ebc, cnts = synth.master_pangenome_counts(1500, D, 8, multi_frac=0.1, loops=0.02)
    out = {"bits": Master(x, ptr, idx, eb), "counts": Master(xc, pc, ic, ebc, edge_counts=cnts)}
    yield out
    for m in out.values():
        m.close()


@pytest.mark.parametrize("kind,tie", [("bits", "libc"), ("counts", "hash")])
def test_evolution_equal_sequential_partition(plain_masters, kind, tie):
    """24 of 40 organisms per chunk: the resamples of 25 .. 39 organisms run partition()'s vote loop on the stream"""
    m = plain_masters[kind]
    chunk_size, ep = 24, dict(ratio=0.1, rmin=2, rmax=30, step=1, limit=None)

    def full_stats(rng):                                      # the main partition() before --evolution, on the same stream
        return m.partition(chunk_size=chunk_size, rng=rng, batch=16, tie=tie, just_stats=True)[0]

    # the reference's --cpu 1 run: every resample through partition() in shuffled order on one stream
    seq_rng = random.Random(11)
    full_seq = full_stats(seq_rng)
    resamples = evolution_resamples(D, rng=seq_rng, **ep)
    want = []
    for r in resamples:
        st = m.partition(organisms=r, chunk_size=chunk_size, rng=seq_rng, batch=16, tie=tie, just_stats=True)[0]
        want.append([len(r)] + [st[s] for s in STATS])
    want = np.array(want, np.int64)
    assert (want[:, 0] > chunk_size).any() and (want[:, 0] <= chunk_size).any()

    rng = random.Random(11)
    full = full_stats(rng)
    rows = m.evolution(rng, chunk_size=chunk_size, tie=tie, batch=16, **ep)
    assert np.array_equal(rows, want)
    assert rng.getstate() == seq_rng.getstate()
    assert evol_stats_text(full, rows, D) == evol_stats_text(full_seq, want, D)
