"""Master.partition -- partition()'s loop over random samples of a large pangenome (ppanggolin.py:995-1105) with the
vote on the device (csrc/nem_vote.hip) -- against the host recipe: the same random.Random draws, the same samples
solved by Master.solve_chunks, their class maps by partitioning.vote_map and the vote by partitioning.vote_host
(CPU-tested against the reference's dict loop in tests/test_vote_host.py).  Plus the vote kernels alone on synthetic
label streams and synthetic parameters."""
import random

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.partitioning import CODES, partition_dicts, vote_final, vote_host, vote_map, vote_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small_master(gpu_lib):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb = synth.master_pangenome(3000, 300, 5)
    m = Master(x, ptr, idx, eb)
    yield m, x
    m.close()


def pan_of(x, organisms):
    return x[:, organisms].any(axis=1)


def stream(rng, pan, count, p_keep):
    """label streams with a leaning per family (most families find a majority), now and then an all-U or a permuted map"""
    pool = [(0, 1, 2)] * 6 + [(3, 3, 3), (2, 0, 1)]
    lean = rng.integers(0, 3, len(pan))
    out = []
    for _ in range(count):
        fam = np.flatnonzero((rng.random(len(pan)) < p_keep) & pan)
        lab = np.where(rng.random(len(fam)) < 0.8, lean[fam], rng.integers(0, 3, len(fam)))
        out.append((fam, lab, pool[rng.integers(0, len(pool))]))
    return out


@pytest.mark.parametrize("seed,chunk_size,batch,p_keep", [(1, 50, 7, 0.5), (2, 100, 64, 0.3), (3, 25, 1, 0.7), (4, 299, 13, 0.9),
                                                          (5, 10, 64, 0.2)])
def test_votes_add_host_equal_vote_host(small_master, seed, chunk_size, batch, p_keep):
    from pangenomenem_amd.chunks import Votes
    m, x = small_master
    rng = np.random.default_rng(seed)
    organisms = rng.permutation(m.d)[:int(rng.integers(150, m.d))]
    pan = pan_of(x, organisms)
    samples = stream(rng, pan, 1500, p_keep)
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


def test_vote_classmap_device_equals_host(gpu_lib):
    from pangenomenem_amd.chunks import vote_classmap_device
    rng = np.random.default_rng(9)
    status, centers, disps = [], [], []
    for t in range(300):
        dc = int(rng.integers(1, 40))
        center = (rng.random((3, dc)) < 0.5).astype(np.float32)
        disp = rng.choice(np.float32([0.1, 0.2, 0.3, 0.5]), (3, dc)).astype(np.float32)
        kind = t % 6
        if kind == 1:
            center[rng.integers(0, 3), rng.integers(0, dc)] = np.nan
            disp[rng.integers(0, 3), rng.integers(0, dc)] = np.nan
        elif kind == 2:
            center[1] = center[0]
            disp[2] = disp[1]
        elif kind == 3:
            disp[0, 0] = np.nan
        elif kind == 4:
            center[0], center[2], disp[1] = 1.0, 0.0, 0.5
        elif kind == 5:                              # float64 sums that float32 would round differently
            disp = rng.random((3, dc)).astype(np.float32)
            center[0] = 1.0
        status.append(2 if t % 7 == 0 else 0)
        centers.append(center)
        disps.append(disp)
    got = vote_classmap_device(status, centers, disps)
    want = np.stack([vote_map(s, c, e) for s, c, e in zip(status, centers, disps)])
    assert np.array_equal(got, want)
    assert (want[:, 0] == 0).any() and (want[:, 0] == 3).any()


def host_partition(m, x, organisms, chunk_size, rng, disper, tie, seed, max_samples=5000):
    """partition()'s sequential loop on the host: samples drawn one at a time, solved by Master.solve_chunks (16 per
    call), their votes by vote_map and vote_host; the draws after the stop undone"""
    organisms = np.asarray(organisms)
    pan = pan_of(x, organisms)
    st = vote_state(m.n, pan)
    while st["samples"] < max_samples:
        states, samples = [], []
        for _ in range(16):
            states.append(rng.getstate())
            samples.append(organisms[rng.sample(range(len(organisms)), chunk_size)])
        res = m.solve_chunks(samples, disper=disper, tie=tie, seed=seed, it_max=100)
        votes = [(r["families"], r["labels"], vote_map(r["status"], r["center"], r["disp"])) for r in res]
        stop = vote_host(st, votes, len(organisms), chunk_size)
        if stop >= 0:
            if stop + 1 < 16:
                rng.setstate(states[stop + 1])
            return st
    raise AssertionError("no end")


def check_partition(m, x, organisms, chunk_size, disper, tie, batch, seed=3):
    rng_h, rng_d = random.Random(seed), random.Random(seed)
    want = host_partition(m, x, organisms, chunk_size, rng_h, disper, tie, 1)
    got, cnt, samples = m.partition(organisms=organisms, chunk_size=chunk_size, rng=rng_d, batch=batch, tie=tie, seed=1,
                                    free_dispersion=disper == "skd")
    fin = vote_final(want)
    assert samples == want["samples"]
    assert np.array_equal(cnt, want["cnt"])
    names = ["fam%d" % (i + 1) for i in range(m.n)]
    assert got == {names[i]: CODES[fin[i]] for i in np.flatnonzero(want["pan"])}
    assert rng_d.getstate() == rng_h.getstate()
    return got, samples


@pytest.mark.parametrize("tie", ["hash", "libc"])
@pytest.mark.parametrize("disper", ["sk_", "skd"])
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_partition_equals_host_loop(small_master, tie, disper, batch):
    m, x = small_master
    got, samples = check_partition(m, x, np.arange(m.d), 50, disper, tie, batch)
    assert samples > 10 and len(set(got.values())) >= 2


def test_partition_large_chunks(gpu_lib):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb = synth.master_pangenome(5000, 1200, 8)
    m = Master(x, ptr, idx, eb)
    try:
        for batch, tie in ((7, "libc"), (64, "hash")):
            check_partition(m, x, np.arange(m.d), 500, "sk_", tie, batch, seed=21)
    finally:
        m.close()


def test_partition_subset_leaves_families_out(small_master):
    m, x = small_master
    organisms = np.random.default_rng(4).permutation(m.d)[:120]
    assert not pan_of(x, organisms).all()
    got, _ = check_partition(m, x, organisms, 40, "sk_", "libc", 16)
    assert len(got) == int(pan_of(x, organisms).sum())
    stats, _, _ = m.partition(organisms=organisms, chunk_size=40, rng=random.Random(3), batch=16, seed=1, just_stats=True)
    core = x[:, organisms].all(axis=1)
    assert stats["core_exact"] == int(core.sum()) and stats["accessory"] == len(got) - int(core.sum())
    long = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
    for c in "PSCU":
        assert stats.get(long[c], 0) == sum(1 for v in got.values() if v == c)


def test_partition_small_case(small_master):
    m, x = small_master
    organisms = np.random.default_rng(6).permutation(m.d)[:45]
    for tie in ("hash", "libc"):
        rng = random.Random(8)
        before = rng.getstate()
        got, cnt, samples = m.partition(organisms=organisms, chunk_size=50, rng=rng, tie=tie, seed=1)
        assert samples == 1 and rng.getstate() == before
        r = m.solve_chunks([organisms], tie=tie, seed=1)[0]
        names = ["fam%d" % (i + 1) for i in r["families"]]
        res = dict(status=r["status"], c=np.eye(3, dtype=np.float32)[r["labels"]], center=r["center"], disp=r["disp"], prop=r["prop"])
        want, _ = partition_dicts(res, names)
        assert got == want


def test_partition_max_samples(small_master):
    m, _ = small_master
    with pytest.raises(NemGpuError):
        m.partition(chunk_size=50, rng=random.Random(1), batch=4, max_samples=8)
