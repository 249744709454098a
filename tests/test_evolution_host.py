"""pangenomenem_amd.evolution without a GPU: the resamples of PPanGGOLiN's --evolution against the reference's own
samplingCombinations + the driver's flatten / filter / shuffle (recorded by tests/golden/make_evolution.py), the
counts and the evol_stats.txt text against literal restatements of partition()'s just_stats branch and resample()'s
line (ppanggolin.py:982-993, 1166-1170; command_line.py:262-281, 606-617), and Master.evolution's scheduling with
fake solvers."""
import glob
import hashlib
import json
import os
import random
from collections import defaultdict

import numpy as np
import pytest

from pangenomenem_amd import evolution
from pangenomenem_amd.evolution import evol_stats_text, evolution_resamples, resample_stats_host, sampling_combinations, write_evol_stats

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evolution")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "*.json")))
SHORT_TO_LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}


def digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def load(path):
    with open(path) as f:
        return json.load(f)


def test_fixtures_cover_the_cases():
    names = {os.path.basename(p)[:-5] for p in CASES}
    assert {"d3", "d4", "d6_seed1", "d40", "d300", "d40_step3", "d40_limit12", "d20_max_below_min"} <= names


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[:-5])
def test_sampling_combinations_equal_reference(path):
    c = load(path)
    rng = random.Random(c["seed"])
    comb = sampling_combinations(c["n_items"], c["ratio"], c["rmin"], c["rmax"], c["sc_step"], rng)
    got = [[k, draws] for k, draws in comb.items()]
    assert [[k, len(d)] for k, d in got] == c["sizes"]
    if "combinations" in c:
        assert got == c["combinations"]
    assert digest(got) == c["combinations_sha256"]


@pytest.mark.parametrize("path", [p for p in CASES if load(p)["sc_step"] == 1], ids=lambda p: os.path.basename(p)[:-5])
def test_evolution_resamples_equal_reference(path):
    c = load(path)
    rng = random.Random(c["seed"])
    got = evolution_resamples(c["n_items"], c["ratio"], c["rmin"], c["rmax"], c["step"], c["limit"], rng)
    assert len(got) == c["n_resamples"]
    if "resamples" in c:
        assert got == c["resamples"]
    assert digest(got) == c["resamples_sha256"]
    assert repr(rng.random()) == c["next_random"]            # the generator is left where the reference leaves it
    assert all(len(set(r)) == len(r) for r in got)
    if c["limit"] is not None:
        assert max(len(r) for r in got) <= c["limit"]
    assert all(len(r) % c["step"] == 0 for r in got)


def test_six_items_drop_repeated_draws():
    """the example of the issue: six items, seed 1 -- k = 1 and k = 2 repeat draws, which are dropped but counted"""
    comb = sampling_combinations(6, 0.1, 10, 30, 1, random.Random(1))
    assert {k: len(v) for k, v in comb.items()} == {1: 6, 2: 9, 3: 10, 4: 10, 5: 10}
    assert 6 not in comb                                      # range(1, item_size) never reaches item_size


def test_draw_count_ignores_sample_ratio():
    """comb_k_n(item_size, k) has its arguments swapped and is 0 for k < item_size: every size gets sample_min draws
    (capped at sample_max), whatever sample_ratio asks for"""
    base = None
    for ratio in (1e-9, 0.001, 0.1, 1.0, 7.5, 1e9):
        rng = random.Random(3)
        comb = sampling_combinations(15, ratio, 10, 30, 1, rng)
        state = (comb, rng.getstate())
        if base is None:
            base = state
        assert state == base
    # the same number of draws from the stream as exactly sample_min draws per size, capped at sample_max
    for rmin, rmax, per_size in ((10, 30, 10), (10, 4, 4), (3, None, 3), (0, 30, 0)):
        rng, want = random.Random(5), random.Random(5)
        sampling_combinations(9, 0.1, rmin, rmax, 1, rng)
        for k in range(1, 9):
            for _ in range(per_size):
                want.sample(range(9), k)
        assert rng.getstate() == want.getstate()


# ---- the counts and the file


def literal_just_stats(x, organisms, partitions):
    """partition()'s just_stats branch as the reference writes it: core exact / accessory from a set of truths per
    family (ppanggolin.py:982-993), then one count per family's class (:1166-1170)"""
    stats = defaultdict(int)
    for fam in range(x.shape[0]):
        data_organisms = set(np.flatnonzero(x[fam]).tolist())
        compressed_vector = set([True if org in data_organisms else False for org in organisms])
        if len(compressed_vector) > 1:
            stats["accessory"] += 1
        elif True in compressed_vector:
            stats["core_exact"] += 1
    for node_name, nem_class in partitions.items():
        stats[SHORT_TO_LONG[nem_class]] += 1
    return stats


@pytest.mark.parametrize("seed", range(6))
def test_resample_stats_host_equal_literal(seed):
    rng = np.random.default_rng(seed)
    n, d = 300, 25
    x = (rng.random((n, d)) < rng.choice([0.05, 0.5, 0.95], n)[:, None]).astype(np.uint8)
    x[:7] = 0                                                 # families in no organism
    x[7:20] = 1                                               # core everywhere
    maps = [(0, 1, 2), (3, 3, 3), (0, 1, 2), (2, 0, 1)]
    for t in range(20):
        organisms = rng.permutation(d)[:int(rng.integers(1, d + 1))].tolist()
        kept = np.flatnonzero(x[:, organisms].any(axis=1))
        labels = rng.integers(0, 3, len(kept))
        codes = np.array(maps[t % len(maps)], np.uint8)
        partitions = {int(f): "PSCU"[codes[lab]] for f, lab in zip(kept, labels)}
        want = literal_just_stats(x, organisms, partitions)
        got = resample_stats_host(x, organisms, labels, codes)
        assert got.tolist() == [want[s] for s in evolution.STATS]
    # a resample that keeps no family: nothing at all
    z = np.zeros((5, 3), np.uint8)
    assert resample_stats_host(z, [1, 2], [], (0, 1, 2)).tolist() == [0] * 6


def literal_evol_text(nb_organisms, pan_partitions, runs):
    """command_line.py:606-617 and resample()'s line (:273-279) as the reference writes them"""
    out = []
    out.append(",".join(["nb_org", "persistent", "shell", "cloud", "core_exact", "accessory", "pangenome"]) + "\n")
    out.append(",".join([str(nb_organisms),
                         str(len(pan_partitions["persistent"])),
                         str(len(pan_partitions["shell"])),
                         str(len(pan_partitions["cloud"])),
                         str(len(pan_partitions["core_exact"])),
                         str(len(pan_partitions["accessory"])),
                         str(len(pan_partitions["accessory"]) + len(pan_partitions["core_exact"]))]) + "\n")
    for nb_org, stats in runs:
        out.append(",".join([str(nb_org),
                             str(stats["persistent"]) if stats["undefined"] == 0 else "NA",
                             str(stats["shell"]) if stats["undefined"] == 0 else "NA",
                             str(stats["cloud"]) if stats["undefined"] == 0 else "NA",
                             str(stats["core_exact"]),
                             str(stats["accessory"]),
                             str(stats["core_exact"] + stats["accessory"])]) + "\n")
    return "".join(out)


def test_write_evol_stats_equal_literal(tmp_path):
    rng = np.random.default_rng(4)
    full = defaultdict(int, persistent=1200, shell=310, cloud=4100, undefined=7, core_exact=980, accessory=4637)
    pan_partitions = {k: ["f"] * full[k] for k in ("persistent", "shell", "cloud", "undefined", "core_exact", "accessory")}
    rows, runs = [], []
    for t in range(40):
        st = defaultdict(int)
        for k in ("persistent", "shell", "cloud", "core_exact", "accessory"):
            v = int(rng.integers(0, 500))
            if v:
                st[k] = v                                     # (defaultdict: a class nobody voted for is absent)
        if t % 3 == 0:
            st["undefined"] = int(rng.integers(1, 50))
        if t % 7 == 0:
            st = defaultdict(int, undefined=90, core_exact=30, accessory=60)     # a run that emptied a class: all U
        if t == 5:
            st = defaultdict(int)                                              # a resample that keeps no family
        nb = int(rng.integers(1, 200))
        runs.append((nb, st))
        rows.append([nb] + [st[s] for s in evolution.STATS])
    want = literal_evol_text(200, pan_partitions, runs)
    assert evol_stats_text(dict(full), np.array(rows), 200) == want
    assert "NA,NA,NA" in want and want.splitlines()[1] == "200,1200,310,4100,980,4637,5617"
    path = tmp_path / "evol_stats.txt"
    write_evol_stats(str(path), (dict(full), None, 0), rows, 200)
    assert path.read_bytes() == want.encode()


# ---- Master.evolution's schedule


def fake_stats(r):
    r = list(r)
    return [sum(r) % 97, len(r) % 5, r[0], (sum(r) // 7) % 3, len(set(r)), r[-1]]


class FakeMaster:
    """Master.evolution's collaborators: a small-resample solver that sees every resample of at most chunk_size in
    one call, and a partition() that draws from rng the way the vote loop does (a data-dependent number of samples)"""

    def __init__(self, d, chunk_size):
        self.d, self.chunk_size = d, chunk_size
        self.small_calls, self.large_calls = [], []

    def resample_stats(self, samples, **kw):
        self.small_calls.append([list(s) for s in samples])
        assert all(len(s) <= self.chunk_size for s in samples)
        return np.array([fake_stats(s) for s in samples], np.int32)

    def partition(self, organisms, chunk_size, rng, just_stats, **kw):
        assert just_stats and len(organisms) > chunk_size == self.chunk_size
        self.large_calls.append(list(organisms))
        for _ in range(1 + sum(organisms) % 4):
            rng.sample(range(len(organisms)), chunk_size)
        return dict(zip(evolution.STATS, fake_stats(organisms))), None, 0


def sequential(d, chunk_size, rng, **ep):
    """the --cpu 1 worker: every resample in shuffled order, one continuing stream"""
    resamples = evolution_resamples(d, rng=rng, **ep)
    fm = FakeMaster(d, chunk_size)
    rows = []
    for r in resamples:
        if len(r) > chunk_size:
            st = fm.partition(r, chunk_size, rng, True)[0]
            rows.append([len(r)] + [st[s] for s in evolution.STATS])
        else:
            rows.append([len(r)] + fake_stats(r))
    return resamples, np.array(rows, np.int64)


@pytest.mark.parametrize("d,chunk_size,ep", [(40, 24, dict(ratio=0.1, rmin=4, rmax=30, step=1, limit=None)),
                                             (30, 10, dict(ratio=0.1, rmin=3, rmax=30, step=2, limit=25)),
                                             (12, 20, dict(ratio=0.1, rmin=5, rmax=30, step=1, limit=None)),
                                             (16, 0, dict(ratio=0.1, rmin=2, rmax=30, step=1, limit=None))])
def test_master_evolution_schedule(d, chunk_size, ep):
    from pangenomenem_amd.chunks import Master
    seq_rng = random.Random(21)
    resamples, want = sequential(d, chunk_size, seq_rng, **ep)
    fm = FakeMaster(d, chunk_size)
    rng = random.Random(21)
    rows = Master.evolution(fm, rng, chunk_size=chunk_size, **ep)
    assert np.array_equal(rows, want)
    assert rng.getstate() == seq_rng.getstate()
    small = [r for r in resamples if len(r) <= chunk_size]
    large = [r for r in resamples if len(r) > chunk_size]
    assert fm.small_calls == ([small] if small else [])       # every small resample in one call, in shuffled order
    assert fm.large_calls == large                            # the large ones one after another, in shuffled order
    if chunk_size == 0:
        assert not small and large


def test_evolution_rows_small_solver_draws_nothing():
    rng = random.Random(3)
    resamples = evolution_resamples(10, rmin=3, rng=rng)
    before = rng.getstate()
    rows = evolution.evolution_rows(resamples, rng, 10, lambda rs: [fake_stats(r) for r in rs], None)
    assert rng.getstate() == before
    assert rows[:, 0].tolist() == [len(r) for r in resamples]
    assert rows[:, 1:].tolist() == [fake_stats(r) for r in resamples]
