"""partition()'s vote over the samples (ppanggolin.py:1015-1105), in numpy (partitioning.vote_host / vote_final /
vote_map: what the device kernels of csrc/nem_vote.hip are held against), checked on the CPU against the reference's
own loop restated with dicts, one sample and one family at a time; and the sampling loop of Master.partition
(chunks.partition_loop) against random.sample drawn one at a time."""
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import partition_loop
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.partitioning import CODES, partition_dicts, vote_final, vote_host, vote_map, vote_state


def by_the_book(samples, pan, n_sel, chunk_size):
    """validate_family + the while loop + the final max (ppanggolin.py:1015-1037, 1057-1105), literally.  Returns
    (final {family: code}, true counts {family: [P, S, C, U]}, samples voted, stop index or -1)."""
    cpt_partition = OrderedDict((f, {"P": 0, "S": 0, "C": 0, "U": 0}) for f in pan)
    true = {f: [0, 0, 0, 0] for f in pan}           # (the counts without the forced sys.maxsize)
    validated = set()
    voted, stop = 0, -1
    for s, (fam, lab, codes) in enumerate(samples):
        if len(validated) >= len(pan):
            break
        voted += 1
        partitions = {int(f): CODES[codes[int(l)]] for f, l in zip(fam, lab)}
        for node, nem_class in partitions.items():
            cpt_partition[node][nem_class] += 1
            true[node][CODES.index(nem_class)] += 1
            sum_partionning = sum(cpt_partition[node].values())
            if (sum_partionning > n_sel / chunk_size and max(cpt_partition[node].values()) >= sum_partionning * 0.5) or (sum_partionning > n_sel):
                if node not in validated:
                    if max(cpt_partition[node].values()) < sum_partionning * 0.5:
                        cpt_partition[node]["U"] = sys.maxsize
                    validated.add(node)
        if len(validated) >= len(pan):
            stop = s
    final = {f: max(data, key=data.get) for f, data in cpt_partition.items()}
    return final, true, voted, stop


def numpy_vote(samples, n, pan, n_sel, chunk_size, batch):
    """vote_host fed `batch` samples at a time, as Master.partition feeds the device"""
    pan_mask = np.zeros(n, bool)
    pan_mask[list(pan)] = True
    st = vote_state(n, pan_mask)
    stop = -1
    for b0 in range(0, len(samples), batch):
        s = vote_host(st, samples[b0:b0 + batch], n_sel, chunk_size)
        if s >= 0:
            stop = b0 + s
            break
    return st, stop


def check(samples, n, pan, n_sel, chunk_size, batch=5):
    final, true, voted, stop = by_the_book(samples, pan, n_sel, chunk_size)
    st, got_stop = numpy_vote(samples, n, pan, n_sel, chunk_size, batch)
    assert got_stop == stop
    assert st["samples"] == voted
    fin = vote_final(st)
    for f in range(n):
        if f in true:
            assert CODES[fin[f]] == final[f], f
            assert list(st["cnt"][f]) == true[f], f
        else:
            assert fin[f] == 0xFF and not st["cnt"][f].any()
    return st, stop


def random_stream(rng, n, pan, count, p_keep, codes_pool):
    out = []
    for _ in range(count):
        fam = np.flatnonzero((rng.random(n) < p_keep) & pan)
        lab = rng.integers(0, 3, len(fam))
        out.append((fam, lab, codes_pool[rng.integers(0, len(codes_pool))]))
    return out


IDENT, ALL_U = (0, 1, 2), (3, 3, 3)


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("n_sel,chunk_size", [(7, 2), (6, 2), (20, 3), (1000, 500), (5, 5)])
def test_random_streams(seed, n_sel, chunk_size):
    rng = np.random.default_rng(seed * 31 + n_sel)
    n = 60
    pan = rng.random(n) < 0.8
    pool = [IDENT, IDENT, IDENT, ALL_U, (2, 1, 0), (0, 0, 3)]
    samples = random_stream(rng, n, pan, 200, rng.uniform(0.2, 0.9), pool)
    check(samples, n, set(np.flatnonzero(pan).tolist()), n_sel, chunk_size, batch=int(rng.integers(1, 9)))


def one_family(votes):
    return [([0], [0], (c, c, c)) for c in votes]


def test_strict_greater_than_integer_quotient():
    # 6 / 2 = 3.0: three votes are not enough, the fourth validates
    st, stop = check(one_family([0, 0, 0, 0, 0]), 1, {0}, 6, 2)
    assert stop == 3 and st["first"][0] == 3


def test_non_integer_quotient():
    # 7 / 2 = 3.5: validated at the fourth vote
    st, stop = check(one_family([1, 1, 1, 1, 1]), 1, {0}, 7, 2)
    assert stop == 3 and vote_final(st)[0] == 1


def test_half_is_a_majority_and_ties_go_in_psc_order():
    # P S P S: 2 * 2 >= 4 validates at the fourth vote; P and S tie, P wins
    st, stop = check(one_family([0, 1, 0, 1]), 1, {0}, 6, 2)
    assert stop == 3 and vote_final(st)[0] == 0 and not st["forced"][0]
    # S C S C: S first
    st, _ = check(one_family([1, 2, 1, 2]), 1, {0}, 6, 2)
    assert vote_final(st)[0] == 1
    # C U C U: C first
    st, _ = check(one_family([2, 3, 2, 3]), 1, {0}, 6, 2)
    assert vote_final(st)[0] == 2


def test_more_votes_than_organisms_forces_u():
    # 4 organisms, chunk 2: P S C U has no majority; the fifth vote exceeds len(organisms): validated, U forced although
    # P then leads
    st, stop = check(one_family([0, 1, 2, 3, 0]), 1, {0}, 4, 2)
    assert stop == 4 and st["forced"][0] and vote_final(st)[0] == 3
    assert list(st["cnt"][0]) == [2, 1, 1, 1]


def test_votes_after_validation_count():
    # family 0 validates at the fourth sample, family 1 only at the eighth: family 0's later votes count
    samples = [([0, 1], [0, 0], (0, 1 if s % 2 else 2, 3)) for s in range(3)]
    samples += [([0], [0], IDENT)] + [([0, 1], [0, 1], (2, 1 if s % 2 else 0, 3)) for s in range(8)]
    st, stop = check(samples, 2, {0, 1}, 6, 2)
    assert stop >= 0 and st["cnt"][0].sum() > 4


def test_stop_in_the_middle_of_a_batch():
    samples = one_family([0] * 10)
    for batch in (1, 3, 4, 7, 64):
        st, stop = check(samples, 1, {0}, 6, 2, batch=batch)
        assert stop == 3 and st["samples"] == 4 and list(st["cnt"][0]) == [4, 0, 0, 0]


def test_samples_that_keep_nothing_count_as_samples():
    samples = [([], [], IDENT)] + one_family([0] * 6)
    st, stop = check(samples, 1, {0}, 6, 2)
    assert stop == 4 and st["samples"] == 5


def params(rng, dc, kind):
    center = (rng.random((3, dc)) < 0.5).astype(np.float32)
    disp = rng.choice(np.float32([0.1, 0.25, 0.5]), (3, dc)).astype(np.float32)
    if kind == "nan":
        center[rng.integers(0, 3), rng.integers(0, dc)] = np.nan
        disp[rng.integers(0, 3), rng.integers(0, dc)] = np.nan
    elif kind == "tie":
        center[1] = center[0]
        disp[2] = disp[1]
    elif kind == "nan_first":
        disp[0, 0] = np.nan
    elif kind == "good":
        center[0] = 1.0
        center[1] = np.where(rng.random(dc) < 0.5, 0.5, 0.0)
        center[2] = 0.0
        disp[1] = 0.5
    return center, disp


@pytest.mark.parametrize("kind", ["random", "nan", "tie", "nan_first", "good"])
@pytest.mark.parametrize("status", [0, 2])
def test_vote_map_matches_partition_dicts(kind, status):
    rng = np.random.default_rng(hash(kind) % 1000 + status)
    for trial in range(40):
        dc = int(rng.integers(1, 12))
        center, disp = params(rng, dc, kind)
        n = 9
        lab = rng.integers(0, 3, n)
        c = np.eye(3, dtype=np.float32)[lab]
        res = dict(status=status, c=c, center=center, disp=disp, prop=np.full(3, 1 / 3, np.float32))
        names = ["f%d" % i for i in range(n)]
        want, _ = partition_dicts(res, names)
        codes = vote_map(status, center, disp)
        assert [CODES[codes[l]] for l in lab] == [want[nm] for nm in names]


def test_vote_map_shapes():
    center = np.stack([np.ones(4), np.full(4, 0.5), np.zeros(4)]).astype(np.float32)
    disp = np.stack([np.full(4, 0.1), np.full(4, 0.5), np.full(4, 0.1)]).astype(np.float32)
    assert list(vote_map(0, center, disp)) == [0, 1, 2]
    assert list(vote_map(2, center, disp)) == [3, 3, 3]
    assert list(vote_map(0, center[::-1].copy(), disp)) == [3, 3, 3]      # persistent class is 2: the ValueError branch


class Draws:
    """A fake solver: every family is validated after the `end`-th sample of the loop"""

    def __init__(self, end):
        self.end, self.seen, self.samples = end, 0, []

    def __call__(self, batch):
        self.samples += batch
        first = self.seen
        self.seen += len(batch)
        return self.end - 1 - first if self.seen >= self.end else -1


@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("end", [1, 6, 7, 8, 64, 65, 130])
def test_partition_loop_leaves_rng_as_the_reference(batch, end):
    rng, ref = random.Random(11), random.Random(11)
    organisms = list(range(40))
    fake = Draws(end)
    assert partition_loop(len(organisms), 9, rng, batch, 10 ** 6, fake) == end
    want = [ref.sample(organisms, 9) for _ in range(end)]          # orgs = sample(organisms, chunck_size), :1062
    assert fake.samples[:end] == want
    assert rng.getstate() == ref.getstate()
    assert rng.random() == ref.random()


def test_partition_loop_on_the_random_module():
    random.seed(5)
    partition_loop(30, 4, random, 7, 10 ** 6, Draws(10))
    after = random.random()
    random.seed(5)
    for _ in range(10):
        random.sample(range(30), 4)
    assert random.random() == after


def test_partition_loop_gives_up():
    with pytest.raises(NemGpuError):
        partition_loop(30, 4, random.Random(1), 7, 20, Draws(10 ** 9))
