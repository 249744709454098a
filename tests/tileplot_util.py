"""Inputs shared by tests/test_tileplot_host.py and tests/test_gpu_tileplot.py."""
import numpy as np

SMALL = (3000, 12)                       # families x organisms
SMALL_SEEDS = (0, 1, 2, 3)
LARGE = (40000, 70)
# seeds of random_matrix whose distances are pairwise distinct, picked on the CPU (of 0 .. 11 at LARGE all but seed 4 qualify:
# a distance is a ratio of two counts, and the organisms' own frequencies spread the counts); every test that uses one
# asserts it
LARGE_SEEDS = (0, 1)


def random_matrix(n, d, seed):
    """presence/absence uint8 [n][d]: every family with a frequency of its own, every organism with a completeness of
    its own"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, d)) < rng.random(n)[:, None] ** 0.5 * rng.uniform(0.2, 1.0, d)[None, :]).astype(np.uint8)


def condensed(square):
    """the upper triangle in pdist's order"""
    square = np.asarray(square)
    return square[np.triu_indices(len(square), 1)]


def distinct(values):
    return len(np.unique(values)) == len(values)


def merged_sets(i2, j2):
    """the leaves of every merge's new cluster, the merges given by the index each side is kept under"""
    members = {}
    out = []
    for a, b in zip(np.asarray(i2).tolist(), np.asarray(j2).tolist()):
        s = members.get(a, frozenset([a])) | members.pop(b, frozenset([b]))
        members[a] = s
        out.append(s)
    return out


def hub_matrix(d=40, hub=200):
    """Every organism below d - 1 has organism d - 1 as its nearest neighbour, and the first merge retires it: the last
    organism carries the hub families alone, the one before it the hub and one more, organism i the hub and i + 2
    private ones, so dist(i, d - 1) = (i + 2) / (hub + i + 2) is below every other distance of row i."""
    blocks = [i + 2 for i in range(d - 2)] + [1]
    x = np.zeros((hub + sum(blocks), d), np.uint8)
    x[:hub] = 1
    at = hub
    for o, size in enumerate(blocks):
        x[at:at + size, o] = 1
        at += size
    return x
