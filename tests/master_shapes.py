"""Masters at pangenome-scale shapes for the device chunk, vote and evolution paths (csrc/nem_chunks.hip, nem_vote.hip,
nem_resample.hip), and the host arithmetic that says which branch of those kernels a sample takes.

The small dense masters of the other tests (synth.master_pangenome's Beta(0.3, 0.3) spectrum, n <= 20 000) never reach
the branches below; tests/test_master_shapes_host.py asserts on the CPU that these fixtures do, and
tests/test_gpu_master_shapes.py runs them on the device against the host recipe."""
import functools

import numpy as np

from pangenomenem_amd import synth
from pangenomenem_amd.partitioning import vote_host, vote_map, vote_state

# ---- the kernels' constants and launch shapes, restated
CHUNK_TILE = 256            # k_chunk_rows: kept families per block
CHUNK_SPAN = 12             # k_chunk_rows: kChunkSpan, the 64-family words of a row one pass stages
CHUNK_ORGS = 256            # k_chunk_rows: kChunkOrgs, the organisms staged per pass
INDEX_WORDS = 1024          # k_chunk_index: 64-family words per pass of its 1024-thread block
CORE_WORDS = 64             # k_resample_core: kResampleCoreWave, words per y-block
VOTE_THREADS = 256          # k_vote_init: organisms per thread stride; k_vote_scan / k_vote_commit: families per block
FUSED_LIMIT = 65536         # density_verify_supported / launch_sweep_counts: fused kernels below this many families


def nw64(n):
    return (n + 63) // 64


def index_passes(n):
    """k_chunk_index's passes over the keep words (base is carried from one to the next)"""
    return -(-nw64(n) // INDEX_WORDS)


def core_y_blocks(n):
    """gridDim.y of k_resample_core"""
    return -(-nw64(n) // CORE_WORDS)


def vote_blocks(n):
    """blocks of k_vote_scan / k_vote_commit"""
    return -(-n // VOTE_THREADS)


def organism_passes(dc):
    """k_chunk_rows' passes over the sample's organisms"""
    return -(-dc // CHUNK_ORGS)


def tile_staged(families):
    """k_chunk_rows' staging decision per 256-family tile of a sample's kept families (master indices, ascending): a
    tile is staged through LDS when its first and last family lie fewer than kChunkSpan 64-family words apart, and
    read straight from the master's rows (the unstaged branch) otherwise"""
    fam = np.asarray(families, np.int64)
    return [bool((fam[min(t + CHUNK_TILE, len(fam)) - 1] >> 6) - (fam[t] >> 6) < CHUNK_SPAN) for t in range(0, len(fam), CHUNK_TILE)]


def tile_shape(nc):
    """(full tiles, families in the last started tile, npad) of a chunk with nc kept families"""
    npad = -(-nc // CHUNK_TILE) * CHUNK_TILE
    last = nc - (npad - CHUNK_TILE) if nc else 0
    return nc // CHUNK_TILE, last, npad


def kept(x, organisms):
    """the master indices of the families a sample keeps"""
    return np.flatnonzero(np.asarray(x)[:, np.asarray(organisms, np.int64)].any(axis=1))


# ---- the masters (cached: the host and the device tests of one session build each once)
@functools.lru_cache(maxsize=None)
def cloud_master():
    """mostly cloud (Beta(0.05, 1)): a sample of a few organisms keeps a small, sparse share of the families, so its
    tiles span more than kChunkSpan words (unstaged); 313 words, 5 core y-blocks"""
    return synth.master_pangenome(20000, 300, 41, a=0.05, b=1.0)


@functools.lru_cache(maxsize=None)
def wide_master():
    """more than 131 072 families (3 index passes, 2 188 words); a single organism keeps fewer than 65 536 of them,
    three or more organisms keep more"""
    return synth.master_pangenome(140000, 300, 42, a=0.3, b=0.6)


@functools.lru_cache(maxsize=None)
def wide_counts_master():
    """wide_master's shape with occurrence counts (nemgpu_master_create_counts), a directed graph's"""
    return synth.master_pangenome_counts(140000, 300, 43, multi_frac=0.05, dense_loops=2, directed=True, a=0.3, b=0.6)


BOUNDARY_SHAPES = ((1, 1), (1, 33), (63, 32), (64, 1), (64, 65), (65, 33), (4097, 32), (4097, 65))


@functools.lru_cache(maxsize=None)
def boundary_master(n, d):
    """n around one 64-family word (the last word partial or exactly full), d around one 32-organism word"""
    return synth.master_pangenome(n, d, 50 + n + d)


TILE_KEEPS = (1, 255, 256, 257)     # the kept families of tile_master's single-organism samples 0 .. 3


@functools.lru_cache(maxsize=None)
def tile_master():
    """600 families, 6 organisms: organism o < 4 alone keeps exactly TILE_KEEPS[o] families (a partial tile, one
    short of a tile, an exact tile, a tile and one), spread over the master; organisms 4 and 5 hold the rest and some
    of the same.  The graph: contiguity_graph's structure, an edge carried by the organisms that hold both ends."""
    n, d = 600, 6
    rng = np.random.default_rng(600)
    x = np.zeros((n, d), np.uint8)
    for o, c in enumerate(TILE_KEEPS):
        x[np.sort(rng.permutation(n)[:c]), o] = 1
    x[:, 4] = x[:, :4].sum(axis=1) == 0
    x[rng.permutation(n)[:200], 5] = 1
    ptr, idx, _ = synth.contiguity_graph(n, 600)
    src = np.repeat(np.arange(n), np.diff(ptr))
    both = x[src] & x[idx]
    eb = np.zeros((len(idx), 4), np.uint8)
    eb[:, :1] = np.packbits(both, axis=1, bitorder="little")
    return x, (ptr, idx), np.ascontiguousarray(eb.view(np.uint32))


# ---- the samples the tests draw
def cloud_samples():
    """single organisms and pairs (unstaged), 5 and 20 (some tiles staged), 100, 257 (a second organism pass with one
    organism in it) and the full set (staged)"""
    rng = np.random.default_rng(41)
    return [rng.permutation(300)[:dc] for dc in (1, 2, 100, 1, 5, 257, 20, 300, 2)]


WIDE_GROUP = 2


def wide_samples():
    """lock-step groups of WIDE_GROUP: every group has one member below 65 536 kept families and one above"""
    rng = np.random.default_rng(42)
    return [rng.permutation(300)[:dc] for dc in (1, 10, 3, 2, 257, 1)]


def boundary_samples(d):
    rng = np.random.default_rng(d)
    out = [[o] for o in sorted({0, d - 1, d // 2})] + [np.arange(d)]
    if d > 2:
        out += [rng.permutation(d)[:d // 2 + 1], rng.permutation(d)]
    return out


def tile_samples():
    return [[0], [1], [2], [3], [3, 0], [0, 1, 2, 3, 4, 5], [5, 1]]


# ---- partition()'s sequential loop on the host
def host_solve(x, ptr, idx, eb, counts, subs, **cfg):
    """the samples formed by form_chunk_host and solved by solve_many (PPanGGOLiN's default .m)"""
    from pangenomenem_amd.batch import solve_many
    from pangenomenem_amd.chunks import form_chunk_host
    host = [form_chunk_host(x, ptr, idx, eb, s, edge_counts=counts) for s in subs]
    probs = [(xc, nei, 3) + synth.default_init(xc.shape[1]) for xc, nei, _ in host]
    return host, solve_many(probs, workers=4, group=8, **cfg)


def host_partition(x, ptr, idx, eb, counts, organisms, chunk_size, rng, tie, seed, batch=16, max_samples=5000):
    """partition()'s sequential loop on the host: the samples formed by form_chunk_host, solved by solve_many, voted by
    vote_map and vote_host; the draws after the stop undone"""
    organisms = np.asarray(organisms)
    st = vote_state(x.shape[0], x[:, organisms].any(axis=1))
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie=tie, seed=seed)
    while st["samples"] < max_samples:
        states, samples = [], []
        for _ in range(batch):
            states.append(rng.getstate())
            samples.append(organisms[rng.sample(range(len(organisms)), chunk_size)])
        host, res = host_solve(x, ptr, idx, eb, counts, samples, **cfg)
        votes = [(fam, r["c"].argmax(1), vote_map(r["status"], r["center"], r["disp"])) for (_, _, fam), r in zip(host, res)]
        stop = vote_host(st, votes, len(organisms), chunk_size)
        if stop >= 0:
            if stop + 1 < batch:
                rng.setstate(states[stop + 1])
            return st
    raise AssertionError("no end")
