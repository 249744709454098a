"""Counts masters (nemgpu_master_create_counts): the samples of partition()'s loop formed on the device with the
reference's coverage -- a sum of occurrence counts -- against the same samples formed on the host
(chunks.form_chunk_host(edge_counts=...), CPU-tested against the reference's own writer in tests/test_nei_counts.py)
and solved by nemgpu_solve_many; Master.partition on them against the host vote; Master.from_graph."""
import json
import os
import random

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.partitioning import CODES, partition_dicts, vote_final
from tests.master_shapes import host_partition, host_solve
from tests.util import maxdiff

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nei_counts")


def same_run(g, w, fam):
    assert np.array_equal(g["families"], fam)
    assert g["status"] == w["status"] and g["iters"] == w["iters"] and g["converged"] == w["converged"]
    assert np.array_equal(g["labels"], w["c"].argmax(1))
    for key in ("prop", "center", "disp", "nbobs_k"):
        assert maxdiff(g[key], w[key]) <= 1e-6, key
    assert np.allclose(g["crit"], w["crit"], rtol=1e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("n,d,dc,count,seed,directed,dense", [(3000, 200, 50, 8, 1, False, 0), (2500, 320, 33, 6, 2, True, 2),
                                                              (4000, 150, 150, 3, 3, False, 4), (20000, 1000, 500, 4, 4, True, 3)])
def test_counts_chunks_equal_host_formed_ones(gpu_lib, n, d, dc, count, seed, directed, dense):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(n, d, seed, multi_frac=0.05, dense_loops=dense, directed=directed)
    rng = np.random.default_rng(seed)
    subs = [rng.permutation(d)[:dc] for _ in range(count)]
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=40, tie="hash", seed=2)
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    got = m.solve_chunks(subs, workers=4, group=3, **cfg)
    m.close()
    host, want = host_solve(x, ptr, idx, eb, counts, subs, **cfg)
    for g, w, (_, nei, fam) in zip(got, want, host):
        same_run(g, w, fam)
        assert g["nnz"] == len(nei[1])
    # the counts matter: weights and criteria of the presence rule differ
    plain, want0 = host_solve(x, ptr, idx, eb, None, subs, **cfg)
    assert any(not np.array_equal(h[1][2], p[1][2]) for h, p in zip(host, plain))
    assert any(not np.array_equal(g["crit"], w0["crit"]) for g, w0 in zip(got, want0))


def test_counts_of_one_are_the_bits_only_master(gpu_lib):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb = synth.master_pangenome(3000, 200, 6)
    ones = (np.zeros(len(idx) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    rng = np.random.default_rng(6)
    subs = [rng.permutation(200)[:60] for _ in range(6)]
    cfg = dict(algo="ncem", beta=0.5, disper="skd", it_max=40, tie="libc", seed=3)
    a, b = Master(x, ptr, idx, eb), Master(x, ptr, idx, eb, edge_counts=ones)
    ga, gb = a.solve_chunks(subs, workers=2, group=4, **cfg), b.solve_chunks(subs, workers=2, group=4, **cfg)
    a.close(); b.close()
    for u, v in zip(ga, gb):
        for key in ("families", "labels", "prop", "center", "disp", "nbobs_k", "crit", "iters", "status", "nnz"):
            assert np.array_equal(u[key], v[key], equal_nan=True), key


def test_coverage_above_65535(gpu_lib):
    """500 organisms that carry one adjacency 200 times each: weight 100 000 (a 16-bit coverage stops at 65 535); a
    small beta keeps beta * w below exp's overflow, so the criteria see the difference"""
    from pangenomenem_amd.batch import solve_many
    from pangenomenem_amd.chunks import Master, form_chunk_host
    n, d = 400, 500
    x, (ptr, idx), eb = synth.master_pangenome(n, d, 12)
    x = x.copy()
    x[:2] = 1
    heavy = [e for i in (0, 1) for e in range(ptr[i], ptr[i + 1]) if idx[e] == 1 - i]
    assert len(heavy) == 2
    eb = eb.copy()
    eb[heavy] = 0
    eb[heavy, :d // 32] = 0xFFFFFFFF
    eb[heavy, d // 32] = (1 << (d % 32)) - 1
    per = np.zeros(len(idx), np.int64)
    per[heavy] = d
    xptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    counts = (xptr, np.tile(np.arange(d, dtype=np.int32), 2), np.full(2 * d, 200, np.int32))
    sub = np.random.default_rng(1).permutation(d)
    cfg = dict(algo="ncem", beta=1e-3, disper="sk_", it_max=30, tie="hash", seed=1)
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    got = m.solve_chunks([sub], workers=1, group=1, **cfg)[0]
    m.close()
    xc, nei, fam = form_chunk_host(x, ptr, idx, eb, sub, edge_counts=counts)
    assert nei[2].max() == 100000.0
    clamped = (nei[0], nei[1], np.minimum(nei[2], 65535.0))
    init = synth.default_init(d)
    want, want16 = solve_many([(xc, nei, 3) + init, (xc, clamped, 3) + init], workers=1, group=1, **cfg)
    same_run(got, want, fam)
    assert not np.array_equal(want["crit"], want16["crit"])


@pytest.mark.parametrize("tie,directed,batch", [("hash", False, 64), ("libc", True, 7)])
def test_partition_of_a_counts_master_equals_host_loop(gpu_lib, tie, directed, batch):
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(3000, 300, 5, multi_frac=0.05, dense_loops=2, directed=directed)
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    rng_h, rng_d = random.Random(3), random.Random(3)
    want = host_partition(x, ptr, idx, eb, counts, np.arange(300), 50, rng_h, tie, 1)
    got, cnt, samples = m.partition(chunk_size=50, rng=rng_d, batch=batch, tie=tie, seed=1)
    m.close()
    fin = vote_final(want)
    assert samples == want["samples"] > 10
    assert np.array_equal(cnt, want["cnt"])
    assert got == {"fam%d" % (i + 1): CODES[fin[i]] for i in np.flatnonzero(want["pan"])}
    assert rng_d.getstate() == rng_h.getstate()


def test_partition_of_a_counts_master_single_run(gpu_lib):
    """no more organisms than chunk_size: one run on exactly them"""
    from pangenomenem_amd.chunks import Master
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(3000, 300, 7, multi_frac=0.1, dense_loops=2, directed=True)
    organisms = np.random.default_rng(6).permutation(300)[:45]
    m = Master(x, ptr, idx, eb, edge_counts=counts)
    rng = random.Random(8)
    before = rng.getstate()
    got, cnt, samples = m.partition(organisms=organisms, chunk_size=50, rng=rng, tie="libc", seed=1)
    m.close()
    assert samples == 1 and rng.getstate() == before
    host, (r,) = host_solve(x, ptr, idx, eb, counts, [organisms], algo="ncem", beta=0.5, disper="sk_", it_max=100, tie="libc", seed=1)
    fam = host[0][2]
    want, _ = partition_dicts(r, ["fam%d" % (i + 1) for i in fam])
    assert got == want


class RecordedGraph:
    """a recorded graph (tests/golden/nei_counts) behind the networkx calls master_arrays_from_graph makes"""

    def __init__(self, rec):
        self._directed = rec["directed"]
        self._nodes = {f: dict(data) for f, data in rec["nodes"]}
        self._succ = {f: {} for f in self._nodes}
        self.pred = {f: {} for f in self._nodes} if self._directed else self._succ
        for a, b, data in rec["edges"]:
            self._succ[a][b] = data
            (self.pred[b] if self._directed else self._succ[b])[a] = data

    def nodes(self, data=False):
        return list(self._nodes.items()) if data else list(self._nodes)

    def is_directed(self):
        return self._directed

    def __getitem__(self, a):
        return self._succ[a]


def test_from_graph_equals_hand_built_arrays(gpu_lib):
    """digraph6: six families of six organisms; the arrays written out by hand from the recorded graph (a family's
    predecessors, then its other successors; sens + antisens; a self-loop twice)"""
    from pangenomenem_amd.chunks import Master
    rec = json.load(open(os.path.join(GOLDEN, "digraph6.json")))
    orgs = ["org%d" % k for k in range(1, 7)]
    fams = [f for f, _ in rec["nodes"]]
    col, fi = {o: c for c, o in enumerate(orgs)}, {f: i for i, f in enumerate(fams)}
    x = np.array([[1 if o in data else 0 for o in orgs] for _, data in rec["nodes"]], np.uint8)
    succ = {f: {} for f in fams}
    pred = {f: {} for f in fams}
    for a, b, data in rec["edges"]:
        succ[a][b] = data
        pred[b][a] = data
    ptr, idx, bits, xptr, xorg, xcnt = [0], [], [], [0], [], []
    for a in fams:
        for b in list(pred[a]) + [b for b in succ[a] if b not in pred[a]]:
            c = np.zeros(len(orgs), np.int64)
            for u, v in ((a, b), (b, a)):
                for key, val in succ[u].get(v, {}).items():
                    if key in col:
                        c[col[key]] += val
            idx.append(fi[b])
            bits.append(sum(1 << o for o in range(len(orgs)) if c[o] >= 1))
            for o in range(len(orgs)):
                if c[o] >= 2:
                    xorg.append(o)
                    xcnt.append(c[o])
            xptr.append(len(xorg))
        ptr.append(len(idx))
    eb = np.array(bits, np.uint32)[:, None]
    counts = (np.array(xptr, np.int32), np.array(xorg, np.int32), np.array(xcnt, np.int32))
    assert max(xcnt) >= 4
    a = Master.from_graph(RecordedGraph(rec), organisms=orgs)
    b = Master(x, np.array(ptr, np.int32), np.array(idx, np.int32), eb, edge_counts=counts)
    assert a.names == fams and a.organism_names == orgs
    for tie in ("hash", "libc"):
        pa, ca, sa = a.partition(tie=tie, seed=1)
        pb, cb, sb = b.partition(tie=tie, seed=1, names=fams)
        assert pa == pb and sa == sb == 1 and np.array_equal(ca, cb)
        assert sorted(pa) == sorted(fams)
    a.close(); b.close()
