"""Edge weights as occurrence counts: chunks.master_arrays_from_graph and form_chunk_host(edge_counts=...) against the
`.index` / `.dat` / `.nei` that the reference's own __write_nem_input_files wrote for small graphs built through its
own __add_link (tests/golden/nei_counts/, made by tests/golden/make_nei_counts.py), against a dict transcription of
ppanggolin.py:858-878 on synthetic counts masters, and the host checks of nemgpu_master_create_counts."""
import ctypes as C
import glob
import json
import os
import re
from collections import Counter

import numpy as np
import pytest

from pangenomenem_amd import synth
from pangenomenem_amd.chunks import RESERVED_WORDS, form_chunk_host, master_arrays_from_graph, pack_rows

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nei_counts", "*.json")))


class RecordedGraph:
    """the part of a networkx Graph / DiGraph that master_arrays_from_graph reads, rebuilt from a recorded graph"""

    def __init__(self, rec):
        self._directed = rec["directed"]
        self._nodes = {f: dict(data) for f, data in rec["nodes"]}
        self._succ = {f: {} for f in self._nodes}
        self.pred = {f: {} for f in self._nodes} if self._directed else self._succ
        for a, b, data in rec["edges"]:
            self._succ[a][b] = data
            if self._directed:
                self.pred[b][a] = data
            else:
                self._succ[b][a] = data

    def nodes(self, data=False):
        return list(self._nodes.items()) if data else list(self._nodes)

    def is_directed(self):
        return self._directed

    def __getitem__(self, a):
        return self._succ[a]


def parse_nei(text):
    """{family index (1-based): Counter of (neighbour index, weight)} of a .nei"""
    lines = text.strip().split("\n")
    assert lines[0] == "1"
    out = {}
    for line in lines[1:]:
        f = line.split("\t")
        i, k = int(f[0]), int(f[1])
        out[i] = Counter(zip((int(v) for v in f[2:2 + k]), (float(v) for v in f[2 + k:2 + 2 * k])))
    return out


def chunk_matches(rec_sample, arrays, organisms, edge_counts):
    """does the host-formed sample equal the reference's files?  (index order, .dat rows, .nei multisets)"""
    x, (ptr, idx), eb, _, families, orgs = arrays
    col = [orgs.index(o) for o in rec_sample["organisms"]]
    xc, (pc, ic, wc), fam = form_chunk_host(x, ptr, idx, eb, col, edge_counts=edge_counts)
    index = [line.split("\t")[1] for line in rec_sample["index"].strip().split("\n")]
    if [families[i] for i in fam] != index:
        return False
    dat = np.array([[int(v) for v in line.split("\t")] for line in rec_sample["dat"].strip().split("\n")], np.uint8)
    if not np.array_equal(xc, dat):
        return False
    nei = parse_nei(rec_sample["nei"])
    got = {j + 1: Counter(zip((ic[pc[j]:pc[j + 1]] + 1).tolist(), wc[pc[j]:pc[j + 1]].astype(float).tolist())) for j in range(len(fam))}
    return got == nei


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-5] for p in FIXTURES])
def test_graph_arrays_reproduce_the_reference_writer(path):
    rec = json.load(open(path))
    g = RecordedGraph(rec)
    arrays = master_arrays_from_graph(g)
    x, (ptr, idx), eb, counts, families, orgs = arrays
    assert families == [f for f, _ in rec["nodes"]]
    assert not set(orgs) & RESERVED_WORDS and any(set(d) & RESERVED_WORDS for _, d in rec["nodes"])
    assert any(idx[e] == i for i in range(len(families)) for e in range(ptr[i], ptr[i + 1]))   # (self-loops)
    assert len(counts[1]) > 0                                                                      # (counts >= 2)
    presence_ok = []
    for s in rec["samples"]:
        assert chunk_matches(s, arrays, s["organisms"], counts), s["organisms"]
        presence_ok.append(chunk_matches(s, arrays, s["organisms"], None))
    assert not all(presence_ok)                               # the presence rule is not the reference's


def test_fixtures_cover_both_graph_kinds():
    kinds = {json.load(open(p))["directed"] for p in FIXTURES}
    assert kinds == {False, True} and len(FIXTURES) >= 4


def test_graph_neighbour_order_and_directed_counts():
    """a DiGraph: predecessors first, then the other successors; sens + antisens; a self-loop twice"""
    rec = dict(directed=True, nodes=[["A", {"o1": 1, "o2": 1, "name": 0}], ["B", {"o1": 1}], ["C", {"o2": 1, "length": 1}]],
               edges=[["A", "B", {"o1": 2, "weight": 1.0}], ["C", "A", {"o2": 1}], ["B", "A", {"o1": 1}], ["A", "A", {"o2": 3}]])
    x, (ptr, idx), eb, (xp, xo, xc), fam, orgs = master_arrays_from_graph(RecordedGraph(rec))
    assert fam == ["A", "B", "C"] and orgs == ["o1", "o2"]
    assert np.array_equal(x, [[1, 1], [1, 0], [0, 1]])
    assert ptr.tolist() == [0, 3, 4, 5] and idx.tolist() == [2, 1, 0, 0, 0]
    assert eb[:, 0].tolist() == [2, 1, 2, 1, 2]
    counts = {(e, int(o)): int(c) for e in range(len(idx)) for o, c in zip(xo[xp[e]:xp[e + 1]], xc[xp[e]:xp[e + 1]])}
    assert counts == {(1, 0): 3, (2, 1): 6, (3, 0): 3}
    x2, _, _, _, _, orgs2 = master_arrays_from_graph(RecordedGraph(rec), organisms=["o2"])
    assert orgs2 == ["o2"] and x2[:, 0].tolist() == [1, 0, 1]


def by_the_book_counts(x, ptr, idx, edge_bits, edge_counts, organisms):
    """ppanggolin.py:843-878 on a dict graph: node_organisms per family, graph[i][j] = {organism: count} per directed
    master edge (a directed graph's sens + antisens already summed into it), coverage = sum(pre_abs ...)"""
    n, d = x.shape
    xp, xo, xc = edge_counts
    graph = {}
    for i in range(n):
        for e in range(ptr[i], ptr[i + 1]):
            carried = np.flatnonzero(np.unpackbits(edge_bits[e].view(np.uint8), bitorder="little")[:d]).tolist()
            pre = {o: 1 for o in carried}
            for t in range(xp[e], xp[e + 1]):
                pre[int(xo[t])] = int(xc[t])
            graph.setdefault(i, {})[int(idx[e])] = pre
    orgs = [int(o) for o in organisms]
    index_fam, rows = {}, []
    for i in range(n):
        node_organisms = set(np.flatnonzero(x[i]).tolist())
        if not set(orgs).isdisjoint(node_organisms):
            rows.append([1 if o in node_organisms else 0 for o in orgs])
            index_fam[i] = len(index_fam)
    nei = []
    for i in index_fam:
        row = []
        for j, pre in graph.get(i, {}).items():
            coverage = sum([pre_abs for org, pre_abs in pre.items() if org in orgs])
            if coverage == 0 or j not in index_fam:
                continue
            row.append((index_fam[j], float(coverage)))
        nei.append(row)
    return np.array(rows, np.uint8), nei, list(index_fam)


@pytest.mark.parametrize("n,d,dc,seed,directed,dense", [(300, 70, 20, 1, False, 0), (257, 100, 7, 3, True, 2), (400, 33, 33, 2, True, 0),
                                                        (200, 130, 64, 5, False, 3)])
def test_host_formation_with_counts_follows_the_reference_recipe(n, d, dc, seed, directed, dense):
    x, (ptr, idx), eb, counts = synth.master_pangenome_counts(n, d, seed, multi_frac=0.1, dense_loops=dense, directed=directed,
                                                            chord_frac=0.3)
    rng = np.random.default_rng(seed)
    differs = 0
    for _ in range(3):
        org = rng.permutation(d)[:dc]
        xc, (pc, ic, wc), fam = form_chunk_host(x, ptr, idx, eb, org, edge_counts=counts)
        rows, nei, index_fam = by_the_book_counts(x, ptr, idx, eb, counts, org)
        assert fam.tolist() == index_fam and np.array_equal(xc, rows)
        for j, row in enumerate(nei):
            assert list(zip(ic[pc[j]:pc[j + 1]].tolist(), wc[pc[j]:pc[j + 1]].tolist())) == row, j
        _, (_, _, w1), _ = form_chunk_host(x, ptr, idx, eb, org)
        differs += int(not np.array_equal(w1, wc))
    assert differs > 0


def test_master_pangenome_counts_keeps_the_bits_master():
    """the counts generator adds self-loops and counts to master_pangenome's adjacencies, not other organisms"""
    x0, (p0, i0), e0 = synth.master_pangenome(300, 70, 4)
    x, (ptr, idx), eb, (xp, xo, xc) = synth.master_pangenome_counts(300, 70, 4, dense_loops=1)
    assert np.array_equal(x, x0)
    src = np.repeat(np.arange(300), np.diff(ptr))
    loop = src == idx
    assert loop.sum() >= 2 and np.array_equal(idx[~loop], i0) and np.array_equal(eb[~loop], e0)
    assert (xc >= 2).all() and len(xo) == xp[-1]


# ---- nemgpu_master_create_counts: the host checks (before any HIP call)

E_ARG, E_DEVICE = 3, 9                                        # NEMGPU_E_ARG, NEMGPU_E_DEVICE (include/nem_mi355x.h)

@pytest.fixture(scope="module")
def lib():
    from pangenomenem_amd import build, engine
    build.build()
    lib = engine.load_library()
    lib.nemgpu_master_create_counts.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    lib.nemgpu_master_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_master_destroy.restype = None
    return lib


def create(lib, x, ptr, idx, eb, xp, xo, xc):
    rows = pack_rows(x)
    arrs = [None if a is None else np.ascontiguousarray(a, t)
            for a, t in ((ptr, np.int32), (idx, np.int32), (eb, np.uint32), (xp, np.int32), (xo, np.int32), (xc, np.int32))]
    h = C.c_void_p()
    rc = lib.nemgpu_master_create_counts(C.byref(h), 0, x.shape[0], x.shape[1], rows.ctypes.data,
                                         *[a.ctypes.data if a is not None and a.size else None for a in arrs])
    if h.value:
        lib.nemgpu_master_destroy(h)
    return rc, lib.nemgpu_last_error().decode()


def test_master_create_counts_checks_its_arguments(lib):
    from pangenomenem_amd import engine
    x = np.ones((3, 40), np.uint8)
    ptr, idx = [0, 2, 3, 4], [1, 0, 0, 2]                     # 0->1, 0->0, 1->0, 2->2
    eb = np.zeros((4, 2), np.uint32)
    eb[:, 0] = 0b1011
    eb[1, 1] = 1 << 3                                         # (organism 35 carries the self-loop)
    good = ([0, 1, 3, 3, 3], [1, 0, 35], [2, 3, 5])
    bad = [(([1, 1, 3, 3, 3], good[1], good[2]), "extra_ptr\\[0\\]"),
           (([0, 2, 1, 3, 3], [1, 0, 35], [2, 3, 5]), "monotone"),
           (([0, 1, 3, 3, 3], [1, 35, 0], [2, 3, 5]), "increasing"),
           (([0, 1, 3, 3, 3], [1, 0, 0], [2, 3, 5]), "increasing"),
           (([0, 1, 3, 3, 3], [1, 0, 40], [2, 3, 5]), "out of range"),
           (([0, 1, 3, 3, 3], [-1, 0, 35], [2, 3, 5]), "out of range"),
           (([0, 1, 3, 3, 3], [2, 0, 35], [2, 3, 5]), "edge_bits"),
           (([0, 1, 3, 3, 3], [1, 0, 35], [1, 3, 5]), "below 2"),
           (([0, 1, 3, 3, 3], [1, 0, 35], [2, 3, -4]), "below 2"),
           (([0, 1, 3, 3, 3], [1, 0, 35], [2, (1 << 24) - 3, 2]), "2\\^24")]     # (4 carriers + 2^24 - 4 + 1)
    for (xp, xo, xc), what in bad:
        rc, msg = create(lib, x, ptr, idx, eb, xp, xo, xc)
        assert rc == E_ARG and re.search(what, msg), (xp, xo, xc, rc, msg)
    # well-formed (the second: a total of exactly 2^24, still exact) -- past the checks: a master, or no device
    want = 0 if engine.device_count() > 0 else E_DEVICE
    assert create(lib, x, ptr, idx, eb, *good)[0] == want
    assert create(lib, x, ptr, idx, eb, good[0], good[1], [2, (1 << 24) - 4, 2])[0] == want
    assert create(lib, x, ptr, idx, eb, None, [], [])[0] == want
