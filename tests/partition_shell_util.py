"""What tests/test_partition_shell_host.py and tests/test_gpu_partition_shell.py share: the records of
tests/golden/partition_shell/ (made by tests/golden/make_partition_shell.py from the reference's own partition_shell(),
its own writer and the compiled reference's random starts), a fixture's numpy master and selection, the writer's files as
arrays, and synthetic masters with selections at the shapes where the kernels can go wrong."""
import glob
import gzip
import json
import os
from collections import Counter, OrderedDict

import numpy as np

from pangenomenem_amd.shell import form_subproblem_host
from tests.projection_util import fixture_master_host

HERE = os.path.dirname(os.path.abspath(__file__))
SHELL_FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "partition_shell", "*.json.gz")))
SHELL_IDS = [os.path.basename(p)[:-8] for p in SHELL_FIXTURES]
REF_SEED = 20271019                                           # make_partition_shell.py's
REF_QS = (2, 4, 7)
TOL = 1e-6                                                    # tests/test_gpu_parity.py's rule: labels exact, parameters within 1e-6

_cache = {}


def load(path):
    """a fixture's record with its numpy master, family names and selection, read once"""
    if path not in _cache:
        with gzip.open(path, "rb") as f:
            rec = json.loads(f.read())
        m, _, names = fixture_master_host(rec)
        rec["master"], rec["names"] = m, names
        rec["everyone"] = rec["organisms"] + rec["new_organisms"]
        rec["select"] = np.asarray([rec["labels"][f] == "S" for f in names], bool)
        npz = path[:-8] + ".npz"
        rec["ref"] = dict(np.load(npz)) if os.path.isfile(npz) else None
        _cache[path] = rec
    return _cache[path]


def host_problem(rec, edges="induced", organisms=None):
    """form_subproblem_host on a fixture's master, all organisms in column order by default"""
    m = rec["master"]
    organisms = np.arange(m[0].shape[1]) if organisms is None else organisms
    return form_subproblem_host(m[0], m[1][0], m[1][1], m[2], organisms, rec["select"], m[3], edges)


def parse_files(files):
    """the writer's files as (family names in index order, x uint8 [n][d], {1-based family: Counter of (1-based neighbour,
    weight)}, (n, d) of the .str)"""
    index = [line.split("\t")[1] for line in files["index"].strip().split("\n")] if files["index"].strip() else []
    dat = np.array([[int(v) for v in line.split("\t")] for line in files["dat"].strip().split("\n")], np.uint8) if files["dat"].strip() else None
    lines = files["nei"].strip().split("\n")
    assert lines[0] == "1"
    nei = {}
    for line in lines[1:]:
        f = line.split("\t")
        i, k = int(f[0]), int(f[1])
        nei[i] = Counter(zip((int(v) for v in f[2:2 + k]), (float(v) for v in f[2 + k:2 + 2 * k])))
    shape = tuple(int(v) for v in files["str"].split()[1:3])
    return index, dat, nei, shape


def nei_sets(ptr, idx, w):
    """a CSR graph as parse_files gives a .nei: neighbour sets per row (the reference walks a set)"""
    return {j + 1: Counter(zip((idx[ptr[j]:ptr[j + 1]] + 1).tolist(), np.asarray(w[ptr[j]:ptr[j + 1]], float).tolist())) for j in range(len(ptr) - 1)}


def init_of(recorded):
    """a recorded init_using_qual back as partition_shell takes it"""
    if recorded is None:
        return None
    if "dict" in recorded:
        return OrderedDict((k, set(v)) for k, v in recorded["dict"])
    return [set(v) for v in recorded["list"]]


def parse_m(text, Q, d):
    """a `.m` as ReadParamFile reads it: (the Q - 1 written proportions, center [Q][d], disp [Q][d])"""
    v = text.split()
    assert v[0] == "1" and len(v) == 1 + (Q - 1) + 2 * Q * d
    head = [float(t) for t in v[1:Q]]
    rest = np.asarray([float(t) for t in v[Q:]], np.float32)
    return head, rest[:Q * d].reshape(Q, d), rest[Q * d:].reshape(Q, d)


def grouped_matrix(seed=3, d=24, per=40):
    """x uint8 [4 * per][d] for the inits of partition_shell: three groups of organisms (the last organism in none), `per`
    families typical of each (4 % of the cells flipped) and `per` families in a random half of the organisms.
    Returns x and the groups (ranges of columns)."""
    rng = np.random.default_rng(seed)
    groups = [range(0, d // 3), range(d // 3, 2 * (d // 3)), range(2 * (d // 3), d - 1)]
    n = 4 * per
    x = np.zeros((n, d), np.uint8)
    for g, orgs in enumerate(groups):
        x[g * per:(g + 1) * per, list(orgs)] = 1
    x[3 * per:] = rng.random((per, d)) < 0.5
    x ^= (rng.random((n, d)) < 0.04).astype(np.uint8)
    x[np.arange(n), rng.integers(0, d, n)] = 1
    return x, groups


def synthetic_master(n, d, seed, loops=False, extras=(), density=0.5, x=None):
    """arrays of a random counts master: x uint8 [n][d] (a few families in no organism of the first half), a graph of a
    path plus random chords (symmetric; with loops: a few self-loops), edge organism sets inside both ends' organisms,
    and extras: one list of multi-copy pairs per length in `extras` (capped by the edge's organisms).  x: the matrix to
    use instead of a random one.  Returns x, ptr, idx, edge_bits, edge_counts."""
    rng = np.random.default_rng(seed)
    if x is None:
        x = (rng.random((n, d)) < density).astype(np.uint8)
        x[np.arange(n), rng.integers(0, d, n)] = 1
    pairs = {(i, i + 1) for i in range(n - 1)} | {tuple(sorted(p)) for p in rng.integers(0, n, (n // 2, 2)).tolist() if p[0] != p[1]}
    if n > 4:
        pairs -= {(2, 3), (3, 4), (1, 2)}                     # (family 2 and 3 lose their path edges: low or zero degree)
        pairs = {p for p in pairs if 3 not in p}              # family 3 has degree 0
    if loops:
        pairs |= {(i, i) for i in rng.integers(0, n, max(1, n // 8)).tolist() if i != 3}
    rows = [[] for _ in range(n)]
    for a, b in sorted(pairs):
        both = x[a] & x[b]
        if not both.any():
            continue
        orgs = both & (rng.random(d) < 0.8).astype(np.uint8)
        if not orgs.any():
            orgs = both
        rows[a].append((b, orgs))
        if a != b:
            rows[b].append((a, orgs))
    wf = (d + 31) // 32
    ptr, idx, bits = np.zeros(n + 1, np.int32), [], []
    for i, row in enumerate(rows):
        for b, orgs in row:
            idx.append(b)
            full = np.zeros(wf * 32, np.uint8)
            full[:d] = orgs
            bits.append(np.packbits(full, bitorder="little").view(np.uint32))
        ptr[i + 1] = len(idx)
    idx = np.asarray(idx, np.int32)
    eb = np.stack(bits) if bits else np.zeros((0, wf), np.uint32)
    nnz = len(idx)
    # extras: the longest lists go to the entries with the most organisms (symmetric entries get their own lists: the
    # master does not need the two directions to agree)
    xptr, xorg, xcnt = np.zeros(nnz + 1, np.int32), [], []
    if extras and nnz:
        popc = np.unpackbits(eb.view(np.uint8), axis=1).sum(axis=1)
        order = np.argsort(-popc, kind="stable")[:len(extras)]
        want = dict(zip(order.tolist(), extras))
        for e in range(nnz):
            if e in want:
                orgs = np.flatnonzero(np.unpackbits(eb[e].view(np.uint8), bitorder="little")[:d])[:want[e]]
                xorg += orgs.tolist()
                xcnt += (2 + rng.integers(0, 3, len(orgs))).tolist()
            xptr[e + 1] = len(xorg)
    return x, ptr, idx, eb, (xptr, np.asarray(xorg, np.int32), np.asarray(xcnt, np.int32))
