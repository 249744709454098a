"""The chunks of PPanGGOLiN's voting loop, formed on the device (the reference's real use).

``partition()`` solves a pangenome of more than 500 organisms as many NEM problems, each on a random sample of the
organisms (ppanggolin/ppanggolin.py:1045-1086: ``orgs = sample(organisms, chunck_size)``), and writes every sample's
input files from ONE graph (``__write_nem_input_files``, ppanggolin.py:821-930):

  * the matrix columns are the sampled organisms, in sample order (:850);
  * a family with no sampled organism is dropped, the others are numbered in the graph's order (:849-852);
  * an edge's weight is its ``coverage`` (:866-878): the sum over the sampled organisms of the adjacency's occurrence
    count in that organism (``graph[a][b][org]``, which ``__add_link`` increments, :451), sens + antisens
    (``graph[a][b][org] + graph[b][a][org]``) when the graph is directed; an edge of coverage 0 is dropped; a family's
    neighbours keep the order the master lists them in.

A master carries, per directed edge, the bit set of the organisms with count >= 1 (``edge_bits``) and, optionally,
``edge_counts = (extra_ptr, extra_org, extra_count)``: the (edge, organism) pairs whose count is 2 or more, in CSR over
the edges.  A bits-only master takes every count as 1, which is the reference's weight only where no adjacency occurs
twice in an organism (tandem duplicates, repeated operons and every edge of a directed graph do).
``master_arrays_from_graph`` / ``Master.from_graph`` take PPanGGOLiN's graph as it is and make the counts.

``Master.from_orders`` / ``Master.from_annotations`` build the same master on the device from the organisms' gene orders
(``nemgpu_master_create_orders``, csrc/nem_orders.hip): no graph, no networkx; ``master_arrays_from_orders`` is that build
in numpy.  ``Master.add_orders`` / ``Master.add_annotations`` grow a master by new organisms
(PPanGGOLiN.add_organism, ppanggolin.py:342-358) from their gene orders alone (``nemgpu_master_append_orders``);
``master_arrays_append_orders`` is that append in numpy.  ``Master.merge`` / ``Master.merge_named`` join two resident masters
(PPanGGOLiN.__iadd__, ppanggolin.py:368-391) from the masters alone (``nemgpu_master_merge``, csrc/nem_merge.hip);
``master_arrays_merge`` is that merge in numpy.

``Master`` puts that one pangenome on the device (``nemgpu_master_create[_counts]``); ``solve_chunks`` solves any number of
samples in ONE library call (``nemgpu_solve_chunks``): the device forms every sample's problem straight into its engine's
buffers, the lock-step pipeline of ``batch.solve_many`` runs them.  ``form_chunk_host`` is the same formation in numpy --
what the tests hold the device against (through ``batch.solve_many``) and what documents the index maps.

``Master.partition`` is the whole loop: the samples drawn as the reference draws them, solved ``batch`` at a time and
voted on the device (``nemgpu_votes_solve``: validate_family, ppanggolin.py:1015-1037) until every family is validated;
``partitioning.vote_host`` is the same vote in numpy.
"""
import ctypes as C
import random
from collections import defaultdict

import numpy as np

from .engine import ALGO, CVT, DISP, PROP, STATUS_OK, TIE, Config, NemGpuError, Result, load_library
from .projection import check_orders


class Chunk(C.Structure):
    """nemgpu_chunk (include/nem_mi355x.h)"""
    _fields_ = [("organisms", C.c_void_p), ("dc", C.c_int), ("n", C.c_int), ("nnz", C.c_int),
                ("keep", C.c_void_p), ("labels", C.c_void_p),
                ("out_prop", C.c_void_p), ("out_center", C.c_void_p), ("out_disp", C.c_void_p), ("out_nbobs_k", C.c_void_p),
                ("result", Result), ("rc", C.c_int)]


def pack_rows(x):
    """uint8 [n][d] of 0/1 -> uint32 bit rows [n][ceil(d/32)] (bit o of a row = column o)"""
    x = np.ascontiguousarray(x, np.uint8)
    n, d = x.shape
    wf = (d + 31) // 32
    rows = np.zeros((n, wf * 4), np.uint8)
    bits = np.packbits(x, axis=1, bitorder="little")
    rows[:, :bits.shape[1]] = bits
    return rows.view(np.uint32)


def _bind_master(lib):
    lib.nemgpu_master_create_orders.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.nemgpu_master_append_orders.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.nemgpu_master_merge.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.nemgpu_master_project.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.nemgpu_master_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
    lib.nemgpu_master_fetch.argtypes = [C.c_void_p] * 9
    lib.nemgpu_master_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nemgpu_master_create_counts.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nemgpu_master_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_master_destroy.restype = None
    lib.nemgpu_solve_chunks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(Config), C.c_int, C.c_int]
    return lib


def form_chunk_host(x, ptr, idx, edge_bits, organisms, edge_counts=None):
    """One sample's NEM problem the way __write_nem_input_files makes it (ppanggolin.py:821-930), in numpy.
    x: uint8 [n][d]; (ptr, idx): the master graph in CSR; edge_bits: uint32 [nnz][ceil(d/32)], the organisms that carry
    each directed edge (count >= 1); edge_counts: None (every count 1) or (extra_ptr, extra_org, extra_count), the
    pairs with count >= 2 (nemgpu_master_create_counts); organisms: the sample (column order).  An edge's weight is the
    sum of its counts over the sample.  Returns (x_chunk uint8 [n_c][d_c], (ptr_c, idx_c, w_c), families int64 [n_c]:
    the master index of the chunk's family j)."""
    x = np.asarray(x, np.uint8)
    organisms = np.asarray(organisms, np.int64)
    n, d = x.shape
    sub = x[:, organisms]
    keep = sub.any(axis=1)                                    # `not organisms.isdisjoint(node_organisms)`, :849
    families = np.flatnonzero(keep)
    renum = np.full(n, -1, np.int64)
    renum[families] = np.arange(len(families))                # index_fam, :851 (1-based there)
    mask = np.zeros(edge_bits.shape[1] * 32, np.uint8)
    mask[organisms] = 1
    mask_words = np.packbits(mask, bitorder="little").view(np.uint32)
    nnz = len(idx)
    cov = np.zeros(nnz, np.int64)
    if nnz:
        anded = np.bitwise_and(np.asarray(edge_bits, np.uint32), mask_words[None, :])
        cov = np.unpackbits(anded.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)     # coverage, :866-876
    if nnz and edge_counts is not None:
        extra_ptr, extra_org, extra_count = (np.asarray(a, np.int64) for a in edge_counts)
        edge_of = np.repeat(np.arange(nnz), np.diff(extra_ptr))
        np.add.at(cov, edge_of, (extra_count - 1) * mask[extra_org])      # the copies beyond the first
    src = np.repeat(np.arange(n), np.diff(ptr))
    ok = (cov > 0) & keep[src] & (renum[np.asarray(idx, np.int64)] >= 0) if nnz else np.zeros(0, bool)   # `if coverage == 0: continue`, :877
    deg = np.bincount(renum[src[ok]], minlength=len(families)) if nnz else np.zeros(len(families), np.int64)
    ptr_c = np.zeros(len(families) + 1, np.int32)
    ptr_c[1:] = np.cumsum(deg)
    idx_c = renum[np.asarray(idx, np.int64)[ok]].astype(np.int32)     # (rows stay in master order: src is sorted)
    w_c = cov[ok].astype(np.float32)
    return np.ascontiguousarray(sub[keep]), (ptr_c, idx_c, w_c), families


RESERVED_WORDS = frozenset(["id", "label", "name", "weight", "partition", "partition_exact", "length", "length_min", "length_max",
                            "length_avg", "length_med", "product", "nb_genes", "subpartition_shell", "viz"])   # ppanggolin.py:31


def master_arrays_from_graph(graph, organisms=None):
    """A master's arrays from PPanGGOLiN's neighbours graph as it builds it (a networkx Graph or DiGraph, read through
    nodes(data=True), graph[a], is_directed() and, when directed, graph.pred[a]; networkx itself is not needed):
    node data = organism name -> genes (plus RESERVED_WORDS attributes), edge data = organism name -> occurrence count
    (plus weight / length).  organisms: the master's organisms in column order (default: every non-reserved node key,
    in the order first met walking the nodes).  Keys that are not among them, reserved words included, are ignored.
    Families come in graph node order (index_fam's order, ppanggolin.py:843).  A family's neighbours are
    nx.all_neighbors, each once: for a Graph its adjacency in graph[a] order; for a DiGraph its predecessors in
    graph.pred[a] order, then its successors not already listed, in graph[a] order.  count[e][o] is graph[a][b][o],
    or graph[a][b][o] + graph[b][a][o] for a DiGraph (a directed self-loop counts twice), as the coverage sums them.
    Returns x uint8 [n][d], (ptr, idx), edge_bits uint32 [nnz][ceil(d/32)], edge_counts (extra_ptr, extra_org,
    extra_count: the pairs with count >= 2), family names, organism names."""
    nodes = list(graph.nodes(data=True))
    families = [f for f, _ in nodes]
    if organisms is None:
        seen = {}
        for _, data in nodes:
            for key in data:
                if key not in RESERVED_WORDS and key not in seen:
                    seen[key] = len(seen)
        organisms = list(seen)
    organisms = list(organisms)
    col = {o: c for c, o in enumerate(organisms)}
    if len(col) != len(organisms):
        raise ValueError("organisms: distinct names")
    fam_index = {f: i for i, f in enumerate(families)}
    n, d = len(families), len(organisms)
    wf = (d + 31) // 32
    x = np.zeros((n, d), np.uint8)
    for i, (_, data) in enumerate(nodes):
        for key in data:
            c = col.get(key)
            if c is not None and key not in RESERVED_WORDS:
                x[i, c] = 1
    directed = bool(graph.is_directed())

    def counts_of(a, b):
        out = defaultdict(int)
        pairs = [(a, b), (b, a)] if directed else [(a, b)]
        for u, v in pairs:
            if v in graph[u]:
                for key, val in graph[u][v].items():
                    c = col.get(key)
                    if c is not None and key not in RESERVED_WORDS:
                        out[c] += int(val)
        return out

    ptr = np.zeros(n + 1, np.int32)
    idx, bits, xptr, xorg, xcnt = [], [], [0], [], []
    for i, a in enumerate(families):
        nbrs = list(graph.pred[a]) + [b for b in graph[a] if b not in graph.pred[a]] if directed else list(graph[a])
        for b in nbrs:
            idx.append(fam_index[b])
            row = np.zeros(wf * 32, np.uint8)
            for c, k in sorted(counts_of(a, b).items()):
                if k >= 1:
                    row[c] = 1
                if k >= 2:
                    xorg.append(c)
                    xcnt.append(k)
            bits.append(np.packbits(row, bitorder="little").view(np.uint32))
            xptr.append(len(xorg))
        ptr[i + 1] = len(idx)
    edge_bits = np.stack(bits) if bits else np.zeros((0, wf), np.uint32)
    edge_counts = (np.asarray(xptr, np.int32), np.asarray(xorg, np.int32), np.asarray(xcnt, np.int32))
    return x, (ptr, np.asarray(idx, np.int32)), edge_bits, edge_counts, families, organisms


FAMILY = 1                  # index of the family in a gene's annotation (ppanggolin.py:25)


def orders_from_annotations(annotations, organisms, circular_contigs=(), repeated=(), family=FAMILY, families=()):
    """PPanGGOLiN's ``annotations`` ({organism: {contig: OrderedDict(gene -> info)}}, the family at info[family]) as the
    flat gene orders of nemgpu_master_create_orders.  organisms: the master's organisms in column order (every organism
    of annotations must be among them); circular_contigs: the contig names of circular_contig_size; repeated: the
    family names of families_repeted.  The walk is __neighborhood_computation's (ppanggolin.py:478-481): annotations'
    organisms, their contigs, their genes, each in dict order.  Returns a dict: genes int32 [G], contig_ptr int32
    [C + 1], contig_org int32 [C], contig_circular uint8 [C], repeated uint8 [F], d, families (the family name of every
    id, in order of first gene), organisms.  families: the names that have ids already (0, 1, ...: an earlier call's
    `families`, for the orders of an update -- Master.add_annotations); the new names follow them."""
    organisms = list(organisms)
    col = {o: c for c, o in enumerate(organisms)}
    if len(col) != len(organisms):
        raise ValueError("organisms: distinct names")
    circular_contigs = set(circular_contigs)
    fam_id = {name: i for i, name in enumerate(families)}
    genes, cptr, corg, circ = [], [0], [], []
    for org, contigs in annotations.items():
        if org not in col:
            raise ValueError("organism %r of the annotations is not among `organisms`" % (org,))
        for contig, annot in contigs.items():
            for info in annot.values():
                genes.append(fam_id.setdefault(info[family], len(fam_id)))
            cptr.append(len(genes))
            corg.append(col[org])
            circ.append(1 if contig in circular_contigs else 0)
    rep = np.zeros(max(len(fam_id), 1), np.uint8)
    for name in repeated:
        if name in fam_id:
            rep[fam_id[name]] = 1
    return dict(genes=np.asarray(genes, np.int32), contig_ptr=np.asarray(cptr, np.int32), contig_org=np.asarray(corg, np.int32),
                contig_circular=np.asarray(circ, np.uint8), repeated=rep, d=len(organisms), families=list(fam_id), organisms=organisms)


def _check_orders(genes, contig_ptr, contig_org, contig_circular, repeated, d, f):
    """the rules nemgpu_master_create_orders and nemgpu_master_append_orders refuse by"""
    return check_orders(genes, contig_ptr, contig_org, repeated, d, f, circular=contig_circular)


def master_arrays_from_orders(genes, contig_ptr, contig_org, contig_circular, d, repeated=None, f=None, directed=False):
    """The master that master_arrays_from_graph makes of the graph __neighborhood_computation (ppanggolin.py:463-530)
    builds, from the flat gene orders (nemgpu_master_create_orders' arguments; include/nem_mi355x.h), in numpy: the
    statement of what csrc/nem_orders.hip computes, step by step the same.
      * a gene of a repeated family does not exist; a gene's previous kept gene is the last kept one before it, if in its contig;
      * families in the order of their first kept gene;
      * a link per kept gene that has a previous one (time: its position + its contig's index), a link (first kept, last
        kept) per circular contig with a kept gene (time: the contig's end + its index);
      * a link (a, b) is the half-edges (row a, neighbour b) and (row b, neighbour a) -- one when a = b and the graph is
        undirected; in a DiGraph the first is a successor entry, the second a predecessor entry;
      * count[row, neighbour, organism] = its half-edges; a row's neighbours: those with a predecessor entry (always, for
        a Graph) by the first time of one, then the others by the first time of a successor entry.
    Returns x uint8 [n][d], (ptr, idx), edge_bits uint32 [nnz][ceil(d/32)], edge_counts (extra_ptr, extra_org,
    extra_count), order int32 [n] (master family i = caller id order[i]), range(d)."""
    genes, contig_ptr, contig_org, contig_circular, repeated, d, f = _check_orders(genes, contig_ptr, contig_org, contig_circular, repeated, d, f)
    g, c = len(genes), len(contig_org)
    wf = (d + 31) // 32
    pos = np.arange(g, dtype=np.int64)
    kept = np.ones(g, bool) if repeated is None else repeated[genes] == 0
    contig_of = np.repeat(np.arange(c, dtype=np.int64), np.diff(contig_ptr))
    last = np.maximum.accumulate(np.where(kept, pos, -1)) if g else pos
    prev = np.concatenate([[-1], last[:-1]]) if g else pos
    kp = np.flatnonzero(kept)
    fam_of, first = np.unique(genes[kp], return_index=True)
    order = fam_of[np.argsort(first, kind="stable")].astype(np.int32)
    n = len(order)
    newid = np.full(f, -1, np.int64)
    newid[order] = np.arange(n)
    x = np.zeros((n, d), np.uint8)
    x[newid[genes[kp]], contig_org[contig_of[kp]]] = 1
    cj = contig_of[kp]
    start, end = contig_ptr[cj].astype(np.int64), contig_ptr[cj + 1].astype(np.int64)
    linked = prev[kp] >= start
    closing = ~linked & (contig_circular[cj] != 0)
    has = linked | closing
    other = np.where(linked, prev[kp], last[np.maximum(end - 1, 0)])[has]
    t = np.where(linked, kp + cj, end + cj)[has]
    a, b, o = newid[genes[kp[has]]], newid[genes[other]], contig_org[cj[has]].astype(np.int64)
    if directed:
        row, nbr, org, key = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([o, o]), np.concatenate([t + (1 << 31), t])
    else:
        two = a != b
        row, nbr, org, key = np.concatenate([a, b[two]]), np.concatenate([b, a[two]]), np.concatenate([o, o[two]]), np.concatenate([t, t[two]])
    srt = np.lexsort((org, nbr, row))
    row, nbr, org, key = row[srt], nbr[srt], org[srt], key[srt]
    m = len(row)
    new_pair = np.ones(m, bool)
    new_pair[1:] = (row[1:] != row[:-1]) | (nbr[1:] != nbr[:-1]) | (org[1:] != org[:-1])
    new_edge = np.ones(m, bool)
    new_edge[1:] = (row[1:] != row[:-1]) | (nbr[1:] != nbr[:-1])
    pair_at, edge_at = np.flatnonzero(new_pair), np.flatnonzero(new_edge)
    pair_count = np.diff(np.append(pair_at, m))
    pair_edge = np.cumsum(new_edge)[pair_at] - 1
    nnz = len(edge_at)
    edge_first = np.minimum.reduceat(key, edge_at) if nnz else np.zeros(0, np.int64)
    perm = np.lexsort((edge_first, row[edge_at]))             # CSR entry e is edge perm[e]
    inv = np.empty(nnz, np.int64)
    inv[perm] = np.arange(nnz)
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(row[edge_at], minlength=n))
    idx = nbr[edge_at][perm].astype(np.int32)
    edge_bits = np.zeros((nnz, wf), np.uint32)
    entry = inv[pair_edge]
    np.bitwise_or.at(edge_bits, (entry, org[pair_at] >> 5), (np.uint32(1) << (org[pair_at] & 31).astype(np.uint32)))
    multi = pair_count >= 2
    xs = np.lexsort((org[pair_at][multi], entry[multi]))
    xptr = np.zeros(nnz + 1, np.int32)
    xptr[1:] = np.cumsum(np.bincount(entry[multi], minlength=nnz))
    edge_counts = (xptr, org[pair_at][multi][xs].astype(np.int32), pair_count[multi][xs].astype(np.int32))
    return x, (ptr, idx), edge_bits, edge_counts, order, list(range(d))


def master_arrays_append_orders(master_arrays, order, f_old, genes, contig_ptr, contig_org, contig_circular, d_new, repeated=None, f=None):
    """The master that master_arrays_from_graph makes of the nx.Graph after PPanGGOLiN.add_organism (ppanggolin.py:342-358:
    the graph kept, families_repeted united, __neighborhood_computation(update=new_orgs) walking the new organisms
    alone), from the old master's arrays and the new organisms' gene orders, in numpy: the statement of what
    nemgpu_master_append_orders computes.  master_arrays: (x uint8 [n][d], (ptr, idx), edge_bits, edge_counts, ...) of
    an undirected master; order int32 [n]: its family i is caller id order[i]; f_old: the id space it was made with;
    the orders as master_arrays_from_orders takes them with contig_org the ABSOLUTE columns d .. d + d_new - 1 and
    repeated [f] the union after the update (f >= f_old).
      * genes, links, times: master_arrays_from_orders' rules, undirected, on the update's genes;
      * an id in the master keeps its number (repeated only from now on: its node and old edges stay, its new genes do
        not exist); the other ids with a kept gene are numbered n, n + 1, ... by first kept gene;
      * an existing (row, neighbour) keeps its place in its row; a new one goes behind the row's old entries, by the first
        time among the update's records (nx.all_neighbors after add_edge);
      * count[entry, new organism] = its half-edges: >= 1 sets the bit (stride ceil((d + d_new) / 32)), >= 2 lists the
        count behind the entry's old extras; the old rows keep their bits, new families are absent from old organisms.
    Returns what master_arrays_from_orders returns: x, (ptr, idx), edge_bits, edge_counts, order (grown), range(d + d_new)."""
    x0 = np.asarray(master_arrays[0], np.uint8)
    ptr0, idx0 = (np.asarray(a, np.int64) for a in master_arrays[1])
    n0, d0 = x0.shape
    nnz0 = len(idx0)
    wf0 = (d0 + 31) // 32
    eb0 = np.asarray(master_arrays[2], np.uint32).reshape(nnz0, wf0)
    xptr0, xorg0, xcnt0 = (np.asarray(a, np.int64) for a in master_arrays[3])
    order0 = np.asarray(order, np.int64)
    if order0.shape != (n0,) or ptr0.shape != (n0 + 1,) or xptr0.shape != (nnz0 + 1,):
        raise ValueError("append: the master's arrays and its order [n]")
    if d_new <= 0:
        raise ValueError("append: d_new must be positive")
    d = d0 + int(d_new)
    if f is None and repeated is None:
        f = max(int(f_old), int(np.max(genes)) + 1 if len(genes) else 1)
    genes, contig_ptr, contig_org, contig_circular, repeated, d, f = _check_orders(genes, contig_ptr, contig_org, contig_circular, repeated, d, f)
    if f < f_old or (n0 and order0.max() >= f_old):
        raise ValueError("append: f may not be below the master's id space")
    if contig_org.min() < d0:
        raise ValueError("orders: contig organism out of range (a column of the old master)")
    g, c = len(genes), len(contig_org)
    wf = (d + 31) // 32
    pos = np.arange(g, dtype=np.int64)
    kept = np.ones(g, bool) if repeated is None else repeated[genes] == 0
    contig_of = np.repeat(np.arange(c, dtype=np.int64), np.diff(contig_ptr))
    last = np.maximum.accumulate(np.where(kept, pos, -1)) if g else pos
    prev = np.concatenate([[-1], last[:-1]]) if g else pos
    kp = np.flatnonzero(kept)
    # the numbering: the old one, then the ids it lacks by first kept gene
    newid = np.full(f, -1, np.int64)
    newid[order0] = np.arange(n0)
    fresh = kp[newid[genes[kp]] < 0]
    fam_of, first = np.unique(genes[fresh], return_index=True)
    added = fam_of[np.argsort(first, kind="stable")]
    n = n0 + len(added)
    newid[added] = n0 + np.arange(len(added))
    x = np.zeros((n, d), np.uint8)
    x[:n0, :d0] = x0
    x[newid[genes[kp]], contig_org[contig_of[kp]]] = 1
    # the update's half-edge records, as master_arrays_from_orders makes them
    cj = contig_of[kp]
    start, end = contig_ptr[cj].astype(np.int64), contig_ptr[cj + 1].astype(np.int64)
    linked = prev[kp] >= start
    closing = ~linked & (contig_circular[cj] != 0)
    has = linked | closing
    other = np.where(linked, prev[kp], last[np.maximum(end - 1, 0)])[has]
    t = np.where(linked, kp + cj, end + cj)[has]
    a, b, o = newid[genes[kp[has]]], newid[genes[other]], contig_org[cj[has]].astype(np.int64)
    two = a != b
    row, nbr, org, key = np.concatenate([a, b[two]]), np.concatenate([b, a[two]]), np.concatenate([o, o[two]]), np.concatenate([t, t[two]])
    srt = np.lexsort((org, nbr, row))
    row, nbr, org, key = row[srt], nbr[srt], org[srt], key[srt]
    m = len(row)
    new_pair = np.ones(m, bool)
    new_pair[1:] = (row[1:] != row[:-1]) | (nbr[1:] != nbr[:-1]) | (org[1:] != org[:-1])
    new_edge = np.ones(m, bool)
    new_edge[1:] = (row[1:] != row[:-1]) | (nbr[1:] != nbr[:-1])
    pair_at, edge_at = np.flatnonzero(new_pair), np.flatnonzero(new_edge)
    pair_count = np.diff(np.append(pair_at, m))
    pair_edge = np.cumsum(new_edge)[pair_at] - 1
    erow, enbr = row[edge_at], nbr[edge_at]
    edge_first = np.minimum.reduceat(key, edge_at) if len(edge_at) else np.zeros(0, np.int64)
    # every edge of the update in its old row, or new
    row0 = np.repeat(np.arange(n0, dtype=np.int64), np.diff(ptr0))
    okey = row0 * n + idx0
    by = np.argsort(okey, kind="stable")
    at = np.searchsorted(okey[by], erow * n + enbr)
    found = np.zeros(len(edge_at), bool)
    inside = at < nnz0
    found[inside] = okey[by][at[inside]] == (erow * n + enbr)[inside]
    oldpos = np.where(found, by[np.minimum(at, max(nnz0 - 1, 0))] if nnz0 else 0, -1)
    deg0 = np.zeros(n, np.int64)
    deg0[:n0] = np.diff(ptr0)
    grown = np.bincount(erow[~found], minlength=n)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg0 + grown)
    nnz = int(ptr[-1])
    fwd = ptr[row0] + (np.arange(nnz0) - ptr0[row0])          # old entry t -> its entry now
    perm = np.lexsort((edge_first, erow))
    fresh_e = perm[~found[perm]]                              # the new edges by (row, first time)
    rank = np.arange(len(fresh_e)) - (np.cumsum(grown) - grown)[erow[fresh_e]]
    entry = np.empty(len(edge_at), np.int64)
    entry[found] = fwd[oldpos[found]]
    entry[fresh_e] = ptr[erow[fresh_e]] + deg0[erow[fresh_e]] + rank
    idx = np.empty(nnz, np.int32)
    idx[fwd] = idx0
    idx[entry[fresh_e]] = enbr[fresh_e]
    edge_bits = np.zeros((nnz, wf), np.uint32)
    if nnz0:
        keep = eb0.copy()
        if d0 & 31:
            keep[:, -1] &= np.uint32((1 << (d0 & 31)) - 1)    # (the bits above the last old organism are not data)
        edge_bits[fwd, :wf0] = keep
    pe = entry[pair_edge]
    np.bitwise_or.at(edge_bits, (pe, org[pair_at] >> 5), (np.uint32(1) << (org[pair_at] & 31).astype(np.uint32)))
    # the extras: an entry's old ones, then the update's (every new column is larger than every old one)
    multi = pair_count >= 2
    xe = np.concatenate([fwd[np.repeat(np.arange(nnz0), np.diff(xptr0))], pe[multi]])
    xo = np.concatenate([xorg0, org[pair_at][multi]])
    xc = np.concatenate([xcnt0, pair_count[multi]])
    xs = np.lexsort((xo, xe))
    xptr = np.zeros(nnz + 1, np.int32)
    xptr[1:] = np.cumsum(np.bincount(xe, minlength=nnz))
    edge_counts = (xptr, xo[xs].astype(np.int32), xc[xs].astype(np.int32))
    grown_order = np.concatenate([order0, added]).astype(np.int32)
    return x, (ptr.astype(np.int32), idx), edge_bits, edge_counts, grown_order, list(range(d))


def master_arrays_merge(a_arrays, order_a, b_arrays, ids_b):
    """The master that master_arrays_from_graph makes of the union of two nx.Graphs, had B's organisms been walked after
    A's (PPanGGOLiN.__iadd__, ppanggolin.py:368-391, which rebuilds the graph from both pangenomes' annotations), from the
    two masters' arrays alone, in numpy: the statement of what nemgpu_master_merge computes.  a_arrays, b_arrays:
    (x uint8 [n][d], (ptr, idx), edge_bits, edge_counts, ...) of undirected masters with known counts; order_a int [n_a]:
    A's family i is caller id order_a[i]; ids_b int [n_b]: the id of B's family j in A's id space (distinct).
      * organisms: A's columns 0 .. d_a - 1, then B's in B's order as d_a .. d_a + d_b - 1;
      * families: A's keep their numbers; B's whose id A lacks are numbered n_a, n_a + 1, ... in B's order;
      * an entry (row, neighbour) of A keeps its place; an entry of B whose (mapped row, mapped neighbour) A lacks goes
        behind the row's A entries, in the order B's row lists them; a row new in B is B's row, mapped;
      * edge_bits (stride ceil((d_a + d_b) / 32)): A's bits below d_a, B's bits d_a further up; the extras A's, then B's
        with organism + d_a, counts unchanged; an entry's total count (A's + B's) may not exceed 2^24;
      * presence: A's rows, B's with their families mapped; absent elsewhere.
    It equals master_arrays_from_orders of A's orders followed by B's only when both were built with the same repeated
    families: a family repeated in one part alone keeps the node and the edges the other part gave it.
    Returns what master_arrays_from_orders returns: x, (ptr, idx), edge_bits, edge_counts, order (grown), range(d_a + d_b)."""
    def parts(m):
        x = np.asarray(m[0], np.uint8)
        ptr, idx = (np.asarray(v, np.int64) for v in m[1])
        n, d = x.shape
        eb = np.ascontiguousarray(m[2], np.uint32).reshape(len(idx), (d + 31) // 32)
        xptr, xorg, xcnt = (np.asarray(v, np.int64) for v in m[3])
        if ptr.shape != (n + 1,) or xptr.shape != (len(idx) + 1,) or len(xorg) != len(xcnt):
            raise ValueError("merge: a master's arrays")
        bits = np.unpackbits(eb.view(np.uint8), axis=1, bitorder="little")[:, :d] if len(idx) else np.zeros((0, d), np.uint8)
        return x, ptr, idx, bits, xptr, xorg, xcnt, np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))

    xa, ptr_a, idx_a, bits_a, xptr_a, xorg_a, xcnt_a, row_a = parts(a_arrays)
    xb, ptr_b, idx_b, bits_b, xptr_b, xorg_b, xcnt_b, row_b = parts(b_arrays)
    (n_a, d_a), (n_b, d_b) = xa.shape, xb.shape
    nnz_a, nnz_b = len(idx_a), len(idx_b)
    order_a, ids_b = np.asarray(order_a, np.int64), np.asarray(ids_b, np.int64)
    if order_a.shape != (n_a,) or ids_b.shape != (n_b,):
        raise ValueError("merge: order_a [n_a] and ids_b [n_b]")
    if (len(ids_b) and ids_b.min() < 0) or len(np.unique(ids_b)) != n_b or len(np.unique(order_a)) != n_a:
        raise ValueError("merge: distinct family ids, none negative")
    # the numbering
    table = np.full(int(max(order_a.max(initial=-1), ids_b.max(initial=-1))) + 1, -1, np.int64)
    table[order_a] = np.arange(n_a)
    new = table[ids_b] < 0
    mapb = np.where(new, n_a + np.cumsum(new) - 1, table[ids_b])
    n, d = n_a + int(new.sum()), d_a + d_b
    order = np.concatenate([order_a, ids_b[new]]).astype(np.int32)
    x = np.zeros((n, d), np.uint8)
    x[:n_a, :d_a] = xa
    x[mapb, d_a:] = xb
    # every entry of B in A's row, or new
    r, c = mapb[row_b], mapb[idx_b]
    akey = row_a * n + idx_a
    by = np.argsort(akey, kind="stable")
    at = np.searchsorted(akey[by], r * n + c)
    found = np.zeros(nnz_b, bool)
    inside = at < nnz_a
    found[inside] = akey[by][at[inside]] == (r * n + c)[inside]
    deg_a = np.zeros(n, np.int64)
    deg_a[:n_a] = np.diff(ptr_a)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(deg_a + np.bincount(r[~found], minlength=n))
    nnz = int(ptr[-1])
    fwd_a = ptr[row_a] + (np.arange(nnz_a) - ptr_a[row_a])    # A's entry t -> its entry now
    before = np.concatenate([[0], np.cumsum(~found)])         # the new entries before B's entry t
    fwd_b = np.empty(nnz_b, np.int64)
    fwd_b[found] = fwd_a[by[at[found]]]
    fwd_b[~found] = (ptr[r] + deg_a[r] + before[:-1] - before[ptr_b[row_b]])[~found]
    idx = np.empty(nnz, np.int32)
    idx[fwd_a] = idx_a
    idx[fwd_b[~found]] = c[~found]
    wf = (d + 31) // 32
    bits = np.zeros((nnz, wf * 32), np.uint8)
    bits[fwd_a, :d_a] = bits_a
    bits[fwd_b, d_a:d] = bits_b
    edge_bits = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint32).reshape(nnz, wf)
    # the extras: an entry's A ones, then its B ones (every column of B lies behind every column of A)
    xe = np.concatenate([fwd_a[np.repeat(np.arange(nnz_a), np.diff(xptr_a))], fwd_b[np.repeat(np.arange(nnz_b), np.diff(xptr_b))]])
    xo = np.concatenate([xorg_a, xorg_b + d_a])
    xc = np.concatenate([xcnt_a, xcnt_b])
    total = bits.sum(axis=1, dtype=np.int64) + np.bincount(xe, weights=xc - 1, minlength=nnz).astype(np.int64)
    if nnz and total.max() > 1 << 24:
        raise ValueError("merge: an edge's total count above 2^24 (a float weight would not be exact)")
    xs = np.lexsort((xo, xe))
    xptr = np.zeros(nnz + 1, np.int32)
    xptr[1:] = np.cumsum(np.bincount(xe, minlength=nnz))
    edge_counts = (xptr, xo[xs].astype(np.int32), xc[xs].astype(np.int32))
    return x, (ptr.astype(np.int32), idx), edge_bits, edge_counts, order, list(range(d))


class Master:
    """One pangenome on the device: presence/absence matrix, neighbourhood graph, per directed edge its organisms."""

    def __init__(self, x, ptr, idx, edge_bits, device=0, edge_counts=None):
        """edge_counts: None (every count 1: nemgpu_master_create) or (extra_ptr, extra_org, extra_count), the
        (edge, organism) pairs whose occurrence count is 2 or more (nemgpu_master_create_counts)"""
        self.lib = _bind_master(load_library())
        lib = self.lib
        x = np.asarray(x)
        if x.dtype == np.uint32:
            raise ValueError("Master takes the 0/1 byte matrix (it packs the rows itself)")
        self.n, self.d = x.shape
        self.wf = (self.d + 31) // 32
        rows = pack_rows(x)
        self._rows_host = rows                                # (partition(): which families are core exact)
        ptr = np.ascontiguousarray(ptr, np.int32)
        idx = np.ascontiguousarray(idx, np.int32)
        edge_bits = np.ascontiguousarray(edge_bits, np.uint32).reshape(len(idx), self.wf) if len(idx) else np.zeros((1, self.wf), np.uint32)
        assert ptr.shape == (self.n + 1,)
        self._h = C.c_void_p()
        if edge_counts is None:
            rc = lib.nemgpu_master_create(C.byref(self._h), int(device), self.n, self.d, rows.ctypes.data, ptr.ctypes.data,
                                          idx.ctypes.data if len(idx) else None, edge_bits.ctypes.data if len(idx) else None)
            what = "nemgpu_master_create"
        else:
            xptr, xorg, xcnt = (np.ascontiguousarray(a, np.int32) for a in edge_counts)
            if xptr.shape != (len(idx) + 1,) or len(xorg) != len(xcnt) or len(xorg) != int(xptr[-1]):
                raise ValueError("edge_counts: extra_ptr [nnz + 1], extra_org and extra_count [extra_ptr[nnz]]")
            rc = lib.nemgpu_master_create_counts(C.byref(self._h), int(device), self.n, self.d, rows.ctypes.data, ptr.ctypes.data,
                                                 idx.ctypes.data if len(idx) else None, edge_bits.ctypes.data if len(idx) else None,
                                                 xptr.ctypes.data, xorg.ctypes.data if len(xorg) else None,
                                                 xcnt.ctypes.data if len(xcnt) else None)
            what = "nemgpu_master_create_counts"
        if rc != 0:
            raise NemGpuError("%s failed (status %d): %s" % (what, rc, lib.nemgpu_last_error().decode()))
        self.order = np.arange(self.n, dtype=np.int32)       # (made from arrays: family i is caller id i)
        self.directed, self.f = False, self.n

    @classmethod
    def from_graph(cls, graph, organisms=None, device=0):
        """A counts master of PPanGGOLiN's neighbours graph (master_arrays_from_graph); its family and organism names are
        kept (.names, .organism_names): partition() names its families by them"""
        x, (ptr, idx), edge_bits, edge_counts, families, orgs = master_arrays_from_graph(graph, organisms)
        m = cls(x, ptr, idx, edge_bits, device=device, edge_counts=edge_counts)
        m.names, m.organism_names = list(families), list(orgs)
        m.id_names = list(families)
        m.directed = bool(graph.is_directed())
        return m

    @classmethod
    def from_orders(cls, genes, contig_ptr, contig_org, contig_circular, d, repeated=None, f=None, directed=False, device=0):
        """The master of these gene orders, built on the device (nemgpu_master_create_orders; the arguments of
        master_arrays_from_orders, which states what it computes).  .order int32 [n]: master family i is the caller's
        family id order[i]."""
        genes, contig_ptr, contig_org, contig_circular, repeated, d, f = _check_orders(genes, contig_ptr, contig_org, contig_circular, repeated, d, f)
        return cls._of_orders(_bind_master(load_library()), "nemgpu_master_create_orders", (int(device), d, f, 1 if directed else 0),
                              genes, contig_ptr, contig_org, contig_circular, repeated, bool(directed), f)

    @classmethod
    def _of_orders(cls, lib, what, head, genes, contig_ptr, contig_org, contig_circular, repeated, directed, f):
        """the master that the entry point `what` makes of checked gene orders (head: its arguments between the handle
        and the orders), with its numbering read back"""
        return cls._of_call(lib, what, head + (genes.ctypes.data, len(genes), contig_ptr.ctypes.data, contig_org.ctypes.data,
                                               contig_circular.ctypes.data, len(contig_org), repeated.ctypes.data if repeated is not None else None),
                            directed, f)

    @classmethod
    def _of_call(cls, lib, what, args, directed, f):
        """the master that the entry point `what` makes on the device (args: its arguments behind the handle), with its
        numbering read back"""
        m = cls.__new__(cls)
        m.lib = lib
        m._h = C.c_void_p()
        rc = getattr(lib, what)(C.byref(m._h), *args)
        if rc != 0:
            raise NemGpuError("%s failed (status %d): %s" % (what, rc, lib.nemgpu_last_error().decode()))
        m.n, m.d, _, _ = m.shape()
        m.wf = (m.d + 31) // 32
        m.order = np.zeros(m.n, np.int32)
        m._fetch(order=m.order)
        m.directed, m.f = directed, f
        return m

    @classmethod
    def from_annotations(cls, annotations, organisms, circular_contigs=(), repeated=(), directed=False, device=0, family=FAMILY):
        """Master.from_orders of orders_from_annotations(...): PPanGGOLiN's annotations straight to the device.  Keeps the
        family and organism names (.names, .organism_names) as Master.from_graph does."""
        o = orders_from_annotations(annotations, organisms, circular_contigs, repeated, family)
        m = cls.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"],
                            directed=directed, device=device)
        m.names, m.organism_names = [o["families"][i] for i in m.order], list(o["organisms"])
        m.id_names = list(o["families"])                      # (every caller id's name: add_annotations numbers on from them)
        m.repeated_by_organism = {org: frozenset(repeated) for org in o["organisms"]}     # (family_table: a node keeps the genes it got)
        return m

    @classmethod
    def from_files(cls, organisms_file, families_file, lim_occurence=0, infer_singletons=False, directed=False, device=0, **load_options):
        """PPanGGOLiN("file", organisms_file, families_tsv, lim_occurence, infer_singletons, directed): the GFFs and the
        families table loaded on the device (loader.load_files), then Master.from_orders of everything with the union of
        the repeated families -- the reference too loads every organism before it builds the graph.  Carries the names as
        a from_annotations master does; .loaded is the loader's result (orders, spans, annotations())."""
        from .loader import load_files
        ld = load_files(organisms_file, families_file, lim_occurence, infer_singletons, device=device, **load_options)
        o = ld.orders
        m = cls.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"],
                            directed=directed, device=device)
        m.names, m.organism_names = [o["families"][i] for i in m.order], list(o["organisms"])
        m.id_names = list(o["families"])
        m.repeated_by_organism = {org: frozenset(ld.families_repeted) for org in o["organisms"]}
        m.loaded = ld
        return m

    def add_orders(self, genes, contig_ptr, contig_org, contig_circular, d_new, repeated=None, f=None):
        """A NEW master = this one + the gene orders of d_new new organisms (nemgpu_master_append_orders;
        master_arrays_append_orders states what it computes): contig_org holds their absolute columns d .. d + d_new - 1,
        repeated [f] the union of the repeated families, f >= this master's .f.  This master is only read and stays
        usable.  Not for a directed master, nor for a bits-only one."""
        if f is None and repeated is None:
            f = max(self.f, int(np.max(genes)) + 1 if len(genes) else 1)
        genes, contig_ptr, contig_org, contig_circular, repeated, d, f = _check_orders(genes, contig_ptr, contig_org, contig_circular, repeated,
                                                                                       self.d + int(d_new), f)
        return Master._of_orders(self.lib, "nemgpu_master_append_orders", (self._h, int(d_new), f), genes, contig_ptr, contig_org,
                                 contig_circular, repeated, False, f)

    def add_annotations(self, new_annotations, new_organisms, circular_contigs=(), repeated=(), family=FAMILY):
        """PPanGGOLiN.add_organism (ppanggolin.py:342-358) on a master that carries names (from_annotations, from_graph or
        an earlier add_annotations): new_annotations of new_organisms (their columns follow this master's), circular_contigs
        the new contigs' names, repeated the UNION of the repeated families' names.  Returns the new master, its .names
        and .organism_names grown."""
        if getattr(self, "id_names", None) is None:
            raise ValueError("add_annotations: this master carries no names (use add_orders)")
        if self.directed:
            raise NemGpuError("add_annotations: the master was built directed (a row's order cannot be recovered); rebuild it")
        new_organisms = list(new_organisms)
        if set(new_organisms) & set(self.organism_names):
            raise ValueError("add_annotations: an organism the master already has")
        o = orders_from_annotations(new_annotations, self.organism_names + new_organisms, circular_contigs, repeated, family,
                                    families=self.id_names)
        m = self.add_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], len(new_organisms), repeated=o["repeated"])
        m.id_names = list(o["families"])
        m.names, m.organism_names = [m.id_names[i] for i in m.order], list(o["organisms"])
        if getattr(self, "repeated_by_organism", None) is not None:
            m.repeated_by_organism = dict(self.repeated_by_organism, **{org: frozenset(repeated) for org in new_organisms})
        return m

    def merge(self, other, ids=None, f=None):
        """A NEW master = this one + another resident master (PPanGGOLiN's `+=`, __iadd__, ppanggolin.py:368-391;
        nemgpu_master_merge; master_arrays_merge states what it computes): the union of the two graphs as built, other's
        organisms behind this master's.  ids int [other.n]: the id of other's family j in this master's id space
        (default: other.order, one id space shared by both); f: the merged id space (default: the smallest that holds
        both).  Both masters are only read and stay usable; neither's arrays leave the device.  Not for a directed
        master, nor for a bits-only one, on either side.  It equals from_orders of everything only when both masters were
        built with the same repeated families."""
        if not isinstance(other, Master):
            raise TypeError("merge: a Master")
        if self.directed or other.directed:                   # (the library knows it of a master built from orders; from_graph's is known here)
            raise NemGpuError("merge: a master was built directed (a row's order cannot be recovered); rebuild it")
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            if ids.shape != (other.n,):
                raise ValueError("merge: ids [other.n]")
        if f is None:
            f = max(self.f, other.f) if ids is None else max(self.f, int(ids.max()) + 1 if len(ids) else 1)
        return Master._of_call(self.lib, "nemgpu_master_merge", (self._h, other._h, ids.ctypes.data if ids is not None else None, int(f)),
                               False, int(f))

    def merge_named(self, other):
        """merge() of two masters that carry names (from_annotations, from_files, from_graph or add_annotations): other's
        families are joined to this master's id_names by name, new names extend them; an organism name that both
        masters carry raises ValueError.  Returns the new master with .names, .organism_names, .id_names and the union
        of repeated_by_organism."""
        if getattr(self, "id_names", None) is None or getattr(other, "id_names", None) is None:
            raise ValueError("merge_named: both masters must carry names (use merge)")
        if set(self.organism_names) & set(other.organism_names):
            raise ValueError("merge_named: an organism that both masters have")
        fam_id = {name: i for i, name in enumerate(self.id_names)}
        ids = np.asarray([fam_id.setdefault(name, len(fam_id)) for name in other.names], np.int32)
        m = self.merge(other, ids=ids, f=max(len(fam_id), self.f))
        m.id_names = list(fam_id)
        m.names, m.organism_names = [m.id_names[i] for i in m.order], list(self.organism_names) + list(other.organism_names)
        mine, theirs = getattr(self, "repeated_by_organism", None), getattr(other, "repeated_by_organism", None)
        if mine is not None and theirs is not None:
            m.repeated_by_organism = dict(mine, **theirs)
        return m

    def project_orders(self, part, genes, contig_ptr, contig_org, repeated=None, f=None):
        """nemgpu_master_project on flat gene orders (projection.projection_arrays states what it computes and takes the
        same orders): part uint8 [n]; contig_org the master's columns.  Returns gene_family int32 [g], gene_copies int32
        [g], nei_counts int32 [n][3], org_counts int32 [d][7]."""
        part = np.ascontiguousarray(part, np.uint8)
        genes = np.ascontiguousarray(genes, np.int32)
        contig_ptr = np.ascontiguousarray(contig_ptr, np.int32)
        contig_org = np.ascontiguousarray(contig_org, np.int32)
        if part.shape != (self.n,) or genes.ndim != 1 or contig_ptr.shape != (len(contig_org) + 1,):
            raise ValueError("projection: part [n], genes [G], contig_ptr [C + 1], contig_org [C]")
        if f is None:
            f = len(repeated) if repeated is not None else max(self.f, int(genes.max()) + 1 if len(genes) else 1)
        if repeated is not None:
            repeated = np.ascontiguousarray(repeated, np.uint8)
            if repeated.shape != (f,):
                raise ValueError("projection: repeated [F]")
        g = len(genes)
        fam, copies = np.zeros(g, np.int32), np.zeros(g, np.int32)
        nei, org = np.zeros((self.n, 3), np.int32), np.zeros((self.d, 7), np.int32)
        rc = self.lib.nemgpu_master_project(self._h, part.ctypes.data, int(f), genes.ctypes.data if g else None, g, contig_ptr.ctypes.data,
                                            contig_org.ctypes.data if len(contig_org) else None, len(contig_org),
                                            repeated.ctypes.data if repeated is not None else None, org.ctypes.data, nei.ctypes.data,
                                            fam.ctypes.data if g else None, copies.ctypes.data if g else None)
        if rc != 0:
            raise NemGpuError("nemgpu_master_project failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))
        return fam, copies, nei, org

    def projection(self, partitions, annotations=None, organisms=None, repeated=(), *, orders=None, family=FAMILY):
        """PPanGGOLiN.projection (ppanggolin.py:1698-1755) of a finished partition on this master, on the device.
        partitions: what Master.partition returned ({family name: 'P' | 'S' | 'C' | 'U'}; a family it does not name is
        undefined) or uint8 [n] in the same codes.  annotations: PPanGGOLiN's (they go through orders_from_annotations
        with this master's ids, so a master grown by add_annotations works); organisms: the names to project, in the
        caller's order (default: all the master's); repeated: families_repeted.  orders=(genes, contig_ptr, contig_org[,
        repeated[, f]]) instead of annotations: flat arrays, for a master without names (contig_org: its columns; the
        projected organisms are then the columns in order of first contig).  A gene whose family the master does not
        have raises KeyError naming it, as the reference would.  Returns a projection.Projection (the four arrays of
        projection_arrays, means(), write())."""
        from . import projection as pj
        names = getattr(self, "names", None)
        if isinstance(partitions, dict):
            if names is None:
                raise ValueError("projection: this master carries no names (give the classes as uint8 [n])")
            part = pj.part_codes(partitions, names)
        else:
            part = np.ascontiguousarray(partitions, np.uint8)
        if self.directed:
            raise NemGpuError("projection: the master was built directed (nx.all_neighbors lists a predecessor that is also a successor "
                              "twice, the master's row once: the neighbour counts cannot be recovered)")
        if orders is not None:
            if annotations is not None:
                raise ValueError("projection: annotations or orders=, not both")
            genes, contig_ptr, contig_org = orders[:3]
            rep = orders[3] if len(orders) > 3 else None
            fam, copies, nei, org = self.project_orders(part, genes, contig_ptr, contig_org, rep, orders[4] if len(orders) > 4 else None)
            bad = np.flatnonzero(fam == pj.UNKNOWN)
            if len(bad):
                raise KeyError(int(np.asarray(genes)[bad[0]]))
            columns = list(dict.fromkeys(int(o) for o in np.asarray(contig_org)))
            return pj.Projection(fam, copies, nei, org, part, columns, names, getattr(self, "organism_names", None))
        if annotations is None or getattr(self, "id_names", None) is None:
            raise ValueError("projection: annotations and a master that carries names, or orders=")
        organisms = list(self.organism_names if organisms is None else organisms)
        col = {o: c for c, o in enumerate(self.organism_names)}
        sub = {o: annotations[o] for o in organisms}          # (an organism without annotations: KeyError, as the reference's)
        if len(sub) != len(organisms):
            raise ValueError("projection: an organism named twice")
        o = orders_from_annotations(sub, self.organism_names, (), repeated, family, families=self.id_names)
        fam, copies, nei, org = self.project_orders(part, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"])
        bad = np.flatnonzero(fam == pj.UNKNOWN)
        if len(bad):
            raise KeyError(o["families"][o["genes"][bad[0]]])
        return pj.Projection(fam, copies, nei, org, part, [col[name] for name in organisms], names, self.organism_names)

    def family_table(self, annotations=None, repeated=(), *, orders=None, lengths=None, family=FAMILY):
        """The per-family table of the pangenome matrix (PPanGGOLiN.write_matrix, ppanggolin.py:1400-1452), computed on the
        device from this master and the gene orders of ALL its organisms (nemgpu_family_table_create;
        matrix.family_table_arrays states what it computes).  annotations: PPanGGOLiN's, of every organism of the master
        (they go through orders_from_annotations with this master's ids, so a master grown by add_annotations works;
        every gene's END - START is read in the same walk); repeated: families_repeted, for a master that was not made by
        from_annotations / add_annotations -- one that was remembers which families were repeated when each organism
        came, as the reference's nodes keep the genes they got before a family was declared repeated.  orders=(genes, contig_ptr,
        contig_org[, repeated[, f]]) with lengths= int32 [G] instead of annotations: flat arrays, for a master without
        names.  Orders that are not this master's (their cells are not its presence bits) raise NemGpuError.  A directed
        master is fine.  Returns a matrix.FamilyTable (the arrays, copies(), write_matrix(), close())."""
        from . import matrix as mx
        if orders is not None:
            if annotations is not None or lengths is None:
                raise ValueError("family_table: annotations, or orders= with lengths=")
            return mx.FamilyTable(self, orders[0], lengths, orders[1], orders[2], orders[3] if len(orders) > 3 else None,
                                  orders[4] if len(orders) > 4 else None)
        if annotations is None or getattr(self, "id_names", None) is None:
            raise ValueError("family_table: annotations and a master that carries names, or orders= with lengths=")
        by_org = getattr(self, "repeated_by_organism", None)
        if by_org is None:
            by_org = {org: frozenset(repeated) for org in self.organism_names}
        o = mx.table_orders(annotations, self.organism_names, self.id_names, by_org, family, lengths)
        return mx.FamilyTable(self, o["genes"], o["lengths"], o["contig_ptr"], o["contig_org"], o["repeated"], repeated_names=by_org)

    def edge_table(self, annotations=None, repeated=(), circular_contig_size=None, *, orders=None, starts=None, ends=None, contig_sizes=None,
                   family=FAMILY):
        """The per-edge table of the GEXF export (PPanGGOLiN.export_to_GEXF, ppanggolin.py:1294-1362), computed on the
        device from this master and the gene orders of ALL its organisms (nemgpu_edge_table_create;
        gexf.edge_table_arrays states what it computes).  annotations, repeated: as family_table takes them, the organisms
        in column order (every gene's START and END are read in the same walk); circular_contig_size: {contig name: size},
        as PPanGGOLiN holds it.  orders=(genes, contig_ptr, contig_org[, repeated[, f]]) with starts=, ends= int32 [G] and
        contig_sizes= int32 [C] (-1: linear) instead: flat arrays, for a master without names.  Orders whose links are not
        this master's edges, organisms and counts raise NemGpuError; so does a directed master.  Returns a
        gexf.EdgeTable (the arrays, attvalues(), set_metadata() / metavalues(), close())."""
        from . import gexf
        if orders is not None:
            if annotations is not None or starts is None or ends is None or contig_sizes is None:
                raise ValueError("edge_table: annotations, or orders= with starts=, ends= and contig_sizes=")
            return gexf.EdgeTable(self, orders[0], starts, ends, orders[1], orders[2], contig_sizes, orders[3] if len(orders) > 3 else None,
                                  orders[4] if len(orders) > 4 else None)
        if annotations is None or getattr(self, "id_names", None) is None:
            raise ValueError("edge_table: annotations and a master that carries names, or orders= with starts=, ends= and contig_sizes=")
        by_org = getattr(self, "repeated_by_organism", None)
        if by_org is None:
            by_org = {org: frozenset(repeated) for org in self.organism_names}
        o = gexf.gexf_orders(annotations, self.organism_names, self.id_names, by_org, circular_contig_size, family)
        return gexf.EdgeTable(self, o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"], o["contig_sizes"], o["repeated"])

    def node_table(self, loaded=None, *, orders=None, text=None, spans=None, batch_bytes=256 << 20, _hash_bits=0):
        """The nodes' <attvalue> text of the GEXF export, formatted on the device from this master, the flat orders of ALL
        its organisms and every gene's ID, NAME and PRODUCT as (offset, length) spans of the load's text
        (nemgpu_node_table_*; gexf.node_text_host states it): write_gexf(node_table=) then needs no annotations.
        loaded: a loader.Loaded (default: this master's .loaded, what from_files keeps) supplies the orders, the files'
        text and the spans; the text goes up a second time, in runs of whole files of at most batch_bytes (a file above
        it alone), and only the escaped spans of the kept genes stay on the device.  Or orders=(genes, contig_ptr,
        contig_org[, repeated[, f]]) with text= (bytes or uint8) and spans=(span_off int64 [3][G], span_len int32 [3][G]):
        flat arrays; the text then goes up in runs of genes whose spans lie within batch_bytes.  A master whose repeated
        families differ between organisms (grown by add_annotations with other sets) is refused with ValueError when the
        orders come from a Loaded, whose flags are one global set: that case stays on write_gexf's annotations path.
        Orders whose cells are not this master's presence bits, and a span past the end of the text, raise NemGpuError
        before any launch.  _hash_bits (tests): keep only that many bits of the string hash.  Returns a gexf.NodeTable
        (titles(), ids(), lines_size(), lines(), close())."""
        from . import gexf
        if orders is not None:
            if loaded is not None or text is None or spans is None:
                raise ValueError("node_table: a Loaded, or orders= with text= and spans=")
            t = gexf.NodeTable(self, orders[0], orders[1], orders[2], orders[3] if len(orders) > 3 else None, orders[4] if len(orders) > 4 else None,
                               _hash_bits=_hash_bits)
            try:
                text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
                off, length = np.asarray(spans[0], np.int64), np.asarray(spans[1], np.int32)
                if off.shape != (3, t.g) or length.shape != (3, t.g):
                    raise ValueError("node_table: spans = (span_off [3][G], span_len [3][G])")
                lo = np.where(length > 0, off, np.iinfo(np.int64).max).min(axis=0)       # (an empty span lies anywhere)
                hi = np.where(length > 0, off + length, 0).max(axis=0)
                gene0 = 0
                while gene0 < t.g:
                    a, b, gene1 = int(lo[gene0]), int(hi[gene0]), gene0 + 1
                    while gene1 < t.g and max(b, int(hi[gene1])) - min(a, int(lo[gene1])) <= batch_bytes:
                        a, b, gene1 = min(a, int(lo[gene1])), max(b, int(hi[gene1])), gene1 + 1
                    a = max(min(a, b), 0)                      # (no span with a byte in the run: an empty text)
                    part = off[:, gene0:gene1] - a             # (a span outside the text stays outside its slice: the library refuses it)
                    t.add_text(text[a:b], gene0, gene1, np.where(length[:, gene0:gene1] > 0, part, 0), length[:, gene0:gene1])
                    gene0 = gene1
                return t.finish()
            except Exception:
                t.close()
                raise
        ld = getattr(self, "loaded", None) if loaded is None else loaded
        if ld is None:
            raise ValueError("node_table: a Loaded (a master made by from_files keeps its own), or orders= with text= and spans=")
        by_org = getattr(self, "repeated_by_organism", None)
        if by_org is not None and len(set(by_org.values())) > 1:
            raise ValueError("node_table: this master's repeated families differ between organisms (it was grown by add_annotations with other "
                             "sets); a Loaded flags one global set -- use write_gexf(annotations=)")
        o = ld.orders
        t = gexf.NodeTable(self, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"], _hash_bits=_hash_bits)
        try:
            files, base = ld._files, ld._base
            ptr, corg = np.asarray(o["contig_ptr"], np.int64), np.asarray(o["contig_org"], np.int64)
            # the genes of file k (organism k): the contigs of organism k are adjacent, in column order
            gene_at = ptr[np.searchsorted(corg, np.arange(len(files) + 1))]
            i = 0
            while i < len(files):
                j, total = i + 1, len(files[i]) + 1
                while j < len(files) and total + len(files[j]) + 1 <= batch_bytes:
                    total, j = total + len(files[j]) + 1, j + 1
                gene0, gene1 = int(gene_at[i]), int(gene_at[j])
                if gene1 > gene0:
                    t.add_text(b"\n".join(files[i:j]), gene0, gene1, ld.span_off[:3, gene0:gene1] - int(base[i]), ld.span_len[:3, gene0:gene1])
                i = j
            return t.finish()
        except Exception:
            t.close()
            raise

    def layout(self, iterations=500, pos=None, rng=None, repulsion="exact", theta=1.2, **params):
        """The family graph laid out on the device (PPanGGOLiN.compute_layout, ppanggolin.py:1250-1292; nemgpu_layout_*;
        layout.layout_arrays states what it computes: ForceAtlas2 with an exact all-pairs repulsion, n^2 per iteration).
        pos: the start positions float64 [n][2], or rng (default: the `random` module): per family in master order x =
        rng.random(), then y = rng.random(); params: compute_layout's, in layout.DEFAULTS' names.  `iterations` are
        enqueued at once.  LinLog, adjust_sizes, strong_gravity=False and a directed master raise ValueError.
        repulsion="barnes_hut" (compute_layout's barnesHutOptimize=True) sums the repulsion over a tree instead, n log n
        per iteration, theta (barnesHutTheta, 1.2; >= 0 and finite, read for this repulsion alone) the opening angle:
        layout_bh.layout_bh_arrays states it; the tree is this project's, not fa2's.  Any other repulsion: ValueError.
        Returns a layout.Layout (run(k), positions(), forces(), state(), tree(), close()); this master is only read."""
        from . import layout as ly
        return ly.Layout(self, pos=pos, rng=rng, repulsion=repulsion, theta=theta, **params).run(iterations)

    def partition_shell(self, partitions=None, Q="auto", mean_shell=None, beta=0.5, free_dispersion=False, exclusity_th=0.1,
                        init_using_qual=None, edges="induced", seed=None, subpart_name="subpartition_shell", *, select=None,
                        annotations=None, repeated=(), low_disp=0.1):
        """PPanGGOLiN.partition_shell (ppanggolin.py:1175-1248, the CLI's -ss) on this master: the NEM problem of the shell
        families and all organisms is formed on the device (nemgpu_master_subproblem; shell.form_subproblem_host states
        it), run there and labelled as the reference labels it (shell.shell_labels).  partitions: what Master.partition
        returned ({family: 'P' | 'S' | 'C' | 'U'}); or select= bool [n] for a master without names.
        Q: "auto" (without init_using_qual: projection.shell_q_auto of mean_shell = Projection.means()[1], or of the
        projection this call runs itself when given annotations= [and repeated=]; with a dict: len + 1; with a list: 3) or
        an int; 1 or less is the reference's error (ValueError), more than 32 is refused.
        edges: "induced" (default) keeps the edges between shell families -- the writer's evident intent.  "reference" is
        the writer as written: its test at :859 is inverted (a neighbour that IS shell is skipped, one that is NOT has no
        index), so it raises KeyError naming a non-shell neighbour as soon as a shell family has one, and runs on an
        empty graph when the shell is closed under adjacency; on a real pangenome it cannot return.
        init_using_qual: None (INIT_RANDOM, 50 starts), a dict {group: set(organisms)} or a list (positive, negative):
        shell.shell_init_params' parameter file (ValueError where nem() refuses it), set_params + run.
        seed: None is time(), as the reference seeds; it is the starts' stream and the tie stream (one random() stream, as
        in nem()).  The numbers in the labels and in .parameters went through the `.mf`'s print formats ("%5.3g",
        "%10g", "%10.3g"), as the reference reads them.  A run that emptied a class raises KeyError('U'), as the
        reference does.  Not here: the untangled graph.  The CLI's -ss 0 builds its dict from the metadata file:
        gexf.shell_init_from_metadata(gexf.read_metadata(file, organisms)).  A directed master raises NemGpuError.  This master is only read.
        Returns a shell.ShellSubpartition: Q, parameters {label: ([organisms], mean eps, proportion)}, organisms
        {organism: {labels}}, families {label: [families]}, node_attribute {family: label | its partition's long name}."""
        from . import shell
        return shell.partition_shell(self, partitions, Q, mean_shell, beta, free_dispersion, exclusity_th, init_using_qual, edges, seed,
                                     subpart_name, select, annotations, repeated, low_disp)

    def organism_clustering(self):
        """The organisms clustered on the device for the CLI's presence/absence plot (the R script's
        hclust(dist(t(binary_matrix), method="binary")), command_line.py:79; nemgpu_orgclust_*): the Jaccard distances of
        all pairs over this master's presence bits (tileplot.organism_distances_host states them) and R's complete
        linkage on them (tileplot.hclust_complete_host).  At most 32 768 organisms (NemGpuError above).  A bits-only
        master and a directed one are fine: the adjacency is not read.  This master is only read and must stay open as
        long as the result.  Returns a tileplot.OrganismClustering: distances(i0, rows), merge, height, order, labels,
        close()."""
        from . import tileplot
        return tileplot.OrganismClustering(self)

    def tile_plot(self, partitions):
        """What the presence/absence plot draws (command_line.py:75-101): the organisms in the clustering's leaf order,
        the families in tileplot.family_plot_order, the raster gathered on the device in batches.  partitions: what
        Master.partition returned, or uint8 [n] (P 0, S 1, C 2, U 3).  Returns a tileplot.TilePlot: organism_order,
        organism_labels, family_order, cells(row0, rows), close()."""
        from . import tileplot
        return tileplot.TilePlot(self, partitions)

    def shape(self):
        """(n families, d organisms, nnz CSR entries, pairs with count >= 2) as the device holds them (nemgpu_master_shape)"""
        v = [C.c_int() for _ in range(4)]
        rc = self.lib.nemgpu_master_shape(self._h, *(C.byref(a) for a in v))
        if rc != 0:
            raise NemGpuError("nemgpu_master_shape failed (status %d)" % rc)
        return tuple(a.value for a in v)

    def _fetch(self, rows=None, ptr=None, idx=None, edge_bits=None, xptr=None, xorg=None, xcnt=None, order=None):
        args = [a.ctypes.data if a is not None and a.size else None for a in (rows, ptr, idx, edge_bits, xptr, xorg, xcnt, order)]
        rc = self.lib.nemgpu_master_fetch(self._h, *args)
        if rc != 0:
            raise NemGpuError("nemgpu_master_fetch failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))

    @property
    def _rows(self):
        """the packed rows uint32 [n][ceil(d/32)] on the host; a master built on the device fetches them once"""
        if getattr(self, "_rows_host", None) is None:
            self._rows_host = np.zeros((self.n, self.wf), np.uint32)
            self._fetch(rows=self._rows_host)
        return self._rows_host

    def arrays(self):
        """The master read back from the device (nemgpu_master_fetch), of whichever constructor: rows uint32
        [n][ceil(d/32)] (packed: pack_rows of the byte matrix), (ptr, idx), edge_bits uint32 [nnz][ceil(d/32)],
        edge_counts (extra_ptr, extra_org, extra_count), order int32 [n]."""
        n, d, nnz, nx = self.shape()
        wf = (d + 31) // 32
        rows, ptr, idx = np.zeros((n, wf), np.uint32), np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32)
        eb, xptr = np.zeros((nnz, wf), np.uint32), np.zeros(nnz + 1, np.int32)
        xorg, xcnt, order = np.zeros(nx, np.int32), np.zeros(nx, np.int32), np.zeros(n, np.int32)
        self._fetch(rows, ptr, idx, eb, xptr, xorg, xcnt, order)
        return rows, (ptr, idx), eb, (xptr, xorg, xcnt), order

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nemgpu_master_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _config(k, prop, center_k, disp_k, algo, beta, disper, propor, cvtest, cvthres, it_max, param_fix, tie, seed):
        prop = list(prop)
        if prop[-1] is None:
            rem = np.float32(1.0)
            for v in prop[:-1]:
                rem = np.float32(rem - np.float32(v))
            prop[-1] = rem
        prop = np.ascontiguousarray(prop, np.float32)
        center_k = np.ascontiguousarray(center_k, np.float32)
        disp_k = np.ascontiguousarray(disp_k, np.float32)
        assert len(prop) == k and len(center_k) == k and len(disp_k) == k
        cfg = Config(ALGO[algo], beta, DISP[disper], PROP[propor], CVT[cvtest], cvthres, it_max, int(param_fix), TIE[tie], seed)
        return prop, center_k, disp_k, cfg

    def partition(self, organisms=None, chunk_size=500, beta=0.5, free_dispersion=False, rng=None, batch=64, tie="libc", seed=0,
                  max_samples=100000, names=None, just_stats=False, workers=8, group=32):
        """PPanGGOLiN's partition() (ppanggolin.py:932-1173, algo ncem, the default .m, its sequential loop) on this master:
        organisms = an ordered selection of the master's organisms (default: all).  More than chunk_size of them: samples
        drawn one at a time as rng.sample(organisms, chunk_size) (rng: the `random` module by default, as the reference's
        `from random import sample`), solved `batch` at a time (nemgpu_votes_solve) and voted on the device until every
        family of the pangenome is validated; rng is left as the reference's loop leaves it.  Otherwise one run on
        exactly `organisms`.  Returns (partitions, cnt, samples): {name: 'P'|'S'|'C'|'U'} for the families of the
        pangenome in the master's order (names: "fam1", ... or, for Master.from_graph, the graph's; with just_stats the
        reference's stats: accessory / core_exact / persistent / shell / cloud / undefined counts), the votes int32
        [n][4] (P, S, C, U) and the number of samples voted.
        More than max_samples samples without an end raise NemGpuError (the reference would loop forever)."""
        from .partitioning import CODES
        lib = self.lib
        _bind_votes(lib)
        organisms = np.ascontiguousarray(np.arange(self.d) if organisms is None else organisms, np.int32)
        d_sel = len(organisms)
        if d_sel == 0 or len(np.unique(organisms)) != d_sel or organisms.min() < 0 or organisms.max() >= self.d:
            raise ValueError("organisms: distinct indices of the master's organisms")
        rng = random if rng is None else rng
        small = d_sel <= chunk_size
        prop, center_k, disp_k, cfg = self._config(3, (0.33333, 0.33333, None), (1.0, 0.5, 0.0), (0.1, 0.5, 0.1), "ncem", beta,
                                                   "skd" if free_dispersion else "sk_", "pk", "clas", 1e-8, 100, False, tie, seed)
        h = C.c_void_p()
        rc = lib.nemgpu_votes_create(C.byref(h), self._h, organisms.ctypes.data, d_sel, int(chunk_size), 1 if small else int(batch))
        if rc != STATUS_OK:
            raise NemGpuError("nemgpu_votes_create failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
        try:
            cnt = np.zeros((self.n, 4), np.int32)
            final = np.zeros(self.n, np.uint8)
            first = np.zeros(self.n, np.int32)
            nvoted = C.c_int64()
            lib.nemgpu_votes_result(h, None, final.ctypes.data, None, None)
            pan = final != 0xFF

            def run(samples):
                arr = (Chunk * len(samples))()
                hold = [np.ascontiguousarray(smp, np.int32) for smp in samples]
                for q, org in zip(arr, hold):
                    q.organisms, q.dc = org.ctypes.data, len(org)
                stop = C.c_int(-1)
                rc = lib.nemgpu_votes_solve(h, arr, len(samples), 3, prop.ctypes.data, center_k.ctypes.data, disp_k.ctypes.data,
                                            C.byref(cfg), int(workers), int(group), C.byref(stop))
                if rc != STATUS_OK:
                    raise NemGpuError("nemgpu_votes_solve failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
                return stop.value

            if not pan.any():
                pass                                          # (no family: the reference's loop draws nothing)
            elif small:
                run([organisms])                              # (one run, its labels are the partition: ppanggolin.py:1122-1125)
            else:
                partition_loop(d_sel, chunk_size, rng, batch, max_samples, lambda pos: run([organisms[p] for p in pos]))
            rc = lib.nemgpu_votes_result(h, cnt.ctypes.data, final.ctypes.data, first.ctypes.data, C.byref(nvoted))
            if rc != STATUS_OK:
                raise NemGpuError("nemgpu_votes_result failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
        finally:
            lib.nemgpu_votes_destroy(h)
        if names is None:
            names = getattr(self, "names", None)                # (Master.from_graph: the graph's family names)
        names = list(names) if names is not None else ["fam%d" % (i + 1) for i in range(self.n)]
        fam = np.flatnonzero(pan)
        partitions = {names[i]: CODES[final[i]] for i in fam}
        if just_stats:
            stats = defaultdict(int)
            core = self.core_exact(organisms)
            stats["accessory"] = int(np.count_nonzero(pan & ~core))
            stats["core_exact"] = int(np.count_nonzero(core))
            long = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
            for c in partitions.values():
                stats[long[c]] += 1
            return stats, cnt, int(nvoted.value)
        return partitions, cnt, int(nvoted.value)

    def resample_stats(self, samples, beta=0.5, free_dispersion=False, tie="libc", seed=0, workers=8, group=32):
        """evolution.resample_stats: every sample (a list of distinct organism indices) as partition(just_stats=True)
        solves a selection of at most chunk_size organisms, in one library call (nemgpu_resamples_solve).  Returns
        int32 [count][6]: persistent, shell, cloud, undefined, core_exact, accessory."""
        from . import evolution
        return evolution.resample_stats(self, samples, beta=beta, free_dispersion=free_dispersion, tie=tie, seed=seed,
                                        workers=workers, group=group)

    def evolution(self, rng=None, ratio=0.1, rmin=10, rmax=30, step=1, limit=None, chunk_size=500, beta=0.5, free_dispersion=False,
                  tie="libc", seed=0, batch=64, workers=8, group=32, max_samples=100000):
        """The CLI's --evolution on this master as its --cpu 1 run makes it (command_line.py:591-625, evolution.py): the
        resamples drawn and shuffled on rng (the `random` module by default) with -ep ratio rmin rmax step limit (None:
        Inf), every resample of at most chunk_size organisms solved in one resample_stats call, the larger ones through
        partition()'s vote loop on rng in shuffled order.  rng is left where the reference leaves it.  Returns int64
        [count][7] in shuffled order: nb_org, persistent, shell, cloud, undefined, core_exact, accessory
        (evolution.write_evol_stats writes them)."""
        from . import evolution
        rng = random if rng is None else rng
        resamples = evolution.evolution_resamples(self.d, ratio, rmin, rmax, step, limit, rng)

        def small(rs):
            return self.resample_stats(rs, beta=beta, free_dispersion=free_dispersion, tie=tie, seed=seed, workers=workers, group=group)

        def large(r, rng):
            return evolution.partition_stats_row(self.partition(organisms=r, chunk_size=chunk_size, beta=beta, free_dispersion=free_dispersion,
                                                                rng=rng, batch=batch, tie=tie, seed=seed, max_samples=max_samples,
                                                                just_stats=True, workers=workers, group=group))

        return evolution.evolution_rows(resamples, rng, chunk_size, small, large)

    def core_exact(self, organisms):
        """bool [n]: the families present in every one of `organisms` (ppanggolin.py:982-993)"""
        mask = np.zeros(self.wf * 32, np.uint8)
        mask[np.asarray(organisms, np.int64)] = 1
        words = np.packbits(mask, bitorder="little").view(np.uint32)
        ones = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1)
        hit = ones[np.bitwise_and(self._rows, words[None, :]).view(np.uint8)].sum(axis=1)
        return hit == len(organisms)

    def solve_chunks(self, samples, k=3, prop=(0.33333, 0.33333, None), center_k=(1.0, 0.5, 0.0), disp_k=(0.1, 0.5, 0.1),
                     workers=8, group=32, algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8,
                     it_max=100, param_fix=False, tie="hash", seed=0, want_params=True):
        """samples: sequences of organism indices (a chunk's columns, in order).  Initial parameters as PPanGGOLiN's
        default .m (ppanggolin.py:893-901): proportions (the last one None = the float remainder ReadParamFile computes,
        nem_exe.c:1022-1034), ONE centre and ONE dispersion per class.  Returns one dict per sample: families (master
        index of the chunk's family j), labels (uint8 per kept family), prop / center / disp / nbobs_k, iters, status, ..."""
        lib = self.lib
        prop, center_k, disp_k, cfg = self._config(k, prop, center_k, disp_k, algo, beta, disper, propor, cvtest, cvthres, it_max,
                                                   param_fix, tie, seed)
        arr = (Chunk * len(samples))()
        hold, outs = [], []
        nw64 = (self.n + 63) // 64
        for q, s in zip(arr, samples):
            org = np.ascontiguousarray(s, np.int32)
            dc = len(org)
            o = dict(keep=np.zeros(nw64, np.uint64), labels=np.zeros(self.n, np.uint8))
            q.organisms, q.dc = org.ctypes.data, dc
            q.keep, q.labels = o["keep"].ctypes.data, o["labels"].ctypes.data
            if want_params:
                o.update(prop=np.empty(k, np.float32), center=np.empty((k, dc), np.float32), disp=np.empty((k, dc), np.float32),
                         nbobs_k=np.empty(k, np.float32))
                q.out_prop, q.out_center, q.out_disp, q.out_nbobs_k = (o[f].ctypes.data for f in ("prop", "center", "disp", "nbobs_k"))
            hold.append(org)
            outs.append(o)
        import time
        t0 = time.perf_counter()
        rc = lib.nemgpu_solve_chunks(self._h, arr, len(samples), int(k), prop.ctypes.data, center_k.ctypes.data, disp_k.ctypes.data,
                                     C.byref(cfg), int(workers), int(group))
        self.last_call_seconds = time.perf_counter() - t0     # (the library call alone: what follows is numpy bookkeeping)
        if rc != STATUS_OK:
            raise NemGpuError("nemgpu_solve_chunks failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
        res = []
        for q, o in zip(arr, outs):
            r = q.result
            bits = np.unpackbits(o["keep"].view(np.uint8), bitorder="little")[:self.n]
            fam = np.flatnonzero(bits)
            assert len(fam) == q.n
            meta = dict(status=r.status, iters=r.iters, converged=bool(r.converged), emptyk=r.emptyk, n=q.n, nnz=q.nnz,
                        n_zero_density=r.zero_density_sites, sweep_rounds=r.sweep_rounds, crit=np.array(list(r.crit), np.float32),
                        families=fam, labels=o["labels"][:q.n].copy())
            for f in ("prop", "center", "disp", "nbobs_k"):
                if f in o:
                    meta[f] = o[f]
            res.append(meta)
        return res


def partition_loop(n_sel, chunk_size, rng, batch, max_samples, run_batch):
    """partition()'s sampling loop (ppanggolin.py:1045-1086) in batches: draws up to `batch` samples, each
    rng.sample(range(n_sel), chunk_size) (random.sample picks by position: the same positions as sampling the
    organisms themselves), hands their positions to run_batch, which returns the index of the sample after which every
    family is validated, or -1; repeats until it is not -1.  The draws after that sample are undone: rng ends in the
    state the reference's loop leaves it in.  Returns the number of samples the loop counted."""
    done = 0
    while True:
        if done >= max_samples:
            raise NemGpuError("partition: no end after %d samples (max_samples)" % done)
        states, samples = [], []
        for _ in range(min(batch, max_samples - done)):
            states.append(rng.getstate())
            samples.append(rng.sample(range(n_sel), chunk_size))
        stop = run_batch(samples)
        if stop >= 0:
            if stop + 1 < len(samples):
                rng.setstate(states[stop + 1])
            return done + stop + 1
        done += len(samples)


def _bind_votes(lib):
    if getattr(lib, "_votes_bound", False):
        return
    lib.nemgpu_votes_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.nemgpu_votes_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_votes_destroy.restype = None
    lib.nemgpu_votes_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(Config), C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.nemgpu_votes_add_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    lib.nemgpu_vote_classmap_host.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nemgpu_votes_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib._votes_bound = True


class Votes:
    """A nemgpu_votes of a Master, driven with synthetic samples (nemgpu_votes_add_host): the vote rule on the device
    without the runs."""

    def __init__(self, master, organisms, chunk_size, batch):
        self.lib = master.lib
        _bind_votes(self.lib)
        self.n = master.n
        org = np.ascontiguousarray(organisms, np.int32)
        self._h = C.c_void_p()
        rc = self.lib.nemgpu_votes_create(C.byref(self._h), master._h, org.ctypes.data, len(org), int(chunk_size), int(batch))
        if rc != STATUS_OK:
            raise NemGpuError("nemgpu_votes_create failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))

    def add(self, samples):
        """samples: (families, labels, codes) as partitioning.vote_host takes them.  Returns the stop index or -1."""
        nw64 = (self.n + 63) // 64
        cnt = len(samples)
        keep = np.zeros((cnt, nw64 * 64), np.uint8)
        lab = np.zeros((cnt, self.n), np.uint8)
        maps = np.zeros((cnt, 3), np.uint8)
        for s, (fam, l, codes) in enumerate(samples):
            fam = np.asarray(fam, np.int64)
            order = np.argsort(fam, kind="stable")
            keep[s, fam] = 1
            lab[s, :len(fam)] = np.asarray(l, np.uint8)[order]
            maps[s] = codes
        keep = np.packbits(keep, axis=1, bitorder="little").view(np.uint64)
        stop = C.c_int(-1)
        rc = self.lib.nemgpu_votes_add_host(self._h, cnt, keep.ctypes.data, lab.ctypes.data, maps.ctypes.data, C.byref(stop))
        if rc != STATUS_OK:
            raise NemGpuError("nemgpu_votes_add_host failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))
        return stop.value

    def result(self):
        cnt = np.zeros((self.n, 4), np.int32)
        final = np.zeros(self.n, np.uint8)
        first = np.zeros(self.n, np.int32)
        nv = C.c_int64()
        rc = self.lib.nemgpu_votes_result(self._h, cnt.ctypes.data, final.ctypes.data, first.ctypes.data, C.byref(nv))
        if rc != STATUS_OK:
            raise NemGpuError("nemgpu_votes_result failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))
        return dict(cnt=cnt, final=final, first=first, samples=int(nv.value))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nemgpu_votes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def vote_classmap_device(status, centers, disps):
    """nemgpu_vote_classmap_host: the code map (uint8 [count][3]) of runs with these statuses and final parameters
    (each [3][dc])."""
    lib = load_library()
    _bind_votes(lib)
    cnt = len(status)
    dc = np.ascontiguousarray([np.asarray(c).shape[1] for c in centers], np.int32)
    cen = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).ravel() for c in centers]), np.float32)
    dis = np.ascontiguousarray(np.concatenate([np.asarray(e, np.float32).ravel() for e in disps]), np.float32)
    st = np.ascontiguousarray(status, np.int32)
    maps = np.zeros((cnt, 3), np.uint8)
    rc = lib.nemgpu_vote_classmap_host(cnt, 3, dc.ctypes.data, cen.ctypes.data, dis.ctypes.data, st.ctypes.data, maps.ctypes.data)
    if rc != STATUS_OK:
        raise NemGpuError("nemgpu_vote_classmap_host failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
    return maps
