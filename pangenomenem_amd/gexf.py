"""The pangenome graph as GEXF (PPanGGOLiN.export_to_GEXF, ppanggolin.py:1294-1362, full and ``_light``) and the series
of the U-shaped plot (``ushaped_plot``, :1486-1523), from a resident master: no networkx graph is built or walked.

``export_to_GEXF`` copies the graph, turns every node's set of gene lengths and every edge's set of link lengths
(``__add_link``'s ``length``, :456-459) into avg / med / min / max and hands the copy to networkx's ``write_gexf``, which
builds an ElementTree with one ``<attvalue>`` per (edge, organism).  Everything it writes is a function of the master
(its CSR, its edge bit rows and extras, its numbering), the family table (matrix.py) and the flat gene orders of all the
master's organisms with every gene's START and END and every circular contig's size:

``edge_table_arrays`` states the per-edge table in numpy and ``attvalues_host`` the edges' organism lines;
``nemgpu_edge_table_create`` / ``nemgpu_edge_table_attvalues`` (csrc/nem_edges.hip) compute both on the device,
``Master.edge_table`` (chunks.py) is their Python surface; ``EdgeTable`` / ``HostEdgeTable`` hold the result;
``write_gexf`` streams the file, byte for byte what networkx writes, and ``ushape_counts`` gives the plot's series.

``export_to_GEXF(metadata=)`` (:1339-1354) gives every edge, per metadata attribute, the sorted set of the values of the
organisms that carry it: ``read_metadata`` is the CLI's parse of the ``-mt`` file, ``rank_metadata`` ranks and escapes
the values on the host, ``edge_metadata_arrays`` states the edges' present-value masks and ``metavalues_host`` their
lines; ``nemgpu_edge_table_metadata`` / ``_metamasks`` / ``_metavalues`` (csrc/nem_edge_meta.hip) compute both on the
device; ``shell_init_from_metadata`` turns the same dict into ``partition_shell``'s ``init_using_qual``.

The nodes' organism, name and product lines need the genes' ids, names and products.  ``write_gexf`` reads them from
the nested ``annotations``, or -- for a load from files, which has no nested dict -- takes them from a node table:
``node_text_host`` states the nodes' text in plain Python on the flat orders, a text and the (offset, length) spans of
every gene's ID, NAME and PRODUCT; ``nemgpu_node_table_*`` (csrc/nem_nodes.hip) format it on the device,
``Master.node_table`` is their Python surface, ``NodeTable`` / ``HostNodeTable`` hold the result.

Where the reference's bytes are not determined -- ``"|".join(set)`` of a node's names, products and an organism's genes
follows string hash order; the ``<meta>`` element holds the date and networkx's version -- the values are joined in walk
order here and ``<meta>`` names this package.
"""
import ctypes as C
import gzip
import os
import time

import numpy as np

from .matrix import TEXT_BUDGET, DeviceTable, _long_names, table_orders
from .projection import FAMILY, START, END, PRODUCT, check_projection_orders, part_codes

NAME = 5                                                      # a gene's info: TYPE, FAMILY, START, END, STRAND, NAME, PRODUCT
EDGE_FIELDS = ("src", "dst", "weight", "len_min", "len_max", "len_distinct", "len_sum", "len_mid_lo", "len_mid_hi", "fam_mid_lo", "fam_mid_hi",
               "org_first_edge")
COLORS_RGB = {"accessory": (235, 55, 237), "core_exact": (255, 40, 40), "shell": (0, 216, 96), "persistent": (247, 165, 7),
              "cloud": (121, 222, 255), "undefined": (130, 130, 130)}                             # ppanggolin.py:34 (a is 0)
LINE_MAX = 59                                                 # an organism line of an edge: 39 bytes and two numbers of 10 digits
LINE_FIXED = 39                                               # an <attvalue> line without its id and its value
LENGTH_TITLES = ("length_avg", "length_med", "length_min", "length_max")
META_VALUES_MAX = 65536                                       # distinct values of one attribute the device holds (nem_edges.hpp)
HEAD = ("<?xml version='1.0' encoding='utf-8'?>\n"
        '<gexf xmlns:viz="http://www.gexf.net/1.2draft/viz" xmlns="http://www.gexf.net/1.2draft" '
        'xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
        'xsi:schemaLocation="http://www.gexf.net/1.2draft http://www.gexf.net/1.2draft/gexf.xsd" version="1.2">\n'
        '  <meta lastmodifieddate="%s">\n    <creator>pangenomenem_amd</creator>\n  </meta>\n'
        '  <graph defaultedgetype="undirected" mode="static" name="">\n')
INT32 = (-2 ** 31, 2 ** 31 - 1)


def gexf_orders(annotations, organisms, families, repeated, circular_contig_size=None, family=FAMILY):
    """The flat orders an edge table is made from: matrix.table_orders of ALL the organisms (a skipped gene gets the one
    id flagged in `repeated`) with every gene's START and END in the same walk and per contig its circular size
    (circular_contig_size: {contig name: size}, as PPanGGOLiN holds it), -1 for a linear contig.
    Returns table_orders' dict with starts, ends, contig_sizes."""
    o = table_orders(annotations, organisms, families, repeated, family, lengths=np.zeros(0, np.int32))
    infos = [info for contigs in annotations.values() for annot in contigs.values() for info in annot.values()]
    sizes = circular_contig_size or {}
    o["starts"] = np.asarray([info[START] for info in infos], np.int64)
    o["ends"] = np.asarray([info[END] for info in infos], np.int64)
    o["contig_sizes"] = np.asarray([sizes.get(contig, -1) for contigs in annotations.values() for contig in contigs], np.int64)
    for name in ("starts", "ends", "contig_sizes"):
        if len(o[name]) and (o[name].min() < INT32[0] or o[name].max() > INT32[1]):
            raise ValueError("gexf_orders: %s outside int32" % name)
        o[name] = o[name].astype(np.int32)
    return o


def _segments(seg, val, count):
    """over the DISTINCT (seg, val) pairs, per segment 0 .. count - 1: distinct, sum (int64), min, max and the two middle
    elements of the sorted distinct values (0 where there is none)"""
    out = dict(distinct=np.zeros(count, np.int32), sum=np.zeros(count, np.int64), min=np.zeros(count, np.int32), max=np.zeros(count, np.int32),
               lo=np.zeros(count, np.int32), hi=np.zeros(count, np.int32))
    if not len(seg):
        return out
    pairs = np.unique(np.stack([np.asarray(seg, np.int64), np.asarray(val, np.int64)], axis=1), axis=0)     # by segment, then value
    s, v = pairs[:, 0], pairs[:, 1]
    cnt = np.bincount(s, minlength=count)
    first = np.cumsum(cnt) - cnt
    has = cnt > 0
    out["distinct"] = cnt.astype(np.int32)
    np.add.at(out["sum"], s, v)
    out["min"][has] = v[first[has]]
    out["max"][has] = v[first[has] + cnt[has] - 1]
    out["lo"][has] = v[first[has] + (cnt[has] - 1) // 2]
    out["hi"][has] = v[first[has] + cnt[has] // 2]
    return out


def _edge_bits_bool(edge_bits, nnz, d):
    wf = (d + 31) // 32
    eb = np.ascontiguousarray(edge_bits, np.uint32).reshape(-1, wf)[:nnz]
    return np.unpackbits(eb.view(np.uint8).reshape(nnz, -1), axis=1, bitorder="little")[:, :d].astype(bool)


def master_edges(ptr, idx):
    """nx.Graph.edges() of a master's CSR: the entries with idx >= row, in CSR order: (src, dst, entry)"""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    row = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    entry = np.flatnonzero(idx >= row)
    return row[entry].astype(np.int32), idx[entry].astype(np.int32), entry


def links_of_orders(fam, kept, gene_start, gene_end, contig_ptr, contig_org, contig_size):
    """The links of __neighborhood_computation (ppanggolin.py:485-520) as arrays: per link (a, b, organism, length):
    a kept gene and the previous kept gene of its contig, START[gene] - END[previous]; per circular contig with a kept
    gene its first and last kept gene, (size - END[last]) + START[first].  fam: every gene's family; int64."""
    gs, ge = np.asarray(gene_start, np.int64), np.asarray(gene_end, np.int64)
    cid = np.repeat(np.arange(len(contig_org), dtype=np.int64), np.diff(contig_ptr))
    kp = np.flatnonzero(kept)
    org = np.asarray(contig_org, np.int64)
    a, b = kp[1:], kp[:-1]
    same = cid[a] == cid[b]
    a, b = a[same], b[same]
    gene = (fam[a], fam[b], org[cid[a]], gs[a] - ge[b])
    kc = cid[kp]
    first = kp[np.concatenate([[True], kc[1:] != kc[:-1]])] if len(kp) else kp
    last = kp[np.concatenate([kc[1:] != kc[:-1], [True]])] if len(kp) else kp
    size = np.asarray(contig_size, np.int64)[cid[first]]
    ring = size >= 0
    first, last, size = first[ring], last[ring], size[ring]
    closing = (fam[first], fam[last], org[cid[first]], (size - ge[last]) + gs[first])
    return tuple(np.concatenate([x, y]) for x, y in zip(gene, closing))


def edge_table_arrays(graph, edge_bits, edge_counts, order, genes, gene_start, gene_end, contig_ptr, contig_org, contig_size, repeated=None,
                      f=None, d=None, bits_only=False):
    """What nemgpu_edge_table_create computes, in numpy.
    graph (ptr, idx), edge_bits uint32 [nnz][ceil(d/32)], edge_counts (extra_ptr, extra_org, extra_count) or None, order
    int32 [n]: the master as Master.arrays() gives it, d its organisms; the rest: the flat orders of ALL its organisms
    (family_table_arrays' layout) with every gene's START and END and every contig's circular size or -1.
      * the links: links_of_orders; lengths in 64 bits, one outside int32 raises ValueError;
      * an undirected link (a, b) belongs to edge (min, max) in master numbering, a self-loop is an edge;
      * the edges are the CSR entries with idx >= row in CSR order (E of them): src, dst;
      * weight: the organisms on the edge; len_min, len_max, len_distinct, len_sum (int64), len_mid_lo, len_mid_hi over
        the DISTINCT lengths of its links (the two middle elements of the sorted distinct lengths);
      * fam_mid_lo, fam_mid_hi [n]: the same middles over the family's distinct kept-gene lengths END - START;
      * org_first_edge [d]: the first edge that carries the organism, E if none;
      * the (edge, organism, count) triples of the links must be the master's edge bits and extras (bits_only: the bits
        alone): ValueError otherwise (the orders are not this master's);
      * contig_org must be non-decreasing.
    Returns a dict of those arrays."""
    ptr, idx = (np.asarray(a, np.int64) for a in graph)
    n, nnz = len(ptr) - 1, len(idx)
    if d is None:
        raise ValueError("edge_table_arrays: d, the master's organisms")
    order = np.asarray(order, np.int64)
    if f is None:
        f = len(repeated) if repeated is not None else max(int(order.max()) + 1 if n else 1, int(np.max(genes)) + 1 if len(genes) else 1)
    genes, contig_ptr, contig_org, repeated = check_projection_orders(genes, contig_ptr, contig_org, repeated, d, int(f))
    if (np.diff(contig_org) < 0).any():
        raise ValueError("edge_table_arrays: contig_org must be non-decreasing (the organisms walked in column order)")
    gene_start, gene_end = np.ascontiguousarray(gene_start, np.int32), np.ascontiguousarray(gene_end, np.int32)
    contig_size = np.ascontiguousarray(contig_size, np.int32)
    if gene_start.shape != genes.shape or gene_end.shape != genes.shape or contig_size.shape != contig_org.shape:
        raise ValueError("edge_table_arrays: gene_start [G], gene_end [G], contig_size [C]")
    inv = np.full(int(f), -2, np.int64)
    inside = order < f
    inv[order[inside]] = np.flatnonzero(inside)
    fam = inv[genes] if len(genes) else np.zeros(0, np.int64)
    kept = np.ones(len(genes), bool) if repeated is None else repeated[genes] == 0
    if (fam[kept] < 0).any():
        raise ValueError("these orders are not this master's: a kept gene's family is not in the master")
    glen = gene_end.astype(np.int64)[kept] - gene_start.astype(np.int64)[kept]
    la, lb, lorg, llen = links_of_orders(fam, kept, gene_start, gene_end, contig_ptr, contig_org, contig_size)
    for v in (glen, llen):
        if len(v) and (v.min() < INT32[0] or v.max() > INT32[1]):
            raise ValueError("a link's or a gene's length is outside int32")
    src, dst, entry = master_edges(ptr, idx)
    ne = len(entry)
    ekey = src.astype(np.int64) * n + dst
    by = np.argsort(ekey, kind="stable")
    lkey = np.minimum(la, lb) * n + np.maximum(la, lb)
    at = np.searchsorted(ekey[by], lkey)
    if len(lkey) and (ne == 0 or (ekey[by][np.minimum(at, ne - 1)] != lkey).any()):
        raise ValueError("these orders are not this master's: two adjacent kept genes' families are not an edge of the master")
    eid = by[at] if len(lkey) else np.zeros(0, np.int64)
    # the triples against the master's
    pair, copies = np.unique(eid * d + lorg, return_counts=True)
    bits = _edge_bits_bool(edge_bits, nnz, d)[entry] if ne else np.zeros((0, d), bool)
    want = np.flatnonzero(bits.ravel())
    if not np.array_equal(pair, want):
        raise ValueError("these orders are not this master's: their (edge, organism) pairs are not its edge bits")
    if not bits_only:
        count = np.ones(len(want), np.int64)
        if edge_counts is not None and len(edge_counts[1]):
            xptr, xorg, xcnt = (np.asarray(a, np.int64) for a in edge_counts)
            xe = np.repeat(np.arange(nnz, dtype=np.int64), np.diff(xptr))
            to_edge = np.full(nnz, -1, np.int64)
            to_edge[entry] = np.arange(ne)
            mine = to_edge[xe] >= 0
            xkey = to_edge[xe[mine]] * d + xorg[mine]
            where = np.searchsorted(want, xkey)
            if (where >= len(want)).any() or (want[np.minimum(where, len(want) - 1)] != xkey).any():
                raise ValueError("these orders are not this master's: an extra without its edge bit")
            count[where] = xcnt[mine]
        if not np.array_equal(copies, count):
            raise ValueError("these orders are not this master's: an (edge, organism) pair's number of links is not the master's count")
    le = _segments(eid, llen, ne)
    lf = _segments(fam[kept], glen, n)
    first = np.where(bits.any(axis=0), bits.argmax(axis=0), ne).astype(np.int32) if ne else np.zeros(d, np.int32)
    return dict(src=src, dst=dst, weight=bits.sum(axis=1).astype(np.int32), len_min=le["min"], len_max=le["max"], len_distinct=le["distinct"],
                len_sum=le["sum"], len_mid_lo=le["lo"], len_mid_hi=le["hi"], fam_mid_lo=lf["lo"], fam_mid_hi=lf["hi"], org_first_edge=first)


def attvalues_host(graph, edge_bits, edge_counts, attr_id, d, row0=0, rows=None):
    """What nemgpu_edge_table_attvalues writes, in numpy: for edges row0 .. row0 + rows - 1 (master_edges' numbering), per
    organism on the edge in increasing column order, the line `          <attvalue for="ID" value="COUNT" />\\n` with ID
    = attr_id[organism] and COUNT the pair's count (1, or the master's extra count).
    Returns (text uint8 [bytes], edge_end int64 [rows]: every edge's end offset)."""
    ptr, idx = graph
    _, _, entry = master_edges(ptr, idx)
    rows = len(entry) - row0 if rows is None else rows
    if row0 < 0 or rows <= 0 or row0 + rows > len(entry):
        raise ValueError("attvalues_host: rows outside the table")
    attr_id = np.asarray(attr_id, np.int64)
    if attr_id.shape != (d,) or (attr_id < 0).any():
        raise ValueError("attvalues_host: attr_id [d] >= 0")
    entry = entry[row0:row0 + rows]
    bits = _edge_bits_bool(edge_bits, len(idx), d)[entry]
    count = bits.astype(np.int64)
    if edge_counts is not None and len(edge_counts[1]):
        xptr, xorg, xcnt = (np.asarray(a, np.int64) for a in edge_counts)
        for r, t in enumerate(entry):
            a, b = xptr[t], xptr[t + 1]
            count[r, xorg[a:b]] = xcnt[a:b]
    parts, ends, size = [], np.zeros(rows, np.int64), 0
    for r in range(rows):
        line = "".join('          <attvalue for="%d" value="%d" />\n' % (attr_id[o], count[r, o]) for o in np.flatnonzero(bits[r])).encode()
        parts.append(line)
        size += len(line)
        ends[r] = size
    return np.frombuffer(b"".join(parts), np.uint8).copy(), ends


def read_metadata(file, organisms):
    """The CLI's parse of its -mt METADATA_FILE (command_line.py:439-447, 487): tab-separated, the first line the attribute
    names, line i + 1 the values of the i-th organism of `organisms` (pan.organisms), every element stripped; zip() cuts
    a line at the header's length and the lines at the organisms' number, as there.  file: a path or an iterable of
    lines.  Returns {organism: {attribute: value}}, both ordered: what write_gexf(metadata=) takes."""
    lines = open(file, encoding="utf-8") if isinstance(file, (str, bytes, os.PathLike)) else file
    try:
        names, rows = [], []
        for num, line in enumerate(lines):
            elements = [el.strip() for el in line.split("\t")]
            if num == 0:
                names = elements
            else:
                rows.append(dict(zip(names, elements)))
    finally:
        if lines is not file:
            lines.close()
    return dict(zip(list(organisms), rows))


def shell_init_from_metadata(metadata, attribute=None):
    """{value: set(organisms)} of one metadata column -- the first one (the -ss help text: "use the first column of
    metadata"), or `attribute` -- ready for Master.partition_shell(init_using_qual=).  The reference's own lines
    (command_line.py:494-497) use an organism's whole dict as the key and raise TypeError; this follows the help text."""
    init = {}
    for org, values in metadata.items():
        if attribute is None and not values:
            raise ValueError("shell_init_from_metadata: organism %r has no metadata" % (org,))
        key = next(iter(values)) if attribute is None else attribute
        if key not in values:
            raise ValueError("shell_init_from_metadata: organism %r has no attribute %r" % (org, key))
        init.setdefault(values[key], set()).add(org)
    return init


def rank_metadata(metadata, organisms, reserved=()):
    """export_to_GEXF's metadata ({organism: ordered {attribute: str}}) as the arrays the edge tables take, made on the
    host: per attribute its distinct values sorted as Python sorts str (code points: the order of their UTF-8 bytes too),
    every organism's value as its rank among them, and the values escaped as ElementTree escapes them, in one blob.
    ValueError: an organism of `organisms` without an entry; a value that is not a str; organisms whose attribute names or
    their order differ (the CLI's zip over one header row cannot make that); an attribute named like an organism or one
    of `reserved`; more than META_VALUES_MAX distinct values.
    Returns a dict: titles [n_attr], value_rank int32 [n_attr][d], n_values int32 [n_attr], value_ptr int64 [V + 1],
    value_text uint8 [bytes]."""
    organisms = list(organisms)
    for org in organisms:
        if org not in metadata:
            raise ValueError("metadata: organism %r is missing" % (org,))
    titles = list(metadata[organisms[0]]) if organisms else []
    taken = set(organisms) | set(reserved)
    for title in titles:
        if not isinstance(title, str) or title in taken:
            raise ValueError("metadata: attribute %r is named like an organism or another edge attribute" % (title,))
    for org in organisms:
        if list(metadata[org]) != titles:
            raise ValueError("metadata: organism %r has attributes %r, %r has %r" % (org, list(metadata[org]), organisms[0], titles))
        for title, value in metadata[org].items():
            if not isinstance(value, str):
                raise ValueError("metadata: %r of organism %r is %r, not a str" % (title, org, value))
    rank = np.zeros((len(titles), len(organisms)), np.int32)
    n_values, ptr, blob = [], [0], []
    for a, title in enumerate(titles):
        values = sorted(set(metadata[org][title] for org in organisms))
        if len(values) > META_VALUES_MAX:
            raise ValueError("metadata: attribute %r has %d distinct values, %d are held" % (title, len(values), META_VALUES_MAX))
        at = {value: k for k, value in enumerate(values)}
        rank[a] = [at[metadata[org][title]] for org in organisms]
        n_values.append(len(values))
        for value in values:
            blob.append(escape(value).encode("utf-8"))
            ptr.append(ptr[-1] + len(blob[-1]))
    return dict(titles=titles, value_rank=rank, n_values=np.asarray(n_values, np.int32), value_ptr=np.asarray(ptr, np.int64),
                value_text=np.frombuffer(b"".join(blob), np.uint8).copy())


def _check_ranks(value_rank, n_values):
    if (n_values < 1).any() or (n_values > META_VALUES_MAX).any():
        raise ValueError("metadata: an attribute has 1 .. %d values" % META_VALUES_MAX)
    if (value_rank < 0).any() or (value_rank >= n_values[:, None]).any():
        raise ValueError("metadata: a rank outside its attribute's values")


def _check_metadata(attr_id, value_rank, n_values, value_ptr, value_text, d):
    """the arrays nemgpu_edge_table_metadata takes, checked as it checks them: (attr_id, value_rank, n_values, value_ptr,
    value_text) contiguous in its types"""
    attr_id, n_values = np.ascontiguousarray(attr_id, np.int32), np.ascontiguousarray(n_values, np.int32)
    value_rank, value_ptr = np.ascontiguousarray(value_rank, np.int32), np.ascontiguousarray(value_ptr, np.int64)
    value_text = np.ascontiguousarray(value_text, np.uint8)
    n_attr = len(attr_id)
    if n_attr < 1 or attr_id.ndim != 1 or n_values.shape != (n_attr,) or value_rank.shape != (n_attr, d):
        raise ValueError("metadata: attr_id [n_attr], n_attr > 0, value_rank [n_attr][d], n_values [n_attr]")
    if (attr_id < 0).any():
        raise ValueError("metadata: an attr_id is negative")
    _check_ranks(value_rank, n_values)
    if value_ptr.shape != (int(n_values.sum()) + 1,) or value_ptr[0] != 0 or (np.diff(value_ptr) < 0).any() or value_ptr[-1] != len(value_text):
        raise ValueError("metadata: value_ptr [values + 1] from 0, ascending, to the bytes of value_text")
    return attr_id, value_rank, n_values, value_ptr, value_text


def _present_values(graph, edge_bits, value_rank, n_values, d, row0, rows, who):
    """per attribute bool [rows][n_values[a]]: the values of the organisms on each edge"""
    ptr, idx = graph
    _, _, entry = master_edges(ptr, idx)
    rows = len(entry) - row0 if rows is None else rows
    if row0 < 0 or rows <= 0 or row0 + rows > len(entry):
        raise ValueError(who + ": rows outside the table")
    bits = _edge_bits_bool(edge_bits, len(idx), d)[entry[row0:row0 + rows]]
    edge, org = np.nonzero(bits)
    out = []
    for rank, count in zip(np.asarray(value_rank, np.int64), n_values):
        present = np.zeros((rows, int(count)), bool)
        present[edge, rank[org]] = True
        out.append(present)
    return out


def edge_metadata_arrays(graph, edge_bits, value_rank, n_values, d, row0=0, rows=None):
    """What nemgpu_edge_table_metamasks computes, in numpy: for edges row0 .. row0 + rows - 1 (master_edges' numbering)
    and every attribute the set of the values of the organisms on the edge, as a bit mask over the values' ranks:
    uint32 [rows][W], W the sum of ceil(n_values[a] / 32), an edge's words the attributes' one after the other, bit
    (rank & 31) of word (rank >> 5).  value_rank int32 [n_attr][d], n_values int32 [n_attr] (rank_metadata)."""
    value_rank, n_values = np.asarray(value_rank, np.int64), np.asarray(n_values, np.int64)
    if value_rank.shape != (len(n_values), d) or not len(n_values):
        raise ValueError("edge_metadata_arrays: value_rank [n_attr][d], n_values [n_attr], n_attr > 0")
    _check_ranks(value_rank, n_values)
    words = []
    for present in _present_values(graph, edge_bits, value_rank, n_values, d, row0, rows, "edge_metadata_arrays"):
        padded = np.zeros((present.shape[0], (present.shape[1] + 31) // 32 * 32), np.uint8)
        padded[:, :present.shape[1]] = present
        words.append(np.packbits(padded, axis=1, bitorder="little").view("<u4"))
    return np.ascontiguousarray(np.concatenate(words, axis=1), np.uint32)


def metavalues_host(graph, edge_bits, attr_id, value_rank, n_values, value_ptr, value_text, d, row0=0, rows=None):
    """What nemgpu_edge_table_metavalues writes, in numpy: for edges row0 .. row0 + rows - 1, per attribute in order, the
    line `          <attvalue for="ID" value="V1|V2|..." />\n` with ID = attr_id[a] and the values present on the edge
    (edge_metadata_arrays) in increasing rank, their bytes value_text[value_ptr[v] : value_ptr[v + 1]].
    Returns (text uint8 [bytes], edge_end int64 [rows]: every edge's end offset)."""
    attr_id, value_rank, n_values, value_ptr, value_text = _check_metadata(attr_id, value_rank, n_values, value_ptr, value_text, d)
    present = _present_values(graph, edge_bits, value_rank, n_values, d, row0, rows, "metavalues_host")
    blob, base = value_text.tobytes(), np.concatenate([[0], np.cumsum(n_values)])
    values = [[blob[value_ptr[base[a] + k]:value_ptr[base[a] + k + 1]] for k in range(n_values[a])] for a in range(len(attr_id))]
    rows = present[0].shape[0]
    parts, ends, size = [], np.zeros(rows, np.int64), 0
    for r in range(rows):
        for a, mine in enumerate(present):
            line = b'          <attvalue for="%d" value="' % attr_id[a] + b"|".join(values[a][k] for k in np.flatnonzero(mine[r])) + b'" />\n'
            parts.append(line)
            size += len(line)
        ends[r] = size
    return np.frombuffer(b"".join(parts), np.uint8).copy(), ends


def _bind_edges(lib):
    lib.nemgpu_edge_table_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.nemgpu_edge_table_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 3
    lib.nemgpu_edge_table_fetch.argtypes = [C.c_void_p] * 13
    lib.nemgpu_edge_table_attvalues_size.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.nemgpu_edge_table_attvalues.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                                C.c_void_p]
    lib.nemgpu_edge_table_metadata.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.nemgpu_edge_table_metamasks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.nemgpu_edge_table_metavalues_size.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.nemgpu_edge_table_metavalues.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    lib.nemgpu_edge_table_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_edge_table_destroy.restype = None
    return lib


class _Edges:
    """what both edge tables share: EdgeTable on the device, HostEdgeTable in numpy"""

    def arrays(self):
        return {name: getattr(self, name) for name in EDGE_FIELDS}

    def attribute_ids(self, first_id, organisms=True, n_attr=0):
        """the ids networkx gives the edge attributes when its counter stands at first_id: it numbers a title where it
        first meets it, walking the edges in order and, inside an edge, its organisms (in column order), then the four
        length_*, then the n_attr metadata attributes (every edge has an organism, so edge 0 has them all).  Returns
        (attr_id int32 [d], 0 for an organism on no edge; the titles in id order as (id, what), what an organism's column,
        one of the length titles or ("metadata", j))."""
        attr_id, titles, k = np.zeros(self.d, np.int32), [], first_id
        behind = list(LENGTH_TITLES) + [("metadata", j) for j in range(n_attr)]
        if self.n_edges == 0:
            return attr_id, titles
        first = self.org_first_edge.astype(np.int64)
        met = [int(o) for o in np.lexsort((np.arange(self.d), first)) if first[o] < self.n_edges] if organisms else []
        placed = False
        for o in met:
            if first[o] > 0 and not placed:
                titles += [(k + j, what) for j, what in enumerate(behind)]
                k, placed = k + len(behind), True
            attr_id[o] = k
            titles.append((k, o))
            k += 1
        if not placed:
            titles += [(k + j, what) for j, what in enumerate(behind)]
        return attr_id, titles

    def _hold_metadata(self, held):
        """_check_metadata's arrays, for the metavalues calls and for _batches"""
        self._metadata = held
        self._metadata_longest = int(np.diff(held[3]).max(initial=0))

    def _metadata_bound(self):
        """per edge, above the bytes a metavalues call takes for it on the device: every attribute's line with its widest
        id and as many of its longest value as the edge can have, and the edge's masks"""
        _, _, n_values, _, _ = self._metadata
        weight = self.weight.astype(np.int64)
        bound = np.full(self.n_edges, 4 * int(((n_values.astype(np.int64) + 31) // 32).sum()), np.int64)
        for count in n_values:
            bound += LINE_FIXED + 10 + np.minimum(weight, int(count)) * (self._metadata_longest + 1)
        return bound

    def _batches(self, budget, organisms=True, metadata=False):
        """(row0, rows) covering the edges, each batch's text within the budget by the widest line (one edge where an edge
        alone is above it): the organism lines (organisms) and the metadata lines (metadata: set_metadata's) together"""
        bound = self.weight.astype(np.int64) * LINE_MAX if organisms else np.zeros(self.n_edges, np.int64)
        if metadata:
            bound = bound + self._metadata_bound()
        bound = np.cumsum(bound)
        row0 = 0
        while row0 < self.n_edges:
            base = bound[row0 - 1] if row0 else 0
            rows = max(1, int(np.searchsorted(bound, base + budget, side="right")) - row0)
            yield row0, rows
            row0 += rows


class EdgeTable(DeviceTable, _Edges):
    """The edge table of a master on the device (nemgpu_edge_table_create) with its arrays read back: src, dst, weight,
    len_min, len_max, len_distinct, len_mid_lo, len_mid_hi int32 [E], len_sum int64 [E], fam_mid_lo, fam_mid_hi int32 [n],
    org_first_edge int32 [d].  The master must stay open as long as the table writes."""
    KIND, ARRAYS, COUNT = "edge_table", EDGE_FIELDS, "n_edges"

    def __init__(self, master, genes, gene_start, gene_end, contig_ptr, contig_org, contig_size, repeated=None, f=None):
        self.lib = _bind_edges(master.lib)
        f, genes, contig_ptr, contig_org, repeated = self._orders(master, genes, contig_ptr, contig_org, repeated, f)
        gene_start, gene_end = np.ascontiguousarray(gene_start, np.int32), np.ascontiguousarray(gene_end, np.int32)
        contig_size = np.ascontiguousarray(contig_size, np.int32)
        if gene_start.shape != genes.shape or gene_end.shape != genes.shape or contig_size.shape != contig_org.shape or not len(genes):
            raise ValueError("edge table: genes [G], gene_start [G], gene_end [G], G > 0, contig_size [C]")
        self._create(master, f, genes, (gene_start, gene_end), contig_ptr, contig_org, (contig_size,), repeated)

    def _sizes(self):
        return (self.n_edges,) * 9 + (self.n, self.n, self.d)

    def _attr_id(self, attr_id):
        attr_id = np.ascontiguousarray(attr_id, np.int32)
        if attr_id.shape != (self.d,):
            raise ValueError("attvalues: attr_id [d]")
        return attr_id

    def attvalues_size(self, attr_id, row0, rows):
        attr_id, size = self._attr_id(attr_id), C.c_int64()
        self._call("attvalues_size", self._h, self.master._h, attr_id.ctypes.data, int(row0), int(rows), C.byref(size))
        return size.value

    def attvalues(self, attr_id, row0=0, rows=None, out=None):
        """The organism lines of edges row0 .. row0 + rows - 1, formatted on the device (nemgpu_edge_table_attvalues;
        attvalues_host states them): (text uint8 [bytes], edge_end int64 [rows]).  out: a uint8 buffer to write into (too
        small: NemGpuError that says the size needed, nothing written)."""
        rows = self.n_edges - row0 if rows is None else rows
        attr_id = self._attr_id(attr_id)
        if out is None:
            out = np.empty(max(self.attvalues_size(attr_id, row0, rows), 1), np.uint8)
        ends, needed = np.zeros(max(rows, 1), np.int64), C.c_int64()
        return self._text("attvalues", out, needed, self._h, self.master._h, attr_id.ctypes.data, int(row0), int(rows), out.ctypes.data, out.size,
                          C.byref(needed), ends.ctypes.data), ends[:rows]


    def set_metadata(self, attr_id, value_rank, n_values, value_ptr, value_text):
        """The metadata the next metavalues calls format (rank_metadata's arrays; attr_id [n_attr]: the attributes' ids),
        uploaded once (nemgpu_edge_table_metadata) and kept until the next call or close().  Outside its bounds: ValueError
        here, NemGpuError from the library; the table then keeps the metadata it had."""
        held = _check_metadata(attr_id, value_rank, n_values, value_ptr, value_text, self.d)
        self._call("metadata", self._h, len(held[0]), *(a.ctypes.data for a in held))
        self._hold_metadata(held)

    def metamasks(self, row0=0, rows=None):
        """The present-value masks of edges row0 .. row0 + rows - 1 from the device (nemgpu_edge_table_metamasks;
        edge_metadata_arrays states them): uint32 [rows][W]."""
        rows = self.n_edges - row0 if rows is None else rows
        words = int(((self._metadata[2].astype(np.int64) + 31) // 32).sum())
        out = np.zeros((max(rows, 1), words), np.uint32)
        self._call("metamasks", self._h, self.master._h, int(row0), int(rows), out.ctypes.data)
        return out[:rows]

    def metavalues_size(self, row0, rows):
        size = C.c_int64()
        self._call("metavalues_size", self._h, self.master._h, int(row0), int(rows), C.byref(size))
        return size.value

    def metavalues(self, row0=0, rows=None, out=None):
        """The metadata lines of edges row0 .. row0 + rows - 1, formatted on the device (nemgpu_edge_table_metavalues;
        metavalues_host states them): (text uint8 [bytes], edge_end int64 [rows]).  out: as attvalues'."""
        rows = self.n_edges - row0 if rows is None else rows
        if out is None:
            out = np.empty(max(self.metavalues_size(row0, rows), 1), np.uint8)
        ends, needed = np.zeros(max(rows, 1), np.int64), C.c_int64()
        return self._text("metavalues", out, needed, self._h, self.master._h, int(row0), int(rows), out.ctypes.data, out.size, C.byref(needed),
                          ends.ctypes.data), ends[:rows]


class HostEdgeTable(_Edges):
    """The same table from the numpy statement (edge_table_arrays, attvalues_host): what the device is held against, and a
    table for a caller who has the master's arrays on the host.  graph, edge_bits, edge_counts, order, d: the master's."""

    def __init__(self, graph, edge_bits, edge_counts, order, genes, gene_start, gene_end, contig_ptr, contig_org, contig_size, repeated=None,
                 f=None, d=None, bits_only=False):
        self._master = (graph, edge_bits, edge_counts)
        for name, a in edge_table_arrays(graph, edge_bits, edge_counts, order, genes, gene_start, gene_end, contig_ptr, contig_org, contig_size,
                                         repeated, f, d, bits_only).items():
            setattr(self, name, a)
        self.n, self.d, self.n_edges = len(graph[0]) - 1, d, len(self.src)

    def attvalues(self, attr_id, row0=0, rows=None):
        return attvalues_host(*self._master, attr_id, self.d, row0, rows)

    def attvalues_size(self, attr_id, row0, rows):
        return len(self.attvalues(attr_id, row0, rows)[0])

    def set_metadata(self, attr_id, value_rank, n_values, value_ptr, value_text):
        self._hold_metadata(_check_metadata(attr_id, value_rank, n_values, value_ptr, value_text, self.d))

    def metamasks(self, row0=0, rows=None):
        return edge_metadata_arrays(*self._master[:2], self._metadata[1], self._metadata[2], self.d, row0, rows)

    def metavalues(self, row0=0, rows=None):
        return metavalues_host(*self._master[:2], *self._metadata, self.d, row0, rows)

    def metavalues_size(self, row0, rows):
        return len(self.metavalues(row0, rows)[0])

    def close(self):
        pass


def escape(text):
    """XML attribute escaping as ElementTree does it (_escape_attrib)"""
    for a, b in (("&", "&amp;"), ("<", "&lt;"), (">", "&gt;"), ('"', "&quot;"), ("\r", "&#13;"), ("\n", "&#10;"), ("\t", "&#09;")):
        if a in text:
            text = text.replace(a, b)
    return text


_ESCAPED = {ord("&"): b"&amp;", ord("<"): b"&lt;", ord(">"): b"&gt;", ord('"'): b"&quot;", ord("\r"): b"&#13;", ord("\n"): b"&#10;",
            ord("\t"): b"&#09;"}
NODE_TAIL = 6                                                 # partition, partition_exact and the four length_* behind a node's organisms


def escape_bytes(data):
    """escape() on bytes: the same seven replacements, every other byte (those >= 0x80 too) as it is"""
    if not any(ch in _ESCAPED for ch in data):
        return bytes(data)
    return b"".join(_ESCAPED.get(ch, bytes((ch,))) for ch in data)


def node_attribute_ids(first, n, tail=NODE_TAIL):
    """The ids networkx gives the node attributes, a title numbered where it is first met, from first int [d]: every
    organism's first family in master order with a kept gene of it (n: none), when `tail` titles follow a node's
    organisms.  Full: nb_genes 0, node 0's first organism, name, product, node 0's other organisms, the tail, then every
    organism first met at a later node in (node, organism) order; light: nb_genes 0, name 1, product 2, the tail.
    Returns (org_id int32 [d], -1 for an organism without a kept gene; name_id (light, full), product's is one more;
    titles (light, full): each the titles in id order -- "nb_genes", "name", "product", ("tail", j) or an organism's
    column; both empty when n is 0)."""
    first = np.asarray(first, np.int64)
    org_id = np.full(len(first), -1, np.int32)
    if n == 0:
        return org_id, (1, 1), ([], [])
    met = [int(o) for o in np.lexsort((np.arange(len(first)), first)) if first[o] < n]
    here = [o for o in met if first[o] == 0]
    full = ["nb_genes"] + here[:1] + ["name", "product"] + here[1:] + [("tail", j) for j in range(tail)] + met[len(here):]
    for k, what in enumerate(full):
        if isinstance(what, int):
            org_id[what] = k
    return org_id, (1, full.index("name")), (["nb_genes", "name", "product"] + [("tail", j) for j in range(tail)], full)


def node_text_host(x, order, genes, contig_ptr, contig_org, repeated, text, spans, f=None, d=None, tail=NODE_TAIL):
    """What nemgpu_node_table_* compute, in plain Python / numpy on flat arrays: the nodes' <attvalue> text of write_gexf
    without the nested annotations.
    x, order: the master's matrix (uint8 [n][d], or packed rows with d=) and its family order (master family i is caller
    id order[i]); genes, contig_ptr, contig_org, repeated uint8 [f], f: the flat orders of ALL the master's organisms
    (family_table_arrays' layout), contig_org non-decreasing; text: bytes; spans = (span_off int64 [3][g], span_len int32
    [3][g]): every gene's ID, NAME and PRODUCT in text (the loader's SPAN_ID, SPAN_NAME, SPAN_PRODUCT; an absent NAME or
    PRODUCT is an empty span).
      * a gene is kept when its id is not flagged in `repeated`: one global set.  Repeated sets per organism (a dict, as a
        master grown by add_annotations holds them) are refused with ValueError: they stay on the annotations path,
        unless the orders already carry them gene by gene (table_orders' one flagged id);
      * per family i in master order: the organisms with a kept gene of it in walk order (increasing column), per
        organism its kept genes' IDs in walk order, its distinct NAME byte strings in first-occurrence order over the
        walk (the empty string is a value like any other) and its distinct PRODUCT byte strings by the same rule;
      * a node's text is one slice: the first organism's line, the name line, the product line, the other organisms'
        lines, each `          <attvalue for="ID" value="A|B|..." />\\n` with the pieces escaped (escape_bytes); light:
        the name and product lines alone;
      * the ids: node_attribute_ids;
      * the kept genes' (family, organism) cells must be exactly the master's presence bits, every kept gene's family a
        family of the master, every span inside the text: ValueError otherwise.
    Returns a dict: nb_genes int32 [n], first int32 [d], org_id int32 [d], name_id (light, full), titles (light, full),
    text (light, full) uint8, node_end (light, full) int64 [n]."""
    from .matrix import _presence
    if isinstance(repeated, dict):
        raise ValueError("node_text_host: repeated sets per organism stay on the annotations path (one global set of flagged ids is taken)")
    present = _presence(x, d)
    n, d = present.shape
    order = np.asarray(order, np.int64)
    if order.shape != (n,):
        raise ValueError("node_text_host: order [n]")
    if f is None:
        f = len(repeated) if repeated is not None else max(int(order.max()) + 1 if n else 1, int(np.max(genes)) + 1 if len(genes) else 1)
    genes, contig_ptr, contig_org, repeated = check_projection_orders(genes, contig_ptr, contig_org, repeated, d, int(f))
    if (np.diff(contig_org) < 0).any():
        raise ValueError("node_text_host: contig_org must be non-decreasing (the organisms walked in column order)")
    g = len(genes)
    off, ln = np.asarray(spans[0], np.int64), np.asarray(spans[1], np.int64)
    blob = bytes(memoryview(np.ascontiguousarray(text, np.uint8))) if isinstance(text, np.ndarray) else bytes(text)
    if off.shape != (3, g) or ln.shape != (3, g):
        raise ValueError("node_text_host: spans = (span_off [3][g], span_len [3][g])")
    if g and ((off < 0).any() or (ln < 0).any() or (off + ln > len(blob)).any()):
        raise ValueError("node_text_host: a span is past the end of the text")
    inv = np.full(int(f), -2, np.int64)
    inside = order < f
    inv[order[inside]] = np.flatnonzero(inside)
    fam = inv[genes] if g else np.zeros(0, np.int64)
    kept = np.ones(g, bool) if repeated is None else repeated[genes] == 0
    if (fam[kept] < 0).any():
        raise ValueError("these orders are not this master's: a kept gene's family is not in the master")
    org = np.repeat(contig_org.astype(np.int64), np.diff(contig_ptr))
    derived = np.zeros(n * d, bool)
    derived[np.unique(fam[kept] * d + org[kept])] = True
    if not np.array_equal(derived.reshape(n, d), present):
        raise ValueError("these orders are not this master's: their cells are not its presence bits")
    first = np.where(present.any(axis=0), present.argmax(axis=0), n).astype(np.int32) if n else np.full(d, 0, np.int32)
    org_id, name_id, titles = node_attribute_ids(first, n, tail)
    kp = np.flatnonzero(kept)
    walk = kp[np.argsort(fam[kp], kind="stable")]             # a family's kept genes: one segment, in walk order
    start = np.searchsorted(fam[walk], np.arange(n + 1))

    def piece(k, p):
        return escape_bytes(blob[off[k, p]:off[k, p] + ln[k, p]])

    def line(k, pieces):
        return b'          <attvalue for="%d" value="' % k + b"|".join(pieces) + b'" />\n'

    parts, ends = ([], []), (np.zeros(n, np.int64), np.zeros(n, np.int64))
    size = [0, 0]
    for i in range(n):
        cells, names, products = {}, {}, {}                   # (insertion-ordered sets)
        for p in walk[start[i]:start[i + 1]]:
            cells.setdefault(int(org[p]), []).append(piece(0, p))
            names[piece(1, p)] = None
            products[piece(2, p)] = None
        organisms = [line(org_id[o], ids) for o, ids in cells.items()]
        for full in (0, 1):
            both = line(name_id[full], names) + line(name_id[full] + 1, products)
            node = b"".join(organisms[:1]) + both + b"".join(organisms[1:]) if full else both
            parts[full].append(node)
            size[full] += len(node)
            ends[full][i] = size[full]
    return dict(nb_genes=np.diff(start).astype(np.int32), first=first, org_id=org_id, name_id=name_id, titles=titles,
                text=tuple(np.frombuffer(b"".join(p), np.uint8).copy() for p in parts), node_end=ends)


def _bind_nodes(lib):
    lib.nemgpu_node_table_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_int]
    lib.nemgpu_node_table_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.nemgpu_node_table_finish.argtypes = [C.c_void_p, C.c_void_p]
    lib.nemgpu_node_table_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 3
    lib.nemgpu_node_table_fetch.argtypes = [C.c_void_p] * 3
    lib.nemgpu_node_table_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    lib.nemgpu_node_table_lines_size.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.nemgpu_node_table_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    lib.nemgpu_node_table_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_node_table_destroy.restype = None
    return lib


class _Nodes:
    """what both node tables share: NodeTable on the device, HostNodeTable in plain Python.  n, d, nb_genes int32 [n],
    first int32 [d]; after _layout(tail): org_id, name_id, node_end (light, full), _titles (light, full)."""
    tail = None

    def titles(self, full=True, tail=NODE_TAIL):
        """the node attributes' titles in id order, as node_attribute_ids gives them; the text calls that follow format
        for this numbering"""
        if tail != self.tail:
            self._layout(int(tail))
        return self._titles[1 if full else 0]

    def ids(self, tail=NODE_TAIL):
        """(org_id int32 [d], name_id (light, full)) of that numbering"""
        self.titles(True, tail)
        return self.org_id, self.name_id

    def _ends(self, full):
        if self.tail is None:
            self._layout(NODE_TAIL)
        return self.node_end[1 if full else 0]

    def _rows(self, row0, rows):
        rows = self.n - row0 if rows is None else rows
        if row0 < 0 or rows <= 0 or row0 + rows > self.n:
            raise ValueError("node table: rows outside the table")
        return rows

    def lines_size(self, row0=0, rows=None, full=True):
        """the bytes of the text of nodes row0 .. row0 + rows - 1"""
        rows, ends = self._rows(row0, rows), self._ends(full)
        return int(ends[row0 + rows - 1] - (ends[row0 - 1] if row0 else 0))

    def _batches(self, budget, full=True):
        """(row0, rows) covering the nodes, each batch's text within the budget (one node where a node alone is above it)"""
        ends, row0 = self._ends(full), 0
        while row0 < self.n:
            base = ends[row0 - 1] if row0 else 0
            rows = max(1, int(np.searchsorted(ends, base + budget, side="right")) - row0)
            yield row0, rows
            row0 += rows


class NodeTable(DeviceTable, _Nodes):
    """The node text of a master on the device (nemgpu_node_table_*; node_text_host states it).  Made from the flat orders;
    add_text() takes the load's text batch by batch, finish() closes it: Master.node_table does all three.  The master
    must stay open as long as the table writes."""
    KIND = "node_table"

    def __init__(self, master, genes, contig_ptr, contig_org, repeated=None, f=None, _hash_bits=0):
        self.lib = _bind_nodes(master.lib)
        f, genes, contig_ptr, contig_org, repeated = self._orders(master, genes, contig_ptr, contig_org, repeated, f)
        if not len(genes):
            raise ValueError("node table: genes [G], G > 0")
        self.master, self._h = master, C.c_void_p()
        self._call("create", C.byref(self._h), master._h, f, genes.ctypes.data, len(genes), contig_ptr.ctypes.data, contig_org.ctypes.data,
                   len(contig_org), repeated.ctypes.data if repeated is not None else None, int(_hash_bits))
        v = [C.c_int() for _ in range(3)]
        self._call("shape", self._h, *(C.byref(a) for a in v))
        self.n, self.d, self.g = (a.value for a in v)
        self.nb_genes, self.first = np.zeros(self.n, np.int32), np.zeros(self.d, np.int32)
        self._call("fetch", self._h, self.nb_genes.ctypes.data if self.n else None, self.first.ctypes.data if self.d else None)

    def add_text(self, text, gene0, gene1, span_off, span_len):
        """the text of genes gene0 .. gene1 - 1 (the batches in order): text uint8 or bytes, span_off int64 [3][gene1 -
        gene0] into it, span_len int32 of the same shape"""
        text = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8)
        span_off, span_len = np.ascontiguousarray(span_off, np.int64), np.ascontiguousarray(span_len, np.int32)
        if span_off.shape != (3, gene1 - gene0) or span_len.shape != span_off.shape:
            raise ValueError("node table: span_off, span_len [3][gene1 - gene0]")
        self._call("text", self._h, self.master._h, text.ctypes.data if text.size else None, text.size, int(gene0), int(gene1),
                   span_off.ctypes.data, span_len.ctypes.data)

    def finish(self):
        self._call("finish", self._h, self.master._h)
        return self

    def _layout(self, tail):
        org_id, name_id = np.zeros(self.d, np.int32), np.zeros(2, np.int32)
        ends = np.zeros(max(self.n, 1), np.int64), np.zeros(max(self.n, 1), np.int64)
        self._call("ids", self._h, self.master._h, tail, org_id.ctypes.data, name_id.ctypes.data, ends[1].ctypes.data, ends[0].ctypes.data)
        self.org_id, self.name_id = org_id, (int(name_id[0]), int(name_id[1]))
        self.node_end = ends[0][:self.n], ends[1][:self.n]
        self._titles = node_attribute_ids(self.first, self.n, tail)[2]
        self.tail = tail

    def lines(self, row0=0, rows=None, full=True, out=None):
        """The text of nodes row0 .. row0 + rows - 1, formatted on the device (nemgpu_node_table_lines): (text uint8
        [bytes], node_end int64 [rows]).  out: a uint8 buffer to write into (too small: NemGpuError that says the size
        needed, nothing written)."""
        rows = self._rows(row0, rows)
        if out is None:
            out = np.empty(max(self.lines_size(row0, rows, full), 1), np.uint8)
        ends, needed = np.zeros(rows, np.int64), C.c_int64()
        return self._text("lines", out, needed, self._h, self.master._h, 1 if full else 0, int(row0), int(rows), out.ctypes.data, out.size,
                          C.byref(needed), ends.ctypes.data), ends


class HostNodeTable(_Nodes):
    """The same table from the host statement (node_text_host): what the device is held against, and a table for a caller
    who has the master's matrix on the host.  x, order, d: the master's; the rest as node_text_host takes it."""

    def __init__(self, x, order, genes, contig_ptr, contig_org, repeated, text, spans, f=None, d=None):
        self._args = (x, order, genes, contig_ptr, contig_org, repeated, text, spans, f, d)
        self._layout(NODE_TAIL)
        self.n, self.d = len(self.nb_genes), len(self.first)

    def _layout(self, tail):
        made = node_text_host(*self._args, tail=tail)
        self.nb_genes, self.first, self.org_id, self.name_id = made["nb_genes"], made["first"], made["org_id"], made["name_id"]
        self._titles, self._text, self.node_end, self.tail = made["titles"], made["text"], made["node_end"], tail

    def lines(self, row0=0, rows=None, full=True):
        rows, ends, k = self._rows(row0, rows), self._ends(full), 1 if full else 0
        base = int(ends[row0 - 1]) if row0 else 0
        return self._text[k][base:int(ends[row0 + rows - 1])].copy(), ends[row0:row0 + rows] - base

    def close(self):
        pass


def _median(lo, hi, count):
    """utils.median of the reference from the two middle elements: the element itself (an int) when the count is odd, their
    true division when it is even; export_to_GEXF wraps it in float()"""
    return float(int(lo)) if count % 2 else float((int(lo) + int(hi)) / 2)


def _lengths(total, count, lo, hi, low, high):
    """the four values (as text) of length_avg, length_med, length_min, length_max"""
    return (str(float(int(total)) / max(int(count), 1)), str(_median(lo, hi, int(count))), str(int(low)), str(int(high)))


def write_gexf(path, partitions, family_table, edge_table, annotations=None, all_node_attributes=True, all_edge_attributes=True, compressed=False,
               budget=TEXT_BUDGET, positions=None, subpartition=None, metadata=None, node_table=None):
    """<path>.gexf (compressed: <path>.gexf.gz through gzip) as PPanGGOLiN.export_to_GEXF and networkx's write_gexf write
    it for a partitioned nx.Graph (ppanggolin.py:1294-1362), streamed: no networkx, no tree.  partitions: what
    Master.partition returned, or uint8 [n]; family_table, edge_table: Master.family_table / Master.edge_table (or their
    host forms) of the same master and annotations; annotations: the ones the tables were made from, walked in column
    order (the genes' ids, names and products are read from them).  all_node_attributes / all_edge_attributes False: the
    `_light` export, without the organism keys; it formats no text on the device.  An edge's organism lines are the
    device's bytes, a slice per edge.  positions: float64 [n][2] in master order (Layout.positions(), layout.py): every
    node gets the <viz:position> that compute_layout's dict makes networkx write (ppanggolin.py:1285-1292), z = 2 for a
    persistent family, 1 for a shell one, 0 otherwise.  subpartition: (name, {family: value}) -- the node attribute that
    partition_shell sets on every node (ppanggolin.py:1243-1247; Master.partition_shell's .subpart_name and
    .node_attribute): one more string attribute, where the node's data holds it, behind partition_exact.
    metadata: export_to_GEXF's metadata= (:1339-1354; read_metadata makes it from the CLI's file): {organism name:
    ordered {attribute: str}} with an entry per organism of the master.  Every edge gets, per attribute, one string
    attribute behind length_max whose value is "|".join(sorted(set of the values of the edge's organisms)) -- in the full
    and in the light export, which then formats these lines (and still no organism lines) on the device.  The ranking,
    the escaping and the values' blob are made on the host (rank_metadata), the sets and the lines on the device, a
    slice per edge.  ValueError: a missing organism; a value that is not a str; organisms whose attribute names or their
    order differ (the CLI's zip over one header row cannot produce that); an attribute named like an organism, like
    weight or like a length_* title.  An empty metadata (or one without attributes) is none, as in the reference.
    node_table: Master.node_table's (or a HostNodeTable) of the same master and orders; annotations may then be None: the
    genes are not walked, a node's organism, name and product lines are the table's bytes, a slice per node, and the
    host writes a node's head, its viz lines, nb_genes and the tail values around them, one write per node.  Everything
    else is as without it, and the file is the same byte for byte."""
    ft, et, nt = family_table, edge_table, node_table
    names, orgs = ft.names, ft.organism_names
    if names is None or orgs is None:
        raise ValueError("write_gexf: a master that carries names (from_annotations, from_graph, add_annotations)")
    if ft.n != et.n or ft.d != et.d:
        raise ValueError("write_gexf: the two tables are not of one master")
    n, d = ft.n, ft.d
    longs = _long_names(partitions, names, n)
    if positions is not None:
        positions = np.asarray(positions, np.float64)
        if positions.shape != (n, 2):
            raise ValueError("write_gexf: positions float64 [n][2]")
    tail = (("partition", "string"), ("partition_exact", "string"), ("length_avg", "double"), ("length_med", "double"), ("length_min", "long"),
            ("length_max", "long"))
    if subpartition is not None:
        tail = tail[:2] + ((subpartition[0], "string"),) + tail[2:]
    # the attribute ids: one counter over the nodes, then the edges, a title numbered where it is first met
    node_ids, node_titles = {}, []

    def node_id(title, kind):
        if title not in node_ids:
            node_ids[title] = len(node_ids)
            node_titles.append((title, kind))
        return node_ids[title]

    if nt is not None:
        if nt.n != n or nt.d != d or not np.array_equal(nt.nb_genes, ft.nb_genes):
            raise ValueError("write_gexf: the node table is not of the family table's master and orders")
        for what in nt.titles(all_node_attributes, len(tail)):
            if isinstance(what, tuple):
                node_id(*tail[what[1]])
            elif isinstance(what, str):
                node_id(what, "long" if what == "nb_genes" else "string")
            else:
                node_id(orgs[what], "string")
    else:
        if annotations is None:
            raise ValueError("write_gexf: annotations, or a node_table")
        index = {name: i for i, name in enumerate(names)}
        gene_names, products, cells = [dict() for _ in names], [dict() for _ in names], [dict() for _ in names]   # (insertion-ordered sets)
        by_org = ft.repeated_names if isinstance(ft.repeated_names, dict) else None
        for org, contigs in annotations.items():
            skipped = by_org[org] if by_org is not None else ft.repeated_names
            for annot in contigs.values():
                for gene, info in annot.items():
                    if info[FAMILY] in skipped:
                        continue
                    i = index[info[FAMILY]]
                    gene_names[i][info[NAME]] = None
                    products[i][info[PRODUCT]] = None
                    cells[i].setdefault(org, dict())[gene] = None
        node_keys = []                                            # per family: the organisms before and after name and product
        for i in range(n):
            present = list(cells[i]) if all_node_attributes else []
            node_id("nb_genes", "long")
            for org in present[:1]:
                node_id(org, "string")
            node_id("name", "string")
            node_id("product", "string")
            for org in present[1:]:
                node_id(org, "string")
            for title, kind in tail:
                node_id(title, kind)
            node_keys.append(present)
    meta = rank_metadata(metadata, orgs, ("weight",) + LENGTH_TITLES) if metadata else None
    if meta is not None and not (meta["titles"] and et.n_edges):
        meta = None
    attr_id, edge_titles = et.attribute_ids(len(node_ids), organisms=all_edge_attributes, n_attr=len(meta["titles"]) if meta else 0)
    if meta is not None:
        et.set_metadata([k for k, what in edge_titles if isinstance(what, tuple)], meta["value_rank"], meta["n_values"], meta["value_ptr"],
                        meta["value_text"])
    out = gzip.open(path + ".gexf.gz", "wb") if compressed else open(path + ".gexf", "wb")
    with out:
        w = out.write
        w((HEAD % time.strftime("%Y-%m-%d")).encode())
        if edge_titles:
            w(b'    <attributes mode="static" class="edge">\n')
            for k, what in edge_titles:
                if isinstance(what, tuple):
                    title, kind = meta["titles"][what[1]], "string"
                else:
                    title, kind = (what, "double" if what in ("length_avg", "length_med") else "long") if isinstance(what, str) else (orgs[what], "long")
                w(('      <attribute id="%d" title="%s" type="%s" />\n' % (k, escape(title), kind)).encode())
            w(b"    </attributes>\n")
        if node_titles:
            w(b'    <attributes mode="static" class="node">\n')
            for k, (title, kind) in enumerate(node_titles):
                w(('      <attribute id="%d" title="%s" type="%s" />\n' % (k, escape(title), kind)).encode())
            w(b"    </attributes>\n")
        w(b"    <nodes>\n" if n else b"    <nodes />\n")
        att = '          <attvalue for="%d" value="%s" />\n'

        def node(i, middle):
            """node i: its head, viz lines and nb_genes; middle(lines) adds its organism, name and product lines; the tail"""
            nb_org = int(ft.nb_org[i])
            exact = "core_exact" if nb_org == d else "accessory"
            color = COLORS_RGB[longs[i] if longs[i] != "undefined" else exact]
            name = escape(names[i])
            lines = ['      <node id="%s" label="%s">\n' % (name, name),
                     '        <viz:color r="%d" g="%d" b="%d" a="0" />\n' % color,
                     '        <viz:size value="%d" />\n' % nb_org]
            if positions is not None:
                lines.append('        <viz:position x="%s" y="%s" z="%d" />\n'
                             % (str(float(positions[i, 0])), str(float(positions[i, 1])), {"persistent": 2, "shell": 1}.get(longs[i], 0)))
            lines += ["        <attvalues>\n",
                      att % (node_ids["nb_genes"], int(ft.nb_genes[i]))]
            head = middle(lines)
            lines = []
            values = (longs[i], exact) + (() if subpartition is None else (escape(subpartition[1][names[i]]),)) + _lengths(ft.len_sum[i], ft.len_distinct[i], et.fam_mid_lo[i], et.fam_mid_hi[i], ft.len_min[i], ft.len_max[i])
            for (title, _), value in zip(tail, values):
                lines.append(att % (node_ids[title], value))
            lines.append("        </attvalues>\n      </node>\n")
            w(head + "".join(lines).encode())

        def walked(i):
            def middle(lines):
                present = node_keys[i]
                for org in present[:1]:
                    lines.append(att % (node_ids[org], escape("|".join(cells[i][org]))))
                lines.append(att % (node_ids["name"], escape("|".join(gene_names[i]))))
                lines.append(att % (node_ids["product"], escape("|".join(products[i]))))
                for org in present[1:]:
                    lines.append(att % (node_ids[org], escape("|".join(cells[i][org]))))
                return "".join(lines).encode()
            return middle

        if nt is not None:
            for row0, rows in nt._batches(budget, all_node_attributes):
                text, ends = nt.lines(row0, rows, all_node_attributes)
                view = memoryview(text)
                for r in range(rows):
                    node(row0 + r, lambda lines, r=r: "".join(lines).encode() + bytes(view[int(ends[r - 1]) if r else 0:int(ends[r])]))
        else:
            for i in range(n):
                node(i, walked(i))
        if n:
            w(b"    </nodes>\n")
        ne = et.n_edges
        w(b"    <edges>\n" if ne else b"    <edges />\n")
        length_ids = [k for k, what in edge_titles if isinstance(what, str)]
        escaped = [escape(name) for name in names]

        def edge(e, organisms, values_of_metadata=b""):
            weight = str(float(int(et.weight[e])))
            w(('      <edge source="%s" target="%s" id="%d" weight="%s">\n        <viz:thickness value="%s" />\n        <attvalues>\n'
               % (escaped[et.src[e]], escaped[et.dst[e]], e, weight, weight)).encode())
            if organisms is not None:
                w(organisms)
            values = _lengths(et.len_sum[e], et.len_distinct[e], et.len_mid_lo[e], et.len_mid_hi[e], et.len_min[e], et.len_max[e])
            w(b"".join(("".join(att % (k, value) for k, value in zip(length_ids, values)).encode(), values_of_metadata,
                        b"        </attvalues>\n      </edge>\n")))

        def slices(text, ends):
            view = memoryview(text)
            return [view[int(ends[r - 1]) if r else 0:int(ends[r])] for r in range(len(ends))]

        if all_edge_attributes or meta is not None:
            for row0, rows in et._batches(budget, organisms=all_edge_attributes, metadata=meta is not None):
                organisms = slices(*et.attvalues(attr_id, row0, rows)) if all_edge_attributes else [None] * rows
                behind = slices(*et.metavalues(row0, rows)) if meta is not None else [b""] * rows
                for r in range(rows):
                    edge(row0 + r, organisms[r], behind[r])
        else:
            for e in range(ne):
                edge(e, None)
        if ne:
            w(b"    </edges>\n")
        w(b"  </graph>\n</gexf>\n")


def ushape_counts(partitions, family_table):
    """The three series of ushaped_plot (ppanggolin.py:1494-1507): int64 [d][3], row k - 1 the families present in exactly
    k organisms that are persistent / shell / cloud.  On the host, from the table's nb_org."""
    ft = family_table
    if isinstance(partitions, dict):
        if ft.names is None:
            raise ValueError("ushape_counts: this master carries no names (give the classes as uint8 [n])")
        part = part_codes(partitions, ft.names)
    else:
        part = np.ascontiguousarray(partitions, np.uint8)
    if part.shape != (ft.n,):
        raise ValueError("ushape_counts: a class per family")
    out = np.zeros((ft.d, 3), np.int64)
    nb = np.asarray(ft.nb_org, np.int64)
    use = (part < 3) & (nb >= 1) & (nb <= ft.d)
    np.add.at(out, (nb[use] - 1, part[use].astype(np.int64)), 1)
    return out
