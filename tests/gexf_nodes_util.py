"""What tests/test_gexf_nodes_host.py and tests/test_gpu_gexf_nodes.py share: annotations turned into the flat form the node
table takes (orders, one text, the ID / NAME / PRODUCT spans), the comparison of two written files, a fixture's host tables
with its node table, and the built cases at which the node kernels of csrc/nem_nodes.hip take another path, each with the
counts it is meant to reach."""
import gzip

import numpy as np

from pangenomenem_amd.gexf import HostNodeTable, NAME
from pangenomenem_amd.matrix import table_orders
from pangenomenem_amd.projection import PRODUCT
from tests.append_util import build_host

SPECIAL = b'&<>"\r\n\t'                                       # the seven bytes gexf.escape replaces


def text_and_spans(pieces, gap=b"\t"):
    """pieces: per gene (ID, NAME, PRODUCT) as bytes -> (text, (span_off int64 [3][g], span_len int32 [3][g])); an empty
    piece is the empty span at the ID's offset, as the loader gives it"""
    parts, at = [], 0
    off, length = np.zeros((3, len(pieces)), np.int64), np.zeros((3, len(pieces)), np.int32)
    for p, three in enumerate(pieces):
        for k, piece in enumerate(three):
            parts.append(gap)
            at += len(gap)
            off[k, p], length[k, p] = (at, len(piece)) if piece or k == 0 else (off[0, p], 0)
            parts.append(piece)
            at += len(piece)
    return b"".join(parts), (off, length)


def flat_of_annotations(ann, organisms, ids, by_org):
    """annotations -> (table_orders' dict, text, spans): the walk's genes with their id, name and product as UTF-8 bytes"""
    o = table_orders(ann, organisms, ids, by_org)
    pieces = [(gene.encode(), info[NAME].encode(), info[PRODUCT].encode())
              for contigs in ann.values() for annot in contigs.values() for gene, info in annot.items()]
    text, spans = text_and_spans(pieces)
    return o, text, spans


def host_node_table(x, order, o, text, spans, d=None):
    return HostNodeTable(x, order, o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"], text, spans, d=d)


def same_file(got_path, want_path, what):
    """byte for byte except the <meta lastmodifieddate> line (a .gz: its content)"""
    read = lambda path: (gzip.open if path.endswith(".gz") else open)(path, "rb").read().split(b"\n")
    got, want = read(got_path), read(want_path)
    assert len(got) == len(want), "%s: %d lines, %d wanted" % (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        if b.startswith(b"  <meta lastmodifieddate="):
            assert a.startswith(b"  <meta lastmodifieddate="), (what, k)
            continue
        assert a == b, "%s: line %d: %r, wanted %r" % (what, k, a, b)


def same_node_tables(got, want, what, tails=(6, 7)):
    """two node tables: shape, nb_genes, first, and per numbering the ids, the titles, the node ends and every byte"""
    assert (got.n, got.d) == (want.n, want.d), what
    assert np.array_equal(got.nb_genes, want.nb_genes) and np.array_equal(got.first, want.first), what
    for tail in tails:
        for full in (True, False):
            assert got.titles(full, tail) == want.titles(full, tail), (what, tail, full)
            a, b = got.ids(tail), want.ids(tail)
            assert np.array_equal(a[0], b[0]) and tuple(a[1]) == tuple(b[1]), (what, tail, "ids")
            if not want.n:
                continue
            assert got.lines_size(0, None, full) == want.lines_size(0, None, full), (what, tail, full)
            (text, ends), (want_text, want_ends) = got.lines(0, None, full), want.lines(0, None, full)
            assert np.array_equal(ends, want_ends), (what, tail, full, "node ends")
            assert text.tobytes() == want_text.tobytes(), "%s: tail %d full %s: text differs first at byte %d" % (
                what, tail, full, int(np.flatnonzero(text[:len(want_text)] != want_text[:len(text)])[:1].sum()))


# ---- built cases ----------------------------------------------------------------------------------------------------------
def built(contigs, d, flagged=(), n_ids=None):
    """contigs: (organism, [(caller id, ID, NAME, PRODUCT), ...]) -> a case: flat orders (sorted by organism), text, spans.
    flagged: the caller ids whose genes are not kept."""
    contigs = sorted(contigs, key=lambda c: c[0])
    genes = [gene for _, row in contigs for gene in row]
    n_ids = (max(g[0] for g in genes) + 1) if n_ids is None else n_ids
    rep = np.zeros(n_ids, np.uint8)
    rep[list(flagged)] = 1
    text, spans = text_and_spans([g[1:] for g in genes])
    ptr = np.cumsum([0] + [len(row) for _, row in contigs])
    return dict(genes=np.asarray([g[0] for g in genes], np.int32), contig_ptr=ptr.astype(np.int32),
                contig_org=np.asarray([org for org, _ in contigs], np.int32), contig_circular=np.zeros(len(contigs), np.uint8), d=d, repeated=rep,
                text=text, spans=spans)


def host_of(case):
    """the numpy master of a built case and its host node table"""
    host = build_host(case)
    return host, host_node_table(host[0], host[4], case, case["text"], case["spans"], d=case["d"])


def gene(fam, k, name=b"n", product=b"p"):
    return (fam, b"g%d_%d" % (fam, k), name, product)


def one_family_in(d):
    """one family with one gene in each of d organisms: a node of d lines"""
    return built([(o, [gene(0, o)]) for o in range(d)], d)


def copies_on_one_line(k):
    """one organism with k copies of one family: one line of k ids"""
    return built([(0, [gene(0, j) for j in range(k)])], 1)


def hub_beside_singles(copies=1500, singles=700, d=3):
    """a hub family with `copies` genes in every organism between single-gene families: blocks of 256 sorted genes start and
    end inside the hub's segment, and single-gene segments share blocks"""
    rows, fam = [], 1
    for o in range(d):
        row = []
        for j in range(copies):
            row.append(gene(0, o * copies + j, b"hub%d" % (j % 7), b"product %d" % (j % 11)))
            if j * singles // copies != (j + 1) * singles // copies and o == j % d:
                row.append(gene(fam, 0, b"s%d" % fam))
                fam += 1
        rows.append((o, row))
    return built(rows, d)


def names_case(which):
    """one family (or two) in 2 organisms x 3 genes with the names / products the bullet asks for"""
    six = lambda values, fam=0: [(o, [(fam, b"g%d_%d%d" % (fam, o, j), values[3 * o + j], values[5 - 3 * o - j]) for j in range(3)]) for o in range(2)]
    if which == "equal":
        return built(six([b"same"] * 6), 2)
    if which == "distinct":
        return built(six([b"a", b"b", b"c", b"d", b"e", b"f"]), 2)
    if which == "empty_first":
        return built(six([b"", b"x", b"", b"y", b"x", b""]), 2)
    if which == "empty_middle":
        return built(six([b"x", b"", b"y", b"", b"x", b"z"]), 2)
    if which == "empty_only":
        return built(six([b""] * 6), 2)
    if which == "two_families":                               # the same names in both: no class is shared
        a, b = six([b"x", b"y", b"x", b"z", b"y", b"x"], 0), six([b"x", b"y", b"x", b"z", b"y", b"x"], 1)
        return built([(o, a[o][1] + b[o][1]) for o in range(2)], 2)
    raise KeyError(which)


def many_products(count=3000):
    """one family whose `count` genes have as many distinct products and 5 distinct names"""
    return built([(o, [(0, b"g%d" % (2 * j + o), b"name%d" % (j % 5), b"product number %d" % (2 * j + o)) for j in range(count // 2)]) for o in range(2)], 2)


def escapes_case():
    """every escaped byte in an ID, a name and a product; a value made only of them; escaped bytes at each of the 8
    alignments of the text (the pieces' lengths shift every next piece by one more byte); bytes >= 0x80"""
    row, k = [], 0
    for ch in SPECIAL:
        one = bytes((ch,))
        row.append((0, b"i" + one + b"d%d" % k, b"na" + one + b"me", one + b"product" + one))
        k += 1
    row.append((0, SPECIAL, SPECIAL[::-1], SPECIAL * 2))
    for shift in range(8):
        row.append((1, b"x" * shift + b"&" + b"y" * (7 - shift) + b"%d" % shift, b"z" * shift + b"<>", b"\t" + b"w" * shift))
    row.append((1, "géne\u0085".encode(), "nøm 中".encode(), b"\xc3\xa9&\xc3\xa9"))
    return built([(0, row), (1, [(0, b"h<1>", b"", b"\"q\"")])], 2)


def late_organisms(d=1100):
    """d organisms (ids of 1 to 4 digits): organism o has family o of its own, so it is first met at node o; the first
    five also have family 0 and the last organism has family 1: organisms first met at late nodes, and at node 1 an
    organism with a larger column than the node's own"""
    rows = []
    for o in range(d):
        row = [gene(o, o)]
        if o < 5 and o:
            row.insert(0, gene(0, o))
        if o == d - 1:
            row.append(gene(1, o))
        rows.append((o, row))
    return built(rows, d)


def flagged_case():
    """families 1 and 3 are flagged: organism 1 has only genes of them and keeps no gene; the flagged genes carry names and
    products no kept gene has"""
    return built([(0, [gene(0, 0), gene(1, 0, b"gone", b"lost"), gene(2, 0)]),
                  (1, [gene(1, 1, b"gone", b"lost"), gene(3, 1, b"never", b"seen")]),
                  (2, [gene(2, 2), gene(3, 2, b"never", b"seen"), gene(0, 2), gene(4, 2)])], 3, flagged=(1, 3))


def reach(case):
    """what a built case reaches: organisms per family (max), copies per line (max), kept genes, families"""
    host, table = host_of(case)
    kept = case["repeated"][case["genes"]] == 0
    org = np.repeat(case["contig_org"], np.diff(case["contig_ptr"]))
    inv = np.full(len(case["repeated"]), -1, np.int64)
    inv[host[4]] = np.arange(len(host[4]))
    cell, counts = np.unique(inv[case["genes"][kept]] * case["d"] + org[kept], return_counts=True)
    return dict(n=table.n, kept=int(kept.sum()), organisms=int(np.bincount(cell // case["d"]).max()) if len(cell) else 0,
                copies=int(counts.max()) if len(counts) else 0, table=table)
