"""What tests/test_gexf_bounds_host.py, tests/test_gpu_gexf_bounds.py and tests/test_gpu_gexf_metadata.py share: a PLAIN
statement of the edges' GEXF text (class Plain: Python dicts, ints and bytes over the contigs list and the master's family
order, no bit rows, nothing of gexf.py), the shapes at which the bounds of csrc/nem_edges.hip and
csrc/nem_edge_meta.hip are held: organism counts beyond one trip of 64 words, ids of every digit count, a full LDS stage,
attributes of up to 65 536 values, first edges on the 256-edge tile's boundary.  The host file holds the numpy statements
(gexf.edge_table_arrays, attvalues_host, edge_metadata_arrays, metavalues_host) to the plain one at these shapes, the
device file holds the kernels to the numpy statements.  Every shape and every numpy reference is made once per process
(lru_cache) and never changed by a test."""
from functools import lru_cache

import numpy as np

from pangenomenem_amd.gexf import HostEdgeTable, edge_metadata_arrays, metavalues_host
from tests.append_util import build_host
from tests.gexf_util import contigs_orders, path_contigs
from tests.orders_util import same_master

EDGES = 300                                                   # the path's edges: 75 blocks of 4 waves, an edge a wave
ATT_HEAD, ATT_TAIL = '          <attvalue for="%d" value="', '" />\n'
ATT = ATT_HEAD + "%s" + ATT_TAIL
INT32_MAX = 2 ** 31 - 1
# every digit count, every power of ten and its predecessor
ID_CYCLE = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [INT32_MAX]
FIRST_EDGES = 600                                             # the first-edge path: two tiles of 256 edges and a part of one


def shape_contigs(rng, d):
    n = EDGES + 1
    contigs = path_contigs(rng, EDGES, d)
    contigs += [(o, [n, n + 1], -1) for o in range(d)] + [(0, [n + 2, n + 3], -1), (d - 1, [n + 3, n + 4], -1)]
    contigs += [(d // 2, [n + 5, n + 5], -1), (d - 1, [n + 6], 40)]
    return contigs


def shape_orders(rng, d):
    """the path of EDGES edges (organism 0 all of it, the others a stretch), then an edge carried by every organism next
    to edges carried by one, a tandem pair and a circular contig of one gene"""
    return contigs_orders(shape_contigs(rng, d), d, rng)


def attributes(rng, d, counts, ids, force=None):
    """the arrays of len(counts) attributes: every value of an attribute of at most d values is some organism's (of d
    values: every organism another one); the values' bytes differ in length, an empty one, one of a single byte and one
    of 150 bytes among them.  force: per attribute a dict organism -> rank (or None) that overrides the random choice,
    which for more values than organisms never promises rank 0, the last rank or one at a word's boundary."""
    rank = np.zeros((len(counts), d), np.int32)
    texts = []
    for a, nv in enumerate(counts):
        if nv <= d:
            rank[a] = rng.permutation(np.concatenate([np.arange(nv), rng.integers(0, nv, d - nv)]))
        else:
            rank[a] = rng.choice(nv, d, replace=False)
        mine = [("v%d" % k).encode() * int(rng.integers(1, 9)) for k in range(nv)]
        mine[0] = b""
        if nv > 1:
            mine[nv - 1] = b"x"
        if nv > 2:
            mine[nv // 2] = ("long|&amp;%d " % a).encode() * 13 + "Å".encode()
            assert len(mine[nv // 2]) > 128
        texts += mine
    for a, mine in enumerate(force or ()):
        for o, v in (mine or {}).items():
            assert 0 <= v < counts[a] and 0 <= o < d
            rank[a, o] = v
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    return np.asarray(ids, np.int32), rank, np.asarray(counts, np.int32), ptr, np.frombuffer(b"".join(texts), np.uint8).copy()


# ---- the plain statement ------------------------------------------------------------------------------------------
class Plain:
    """contigs: (organism, [family, ...], circular size or -1), walked organism by organism (a stable sort: column order),
    every gene kept; order: the master's numbering (master family i = caller id order[i]).
    pairs: (min family, max family) -> {organism: count} from consecutive genes and the circular closing link;
    edges: nx.Graph.edges() of the master's numbering: row by row, a row's neighbours as the links first met them, the
    entries with idx >= row; first[o]: the lowest edge that has o, else E."""

    def __init__(self, contigs, order, d):
        at = {int(f): i for i, f in enumerate(order)}
        self.d, self.pairs = d, {}
        rows = [dict() for _ in at]
        for org, fams, size in sorted(contigs, key=lambda c: c[0]):
            links = [(fams[k], fams[k - 1]) for k in range(1, len(fams))] + ([(fams[0], fams[-1])] if size >= 0 else [])
            for a, b in links:
                a, b = at[a], at[b]
                mine = self.pairs.setdefault((min(a, b), max(a, b)), {})
                mine[org] = mine.get(org, 0) + 1
                rows[a].setdefault(b)
                rows[b].setdefault(a)
        self.edges = [(u, v) for u, row in enumerate(rows) for v in row if v >= u]
        assert len(self.edges) == len(self.pairs)
        self.orgs = [sorted(self.pairs[e].items()) for e in self.edges]       # per edge (organism, count) in column order
        self.first = [len(self.edges)] * d
        for e in range(len(self.edges) - 1, -1, -1):
            for o, _ in self.orgs[e]:
                self.first[o] = e

    @property
    def n_edges(self):
        return len(self.edges)

    def organism_lines(self, attr_id):
        """per edge the bytes of its organism lines"""
        return [("".join(ATT % (attr_id[o], "%d" % cnt) for o, cnt in mine)).encode() for mine in self.orgs]

    def ranks(self, rank):
        """per edge and attribute the sorted distinct ranks of its organisms"""
        rank = [[int(v) for v in row] for row in rank]
        return [[sorted({row[o] for o, _ in mine}) for row in rank] for mine in self.orgs]

    def masks(self, rank):
        """per edge and attribute a Python int: bit v set where value v is present"""
        out = []
        for per_attr in self.ranks(rank):
            ints = []
            for present in per_attr:
                m = 0
                for v in present:
                    m |= 1 << v
                ints.append(m)
            out.append(ints)
        return out

    def metadata_lines(self, attr_id, rank, n_values, ptr, blob):
        """per edge the bytes of its metadata lines: the present values joined by | in rank order"""
        blob, base = bytes(blob), np.concatenate([[0], np.cumsum(n_values)]).tolist()
        ptr = [int(p) for p in ptr]
        value = lambda a, v: blob[ptr[base[a] + v]:ptr[base[a] + v + 1]]
        return [b"".join((ATT_HEAD % attr_id[a]).encode() + b"|".join(value(a, v) for v in present) + ATT_TAIL.encode()
                         for a, present in enumerate(per_attr)) for per_attr in self.ranks(rank)]


def mask_words(masks, n_values):
    """Plain.masks as edge_metadata_arrays lays them out: uint32 [E][W], the attributes' words one after the other"""
    words = [(int(nv) + 31) // 32 for nv in n_values]
    return np.frombuffer(b"".join(m.to_bytes(4 * nw, "little") for per_attr in masks for m, nw in zip(per_attr, words)),
                         "<u4").reshape(len(masks), sum(words)).astype(np.uint32)


def ends_of(lines):
    return np.cumsum([len(line) for line in lines]).astype(np.int64)


def budget_held(table, true_bytes, what):
    """_Edges._metadata_bound lies above every edge's true metadata bytes and masks, which is what _batches relies on:
    every batch is within its budget by the TRUE bytes (true_bytes(row0, rows): the organism lines, the metadata lines and
    the masks) or is a single edge, and the batches tile [0, E)"""
    ne = table.n_edges
    words = int(((table._metadata[2].astype(np.int64) + 31) // 32).sum())
    for budget in (1, 64 << 10, 4 << 20):
        row = 0
        for row0, rows in table._batches(budget, metadata=True):
            assert row0 == row and rows >= 1, (what, budget, row0)
            assert rows == 1 or true_bytes(row0, rows) + 4 * words * rows <= budget, (what, budget, row0, rows)
            row += rows
        assert row == ne, (what, budget)
    return words


# ---- the shapes ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def organisms_case(d):
    """shape_orders(d) and an edge carried only by organism d - 1 and one carried only by organism 2048 where there is one:
    the last organism of the last word, the first of the second trip of 64 words"""
    rng = np.random.default_rng(900 + d)
    n = EDGES + 1
    contigs = shape_contigs(rng, d) + [(d - 1, [n + 7, n + 8], -1)] + ([(2048, [n + 9, n + 10], -1)] if d > 2048 else [])
    return contigs, contigs_orders(contigs, d, rng)


def id_runs(d):
    """(what, attr_id): every id the widest; then ID_CYCLE over the organisms, shifted by one per run"""
    yield "ids all 2**31 - 1", np.full(d, INT32_MAX, np.int32)
    for shift in range(3):
        yield "ids cycle %d" % shift, np.asarray([ID_CYCLE[(o + shift) % len(ID_CYCLE)] for o in range(d)], np.int32)


STAGE_D, STAGE_LINKS, STAGE_FULL = 192, 1000, 8               # STAGE_FULL: the full edge's number


@lru_cache(maxsize=None)
def stage_case():
    """d = 192: eight edges of one organism each (organisms 0 .. 7, ids of 1 .. 8 digits), then the edge of exactly
    organisms 64 .. 127, STAGE_LINKS times each (ids of 10 digits, counts of 4: 64 lines of 53 bytes), then an edge of
    organism 191 alone; every other organism has one gene and no edge.  Returns contigs, orders, attr_id."""
    contigs = [(k, [2 * k, 2 * k + 1], -1) for k in range(8)]
    contigs += [(o, [16], -1) for o in list(range(8, 64)) + list(range(128, 191))]
    contigs += [(o, [17, 18], -1) for o in range(64, 128) for _ in range(STAGE_LINKS)]
    contigs += [(191, [19, 20], -1)]
    ids = np.full(STAGE_D, INT32_MAX, np.int64) - np.arange(STAGE_D)
    ids[:8] = [7, 42, 999, 1000, 54321, 100000, 9999999, 10000000]
    return contigs, contigs_orders(contigs, STAGE_D, np.random.default_rng(41)), ids.astype(np.int32)


SPARSE_D = 129
SPARSE_SETS = ((2048,), (2049,), (4097, 1, 2049), (65536, 3, 65535), (65536, 65536))
SPARSE_IDS = (INT32_MAX, 0, 12345)
SPARSE_CUT = [(0, 1), (1, 3), (4, 1), (5, 64), (69, EDGES + 6 - 70), (EDGES + 5, 1)]
PAIR = (3, 4)                                                 # the two organisms that share an edge of their own
EVERYONE = (10, 11, 12, 13, 14, 15)                           # organisms forced to the ranks below on the edge of all
EVERYONE_RANKS = (0, 31, 32, 2047, 2048, -1)                  # (-1: the attribute's last)
FAR_RANK = 130 * 32 + 7                                       # in word 130: the third trip of 64 words


@lru_cache(maxsize=None)
def sparse_contigs():
    """shape_orders(129) and an edge carried by the two organisms PAIR alone"""
    rng = np.random.default_rng(829)
    n = EDGES + 1
    contigs = shape_contigs(rng, SPARSE_D) + [(o, [n + 7, n + 8], -1) for o in PAIR]
    return contigs, contigs_orders(contigs, SPARSE_D, rng)


def sparse_force(counts):
    """per attribute of more values than organisms: on the edge of all organisms the ranks at the words' and the trips'
    boundaries; organism 0 (alone on an edge) the last rank, so every earlier trip of its line is empty; the PAIR rank 5
    and a rank two trips on where there is one (else the last), an empty trip between them; and in a set of three the
    last organism (alone on two edges) rank 2050 in the first attribute and rank 7 in the third: the first leaves bits in
    word 64 of the wave's LDS that the third must not have"""
    d, out = SPARSE_D, []
    for a, nv in enumerate(counts):
        if nv <= d:
            out.append(None)
            continue
        mine = {o: (nv - 1 if v < 0 else v) for o, v in zip(EVERYONE, EVERYONE_RANKS) if v < nv}
        mine.update({0: nv - 1, PAIR[0]: 5, PAIR[1]: FAR_RANK if FAR_RANK < nv else nv - 1})
        if len(counts) == 3:
            mine[d - 1] = 2050 if a == 0 else 7
        out.append(mine)
    return out


@lru_cache(maxsize=None)
def sparse_meta(counts):
    rng = np.random.default_rng(1000 + sum(counts))
    return attributes(rng, SPARSE_D, counts, SPARSE_IDS[:len(counts)], force=sparse_force(counts))


DENSE_D = 4100
DENSE_SETS = ((4100,), (4100, 2049))


@lru_cache(maxsize=None)
def dense_contigs():
    rng = np.random.default_rng(4100)
    contigs = shape_contigs(rng, DENSE_D)
    return contigs, contigs_orders(contigs, DENSE_D, rng)


@lru_cache(maxsize=None)
def dense_meta(counts):
    return attributes(np.random.default_rng(77 + len(counts)), DENSE_D, counts, (99999, INT32_MAX)[:len(counts)])


FIRST_AT = (256, 255, 257, 0, 511, 512, FIRST_EDGES - 1)      # where an organism's only edge lies: around the tiles' boundaries


def first_edge_cases(d):
    """(what, contigs): organism 0 walks the path 0 - 1 - ... - FIRST_EDGES; per word of 32 organisms in turn, its
    organisms (but organism 0) get one contig [p, p + 1] each, p from FIRST_AT as far as the word has room; then either
    ("early") every other organism an edge among the first 256, so each full word is met within the first tile and the
    walk stops early, or ("never") up to three organisms of the word a single gene and no edge (first == E: the word is
    never full) and every other one an edge anywhere"""
    ne = FIRST_EDGES
    for word in range((d + 31) // 32):
        for fill in ("early", "never"):
            rng = np.random.default_rng(d * 100 + word * 2 + (fill == "never"))
            slots = [o for o in range(word * 32, min(d, word * 32 + 32)) if o != 0]
            placed = dict(zip(slots, FIRST_AT))
            if fill == "early":
                placed = {o: p for o, p in placed.items() if p < 256} if word == 0 else placed
            edgeless = [o for o in slots if o not in placed][-3:] if fill == "never" else []
            if fill == "never" and not edgeless:              # (a word of one organism: that one)
                edgeless, placed = slots[-1:], {o: p for o, p in placed.items() if o != slots[-1]}
            contigs = [(0, list(range(ne + 1)), -1)]
            for o in range(1, d):
                if o in edgeless:
                    contigs.append((o, [ne + 1], -1))
                else:
                    p = placed[o] if o in placed else int(rng.integers(0, 256 if fill == "early" else ne))
                    contigs.append((o, [p, p + 1], -1))
            yield "d %d word %d %s" % (d, word, fill), contigs, edgeless


# ---- the numpy statements at these shapes, made once ------------------------------------------------------------------
SHAPES = dict(organisms=organisms_case, stage=lambda d: stage_case()[:2], sparse=lambda d: sparse_contigs(), dense=lambda d: dense_contigs())


@lru_cache(maxsize=None)
def host_of(kind, d):
    """contigs, orders, the numpy master (build_host) and its HostEdgeTable"""
    contigs, o = SHAPES[kind](d)
    host = build_host(o)
    et = HostEdgeTable(host[1], host[2], host[3], host[4], o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"],
                       o["contig_sizes"], o["repeated"], d=d)
    return contigs, o, host, et


def organism_ids(kind, d):
    """(what, attr_id) of a shape's runs; the first is the one the batches are cut with"""
    if kind == "stage":
        return [("stage ids", stage_case()[2])]
    return [("ids 3 o + 8", np.arange(d, dtype=np.int32) * 3 + 8)] + list(id_runs(d))


@lru_cache(maxsize=None)
def organism_text(kind, d, run):
    """attvalues_host of all the shape's edges with the ids of its run: (attr_id, text, ends)"""
    attr_id = organism_ids(kind, d)[run][1]
    return (attr_id,) + tuple(host_of(kind, d)[3].attvalues(attr_id))


@lru_cache(maxsize=None)
def metadata_text(kind, d, counts):
    """meta, edge_metadata_arrays and metavalues_host of all the shape's edges: (meta, masks, text, ends)"""
    meta = sparse_meta(counts) if kind == "sparse" else dense_meta(counts)
    _, _, host, _ = host_of(kind, d)
    masks = edge_metadata_arrays(host[1], host[2], meta[1], meta[2], d)
    return (meta, masks) + tuple(metavalues_host(host[1], host[2], *meta, d))


def same_master_arrays(m, host, what):
    """the device master is the numpy one the statements above were made from"""
    got = m.arrays()
    same_master(got, host, what)
    assert np.array_equal(got[4], host[4]), what + ": order"
