"""What tests/test_orders_host.py and tests/test_gpu_orders.py share: the recorded graphs of tests/golden/orders/
(made by tests/golden/make_orders.py from the reference's own __neighborhood_computation), random and synthetic
annotation sets, and the comparison of two masters' arrays."""
import glob
import json
import os
from collections import OrderedDict

import numpy as np

from pangenomenem_amd.chunks import orders_from_annotations, pack_rows

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orders", "*.json")))


def load(path):
    with open(path) as f:
        return json.load(f)


def annotations_of(rec):
    """a fixture's annotations as PPanGGOLiN holds them: {organism: {contig: OrderedDict(gene -> info)}}, info[1] the family"""
    return OrderedDict((org, OrderedDict((contig, OrderedDict((gene, ["CDS", fam]) for gene, fam in genes)) for contig, genes in contigs))
                       for org, contigs in rec["annotations"])


class RecordedGraph:
    """the part of a networkx Graph / DiGraph that master_arrays_from_graph reads, rebuilt from a recorded graph"""

    def __init__(self, rec, directed):
        self._directed = directed
        self._nodes = OrderedDict((f, {o: True for o in orgs}) for f, orgs in rec["nodes"])
        self._succ = {a: OrderedDict((b, dict(data)) for b, data in nbrs) for a, nbrs in rec["adj"]}
        self.pred = {a: OrderedDict((b, self._succ[b][a]) for b in pre) for a, pre in rec["pred"]} if directed else self._succ

    def nodes(self, data=False):
        return list(self._nodes.items()) if data else list(self._nodes)

    def is_directed(self):
        return self._directed

    def __getitem__(self, a):
        return self._succ[a]


def fixture_orders(rec):
    return orders_from_annotations(annotations_of(rec), rec["organisms"], rec["circular"], rec["repeated"])


def orders_args(o, directed):
    return dict(genes=o["genes"], contig_ptr=o["contig_ptr"], contig_org=o["contig_org"], contig_circular=o["contig_circular"], d=o["d"],
                repeated=o["repeated"], directed=directed)


def same_master(got, want, what=""):
    """(rows or x, (ptr, idx), edge_bits, (xptr, xorg, xcnt), ...) field by field; x may be the byte matrix or its packed rows"""
    rows = [a if a.dtype == np.uint32 else pack_rows(a) for a in (np.asarray(got[0]), np.asarray(want[0]))]
    assert rows[0].shape == rows[1].shape and np.array_equal(rows[0], rows[1]), what + ": presence rows"
    for k, name in ((0, "ptr"), (1, "idx")):
        assert np.array_equal(np.asarray(got[1][k]), np.asarray(want[1][k])), what + ": " + name
    assert np.array_equal(np.asarray(got[2]).ravel(), np.asarray(want[2]).ravel()), what + ": edge_bits"
    for k, name in ((0, "extra_ptr"), (1, "extra_org"), (2, "extra_count")):
        assert np.array_equal(np.asarray(got[3][k]), np.asarray(want[3][k])), what + ": " + name


def random_genomes(rng, n_fam, n_org, max_contigs=4, max_len=12, p_repeat=0.15, p_circular=0.4):
    """small annotation sets in which repeated families, circular contigs, tandem duplicates and repeated adjacencies
    are common: few families, genes drawn with replacement, a run of equal families now and then.  Contig names are
    unique per organism except the shared name "plasmid" (circularity goes by contig name in the reference)."""
    fams = ["F%d" % i for i in range(n_fam)]
    repeated = [f for f in fams if rng.random() < p_repeat]
    ann, circular = OrderedDict(), set()
    k = 0
    orgs = ["org%d" % i for i in range(n_org)]
    for o in rng.permutation(n_org):                          # (walk order is not column order)
        org = orgs[o]
        ann[org] = OrderedDict()
        for c in range(int(rng.integers(1, max_contigs + 1))):
            contig = "plasmid" if c == 0 and rng.random() < 0.3 else "%s_c%d" % (org, c)
            if rng.random() < p_circular:
                circular.add(contig)
            genes = OrderedDict()
            length = int(rng.integers(0, max_len + 1))
            j = 0
            while j < length:
                fam = fams[int(rng.integers(0, n_fam))]
                for _ in range(1 + (int(rng.integers(1, 3)) if rng.random() < 0.15 else 0)):      # a tandem run
                    k += 1
                    genes["g%d" % k] = ["CDS", fam]
                    j += 1
            ann[org][contig] = genes
    return ann, orgs, sorted(circular), repeated


def synthetic_orders(n_fam, d, seed, density=0.35, p_repeat=0.02, contigs_per_org=3):
    """gene orders at a master's scale: every organism carries a random subset of the families (at least one organism
    carries each), mostly in family order with local shuffles and a few duplicates, cut into contigs, some circular"""
    rng = np.random.default_rng(seed)
    genes, cptr, corg, circ = [], [0], [], []
    total = 0
    owner = rng.integers(0, d, n_fam)
    for o in range(d):
        have = np.flatnonzero((rng.random(n_fam) < density) | (owner == o))
        have = have[np.argsort(have + rng.normal(0, 2.0, len(have)))]                 # local rearrangements
        dup = rng.random(len(have)) < 0.03
        seq = np.repeat(have, 1 + dup)
        cuts = np.sort(rng.integers(0, len(seq) + 1, contigs_per_org - 1)) if len(seq) else np.zeros(contigs_per_org - 1, np.int64)
        for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(seq)]])):
            genes.append(seq[lo:hi])
            total += hi - lo
            cptr.append(total)
            corg.append(o)
            circ.append(int(rng.random() < 0.4))
    return dict(genes=np.concatenate(genes).astype(np.int32), contig_ptr=np.asarray(cptr, np.int32), contig_org=np.asarray(corg, np.int32),
                contig_circular=np.asarray(circ, np.uint8), d=d, repeated=(rng.random(n_fam) < p_repeat).astype(np.uint8))
