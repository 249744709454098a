"""What tests/test_master_merge_host.py, tests/test_gpu_master_merge.py and tests/test_gpu_merged_consumers.py share: a
pangenome's gene orders cut into two parts that are built alone (each with its own columns 0 .. d - 1, both with the same
repeated families, their family ids in one id space), and the three masters the merge of the two is held against; a part
numbered apart (its ids relabelled into a larger id space); a host master as a from-arrays counts master; two parts with
different repeated families; and orders that carry what every consumer of a master reads."""
import functools

import numpy as np

from pangenomenem_amd.chunks import master_arrays_merge
from tests import master_shapes as ms
from tests.append_util import UPDATE_FIXTURES, append_host, build_host, fixture_parts, part_orders, slice_orders, split_annotations
from tests.orders_util import load, random_genomes, same_master


def alone(o, lo, hi, repeated=None):
    """orders whose columns are the absolute lo .. hi - 1 as the orders of a pangenome of its own: columns 0 .. hi - lo - 1"""
    return dict(o, contig_org=(o["contig_org"] - lo).astype(np.int32), d=hi - lo, repeated=o["repeated"] if repeated is None else repeated)


def two_parts(base, upd, d_a, d_b):
    """base (columns 0 .. d_a - 1) and upd (absolute columns d_a .. d_a + d_b - 1) in one id space, upd's repeated families
    (the union) for both.  Returns (A's orders, B's orders alone, B's orders as an update, the orders of everything)."""
    rep = np.ascontiguousarray(upd["repeated"], np.uint8)
    a = dict(base, d=d_a, repeated=rep)
    u = dict(upd, d=d_a + d_b, repeated=rep)
    return a, alone(u, d_a, d_a + d_b), u, ms.concat_orders([a, u], d_a + d_b)


def kept_genes(o):
    return len(o["genes"]) > 0 and not o["repeated"][o["genes"]].all()


def fixture_cases():
    for path in UPDATE_FIXTURES:
        rec = load(path)
        base, upd = fixture_parts(rec)
        yield rec["name"], two_parts(base, upd, len(rec["organisms"]), len(rec["new_organisms"]))


def random_cases(seed, count, max_fam=9, max_org=8, max_len=12):
    """random_genomes cut at a random organism; the cases in which a part has no kept gene (no master) are left out"""
    rng = np.random.default_rng(seed)
    for case in range(count):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, max_fam)), int(rng.integers(2, max_org)), max_len=max_len)
        cut = int(rng.integers(1, len(orgs)))
        parts, cols = split_annotations(ann, orgs, [cut])
        (a, b), whole = part_orders(parts, cols, circular, repeated)
        assert b["families"] == whole["families"]
        if kept_genes(a) and kept_genes(b):
            yield "random %d" % case, two_parts(a, b, len(parts[0]), len(parts[1]))


def host_merge(ma, mb):
    """the statement on two host masters whose orders share one id space"""
    return master_arrays_merge(ma, ma[4], mb, mb[4])


def same_with_order(got, want, what):
    assert np.array_equal(np.asarray(got[4]), np.asarray(want[4])), what + ": family order"
    same_master(got, want, what)


def host_expectations(a, b, u, whole, what):
    """the statement's merge of the two parts' masters, held against the single build and against the append.  Returns
    (A's master, B's, the merged one)."""
    ma, mb = build_host(a), build_host(b)
    got = host_merge(ma, mb)
    same_with_order(got, build_host(whole), what + ": one build")
    same_with_order(got, append_host(ma, len(a["repeated"]), u, b["d"]), what + ": the append")
    return ma, mb, got


def triple_alone():
    """ms.triple_parts() as pangenomes of their own (one id space, the same repeated families)"""
    cuts = (0,) + ms.TRIPLE_STAGES
    return [alone(p, lo, hi) for p, lo, hi in zip(ms.triple_parts(), cuts[:-1], cuts[1:])]


# ---- a part numbered apart
def scattered_ids(count, f, seed):
    """an injective map of the ids 0 .. count - 1 into 0 .. f - 1, in no order; and its inverse [f] (-1: no id's image)"""
    sigma = np.random.default_rng(seed).permutation(f)[:count].astype(np.int64)
    inverse = np.full(f, -1, np.int64)
    inverse[sigma] = np.arange(count)
    return sigma, inverse


def relabelled(o, sigma, f):
    """the orders o with every family id i written sigma[i], in an id space of f ids (whatever else o carries is kept)"""
    rep = np.zeros(f, np.uint8)
    rep[sigma] = o["repeated"]
    return dict(o, genes=sigma[o["genes"]].astype(np.int32), repeated=rep)


# ---- a host master as a master made from arrays (its family i is id i: the numbering it was built with is gone)
def arrays_master(host):
    from pangenomenem_amd.chunks import Master
    return Master(host[0], host[1][0], host[1][1], host[2], edge_counts=host[3])


def identity_numbered(host):
    """what arrays_master(host) is on the host: the same arrays, its order the identity"""
    return tuple(host[:4]) + (np.arange(len(host[4]), dtype=np.int32),) + tuple(host[5:])


# ---- parts built with different repeated families
def different_repeated_parts():
    """A (two organisms) was built with family 3 repeated, B (one organism) with family 1: A has a node for 1 and none
    for 3, B the other way round.  Returns (A's orders, B's alone)."""
    a = ms.contigs_orders([(0, [0, 1, 2, 3, 4]), (1, [1, 0, 3, 2])], 2, 5, repeated=[3])
    b = ms.contigs_orders([(0, [3, 1, 0, 3, 4])], 1, 5, repeated=[1])
    return a, b


def random_different_repeated_parts(n_fam=50, d_a=12, d_b=12, seed=81, p_repeat=0.12):
    """n_fam families over d_a + d_b organisms cut in two; A built without a repeated family, B with some"""
    from tests.orders_util import synthetic_orders
    o = synthetic_orders(n_fam, d_a + d_b, seed, density=0.5, p_repeat=p_repeat)
    assert o["repeated"].any()
    a = dict(slice_orders(o, 0, d_a), d=d_a, repeated=np.zeros(n_fam, np.uint8))
    return a, alone(dict(slice_orders(o, d_a, d_a + d_b)), d_a, d_a + d_b)


# ---- orders that carry what every consumer reads
CONSUMER_FAMILIES, CONSUMER_SHARED, CONSUMER_D_A, CONSUMER_D_B = 300, 260, 33, 31
CONSUMER_HUB, CONSUMER_HUB_NEIGHBOURS = 5, 240


@functools.lru_cache(maxsize=None)
def consumer_orders():
    """Some 300 families over 33 + 31 organisms through gexf_util.contigs_orders (every gene with a START and an END, a
    circular contig with its size), gene_len beside them: the families from CONSUMER_SHARED on in the last 31 organisms
    alone (new in a second part), some families repeated, tandem pairs (self-loops), an adjacency walked three times in
    organisms of both parts (extras), and family CONSUMER_HUB next to CONSUMER_HUB_NEIGHBOURS others, one organism each
    (a hub row that both parts give entries to).  The contigs lie in column order: slice_orders cuts them."""
    from tests.gexf_util import contigs_orders
    rng = np.random.default_rng(20270301)
    f, d = CONSUMER_FAMILIES, CONSUMER_D_A + CONSUMER_D_B
    contigs = []
    for o in range(d):
        upto = CONSUMER_SHARED if o < CONSUMER_D_A else f
        have = np.flatnonzero(rng.random(upto) < 0.3)
        have = have[np.argsort(have + rng.normal(0, 2.0, len(have)))]
        seq = np.repeat(have, 1 + (rng.random(len(have)) < 0.04)).tolist()        # (a tandem pair now and then)
        cut = int(rng.integers(0, len(seq) + 1))
        contigs += [(o, seq[:cut], 500 if rng.random() < 0.4 else -1), (o, seq[cut:], -1)]
        if o % 5 == 0:
            contigs.append((o, [10, 11, 10, 11, 10], -1))
    for k in range(CONSUMER_HUB_NEIGHBOURS):
        contigs.append((int(rng.integers(0, d)), [CONSUMER_HUB, 20 + k], -1))
    contigs += [(0, list(range(CONSUMER_SHARED)), -1), (d - 1, list(range(CONSUMER_SHARED, f)), 90)]      # (every family has a gene)
    out = contigs_orders([c for c in contigs if len(c[1])], d, rng, n=f)
    out["repeated"][[3, 40, 41, 150, 270, 299]] = 1
    out["gene_len"] = (out["ends"] - out["starts"]).astype(np.int32)
    return out


def consumer_parts():
    """consumer_orders() cut at CONSUMER_D_A: two_parts' four orders"""
    o = consumer_orders()
    d = CONSUMER_D_A + CONSUMER_D_B
    return two_parts(dict(slice_orders(o, 0, CONSUMER_D_A)), dict(slice_orders(o, CONSUMER_D_A, d)), CONSUMER_D_A, CONSUMER_D_B)
