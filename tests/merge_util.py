"""What tests/test_master_merge_host.py and tests/test_gpu_master_merge.py share: a pangenome's gene orders cut into two
parts that are built alone (each with its own columns 0 .. d - 1, both with the same repeated families, their family ids
in one id space), and the three masters the merge of the two is held against."""
import numpy as np

from pangenomenem_amd.chunks import master_arrays_merge
from tests import master_shapes as ms
from tests.append_util import UPDATE_FIXTURES, append_host, build_host, fixture_parts, part_orders, split_annotations
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
