"""Two resident masters merged on the device (nemgpu_master_merge, csrc/nem_merge.hip) against the numpy statement
chunks.master_arrays_merge and against the single build of all the organisms -- which tests/test_master_merge_host.py
holds equal on the host -- through one helper (merged): arrays, .order, shape(), .f and .wf, both inputs left as they
were, the result merged on once more.  On the recorded fixtures, on random annotation sets and at the shapes where a
stride changes or a path is first taken; a part numbered apart (its ids scattered over three times the id space, the
ids that lead back given; either part; the default f, the scattered space, one far above) at the organism-word shapes
and over several scan tiles; masters made from arrays (the identity numbering) as A, as B and as both around a family
word and with extras; a side, or both, without an edge; a master merged with itself and the result with itself; B's
first extras on an entry A has; parts built with different repeated families, held to the statement alone; chains of
merges and appends, and an append after a merge into a larger id space; associativity; partition() on a merged master
and on the master of everything; merge_named; what is refused.  Every other consumer of a merged master:
tests/test_gpu_merged_consumers.py."""
import ctypes as C
import random
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master, master_arrays_merge
from pangenomenem_amd.engine import NemGpuError
from tests import master_shapes as ms
from tests.append_util import append_host, build_host, slice_orders, split_annotations
from tests.merge_util import (alone, arrays_master, different_repeated_parts, fixture_cases, host_expectations, host_merge, identity_numbered,
                              random_cases, random_different_repeated_parts, relabelled, same_with_order, scattered_ids, triple_alone, two_parts)
from tests.orders_util import random_genomes, same_master, synthetic_orders

pytestmark = pytest.mark.gpu


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def usable(*masters):
    """the masters answer as before and merge"""
    for m in masters:
        assert m.shape()[0] == m.n
    if len(masters) == 2:
        ok = masters[0].merge(masters[1])
        assert ok.d == masters[0].d + masters[1].d
        ok.close()


def merged(da, db, want, what, hosts=None, ids=None, f=None):
    """da.merge(db, ids, f), held to `want` (the statement's arrays and order): arrays and .order equal, shape(), .f and
    .wf right, both inputs afterwards what they were (and what hosts = (A's, B's) says they are), the result usable: it
    answers and merges with A once more, which shares its id space.  Returns the merged master, open."""
    before = da.arrays(), db.arrays()
    want_f = f if f is not None else max(da.f, db.f) if ids is None else max(da.f, int(np.max(ids)) + 1)
    m = da.merge(db, ids=ids, f=f)
    try:
        n, d = np.asarray(want[0]).shape
        assert m.shape() == (n, d, len(want[1][1]), len(want[3][1])), what
        assert (m.n, m.d, m.wf, m.f) == (n, d, (d + 31) // 32, want_f), what
        assert np.array_equal(m.order, want[4]), what + ": .order"
        same_with_order(m.arrays(), want, what)
        for k, (dev, was) in enumerate(((da, before[0]), (db, before[1])) if db is not da else ((da, before[0]),)):
            same_with_order(dev.arrays(), was, what + ": an input afterwards")
            if hosts is not None:
                same_with_order(was, hosts[k], what + ": an input")
        usable(m, da)
        same_with_order(m.arrays(), want, what + ": after it was merged on")
    except BaseException:
        m.close()
        raise
    return m


def device_equals_host(case, what):
    """case: merge_util.two_parts' four orders.  The device's merge of the two parts' masters equals the statement's, which
    equals the single build and the append; both inputs are afterwards what they were.  Returns the host masters
    (A's, B's, the merged one)."""
    a, b, u, whole = case
    ma, mb, want = host_expectations(a, b, u, whole, what)
    da, db = from_orders(a), from_orders(b)
    try:
        merged(da, db, want, what, hosts=(ma, mb)).close()
    finally:
        da.close()
        db.close()
    return ma, mb, want


def device_equals_statement(a, b, what):
    """the orders of two parts that no single build states (different repeated families): the device's merge against the
    statement's alone.  Returns the host masters (A's, B's, the merged one)."""
    ma, mb = build_host(a), build_host(b)
    want = host_merge(ma, mb)
    da, db = from_orders(a), from_orders(b)
    try:
        merged(da, db, want, what, hosts=(ma, mb)).close()
    finally:
        da.close()
        db.close()
    return ma, mb, want


def test_fixtures(gpu_lib):
    for name, case in fixture_cases():
        device_equals_host(case, name)


def test_random_annotations(gpu_lib):
    done = fresh = multi = 0
    for name, case in random_cases(20261202, 70, max_fam=60, max_org=24, max_len=30):
        ma, mb, got = device_equals_host(case, name)
        done += 1
        fresh += len(got[4]) - len(ma[4])
        multi += len(mb[3][1])
    assert done >= 55 and fresh > 20 and multi > 300, (done, fresh, multi)


def synthetic_two(nf_a, d_a, nf, d_b, seed, density=0.5):
    """A: nf_a families x d_a organisms; B: d_b organisms over nf >= nf_a family ids; no repeated family"""
    base = synthetic_orders(nf_a, d_a, seed, density=density, p_repeat=0.0)
    upd = slice_orders(synthetic_orders(nf, d_a + d_b, seed + 1000, density=density, p_repeat=0.0), d_a, d_a + d_b)
    upd["repeated"] = np.zeros(nf, np.uint8)
    return two_parts(base, upd, d_a, d_b)


@pytest.mark.parametrize("d_a,d_b", [(1, 1), (31, 33), (32, 64), (33, 31), (64, 65)])
def test_organism_word_boundaries(gpu_lib, d_a, d_b):
    """B's bits go up by d_a: a funnel shift of two words (d_a % 32 != 0) or a word copy; the stride grows or stays"""
    ma, mb, got = device_equals_host(synthetic_two(40, d_a, 50, d_b, 500 + d_a), "d %d + %d" % (d_a, d_b))
    assert ma[0].shape == (40, d_a) and mb[0].shape[1] == d_b and got[0].shape[1] == d_a + d_b and got[0].shape[0] > 40
    assert len(got[1][1]) > len(ma[1][1]) and len(ma[1][1]) + len(mb[1][1]) > len(got[1][1])       # new entries and shared ones


@pytest.mark.parametrize("n_a,new", [(63, 65), (64, 64)])
def test_family_word_boundaries(gpu_lib, n_a, new):
    """the presence rows' last word: A ends inside a word or on its end, B fills up to the end of the next"""
    ma, mb, got = device_equals_host(synthetic_two(n_a, 5, n_a + new, 2, 600 + n_a, density=1.0), "n %d + %d" % (n_a, new))
    assert ma[0].shape[0] == n_a and got[0].shape[0] == n_a + new and mb[0].shape[0] == n_a + new


def test_b_shares_every_family(gpu_lib):
    ma, mb, got = device_equals_host(synthetic_two(30, 6, 30, 2, 71, density=1.0), "no new row")
    assert got[0].shape[0] == ma[0].shape[0] == 30 and len(got[1][1]) > len(ma[1][1])


def test_b_shares_no_family(gpu_lib):
    base = synthetic_orders(30, 6, 72, density=0.5, p_repeat=0.0)
    upd = slice_orders(synthetic_orders(30, 9, 73, density=0.5, p_repeat=0.0), 6, 9)
    upd = dict(upd, genes=(upd["genes"] + 30).astype(np.int32), repeated=np.zeros(60, np.uint8))
    ma, mb, got = device_equals_host(two_parts(base, upd, 6, 3), "disjoint")
    assert got[0].shape[0] == ma[0].shape[0] + mb[0].shape[0] and len(got[1][1]) == len(ma[1][1]) + len(mb[1][1])
    assert not got[0][:30, 6:].any() and not got[0][30:, :6].any()


def test_b_without_a_new_edge(gpu_lib):
    base = synthetic_orders(30, 6, 74, density=0.5, p_repeat=0.0)
    upd = slice_orders(base, 2, 4)                            # (organisms 2 and 3 once more, as 6 and 7)
    upd = dict(upd, contig_org=upd["contig_org"] + 4)
    ma, mb, got = device_equals_host(two_parts(base, upd, 6, 2), "no new edge")
    assert np.array_equal(got[1][0], ma[1][0]) and np.array_equal(got[1][1], ma[1][1]) and np.array_equal(got[0][:, 6:], ma[0][:, 2:4])


def test_b_without_any_edge(gpu_lib):
    """every contig of B is one gene: presence alone, of families A has and of new ones"""
    base = synthetic_orders(30, 6, 75, density=0.5, p_repeat=0.0)
    upd = ms.contigs_orders([(6 + k % 2, [fam]) for k, fam in enumerate((3, 35, 4, 31, 29, 33))], 8, 36)
    ma, mb, got = device_equals_host(two_parts(base, upd, 6, 2), "no edge")
    assert len(mb[1][1]) == 0 and np.array_equal(got[1][1], ma[1][1]) and got[0].shape[0] == 33 and got[0][:, 6:].sum() == 6


def test_a_hub_row_gains_entries(gpu_lib):
    """A's row of some 400 neighbours, which B's entries are looked up in (50 found) and which gains B's new ones: the
    families A lacks, 20 it has elsewhere and the hub's two neighbours in the update's chain of even families"""
    base, upd = ms.hub_parts()
    ma, mb, got = device_equals_host(two_parts(base, upd, 3, 2), "hub")
    deg = lambda m, r: int(m[1][0][r + 1] - m[1][0][r])
    assert deg(ma, ms.HUB) == ms.HUB_OLD + 2 and deg(got, ms.HUB) == deg(ma, ms.HUB) + ms.HUB_NEW + 20 + 2


def test_a_master_without_extras_gains_its_first(gpu_lib):
    rng = np.random.default_rng(76)
    base = ms.contigs_orders([(o, rng.permutation(30)[:15]) for o in range(6)], 6, 30)
    upd = ms.contigs_orders([(6, np.r_[[0, 1, 0, 1], 2 + rng.permutation(28)[:12]])], 7, 30)
    ma, mb, got = device_equals_host(two_parts(base, upd, 6, 1), "first extra")
    assert len(ma[3][1]) == 0 and len(got[3][1]) == len(mb[3][1]) > 0


@pytest.mark.parametrize("b_first", [False, True])
def test_more_than_32_extras(gpu_lib, b_first):
    """entry (0, 1) has 40 extras on one side and 30 on the other: B's go behind A's; with b_first B's entry has the 40"""
    base, upd = ms.extras_parts()
    if b_first:
        a = alone(upd, ms.EXTRAS_BASE, ms.EXTRAS_BASE + ms.EXTRAS_UPDATE)
        case = two_parts(a, dict(base, contig_org=base["contig_org"] + ms.EXTRAS_UPDATE), ms.EXTRAS_UPDATE, ms.EXTRAS_BASE)
    else:
        case = two_parts(base, upd, ms.EXTRAS_BASE, ms.EXTRAS_UPDATE)
    ma, mb, got = device_equals_host(case, "extras")
    assert np.diff(mb[3][0]).max() == (ms.EXTRAS_BASE if b_first else ms.EXTRAS_UPDATE) and np.diff(got[3][0]).max() == ms.EXTRAS_BASE + ms.EXTRAS_UPDATE


def test_entries_over_several_scan_tiles(gpu_lib):
    """B's entries, whose "A lacks it" flags are scanned, and the merged entries span several scan tiles"""
    base, _ = ms.scan_parts()
    upd = ms.part_of(ms.scan_orders(), ms.SCAN_BASE, ms.SCAN_BASE + 16)
    ma, mb, got = device_equals_host(two_parts(base, upd, ms.SCAN_BASE, 16), "scan tiles")
    assert ms.scan_tiles(len(mb[1][1])) >= 4 and ms.scan_tiles(len(got[1][1])) > ms.scan_tiles(len(mb[1][1])) and len(got[3][1]) > 0
    assert ms.scan_tiles(got[0].shape[0]) >= 2


def test_tandem_duplicates_on_both_sides(gpu_lib):
    """self-loops in A and in B, of the same family and of different ones: each stays one entry"""
    base = ms.contigs_orders([(0, [0, 0, 1, 2, 2, 2, 3]), (1, [4, 4, 0, 0, 0])], 2, 8)
    upd = ms.contigs_orders([(2, [0, 0, 5, 5, 1, 1]), (3, [6, 2, 2, 7, 7, 7])], 4, 8)
    ma, mb, got = device_equals_host(two_parts(base, upd, 2, 2), "self-loops")
    loops = lambda m: [r for r in range(m[0].shape[0]) if r in m[1][1][m[1][0][r]:m[1][0][r + 1]]]
    assert got[4].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and loops(ma) == [0, 2, 4] and loops(got) == [0, 1, 2, 4, 5, 7]


# ---- a part numbered apart
def numbered_apart(case, what, f_given=None, seed=7):
    """case: two_parts' four orders.  B built with its ids scattered over 3 x the shared count, merged with the ids that
    lead back; then A built that way, merged with B's ids led into A's space (a table of 3 x the count slots, seeded in
    no order).  Both are held to the statement and to from_orders of everything.  f_given: the f of the first merge
    (None: the default, the smallest that holds both)."""
    a, b, u, whole = case
    shared = len(b["repeated"])
    f = 3 * shared
    sigma, inverse = scattered_ids(shared, f, seed)
    ma, mb, one = build_host(a), build_host(b), build_host(whole)
    apart = relabelled(b, sigma, f)
    mb_apart = build_host(apart)
    single = from_orders(whole)
    da, db, db_apart = from_orders(a), from_orders(b), from_orders(apart)
    da_apart = from_orders(relabelled(a, sigma, f))
    try:
        same_with_order(single.arrays(), one, what + ": the single build")
        assert db_apart.f == f and da.f == shared and np.array_equal(db_apart.order, sigma[db.order])
        ids = inverse[db_apart.order]
        new_ids = ids[~np.isin(ids, da.order)]
        assert len(new_ids) > 1 and (np.diff(sigma[new_ids]) < 0).any()       # (the new families' ids: another order than B's own)
        want = master_arrays_merge(ma, ma[4], mb_apart, inverse[mb_apart[4]])
        same_with_order(want, one, what + ": the statement")
        m = merged(da, db_apart, want, what + ": B apart", hosts=(ma, mb_apart), ids=ids, f=f_given)
        same_with_order(m.arrays(), single.arrays(), what + ": B apart, the single build")
        m.close()
        ma_apart = build_host(relabelled(a, sigma, f))
        want = master_arrays_merge(ma_apart, ma_apart[4], mb, sigma[mb[4]])
        same_with_order(want, tuple(one[:4]) + (sigma[one[4]],), what + ": the statement, A apart")
        m = merged(da_apart, db, want, what + ": A apart", hosts=(ma_apart, mb), ids=sigma[db.order])
        assert m.f == f > 2 * m.n and np.array_equal(m.order, sigma[single.order])
        same_master(m.arrays(), single.arrays(), what + ": A apart, the single build")
        m.close()
    finally:
        for x in (single, da, db, db_apart, da_apart):
            x.close()


@pytest.mark.parametrize("d_a,d_b", [(31, 33), (32, 64), (33, 31), (64, 65)])
@pytest.mark.parametrize("f_given", [None, 150, 1000])
def test_numbered_apart_at_the_organism_word_boundaries(gpu_lib, d_a, d_b, f_given):
    """test_organism_word_boundaries' shapes (50 shared ids) with one part's ids scattered over 150: with the default f,
    with f the scattered space and with an f far above everything"""
    numbered_apart(synthetic_two(40, d_a, 50, d_b, 500 + d_a), "apart d %d + %d f %s" % (d_a, d_b, f_given), f_given, seed=d_a)


def test_numbered_apart_over_several_scan_tiles(gpu_lib):
    """3 000 ids scattered over 9 000: the flags of B's families, whose scan numbers the new ones, and the table's seeding
    run over more than one scan tile and many blocks"""
    base, _ = ms.scan_parts()
    cut = 2 * ms.SCAN_FAMILIES // 3                           # (A: the contigs' genes of the first 2 000 ids, so B brings new families)
    keep = base["genes"] < cut
    ptr = np.concatenate([[0], np.cumsum(keep)])[base["contig_ptr"]].astype(np.int32)
    base = dict(base, genes=base["genes"][keep], contig_ptr=ptr)
    upd = ms.part_of(ms.scan_orders(), ms.SCAN_BASE, ms.SCAN_BASE + 8)
    case = two_parts(base, upd, ms.SCAN_BASE, 8)
    mb = build_host(case[1])
    assert ms.scan_tiles(mb[0].shape[0]) >= 2 and ms.scan_tiles(len(mb[1][1])) >= 4
    assert mb[0].shape[0] - np.isin(mb[4], build_host(case[0])[4]).sum() > 256       # (new families over several blocks)
    numbered_apart(case, "apart, scan tiles", 3 * ms.SCAN_FAMILIES)


# ---- masters made from arrays: the identity numbering
def ids_in_the_numbering_of(ma, mb):
    """the ids of B's families in the id space of A made from arrays (A's family i is id i): a shared family's is its
    number in A, the others' lie behind, in no order of B's"""
    f = int(max(ma[4].max(), mb[4].max())) + 1
    newid = np.full(f, -1, np.int64)
    newid[ma[4]] = np.arange(len(ma[4]))
    rest = np.flatnonzero(newid < 0)
    newid[rest] = len(ma[4]) + np.random.default_rng(f).permutation(len(rest))
    return newid[mb[4]]


def from_arrays_cases(case, what):
    """A, B and both as masters made from arrays of the host masters (their order: the identity, none kept by the
    library), with the ids that join them and, where B is from arrays, without (B's family j is then id j)"""
    a, b, u, whole = case
    ma, mb, one = build_host(a), build_host(b), build_host(whole)
    ia, ib = identity_numbered(ma), identity_numbered(mb)
    made = [from_orders(a), from_orders(b), arrays_master(ma), arrays_master(mb)]
    da, db, xa, xb = made
    try:
        assert np.array_equal(xa.order, np.arange(xa.n)) and (xa.f, xb.f) == (xa.n, xb.n)
        joined = ids_in_the_numbering_of(ma, mb)
        for A, hA, B, hB, ids, name in ((xa, ia, db, mb, joined, "A from arrays"), (da, ma, xb, ib, mb[4], "B from arrays"),
                                        (xa, ia, xb, ib, joined, "both from arrays"), (da, ma, xb, ib, None, "B from arrays, its numbers the ids"),
                                        (xa, ia, xb, ib, None, "both from arrays, one numbering")):
            want = master_arrays_merge(hA, hA[4], hB, ib[4] if ids is None else ids)
            if ids is not None:                               # (the same families joined: the single build's arrays)
                same_master(want, one, what + ": " + name + ": the statement")
            m = merged(A, B, want, what + ": " + name, hosts=(hA, hB), ids=ids)
            m.close()
    finally:
        for x in made:
            x.close()
    return ma, mb, one


@pytest.mark.parametrize("n_a,new", [(62, 1), (63, 1), (63, 2), (64, 64), (65, 3)])
def test_masters_made_from_arrays_around_a_family_word(gpu_lib, n_a, new):
    """63, 64 and 65 families in A, in B and in all: the identity numbering in the table's seeding and in the entry
    point's ids"""
    ma, mb, one = from_arrays_cases(synthetic_two(n_a, 5, n_a + new, 3, 640 + n_a + new, density=1.0), "arrays %d + %d" % (n_a, new))
    assert ma[0].shape[0] == n_a and one[0].shape[0] == n_a + new


def test_masters_made_from_arrays_with_extras(gpu_lib):
    base, upd = ms.extras_parts()
    ma, mb, one = from_arrays_cases(two_parts(base, upd, ms.EXTRAS_BASE, ms.EXTRAS_UPDATE), "arrays, extras")
    assert len(ma[3][1]) > ms.EXTRAS_BASE and len(mb[3][1]) > ms.EXTRAS_UPDATE


# ---- a side without edges
def singles(families, d, f, first=0):
    return ms.contigs_orders([(first + k % d, [fam]) for k, fam in enumerate(families)], first + d, f)


def test_a_without_any_edge(gpu_lib):
    """every contig of A is one gene: no entry to look B's up in, every entry of B new, in rows A has and in new ones"""
    upd = slice_orders(synthetic_orders(36, 9, 79, density=0.5, p_repeat=0.0), 6, 9)
    ma, mb, got = device_equals_host(two_parts(singles(range(0, 30, 2), 6, 36), upd, 6, 3), "A without an edge")
    assert len(ma[1][1]) == 0 and len(mb[1][1]) > 30 and len(got[1][1]) == len(mb[1][1]) and len(got[3][1]) == len(mb[3][1])
    assert 15 < got[0].shape[0] <= 36 and got[0][:15, :6].sum() == 15


def test_neither_side_with_an_edge(gpu_lib):
    ma, mb, got = device_equals_host(two_parts(singles(range(0, 40, 2), 3, 70), singles(range(0, 70, 3), 2, 70, first=3), 3, 2), "no edge at all")
    assert len(got[1][1]) == 0 and got[0].shape == (20 + 24 - 7, 5) and not got[1][0].any() and got[0].sum() == 20 + 24


# ---- a master merged with itself
@pytest.mark.parametrize("which", ["extras", "random"])
def test_a_master_merged_with_itself_and_the_result_with_itself(gpu_lib, which):
    """every entry of B is found, every extra of B goes behind A's: the rows stay, every bit and every extra is there
    twice, d apart.  Then the same of the result (its record was set by the merge)."""
    o = ms.extras_parts()[0] if which == "extras" else ms.with_repeats(synthetic_orders(60, 33, 83, density=0.5, p_repeat=0.03))
    h = build_host(o)
    d = o["d"]
    twice = master_arrays_merge(h, h[4], h, h[4])
    assert np.array_equal(twice[1][0], h[1][0]) and np.array_equal(twice[1][1], h[1][1]) and np.array_equal(twice[4], h[4])
    assert np.array_equal(twice[0], np.concatenate([h[0], h[0]], axis=1)) and np.array_equal(twice[3][0], 2 * h[3][0])
    per = [(twice[3][1][p:q], twice[3][2][p:q]) for p, q in zip(twice[3][0][:-1], twice[3][0][1:])]
    assert all(np.array_equal(org[len(org) // 2:], org[:len(org) // 2] + d) and np.array_equal(cnt[len(cnt) // 2:], cnt[:len(cnt) // 2]) for org, cnt in per)
    assert len(h[3][1]) > 0 and (which != "extras" or np.diff(h[3][0]).max() == ms.EXTRAS_BASE)
    four = master_arrays_merge(twice, twice[4], twice, twice[4])
    a = from_orders(o)
    try:
        m = merged(a, a, twice, which + ": with itself", hosts=(h,), ids=a.order)
        try:
            merged(m, m, four, which + ": the result with itself", hosts=(twice,), ids=m.order).close()
            nothing_given = a.merge(a)                        # (the default ids are other.order)
            same_with_order(nothing_given.arrays(), twice, which + ": ids left out")
            nothing_given.close()
        finally:
            m.close()
    finally:
        a.close()


def test_b_has_extras_a_has_none_on_an_entry_both_have(gpu_lib):
    """A has the entries (0, 1) and (1, 0) with every count 1 and no extras at all; B walks 0 1 0 1: its extras go to an
    entry that was found in A, with no A extras to skip.  (test_a_master_without_extras_gains_its_first's random base
    happens to hold the entry (0, 1) too; here it is there by construction and asserted.)"""
    base = ms.contigs_orders([(0, [0, 1, 2, 3, 4, 5]), (1, [5, 3, 1, 0, 2]), (2, [4, 2, 0])], 3, 8)
    upd = ms.contigs_orders([(3, [0, 1, 0, 1, 6, 2]), (4, [7, 1, 0])], 5, 8)
    ma, mb, got = device_equals_host(two_parts(base, upd, 3, 2), "first extras on a shared entry")
    deg_a = np.zeros(got[0].shape[0], np.int64)
    deg_a[:ma[0].shape[0]] = np.diff(ma[1][0])
    row = np.repeat(np.arange(got[0].shape[0]), np.diff(got[1][0]))
    from_a = np.arange(len(row)) - got[1][0][row] < deg_a[row]
    assert len(ma[3][1]) == 0 and len(mb[3][1]) == 2 and (np.diff(got[3][0]) > 0).sum() == 2 and from_a[np.diff(got[3][0]) > 0].all()


# ---- parts built with different repeated families
def test_parts_built_with_different_repeated_families(gpu_lib):
    """the device keeps what each part gave, as the statement says (tests/test_master_merge_host.py spells the rows out):
    not the single build's master"""
    a, b = different_repeated_parts()
    ma, mb, got = device_equals_statement(a, b, "repeated 3 | repeated 1")
    assert got[4].tolist() == [0, 1, 2, 4, 3] and got[0].tolist() == [[1, 1, 1], [1, 1, 0], [1, 1, 0], [1, 0, 1], [0, 0, 1]]
    a, b = random_different_repeated_parts()
    ma, mb, got = device_equals_statement(a, b, "repeated in B alone")
    rep = np.flatnonzero(b["repeated"])
    assert np.isin(ma[4], rep).sum() >= 3 and not np.isin(mb[4], rep).any() and got[0].shape == (50, 24)


# ---- chains of merges and appends
def add_orders(m, u, d_new, **kw):
    return m.add_orders(u["genes"], u["contig_ptr"], u["contig_org"], u["contig_circular"], d_new, repeated=kw.pop("repeated", u["repeated"]), **kw)


def test_chains_of_merges_and_appends(gpu_lib):
    """ms.triple_parts(): A, then B, C and D as masters of their own (merged) or as updates (appended), every step held to
    the statement applied in the same order and the ends to the appends alone (one id space, the same repeated
    families: from_orders of everything)"""
    parts, alone_parts = ms.triple_parts(), triple_alone()
    widths = np.diff((0,) + ms.TRIPLE_STAGES)
    host = [build_host(p) for p in alone_parts]
    ends = ms.triple_masters()
    made = [from_orders(p) for p in alone_parts]
    everything = from_orders(ms.concat_orders(parts, ms.TRIPLE_STAGES[-1]))
    made.append(everything)
    try:
        same_with_order(everything.arrays(), ends[3], "from_orders of everything")
        # merge(A, B).add_orders(C), then merged with D
        h_ab = host_merge(host[0], host[1])
        ab = merged(made[0], made[1], h_ab, "A + B", hosts=host[:2])
        made.append(ab)
        h_abc = append_host(h_ab, 300, parts[2], widths[2])
        abc = add_orders(ab, parts[2], widths[2])
        made.append(abc)
        same_with_order(abc.arrays(), h_abc, "merge(A, B).add_orders(C)")
        same_with_order(h_abc, ends[2], "merge(A, B).add_orders(C): the appends")
        same_with_order(h_abc, build_host(ms.concat_orders(parts[:3], ms.TRIPLE_STAGES[2])), "merge(A, B).add_orders(C): one build")
        assert np.array_equal(abc.order, h_abc[4]) and abc.f == 300
        same_with_order(ab.arrays(), h_ab, "A + B after the append")
        h_abcd = host_merge(h_abc, host[3])
        same_with_order(h_abcd, ends[3], "merge(merge(A, B).add_orders(C), D): the appends")
        abcd = merged(abc, made[3], h_abcd, "merge(merge(A, B).add_orders(C), D)", hosts=(h_abc, host[3]))
        made.append(abcd)
        same_with_order(abcd.arrays(), everything.arrays(), "merge(merge(A, B).add_orders(C), D): from_orders")
        # A.add_orders(B).merge(C)
        h_ab2 = append_host(host[0], 300, parts[1], widths[1])
        ab2 = add_orders(made[0], parts[1], widths[1])
        made.append(ab2)
        same_with_order(ab2.arrays(), h_ab2, "A.add_orders(B)")
        h_abc2 = host_merge(h_ab2, host[2])
        same_with_order(h_abc2, ends[2], "A.add_orders(B).merge(C): the appends")
        made.append(merged(ab2, made[2], h_abc2, "A.add_orders(B).merge(C)", hosts=(h_ab2, host[2])))
    finally:
        for m in made:
            m.close()


def test_an_append_after_a_merge_into_a_larger_id_space(gpu_lib):
    """merged with f = 900: the merged master's id space is 900 ids, an append may not name fewer and works with as many"""
    parts, alone_parts = ms.triple_parts(), triple_alone()
    sigma, inverse = scattered_ids(300, 900, 11)
    host = [build_host(alone_parts[0]), build_host(relabelled(alone_parts[1], sigma, 900))]
    a, b = from_orders(alone_parts[0]), from_orders(relabelled(alone_parts[1], sigma, 900))
    made = [a, b]
    try:
        want = master_arrays_merge(host[0], host[0][4], host[1], inverse[host[1][4]])
        ab = merged(a, b, want, "A + B apart, f 900", hosts=host, ids=inverse[b.order], f=900)
        made.append(ab)
        before = ab.arrays()
        for f in (300, 899):
            with pytest.raises(NemGpuError, match="below the master's 900 family ids"):
                add_orders(ab, parts[2], 25, repeated=np.r_[parts[2]["repeated"], np.zeros(f - 300, np.uint8)], f=f)
        same_with_order(ab.arrays(), before, "after the refusals")
        abc = add_orders(ab, parts[2], 25, repeated=np.r_[parts[2]["repeated"], np.zeros(600, np.uint8)], f=900)
        made.append(abc)
        assert abc.f == 900
        same_with_order(abc.arrays(), ms.triple_masters()[2], "appended with f = 900")
    finally:
        for m in made:
            m.close()


def test_merge_is_associative(gpu_lib):
    parts = triple_alone()
    host = [ms.host_master(p) for p in parts]
    dev = [from_orders(p) for p in parts]
    made = []
    try:
        for a, b, c in ((0, 1, 2), (1, 2, 3)):
            ab = dev[a].merge(dev[b])
            bc = dev[b].merge(dev[c])
            left, right = ab.merge(dev[c]), dev[a].merge(bc)
            made += [ab, bc, left, right]
            same_with_order(left.arrays(), right.arrays(), "associativity")
            assert left.shape() == right.shape() and np.array_equal(left.order, right.order)
            same_with_order(left.arrays(), host_merge(host_merge(host[a], host[b]), host[c]), "the statement")
    finally:
        for m in made + dev:
            m.close()


def test_partition_on_a_merged_master(gpu_lib):
    """merge(...).partition() is from_orders(everything).partition(): labels, counts, samples and the generator's state,
    where the vote loop runs (40 organisms, chunks of 16)"""
    o = synthetic_orders(300, 40, 7, density=0.5, p_repeat=0.03)
    a, b = dict(slice_orders(o, 0, 32), d=32), alone(slice_orders(o, 32, 40), 32, 40)
    da, db, whole = from_orders(a), from_orders(b), from_orders(o)
    m = da.merge(db)
    try:
        same_with_order(m.arrays(), whole.arrays(), "merged")
        r1, r2 = random.Random(5), random.Random(5)
        rm = m.partition(chunk_size=16, rng=r1, batch=8, tie="libc", seed=3)
        rw = whole.partition(chunk_size=16, rng=r2, batch=8, tie="libc", seed=3)
        assert rm[0] == rw[0] and np.array_equal(rm[1], rw[1]) and rm[2] == rw[2] and rm[2] > 1 and r1.getstate() == r2.getstate()
        ra = da.partition(chunk_size=16, rng=random.Random(5), batch=8, tie="libc", seed=3)      # (the inputs still work)
        assert ra[2] > 0 and len(ra[0]) == da.n
    finally:
        for x in (da, db, whole, m):
            x.close()


def test_merge_named(gpu_lib):
    rng = np.random.default_rng(20261203)
    done = 0
    while done < 5:
        ann, orgs, circular, repeated = random_genomes(rng, 20, 12, max_len=30)
        parts, cols = split_annotations(ann, orgs, [int(rng.integers(1, len(orgs)))])
        d_a = len(parts[0])
        try:
            a = Master.from_annotations(parts[0], cols[:d_a], circular, repeated)
        except (NemGpuError, ValueError):
            continue                                          # (no gene, or none kept)
        try:
            b = Master.from_annotations(parts[1], cols[d_a:], circular, repeated)
        except (NemGpuError, ValueError):
            a.close()
            continue
        whole = Master.from_annotations(OrderedDict((k, v) for part in parts for k, v in part.items()), cols, circular, repeated)
        m = a.merge_named(b)
        try:
            assert m.names == whole.names and m.organism_names == whole.organism_names == cols and m.id_names[:len(a.id_names)] == a.id_names
            assert [m.id_names[i] for i in m.order] == m.names and m.repeated_by_organism == whole.repeated_by_organism
            same_master(m.arrays(), whole.arrays(), "merge_named")
            with pytest.raises(ValueError, match="organism"):
                m.merge_named(b)
            with pytest.raises(ValueError, match="organism"):
                a.merge_named(a)
            assert a.names == whole.names[:a.n] and b.organism_names == cols[d_a:]
        finally:
            for x in (a, b, whole, m):
                x.close()
        done += 1
    plain = from_orders(ms.contigs_orders([(0, [0, 1])], 1, 2))
    named = Master.from_annotations(parts[0], cols[:d_a], circular, repeated)
    with pytest.raises(ValueError, match="names"):
        named.merge_named(plain)
    plain.close()
    named.close()


def test_refusals(gpu_lib):
    base = synthetic_orders(30, 6, 77, density=0.5, p_repeat=0.0)
    good, other = from_orders(base), from_orders(alone(slice_orders(synthetic_orders(30, 8, 78, density=0.5, p_repeat=0.0), 6, 8), 6, 8))
    directed = from_orders(base, directed=True)
    x, (ptr, idx), eb = ms.boundary_master(65, 33)
    bits_only = Master(x, ptr, idx, eb)
    try:
        for bad, word in ((directed, "directed"), (bits_only, "bits-only")):
            for a, b in ((bad, good), (good, bad)):
                with pytest.raises(NemGpuError, match=word):
                    a.merge(b)
            usable(bad)
        for a, b in ((directed, good), (good, directed)):     # (past Python's own check: the library's)
            h = C.c_void_p()
            rc = good.lib.nemgpu_master_merge(C.byref(h), a._h, b._h, None, 30)
            assert rc == 3 and not h.value and "directed" in good.lib.nemgpu_last_error().decode()
        ids = other.order.copy()
        twice = ids.copy()
        twice[-1] = twice[0]
        with pytest.raises(NemGpuError, match="used twice"):
            good.merge(other, ids=twice)
        for value, f in ((-1, None), (30, 30), (200, 100)):
            out = ids.copy()
            out[1] = value
            with pytest.raises(NemGpuError, match="out of range"):
                good.merge(other, ids=out, f=f if f is not None else 30)
        with pytest.raises(NemGpuError, match="family ids"):
            good.merge(other, f=29)                           # (below A's id space)
        usable(good, other)
    finally:
        for m in (good, other, directed, bits_only):
            m.close()


def test_too_many_organisms_in_all(gpu_lib):
    """one-family masters of half the limit and of half the limit + 1 organisms: refused by the sum, before any allocation"""
    half = 131072 // 2
    one = lambda d: from_orders(ms.contigs_orders([(d - 1, [0])], d, 1))
    a, b = one(half), one(half + 1)
    try:
        with pytest.raises(NemGpuError, match="131 072"):
            a.merge(b)
        usable(a)
        usable(b)
        full = a.merge(a)                                     # (the limit itself is taken)
        assert full.shape() == (1, 2 * half, 0, 0)
        full.close()
    finally:
        a.close()
        b.close()


def test_count_bound_crossed_by_the_sum(gpu_lib):
    """entry (0, 1) counts 2^23 in A; with a B that counts 2^23 the sum is taken (2^24 is exact in a float), with one that
    counts 2^23 + 1 it is refused though neither side alone passes the bound"""
    half = ms.COUNT_BOUND // 2
    a, b = from_orders(ms.alternating_orders(half, 0, 1)), from_orders(ms.alternating_orders(half + 1, 0, 1))
    try:
        ok = a.merge(a)
        try:
            _, _, _, (xptr, xorg, xcnt), _ = ok.arrays()
            assert ok.shape() == (2, 2, 2, 4) and xorg.tolist() == [0, 1, 0, 1] and xcnt.tolist() == [half] * 4
        finally:
            ok.close()
        for x, y in ((a, b), (b, a)):
            with pytest.raises(NemGpuError, match="2\\^24"):
                x.merge(y)
        assert a.shape() == (2, 1, 2, 2) and b.shape() == (2, 1, 2, 2)
    finally:
        a.close()
        b.close()
