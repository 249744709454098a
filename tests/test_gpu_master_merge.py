"""Two resident masters merged on the device (nemgpu_master_merge, csrc/nem_merge.hip) against the numpy statement
chunks.master_arrays_merge and against the single build of all the organisms -- which tests/test_master_merge_host.py
holds equal on the host -- on the recorded fixtures, on random annotation sets and at the shapes where a stride changes
or a path is first taken; its associativity; the two inputs left as they were; partition() on a merged master and on
the master of everything; merge_named; what is refused."""
import ctypes as C
import random
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from tests import master_shapes as ms
from tests.append_util import slice_orders, split_annotations
from tests.merge_util import alone, fixture_cases, host_expectations, host_merge, random_cases, same_with_order, triple_alone, two_parts
from tests.orders_util import random_genomes, same_master, synthetic_orders

pytestmark = pytest.mark.gpu


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def device_equals_host(case, what):
    """case: merge_util.two_parts' four orders.  The device's merge of the two parts' masters equals the statement's, which
    equals the single build and the append; both inputs are afterwards what they were.  Returns the host masters
    (A's, B's, the merged one)."""
    a, b, u, whole = case
    ma, mb, want = host_expectations(a, b, u, whole, what)
    da, db = from_orders(a), from_orders(b)
    try:
        before = da.arrays(), db.arrays()
        m = da.merge(db)
        try:
            got = m.arrays()
            assert m.shape() == (want[0].shape[0], want[0].shape[1], len(want[1][1]), len(want[3][1])), what
            assert (m.n, m.d, m.wf, m.f) == (want[0].shape[0], want[0].shape[1], (want[0].shape[1] + 31) // 32, max(da.f, db.f)), what
            assert np.array_equal(m.order, want[4]), what + ": .order"
            same_with_order(got, want, what)
        finally:
            m.close()
        for dev, was, host in ((da, before[0], ma), (db, before[1], mb)):
            same_with_order(dev.arrays(), was, what + ": an input afterwards")
            same_with_order(was, host, what + ": an input")
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


def usable(*masters):
    """the masters answer as before and merge"""
    for m in masters:
        assert m.shape()[0] == m.n
    if len(masters) == 2:
        ok = masters[0].merge(masters[1])
        assert ok.d == masters[0].d + masters[1].d
        ok.close()


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
