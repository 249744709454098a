"""Merging two masters, on the host: chunks.master_arrays_merge (the numpy statement of nemgpu_master_merge) against
master_arrays_from_orders of the concatenated orders and against master_arrays_append_orders, where both parts are built
with the same repeated families -- on the recorded add_organism fixtures split into base and update and on random
annotation sets cut at a random organism; a part numbered apart, in a larger id space, with the ids that lead back
(either part); parts built with different repeated families, where the merge is by construction not the single build:
a hand-written case with every row spelled out and a random one; the 2^24 bound on the summed count; its associativity;
and what the library refuses before it looks at a master."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import master_arrays_merge
from tests import master_shapes as ms
from tests.append_util import build_host, slice_orders
from tests.merge_util import (different_repeated_parts, fixture_cases, host_expectations, host_merge, random_cases,
                              random_different_repeated_parts, relabelled, same_with_order, scattered_ids, triple_alone, two_parts)
from tests.orders_util import synthetic_orders


def test_fixtures_equal_one_build_and_the_append():
    names = []
    for name, (a, b, u, whole) in fixture_cases():
        ma, mb, got = host_expectations(a, b, u, whole, name)
        assert got[0].shape == (len(got[4]), a["d"] + b["d"]) and np.array_equal(got[4][:len(ma[4])], ma[4])
        names.append(name)
    assert len(names) >= 4


def test_random_splits_equal_one_build_and_the_append():
    tally = dict(cases=0, new_family=0, shared_family=0, new_entry=0, shared_entry=0, extras_a=0, extras_b=0, loops=0)
    for name, (a, b, u, whole) in random_cases(20261201, 300, max_fam=14):
        ma, mb, got = host_expectations(a, b, u, whole, name)
        n_a, n_b, n = len(ma[4]), len(mb[4]), len(got[4])
        nnz_a, nnz_b, nnz = len(ma[1][1]), len(mb[1][1]), len(got[1][1])
        tally["cases"] += 1
        tally["new_family"] += n - n_a
        tally["shared_family"] += n_a + n_b - n
        tally["new_entry"] += nnz - nnz_a
        tally["shared_entry"] += nnz_a + nnz_b - nnz
        tally["extras_a"] += len(ma[3][1])
        tally["extras_b"] += len(mb[3][1])
        tally["loops"] += sum(int(r in got[1][1][got[1][0][r]:got[1][0][r + 1]]) for r in range(n))
        assert len(got[3][1]) == len(ma[3][1]) + len(mb[3][1])
    assert tally["cases"] > 200 and all(v > 100 for v in tally.values()), tally


def test_ids_in_another_id_space():
    """B numbered on its own: its ids in A's space are given, the new families take the ids the caller names"""
    a = ms.contigs_orders([(0, [0, 1, 2]), (1, [2, 1, 1])], 2, 3)
    b = ms.contigs_orders([(0, [0, 1, 2, 1])], 1, 3)           # B's ids 0, 1, 2 are A's 7, 1, 5
    ma, mb = build_host(a), build_host(b)
    got = master_arrays_merge(ma, ma[4], mb, np.asarray([7, 1, 5])[mb[4]])
    assert got[4].tolist() == [0, 1, 2, 7, 5] and got[0].tolist() == [[1, 0, 0], [1, 1, 1], [1, 1, 0], [0, 0, 1], [0, 0, 1]]
    rows = [got[1][1][p:q].tolist() for p, q in zip(got[1][0][:-1], got[1][0][1:])]
    assert rows == [[1], [0, 2, 1, 3, 4], [1], [1], [1]]
    with pytest.raises(ValueError):
        master_arrays_merge(ma, ma[4], mb, [7, 1, 7])
    with pytest.raises(ValueError):
        master_arrays_merge(ma, ma[4], mb, [7, 1])


def test_b_numbered_apart_in_a_larger_id_space():
    """B built from its own orders with every id i written sigma[i] (scattered over 3 f ids), merged with the ids that
    lead back (sigma^-1 of B's order): the single build of everything, order included -- at 40 + 10 families x 33 + 31
    organisms (an organism word crossed on either side) and on the fixtures"""
    base = synthetic_orders(40, 33, 533, density=0.5, p_repeat=0.05)
    upd = slice_orders(synthetic_orders(50, 64, 1533, density=0.5, p_repeat=0.0), 33, 64)
    upd["repeated"] = np.r_[base["repeated"], np.zeros(10, np.uint8)]
    cases = [("40 + 10 x 33 + 31", two_parts(base, upd, 33, 31))] + list(fixture_cases())
    for seed, (name, (a, b, u, whole)) in enumerate(cases):
        f = len(b["repeated"])
        sigma, inverse = scattered_ids(f, 3 * f, 90 + seed)
        ma, mb = build_host(a), build_host(relabelled(b, sigma, 3 * f))
        assert np.array_equal(inverse[mb[4]], build_host(b)[4]) and (f < 3 or not np.array_equal(np.argsort(sigma), np.arange(f)))
        got = master_arrays_merge(ma, ma[4], mb, inverse[mb[4]])
        same_with_order(got, build_host(whole), name + ": one build")
        # and the other way round: A numbered apart, B's ids led into A's space; the merged order is sigma of the build's
        ma = build_host(relabelled(a, sigma, 3 * f))
        mb = build_host(b)
        got = master_arrays_merge(ma, ma[4], mb, sigma[mb[4]])
        want = build_host(whole)
        same_with_order(got, tuple(want[:4]) + (sigma[want[4]],), name + ": A numbered apart")
    assert len(cases) >= 5


def test_parts_built_with_different_repeated_families():
    """A was built with family 3 repeated, B with family 1.  The statement keeps what each part gave: family 1 has A's
    node, row and bits and gains nothing from B's genes of it; family 3 has B's node and row, mapped, and is absent from
    A's organisms though A walked genes of it.  The single build with either repeated vector, or their union, is
    another master."""
    a, b = different_repeated_parts()
    ma, mb = build_host(a), build_host(b)
    rows = lambda m: [m[1][1][p:q].tolist() for p, q in zip(m[1][0][:-1], m[1][0][1:])]
    assert ma[4].tolist() == [0, 1, 2, 4] and rows(ma) == [[1, 2], [0, 2], [1, 3, 0], [2]]
    assert mb[4].tolist() == [3, 0, 4] and rows(mb) == [[1, 2], [0], [0]] and mb[3][2].tolist() == [2, 2]
    got = host_merge(ma, mb)
    assert got[4].tolist() == [0, 1, 2, 4, 3]
    assert got[0].tolist() == [[1, 1, 1], [1, 1, 0], [1, 1, 0], [1, 0, 1], [0, 0, 1]]
    assert rows(got) == [[1, 2, 4], [0, 2], [1, 3, 0], [2, 4], [0, 3]]
    assert got[2].ravel().tolist() == [3, 2, 4, 3, 1, 1, 1, 2, 1, 4, 4, 4]
    assert got[3][0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2] and got[3][1].tolist() == [2, 2] and got[3][2].tolist() == [2, 2]
    # family 1 (row 1): as in A
    assert rows(got)[1] == rows(ma)[1] and got[2].ravel()[3:5].tolist() == ma[2].ravel()[2:4].tolist() and got[0][1].tolist() == ma[0][1].tolist() + [0]
    whole = ms.concat_orders([a, dict(b, contig_org=b["contig_org"] + 2)], 3)
    for rep in ([3], [1], [1, 3]):
        one = build_host(dict(whole, repeated=np.isin(np.arange(5), rep).astype(np.uint8)))
        assert one[4].tolist() != got[4].tolist()
    # at random: no repeated family in A, some in B -- those keep A's rows among A's families
    ra, rb = random_different_repeated_parts()
    ma, mb = build_host(ra), build_host(rb)
    got = host_merge(ma, mb)
    rep = np.flatnonzero(rb["repeated"])
    at = np.flatnonzero(np.isin(ma[4], rep))
    assert len(at) >= 3 and not np.isin(mb[4], rep).any() and not got[0][at, ra["d"]:].any()
    assert np.array_equal(got[0][:len(ma[4]), :ra["d"]], ma[0])
    for r in at:                                              # (its row: A's, entry for entry -- B has no node of it to hang an edge on)
        mine = got[1][1][got[1][0][r]:got[1][0][r + 1]]
        assert np.array_equal(mine[:ma[1][0][r + 1] - ma[1][0][r]], ma[1][1][ma[1][0][r]:ma[1][0][r + 1]])
        assert len(mine) == ma[1][0][r + 1] - ma[1][0][r]


def test_the_count_bound_is_on_the_sum():
    half = 1 << 10
    small = [build_host(ms.alternating_orders(k, 0, 1)) for k in (half, half + 1)]
    assert host_merge(small[0], small[1])[3][2].tolist() == [half, half + 1] * 2
    big = tuple(small[0][:3]) + ((small[0][3][0], small[0][3][1], np.asarray([ms.COUNT_BOUND - half] * 2, np.int32)),) + tuple(small[0][4:])
    host_merge(big, small[0])                                 # (2^24 exactly is taken)
    with pytest.raises(ValueError, match="2\\^24"):
        host_merge(big, small[1])


def test_merge_is_associative():
    """merge(merge(A, B), C) is merge(A, merge(B, C)), array for array, and both are the build of everything"""
    parts = triple_alone()
    masters = [build_host(p) for p in parts]
    for a, b, c in (masters[:3], masters[1:]):
        left, right = host_merge(host_merge(a, b), c), host_merge(a, host_merge(b, c))
        same_with_order(left, right, "associativity")
        assert left[0].shape == right[0].shape and np.array_equal(left[0], right[0])
    everything = host_merge(host_merge(host_merge(masters[0], masters[1]), masters[2]), masters[3])
    same_with_order(everything, ms.triple_masters()[-1], "three merges against three appends")


def test_library_refuses_before_it_looks_at_a_master():
    """nemgpu_master_merge without its output, with an f that lies above no id and without a master: refused on the host
    (no device is needed to see it)"""
    from pangenomenem_amd import build
    from pangenomenem_amd.chunks import _bind_master
    from pangenomenem_amd.engine import load_library
    build.build()
    lib = _bind_master(load_library())
    assert lib.nemgpu_master_merge(None, None, None, None, 5) == 8
    for f in (0, -3):
        h = C.c_void_p(1)
        rc = lib.nemgpu_master_merge(C.byref(h), None, None, None, f)
        assert rc == 3 and not h.value and "f must lie above" in lib.nemgpu_last_error().decode(), (f, rc)
    h = C.c_void_p(1)
    rc = lib.nemgpu_master_merge(C.byref(h), None, None, None, 5)
    assert rc == 8 and not h.value and "masters" in lib.nemgpu_last_error().decode()
