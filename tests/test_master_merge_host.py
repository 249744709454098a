"""Merging two masters, on the host: chunks.master_arrays_merge (the numpy statement of nemgpu_master_merge) against
master_arrays_from_orders of the concatenated orders and against master_arrays_append_orders, where both parts are built
with the same repeated families -- on the recorded add_organism fixtures split into base and update and on random
annotation sets cut at a random organism; its associativity; and what the library refuses before it looks at a master."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import master_arrays_merge
from tests import master_shapes as ms
from tests.append_util import build_host
from tests.merge_util import fixture_cases, host_expectations, host_merge, random_cases, same_with_order, triple_alone


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
