"""Appending organisms to a master, on the host: chunks.master_arrays_append_orders (the numpy statement of
nemgpu_master_append_orders) against chunks.master_arrays_from_graph applied to the graph the reference's own
add_organism left (tests/golden/orders_update/, made by tests/golden/make_orders_update.py); against
master_arrays_from_orders of the concatenated orders where both parts have the same repeated families; against the
transcription of tests/test_orders_host.py run base-then-update on one graph where the update adds repeated families;
and what the library refuses before any device call."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import master_arrays_append_orders, master_arrays_from_graph, orders_from_annotations
from tests.append_util import UPDATE_FIXTURES, append_host, build_host, fixture_parts, part_orders, split_annotations
from tests.orders_util import RecordedGraph, load, random_genomes, same_master
from tests.test_orders_host import neighborhood_graph


def row_lists(m):
    ptr, idx = m[1]
    return [list(idx[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]


def reached(base, got, upd):
    """which of the append's cases a (base master, grown master, update orders) triple shows"""
    n0, nnz0 = base[0].shape[0], len(base[1][1])
    rows0, rows1 = row_lists(base), row_lists(got)
    total = lambda m: np.unpackbits(np.asarray(m[2], np.uint32).view(np.uint8), axis=1).sum(axis=1) + \
        np.add.reduceat(np.append(m[3][2] - 1, 0), m[3][0][:-1]) * (np.diff(m[3][0]) > 0) if len(m[1][1]) else np.zeros(0, np.int64)
    t0, t1 = total(base), total(got)
    old_entry = np.concatenate([got[1][0][r] + np.arange(len(rows0[r])) for r in range(n0)]).astype(np.int64) if nnz0 else np.zeros(0, np.int64)
    kept_ids = set(int(i) for i in upd["genes"][upd["repeated"][upd["genes"]] == 0])
    late_rep = set(int(i) for i in base[4]) & set(int(i) for i in upd["genes"][upd["repeated"][upd["genes"]] != 0])
    xd0, xd1 = np.diff(base[3][0]), np.diff(got[3][0])
    return dict(recount=int((t1[old_entry] > t0).sum()) if nnz0 else 0,
                row_end=sum(len(rows1[r]) > len(rows0[r]) for r in range(n0)),
                new_family=got[0].shape[0] - n0,
                unsorted=sum(list(np.sort(r)) != list(r) for r in rows1),
                late_repeated=len(late_rep),
                unseen=len(kept_ids - set(int(i) for i in base[4])),
                extra_on_extra=int(((xd1[old_entry] > xd0) & (xd0 > 0)).sum()) if nnz0 else 0,
                first_extra=int(xd0.sum() == 0 and xd1.sum() > 0),
                loops=sum(r in row for r, row in enumerate(rows1)))


@pytest.mark.parametrize("path", UPDATE_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixture_equals_recorded_graph(path):
    rec = load(path)
    base, upd = fixture_parts(rec)
    m0 = build_host(base)
    assert m0[0].shape[0] == rec["base_nodes"]
    got = append_host(m0, len(base["families"]), upd, len(rec["new_organisms"]))
    want = master_arrays_from_graph(RecordedGraph(rec["undirected"], False), rec["organisms"] + rec["new_organisms"])
    assert [upd["families"][i] for i in got[4]] == list(want[4]), "family order"
    assert np.array_equal(got[4][:len(m0[4])], m0[4])
    same_master(got, want, rec["name"])


def test_fixtures_cover_the_cases():
    assert len(UPDATE_FIXTURES) >= 4
    seen = {}
    for rec in map(load, UPDATE_FIXTURES):
        base, upd = fixture_parts(rec)
        m0 = build_host(base)
        seen[rec["name"]] = reached(m0, append_host(m0, len(base["families"]), upd, len(rec["new_organisms"])), upd)
    g = seen["grow"]
    assert g["recount"] and g["row_end"] and g["new_family"] == 2 and g["unsorted"], g
    assert seen["repeated_late"]["late_repeated"] == 1 and seen["repeated_late"]["new_family"] == 0, seen["repeated_late"]
    assert seen["unseen"]["unseen"] == 2 and seen["unseen"]["new_family"] == 2, seen["unseen"]
    c = seen["circular_dup"]
    assert c["extra_on_extra"] and c["loops"] >= 2 and c["new_family"] == 1, c
    rec = {r["name"]: r for r in map(load, UPDATE_FIXTURES)}["circular_dup"]
    adj = {a: dict((b, data) for b, data in nbrs) for a, nbrs in rec["undirected"]["adj"]}
    assert adj["A"]["B"]["o1"] == 2 and adj["A"]["B"]["o3"] == 3 and adj["A"]["A"]["o3"] >= 2 and adj["B"]["C"]["o3"] == 2
    unseen = {r["name"]: r for r in map(load, UPDATE_FIXTURES)}["unseen"]
    assert "Q" not in adj and all(f not in ("Q", "S") for f, _ in unseen["undirected"]["nodes"])


def random_split(rng, parts_n):
    ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 9)), int(rng.integers(parts_n, 8)))
    cuts = np.sort(rng.choice(np.arange(1, len(orgs)), parts_n - 1, replace=False))
    parts, cols = split_annotations(ann, orgs, cuts)
    return parts, cols, circular, repeated


def test_random_append_equals_one_build():
    """the same repeated families on both sides: append(build(A), B) is the build of A + B, field by field"""
    rng = np.random.default_rng(20261101)
    tally = dict()
    for case in range(300):
        parts, cols, circular, repeated = random_split(rng, 2)
        (a, b), whole = part_orders(parts, cols, circular, repeated)
        m0 = build_host(a)
        got = append_host(m0, len(a["families"]), b, len(parts[1]))
        want = build_host(whole)
        assert b["families"] == whole["families"]             # (one id space: the update numbers on from the base)
        assert np.array_equal(got[4], want[4]), case
        same_master(got, want, "case %d" % case)
        for k, v in reached(m0, got, b).items():
            tally[k] = tally.get(k, 0) + v
    for k in ("recount", "row_end", "new_family", "unsorted", "unseen", "extra_on_extra", "loops"):
        assert tally[k] > 100, (k, tally)
    assert tally["first_extra"] >= 3, tally                   # (a base without a multi-copy pair is rare here)


def test_two_appends_equal_one_build():
    rng = np.random.default_rng(20261102)
    for case in range(100):
        parts, cols, circular, repeated = random_split(rng, 3)
        (a, b, c), whole = part_orders(parts, cols, circular, repeated)
        m1 = append_host(build_host(a), len(a["families"]), b, len(parts[1]))
        m2 = append_host(m1, len(b["families"]), c, len(parts[2]))
        want = build_host(whole)
        assert np.array_equal(m2[4], want[4]), case
        same_master(m2, want, "case %d" % case)


def test_grown_repeated_equals_the_transcription(monkeypatch):
    """the update declares more families repeated: the statement against ppanggolin.py:463-530's transcription walking
    the base, then the update with the united set, on ONE graph"""
    import networkx
    rng = np.random.default_rng(20261103)
    late = bridged_total = 0
    for case in range(300):
        parts, cols, circular, repeated = random_split(rng, 2)
        names = sorted({info[1] for part in parts for contigs in part.values() for annot in contigs.values() for info in annot.values()})
        more = [f for f in names if f not in repeated and rng.random() < 0.2]
        base = orders_from_annotations(parts[0], cols[:len(parts[0])], circular, repeated)
        upd = orders_from_annotations(parts[1], cols, circular, list(repeated) + more, families=base["families"])
        with monkeypatch.context() as mp:
            g, _ = neighborhood_graph(parts[0], set(circular), set(repeated), False)
            mp.setattr(networkx, "Graph", lambda: g)           # (the transcription makes its graph itself: hand it the base's)
            g2, (_, bridged) = neighborhood_graph(parts[1], set(circular), set(repeated) | set(more), False)
        assert g2 is g
        m0 = build_host(base)
        got = append_host(m0, len(base["families"]), upd, len(parts[1]))
        if g.number_of_nodes() == 0:
            assert got[0].shape[0] == 0
            continue
        want = master_arrays_from_graph(g, cols)
        assert [upd["families"][i] for i in got[4]] == list(want[4]), case
        same_master(got, want, "case %d" % case)
        late += reached(m0, got, upd)["late_repeated"]
        bridged_total += bridged
    assert late > 50 and bridged_total > 100, (late, bridged_total)


def good():
    base = build_host(dict(genes=np.array([0, 1, 2, 1], np.int32), contig_ptr=np.array([0, 3, 4], np.int32), contig_org=np.array([0, 1], np.int32),
                           contig_circular=np.array([1, 0], np.uint8), d=2, repeated=np.zeros(3, np.uint8)))
    return base, dict(genes=[0, 3, 2], contig_ptr=[0, 2, 3], contig_org=[2, 3], contig_circular=[0, 1], d_new=2, repeated=[0, 0, 0, 0])


@pytest.mark.parametrize("field,value", [("genes", [0, 4, 2]), ("genes", [0, -1, 2]), ("contig_ptr", [0, 4, 3]), ("contig_ptr", [1, 2, 3]),
                                         ("contig_org", [1, 2]), ("contig_org", [2, 4]), ("contig_circular", [1]), ("repeated", [0, 0]),
                                         ("d_new", 0), ("f", 2)])
def test_malformed_appends_raise(field, value):
    base, upd = good()
    master_arrays_append_orders(base, base[4], 3, **upd)
    with pytest.raises(ValueError):
        args = dict(upd, **{field: value})
        if field == "f":
            args["repeated"] = None
        master_arrays_append_orders(base, base[4], 3, **args)


def test_library_checks_the_update_before_any_device_call():
    """nemgpu_master_append_orders refuses what it can judge without the master on the host, before it looks at the
    master (NEMGPU_E_ARG and a message): no device is needed to see it; then it asks for the master"""
    from pangenomenem_amd import build
    from pangenomenem_amd.chunks import _bind_master
    from pangenomenem_amd.engine import load_library
    build.build()
    lib = _bind_master(load_library())

    def append(genes, ptr, org, circ, d_new, f):
        arrs = [np.ascontiguousarray(genes, np.int32), np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(org, np.int32),
                np.ascontiguousarray(circ, np.uint8)]
        h = C.c_void_p(1)
        rc = lib.nemgpu_master_append_orders(C.byref(h), None, d_new, f, arrs[0].ctypes.data, len(arrs[0]), arrs[1].ctypes.data,
                                             arrs[2].ctypes.data, arrs[3].ctypes.data, len(arrs[2]), None)
        assert not h.value
        return rc, lib.nemgpu_last_error().decode()

    for args, word in ((([0, 1, 3], [0, 3], [0], [0], 1, 3), "family id"), (([0, 1, 2], [0, 2, 1, 3], [0, 0, 0], [0, 0, 0], 1, 3), "monotone"),
                       (([0, 1, 2], [0, 2], [0], [0], 1, 3), "contig_ptr"), (([0, 1, 2], [0, 3], [1], [0], 1, 3), "organism"),
                       (([0, 1, 2], [0, 3], [-1], [0], 1, 3), "organism"), (([0, 1, 2], [0, 3], [0], [0], 0, 3), "d_new"),
                       (([0, 1, 2], [0, 3], [0], [0], -2, 3), "d_new"), (([0, 1, 2], [0, 3], [0], [0], 131072 * 32 + 1, 3), "131 072")):
        rc, msg = append(*args)
        assert rc == 3 and word in msg, (args, rc, msg)
    rc, msg = append([0, 1, 2], [0, 3], [0], [0], 1, 0)         # (what the orders lack is refused as the build refuses it)
    assert rc == 8 and "needed" in msg, (rc, msg)
    rc, msg = append([0, 1, 2], [0, 3], [0], [0], 1, 3)
    assert rc == 8 and "master" in msg, (rc, msg)
