"""The resident master's one block through its three creators (csrc/nem_master.hip: from arrays, from gene orders, by an
append) where its layout branches: no CSR entry at all, entries without a multi-copy pair (no extras section), with one,
and an append that gives a master its first.  Every master is read back whole and compared for equality with the numpy
statement (chunks.master_arrays_from_orders / master_arrays_append_orders), the array-built one with what went in.  And
what nemgpu_master_project refuses of a live master, by code and message."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from tests.append_util import append_host, build_host
from tests.orders_util import same_master

pytestmark = pytest.mark.gpu

D, F = 37, 300                                                # (two words of organisms, the second partly used)
E_ARG, E_FUNCARG = 3, 8


def orders(contigs, orgs, d=D, circular=None):
    ptr = np.cumsum([0] + [len(c) for c in contigs]).astype(np.int32)
    return dict(genes=np.asarray([f for c in contigs for f in c], np.int32), contig_ptr=ptr, contig_org=np.asarray(orgs, np.int32),
                contig_circular=np.asarray(circular if circular is not None else [0] * len(contigs), np.uint8), d=d,
                repeated=np.zeros(F, np.uint8))


def no_edge():
    """one gene per contig, nothing circular"""
    return orders([[f] for f in range(F)], [j % D for j in range(F)])


def single_copies():
    """one contig of 8 consecutive families per organism: every (edge, organism) pair once"""
    return orders([list(range(5 * o, 5 * o + 8)) for o in range(D)], list(range(D)))


def multi_copy_update(first_column):
    """3 organisms behind first_column; the second walks 0 1 0 1 (circular): the pair (0, 1) three times in it"""
    return orders([[190, 191, 192], [0, 1, 0, 1], [7, 250, 8]], [first_column, first_column + 1, first_column + 2], d=first_column + 3,
                  circular=[0, 1, 0])


def with_multi_copies():
    a, b = single_copies(), multi_copy_update(D)
    return dict(genes=np.concatenate([a["genes"], b["genes"]]), contig_ptr=np.concatenate([a["contig_ptr"], a["contig_ptr"][-1] + b["contig_ptr"][1:]]),
                contig_org=np.concatenate([a["contig_org"], b["contig_org"]]), contig_circular=np.concatenate([a["contig_circular"], b["contig_circular"]]),
                d=D + 3, repeated=a["repeated"])


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def check(m, want, what, order):
    try:
        got = m.arrays()
        assert m.shape() == (want[0].shape[0], want[0].shape[1], len(want[1][1]), len(want[3][1])), what
        same_master(got, want, what)
        assert np.array_equal(got[4], order) and np.array_equal(m.order, order), what + ": family order"
    finally:
        m.close()


def test_every_creator_at_every_layout(gpu_lib):
    grown = None
    for what, o, nnz_zero, has_extras in (("no edge", no_edge(), True, False), ("single copies", single_copies(), False, False),
                                          ("multi copies", with_multi_copies(), False, True)):
        want = build_host(o)
        assert (len(want[1][1]) == 0) == nnz_zero and (len(want[3][1]) > 0) == has_extras, what    # (the branch meant)
        check(from_orders(o), want, what + ", from orders", want[4])
        check(Master(want[0], want[1][0], want[1][1], want[2], edge_counts=want[3]), want, what + ", from arrays", np.arange(len(want[0])))
        if what == "single copies":                           # the append that brings the first extras
            upd = multi_copy_update(D)
            grown = append_host(want, F, upd, 3)
            assert len(grown[3][1]) > 0
            m = from_orders(o)
            try:
                assert m.shape()[3] == 0
                check(m.add_orders(upd["genes"], upd["contig_ptr"], upd["contig_org"], upd["contig_circular"], 3, repeated=upd["repeated"]),
                      grown, "first extras by an append", grown[4])
            finally:
                m.close()
        if what == "multi copies":                            # (and the append equals the build of everything)
            same_master(grown, want, "append against build")
    bits = build_host(single_copies())                        # nemgpu_master_create: no counts at all
    check(Master(bits[0], bits[1][0], bits[1][1], bits[2]), bits, "bits only", np.arange(len(bits[0])))


def test_projection_refusals_on_a_live_master(gpu_lib):
    o = single_copies()
    m, directed = from_orders(o), from_orders(o, directed=True)
    lib = m.lib

    def project(h, part=None, genes=(0, 1, 2), ptr=(0, 3), org=(0,), f=F, g=None, null=()):
        arrs = [np.ascontiguousarray(np.zeros(m.n) if part is None else part, np.uint8), np.ascontiguousarray(genes, np.int32),
                np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(org, np.int32)]
        at = [None if i in null else a.ctypes.data for i, a in enumerate(arrs)]
        rc = lib.nemgpu_master_project(h, at[0], f, at[1], len(arrs[1]) if g is None else g, at[2], at[3], len(arrs[3]), None, None, None, None, None)
        return rc, lib.nemgpu_last_error().decode()

    try:
        assert project(m._h)[0] == 0                          # (well-formed, no output asked for)
        assert project(m._h, genes=(), ptr=(0,), org=())[0] == 0
        high = np.zeros(m.n, np.uint8)
        high[m.n - 1] = 4
        for kw, rc_want, word in ((dict(part=high), E_ARG, "class 4"), (dict(org=(D,)), E_ARG, "organism"), (dict(org=(-1,)), E_ARG, "organism"),
                                  (dict(genes=(0, F, 2)), E_ARG, "family id"), (dict(genes=(0, -1, 2)), E_ARG, "family id"),
                                  (dict(ptr=(0, 2)), E_ARG, "contig_ptr"), (dict(ptr=(1, 3)), E_ARG, "contig_ptr"),
                                  (dict(ptr=(0, 2, 1, 3), org=(0, 0, 0)), E_ARG, "monotone"), (dict(g=1 << 30), E_ARG, "2^30"),
                                  (dict(f=0), E_FUNCARG, "needed"), (dict(null=(0,)), E_FUNCARG, "needed"), (dict(null=(1,)), E_FUNCARG, "needed"),
                                  (dict(null=(2,)), E_FUNCARG, "needed"), (dict(null=(3,)), E_FUNCARG, "needed"), (dict(g=-1), E_FUNCARG, "needed")):
            rc, msg = project(m._h, **kw)
            assert rc == rc_want and word in msg and msg.startswith(("nemgpu_master_project", "orders")), (kw, rc, msg)
        rc, msg = project(directed._h)
        assert rc == E_ARG and "directed" in msg, (rc, msg)
    finally:
        m.close()
        directed.close()
