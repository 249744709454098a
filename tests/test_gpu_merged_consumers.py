"""Every consumer of a resident master on a MERGED one (nemgpu_master_merge sets the master's record itself: order,
f_old, nx, the strides, the extras pointers; arrays() shows none of that, nor the padding behind n and d).  Two fixtures
of some 300 families x 33 + 31 organisms (merge_util.consumer_orders: repeated families, extras, self-loops, a hub row,
new families in the second part): whole = from_orders(everything) and m = from_orders(A).merge(from_orders(B)), once in
one id space and once with A numbered apart (m.order scattered ids, m.f three times whole.f, the orders handed to the
consumers relabelled), held equal before anything else runs.  Each consumer's output on m is held to that consumer's
own host statement through the helper of its own test file, at that file's tolerance, and byte for byte to the same
call on whole: family_table, edge_table with its organism lines and metadata, project_orders, partition_shell's formed
problem, organism_clustering, tile_plot, layout and evolution (partition(): tests/test_gpu_master_merge.py).  Afterwards
the three masters are what they were; and a consumer runs on a merged master whose inputs were closed first."""
import random

import numpy as np
import pytest

from pangenomenem_amd import tileplot as tp
from pangenomenem_amd.chunks import Master
from pangenomenem_amd.shell import Subproblem
from tests.merge_util import (CONSUMER_D_A, CONSUMER_D_B, CONSUMER_HUB, consumer_orders, consumer_parts, relabelled, same_with_order,
                              scattered_ids)
from tests.orders_util import same_master
from tests.projection_util import random_part
from tests.test_gpu_gexf import device_equals_statement as edge_table_equals_statement
from tests.test_gpu_gexf import table_of as edge_table_of
from tests.test_gpu_gexf_metadata import attributes, held_to_statement as metadata_held_to_statement
from tests.test_gpu_layout import held_to_the_statement as layout_held_to_the_statement
from tests.test_gpu_matrix import device_equals_statement as family_table_equals_statement
from tests.test_gpu_matrix import table_of as family_table_of
from tests.test_gpu_partition_shell import same_problem
from tests.test_gpu_projection import device_equals_host as projection_equals_host
from tests.test_gpu_tileplot import same_merges

pytestmark = pytest.mark.gpu

D = CONSUMER_D_A + CONSUMER_D_B


def from_orders(o):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])


class Pair:
    """whole and m with the orders each is asked with (mine: m's, in m's id space; plain: whole's)"""

    def __init__(self, apart):
        a, b, _, everything = consumer_parts()
        self.plain = consumer_orders()
        f = len(self.plain["repeated"])
        self.whole = from_orders(everything)
        if apart:
            sigma, _ = scattered_ids(f, 3 * f, 20270302)
            self.da, self.db = from_orders(relabelled(a, sigma, 3 * f)), from_orders(b)
            self.m = self.da.merge(self.db, ids=sigma[self.db.order])
            self.mine = relabelled(self.plain, sigma, 3 * f)
            same_master(self.m.arrays(), self.whole.arrays(), "merged, A numbered apart")
            assert np.array_equal(self.m.order, sigma[self.whole.order]) and self.m.f == 3 * f > self.whole.f == f
            assert (np.diff(self.m.order) < 0).sum() > self.m.n // 4
        else:
            self.da, self.db = from_orders(a), from_orders(b)
            self.m = self.da.merge(self.db)
            self.mine = self.plain
            same_with_order(self.m.arrays(), self.whole.arrays(), "merged")
        self.masters = (self.m, self.da, self.db, self.whole)
        self.before = [x.arrays() for x in self.masters]
        rows, (ptr, idx), eb, counts, _ = self.before[0]
        self.x = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :D]
        self.arrays = (self.x, ptr, idx, eb, counts)
        n, hub = self.m.n, int(np.flatnonzero(self.whole.order == CONSUMER_HUB)[0])
        assert 280 < n <= 300 and self.m.d == D and self.da.d == CONSUMER_D_A and self.m.n > self.da.n + 20      # (new families in B)
        assert len(counts[1]) > len(self.before[1][3][1]) > 0 and len(self.before[2][3][1]) > 0                 # (extras on both sides)
        assert ptr[hub + 1] - ptr[hub] > 200 and ptr[hub + 1] - ptr[hub] > np.diff(self.before[1][1][0]).max()   # (a hub row that grew)
        assert (idx == np.repeat(np.arange(n), np.diff(ptr))).sum() > 20 and self.plain["repeated"].sum() > 3    # (self-loops, repeated)

    def close(self):
        for x in self.masters:
            x.close()


@pytest.fixture(scope="module", params=[False, True], ids=["one id space", "A numbered apart"])
def pair(request, gpu_lib):
    p = Pair(request.param)
    yield p
    p.close()


def both(pair, call):
    """call(master, its orders) on m and on whole"""
    return call(pair.m, pair.mine), call(pair.whole, pair.plain)


def same_bytes(got, want, what):
    assert type(got) is type(want), what
    if isinstance(got, dict):
        assert list(got) == list(want), what
        got, want = list(got.values()), list(want.values())
    if isinstance(got, (tuple, list)):
        assert len(got) == len(want), what
        for k, (a, b) in enumerate(zip(got, want)):
            same_bytes(a, b, "%s [%d]" % (what, k))
        return
    a, b = np.asarray(got), np.asarray(want)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_family_table(pair):
    n = pair.m.n
    family_table_equals_statement(pair.m, pair.mine, "merged", batches=[(0, 40), (40, 60), (100, n - 100)])       # (cut inside a word of families)

    def call(m, o):
        t = family_table_of(m, o)
        try:
            return t.arrays(), t.rtab_cells(), t.rtab_cells(40, 60)
        finally:
            t.close()
    same_bytes(*both(pair, call), "family_table")


def test_edge_table_its_organism_lines_and_its_metadata(pair):
    want = edge_table_equals_statement(pair.m, pair.mine, "merged")
    ne = len(want["src"])
    assert int(want["weight"].max()) > 10 and (want["src"] == want["dst"]).sum() > 20
    attr_id = np.arange(D, dtype=np.int32) * 3 + 8
    meta = attributes(np.random.default_rng(4), D, (D, 3), (7, 12345))           # (an attribute of d values: every organism another one)
    t = edge_table_of(pair.m, pair.mine)
    try:
        assert t.n_edges == ne
        metadata_held_to_statement(pair.m, t, meta, "merged", batches=[(0, 70), (70, ne - 70)])
    finally:
        t.close()

    def call(m, o):
        t = edge_table_of(m, o)
        try:
            t.set_metadata(*meta)
            return t.arrays(), t.attvalues(attr_id), t.metamasks(), t.metavalues()
        finally:
            t.close()
    same_bytes(*both(pair, call), "edge_table")


def test_project_orders_of_all_organisms_and_of_the_second_part(pair):
    part = random_part(np.random.default_rng(6), pair.m.n)
    host = pair.before[0]                                     # (the merged master's own arrays, its own order)

    def of_part(o):
        """the contigs of B's organisms alone: columns d_a .. d - 1"""
        sel = np.flatnonzero(o["contig_org"] >= CONSUMER_D_A)
        g0 = int(o["contig_ptr"][sel[0]])
        assert sel[-1] == len(o["contig_org"]) - 1 and (np.diff(sel) == 1).all()
        return dict(genes=o["genes"][g0:], contig_ptr=o["contig_ptr"][sel[0]:] - g0, contig_org=o["contig_org"][sel[0]:], repeated=o["repeated"])
    for what, cut in (("all organisms", lambda o: o), ("the second part's organisms", of_part)):
        want = projection_equals_host(pair.m, host, part, cut(pair.mine), "merged: " + what, len(pair.mine["repeated"]))
        assert (want[0] == -1).sum() > 50 and (want[1] >= 2).sum() > 400                 # (genes of repeated families; copies)
        if cut is of_part:
            assert not want[3][:CONSUMER_D_A].any() and want[3][CONSUMER_D_A:].any(axis=1).all()

        def call(m, o):
            p = cut(o)
            return m.project_orders(part, p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"], len(p["repeated"]))
        same_bytes(*both(pair, call), "project_orders: " + what)


@pytest.mark.parametrize("organisms", [None, list(range(CONSUMER_D_A + 9, CONSUMER_D_A - 12, -1)) + [0, D - 1]], ids=["all", "astride d_a"])
def test_the_shell_problem(pair, organisms):
    n = pair.m.n
    select = np.arange(n) % 3 != 1
    select[np.flatnonzero(pair.whole.order == CONSUMER_HUB)[0]] = True
    fam, (ptr, idx, w) = same_problem(pair.m, pair.arrays, select, organisms)
    assert len(fam) > n // 2 and int(np.diff(ptr).max()) > 50 and float(w.max()) > 20.0     # (the hub's row; an edge many organisms carry)

    def call(m, o):
        sub = Subproblem(m, select, 3, organisms, "induced")
        try:
            return sub.families, sub.fetch()
        finally:
            sub.close()
    same_bytes(*both(pair, call), "the shell problem")


def test_organism_clustering_and_the_tile_plot(pair):
    part = random_part(np.random.default_rng(8), pair.m.n)
    c = pair.m.organism_clustering()
    try:
        dist = tp.organism_distances_host(pair.x)
        assert c.distances().tobytes() == dist.tobytes(), "merged: distances"
        same_merges(c, tp.hclust_complete_host(dist), "merged")
    finally:
        c.close()
    plot = pair.m.tile_plot(part)
    try:
        assert np.array_equal(plot.family_order, tp.family_plot_order(part, (pair.x != 0).sum(axis=1), D))
        assert plot.cells().tobytes() == tp.tile_cells_host(pair.x, plot.family_order, plot.organism_order).tobytes()
    finally:
        plot.close()

    def call(m, o):
        c, plot = m.organism_clustering(), m.tile_plot(part)
        try:
            return c.distances(), c.i2, c.j2, c.height, c.merge, c.order, plot.family_order, plot.organism_order, plot.cells()
        finally:
            c.close()
            plot.close()
    same_bytes(*both(pair, call), "clustering and tile plot")


def test_layout(pair):
    layout_held_to_the_statement(pair.m, np.random.default_rng(21).random((pair.m.n, 2)), "merged")

    def call(m, o):
        lay = m.layout(iterations=20, rng=random.Random(8))
        try:
            return lay.positions(), lay.forces(), sorted(lay.state().items())
        finally:
            lay.close()
    got, want = both(pair, call)
    assert np.isfinite(got[0]).all() and got[2] == want[2]
    same_bytes(got[:2], want[:2], "layout")


def test_evolution(pair):
    """tests/test_gpu_evolution.py's setting, cut at 30 of the 64 organisms (60 resamples): chunks of 24 organisms, so
    the resamples of 25 .. 30 run the vote loop on the stream"""
    ep = dict(ratio=0.1, rmin=2, rmax=30, step=1, limit=30)

    def call(m, o):
        rng = random.Random(11)
        return m.evolution(rng, chunk_size=24, tie="libc", batch=16, **ep), rng.getstate()
    (rows, state), (want_rows, want_state) = both(pair, call)
    assert rows.shape[1] == 7 and (rows[:, 0] > 24).any() and (rows[:, 0] <= 24).any() and rows[:, 1:5].sum() > 0
    same_bytes(rows, want_rows, "evolution")
    assert state == want_state


def test_the_masters_are_what_they_were(pair):
    """(the last test that uses the fixture: every consumer above has run on m and on whole)"""
    for x, was, what in zip(pair.masters, pair.before, ("m", "A", "B", "whole")):
        same_with_order(x.arrays(), was, what + " after the consumers")
        assert x.shape()[0] == x.n


def test_the_merged_master_owns_its_memory(gpu_lib):
    """A and B closed, and their memory taken again, before anything reads m"""
    a, b, _, everything = consumer_parts()
    o = consumer_orders()
    da, db = from_orders(a), from_orders(b)
    m = da.merge(db)
    da.close()
    db.close()
    whole, again = from_orders(everything), [from_orders(b), from_orders(a)]
    try:
        same_with_order(m.arrays(), whole.arrays(), "merged, its inputs closed")
        edge_table_equals_statement(m, o, "merged, its inputs closed")
        select = np.arange(m.n) % 2 == 0
        rows, (ptr, idx), eb, counts, _ = m.arrays()
        same_problem(m, (np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :D], ptr, idx, eb, counts), select)

        def call(x):
            t = edge_table_of(x, o)
            try:
                return t.arrays(), t.attvalues(np.arange(D, dtype=np.int32))
            finally:
                t.close()
        same_bytes(call(m), call(whole), "edge_table, the inputs closed")
    finally:
        for x in [m, whole] + again:
            x.close()
