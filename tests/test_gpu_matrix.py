"""The family table and the .Rtab cell block on the device (nemgpu_family_table_*, csrc/nem_matrix.hip) against the numpy
statement matrix.family_table_arrays / matrix.rtab_cells_host -- which tests/test_matrix_host.py holds against the
reference's own write_matrix() -- array for array and byte for byte: the recorded fixtures end to end
(Master.from_annotations -> family_table -> write_matrix), and the smallest shapes where each kernel takes another path:
organism counts around a word of 32 and of 64 and a tile of them, family counts around a word and a tile of 256, counts
whose width changes inside an 8-byte store, a family longer than a block next to families of one gene, every kind of
length, batches cut inside a word of families; masters grown, made from arrays, directed; what is refused, and the
master left as it was."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.matrix import family_table_arrays, rtab_cells_host
from tests import master_shapes as ms
from tests.matrix_util import MATRIX_FIXTURES, counts_orders, files_equal_fixture, random_counts, same_table
from tests.orders_util import load, same_master
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

E_ARG = 3


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def table_of(m, o, **kw):
    return m.family_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], kw.get("repeated", o["repeated"]), kw.get("f")), lengths=o["gene_len"])


def device_equals_statement(m, o, what, batches=(), **kw):
    """the table of m and the orders o, its arrays and its whole cell text, against the statement on m's own presence rows;
    batches: (row0, rows) covering the table, whose texts concatenated must be the one call's"""
    rows, order = m.arrays()[0], m.order
    want = family_table_arrays(rows, order, o["genes"], o["gene_len"], o["contig_ptr"], o["contig_org"], kw.get("repeated", o["repeated"]),
                               kw.get("f"), d=m.d)
    t = table_of(m, o, **kw)
    try:
        same_table(t.arrays(), want, what)
        text, ends = t.rtab_cells()
        want_text, want_ends = rtab_cells_host(rows, want["multi_ptr"], want["multi_org"], want["multi_cnt"], d=m.d)
        assert np.array_equal(ends, want_ends), what + ": line ends"
        assert text.tobytes() == want_text.tobytes(), what + ": text differs first at byte %d" % int(np.flatnonzero(text != want_text)[:1].sum())
        assert t.rtab_size(0, t.n) == len(want_text)
        parts, row = [], 0
        for row0, nrows in batches:
            assert row0 == row
            part, part_ends = t.rtab_cells(row0, nrows)
            assert np.array_equal(part_ends, want_ends[row0:row0 + nrows] - (want_ends[row0 - 1] if row0 else 0)), (what, row0)
            parts.append(part.tobytes())
            row += nrows
        if batches:
            assert row == t.n and b"".join(parts) == want_text.tobytes(), what + ": batches"
        for i in (0, t.n - 1):
            assert bytes(want_text[(want_ends[i - 1] if i else 0):want_ends[i]]).decode() == "\t".join(map(str, t.copies(i).tolist())) + "\n"
    finally:
        t.close()
    return want


@pytest.mark.parametrize("path", MATRIX_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixtures_end_to_end(gpu_lib, path, tmp_path):
    rec = load(path)
    ann = annotations_of(rec)
    m = Master.from_annotations(annotations_of(rec, rec["organisms"]), rec["organisms"], rec["circular"], rec["repeated"])
    try:
        if rec["new_organisms"]:
            grown = m.add_annotations(annotations_of(rec, rec["new_organisms"]), rec["new_organisms"],
                                      set(rec["circular"]) | set(rec["update_circular"]), set(rec["repeated"]) | set(rec["update_repeated"]))
            m.close()
            m = grown
        before = m.arrays()
        t = m.family_table(ann, set(rec["repeated"]) | set(rec["update_repeated"]))
        try:
            files_equal_fixture(t, rec, ann, tmp_path)
        finally:
            t.close()
        same_master(m.arrays(), before, rec["name"])
    finally:
        m.close()


@pytest.mark.parametrize("d", [1, 31, 32, 33, 63, 64, 65, 129])
def test_organisms_and_families_around_words_and_tiles(gpu_lib, d):
    rng = np.random.default_rng(100 + d)
    for n in (1, 63, 64, 65, 257):
        o = counts_orders(random_counts(rng, n, d), rng)
        m = from_orders(o)
        try:
            cut = [(0, 1), (1, 40), (41, 100), (141, n - 141)] if n == 257 else [(0, n)] if n < 63 else [(0, 1), (1, 30), (31, n - 31)]
            device_equals_statement(m, o, "n %d d %d" % (n, d), batches=cut)
        finally:
            m.close()


def test_width_changes_inside_a_wide_store_and_across_a_tile_of_organisms(gpu_lib):
    rng = np.random.default_rng(7)
    n, d = 70, 300
    counts = random_counts(rng, n, d, p_multi=0.0)
    for i, o0 in ((3, 0), (4, 1), (5, 7), (40, 252), (41, 254), (69, 295)):       # (a run inside a word, one over a tile's edge, one at the end)
        counts[i, o0:o0 + 5] = [9, 10, 99, 100, 1000]
    counts[6, :] = 2                                                              # every cell of a line is wide
    counts[7, ::2] = 11
    o = counts_orders(counts, rng)
    m = from_orders(o)
    try:
        want = device_equals_statement(m, o, "widths", batches=[(0, 5), (5, 1), (6, 35), (41, 29)])
        assert int(want["multi_cnt"].max()) == 1000 and len(want["multi_cnt"]) >= 30 + d + d // 2
    finally:
        m.close()


@pytest.mark.parametrize("lengths", ["equal", "distinct", "negative", "random"])
def test_a_family_longer_than_a_block_next_to_families_of_one_gene(gpu_lib, lengths):
    rng = np.random.default_rng(11)
    n, d = 12, 5
    counts = np.zeros((n, d), np.int64)
    counts[np.arange(n), np.arange(n) % d] = 1                                    # one gene each ...
    counts[5, :] = [0, 0, 3000, 0, 0]                                             # ... but a hub: its genes span many blocks
    counts[6, :] = [1, 700, 0, 1, 2]
    o = counts_orders(counts, rng, lengths=lengths, contigs=3)
    m = from_orders(o)
    try:
        want = device_equals_statement(m, o, "hub " + lengths)
        at = np.argsort(m.order)                                  # (caller id -> master family)
        assert want["nb_genes"][at[5]] == 3000 and want["nb_org"][at[5]] == 1 and (want["nb_genes"][at[:5]] == 1).all()
        if lengths == "equal":
            assert (want["len_distinct"] == 1).all() and (want["len_min"] == want["len_max"]).all()
        if lengths == "distinct":
            assert (want["len_distinct"] == want["nb_genes"]).all()
        if lengths == "negative":
            assert (want["len_max"] < 0).all() and (want["len_sum"] < 0).all()
    finally:
        m.close()


@pytest.mark.parametrize("size, passes", [("pass", 1), ("pass+1", 2)])
def test_one_gene_past_a_single_pass_of_the_scans_tile_totals(gpu_lib, size, passes):
    """the table scans one item per gene, kept or not: at SCAN_PASS + 1 genes k_scan_partials carries from its first pass
    into a second, in the int scans and in the int64 scan of the distinct lengths alike"""
    o = dict(ms.scan_orders(size))
    g = len(o["genes"])
    assert ms.scan_passes(g) == passes and g == ms.SCAN_PASS + passes - 1
    o["gene_len"] = np.random.default_rng(23).integers(-50, 4000, g).astype(np.int32)
    m = from_orders(o)
    try:
        assert m.d == ms.SCAN_ORGANISMS
        want = device_equals_statement(m, o, "scan " + size, batches=[(0, 1000), (1000, m.n - 1000)])
        assert int(want["len_distinct"].max()) > 1 and len(want["multi_cnt"]) > 0
    finally:
        m.close()


def test_masters_grown_from_arrays_and_directed(gpu_lib):
    rng = np.random.default_rng(13)
    n, d, d0 = 90, 40, 25
    counts = random_counts(rng, n, d)
    o = counts_orders(counts, rng)
    # grown: the first d0 organisms, then the others appended (their contigs are the orders' tail: walked in column order)
    c0 = int(np.searchsorted(o["contig_org"], d0))
    g0 = int(o["contig_ptr"][c0])
    base = dict(o, genes=o["genes"][:g0], contig_ptr=o["contig_ptr"][:c0 + 1], contig_org=o["contig_org"][:c0], contig_circular=o["contig_circular"][:c0], d=d0)
    m0 = from_orders(base)
    grown = m0.add_orders(o["genes"][g0:], o["contig_ptr"][c0:] - g0, o["contig_org"][c0:], o["contig_circular"][c0:], d - d0, repeated=o["repeated"])
    m0.close()
    directed = from_orders(o, directed=True)
    arrays = Master((counts > 0).astype(np.uint8), np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, (d + 31) // 32), np.uint32))
    try:
        for m, what in ((grown, "grown"), (directed, "directed"), (arrays, "from arrays")):
            before = m.arrays()
            want = device_equals_statement(m, o, what)
            same_master(m.arrays(), before, what)
        assert np.array_equal(arrays.order, np.arange(n)) and not np.array_equal(grown.order, np.arange(n))
    finally:
        for m in (grown, directed, arrays):
            m.close()


def raw_create(m, f, genes, gene_len, cptr, corg, rep=None):
    lib = m.lib
    h = C.c_void_p()
    genes, gene_len, cptr, corg = (np.ascontiguousarray(a, np.int32) for a in (genes, gene_len, cptr, corg))
    rc = lib.nemgpu_family_table_create(C.byref(h), m._h, f, genes.ctypes.data, gene_len.ctypes.data, len(genes), cptr.ctypes.data, corg.ctypes.data,
                                        len(corg), rep.ctypes.data if rep is not None else None)
    assert (rc == 0) == bool(h.value)
    if h.value:
        lib.nemgpu_family_table_destroy(h)
    return rc, lib.nemgpu_last_error().decode()


def test_refusals_leave_the_master_as_it_was(gpu_lib):
    rng = np.random.default_rng(17)
    n, d = 20, 9
    counts = random_counts(rng, n, d)
    counts[2, 3], counts[4, 3], counts[4, 0] = 1, 0, 1
    o = counts_orders(counts, rng)
    m = from_orders(o)
    try:
        before = m.arrays()
        t = table_of(m, o)                                    # (binds the entry points)
        good = (o["genes"], o["gene_len"], o["contig_ptr"], o["contig_org"])
        assert raw_create(m, n, *good)[0] == 0
        same_master(m.arrays(), before, "after a good call")
        # one gene's family changed: family 2's only gene in organism 3 becomes family 4's, absent there
        p = int(np.flatnonzero((o["genes"] == 2) & (np.repeat(o["contig_org"], np.diff(o["contig_ptr"])) == 3))[0])
        changed = o["genes"].copy()
        changed[p] = 4
        rc, why = raw_create(m, n, changed, *good[1:])
        assert rc == E_ARG and "not this master's" in why and "presence bit" in why
        with pytest.raises(NemGpuError, match="not this master's"):
            m.family_table(orders=(changed, o["contig_ptr"], o["contig_org"]), lengths=o["gene_len"])
        # the same gene dropped into a repeated family: the master has a bit the orders do not
        dropped, rep = changed.copy(), np.zeros(n + 1, np.uint8)
        dropped[p], rep[n] = n, 1
        rc, why = raw_create(m, n + 1, dropped, *good[1:], rep=rep)
        assert rc == E_ARG and "no kept gene" in why
        # a family the master lacks
        rc, why = raw_create(m, n + 1, dropped, *good[1:])
        assert rc == E_ARG and "not in the master" in why
        # malformed orders: refused on the host by the build's rules
        for bad, word in ((dict(cptr=o["contig_ptr"] + np.where(np.arange(len(o["contig_ptr"])) == len(o["contig_ptr"]) - 1, 1, 0)), "contig_ptr"),
                          (dict(corg=np.where(np.arange(len(o["contig_org"])) == 0, d, o["contig_org"])), "organism out of range"),
                          (dict(genes=np.where(np.arange(len(o["genes"])) == 1, n, o["genes"])), "family id out of range")):
            args = dict(genes=good[0], gene_len=good[1], cptr=good[2], corg=good[3])
            args.update(bad)
            rc, why = raw_create(m, n, **args)
            assert rc == E_ARG and word in why, (rc, why)
            same_master(m.arrays(), before, word)
        # a buffer one byte too small: the size needed is reported, nothing is written, the guard behind it neither
        size = t.rtab_size(0, n)
        buf = np.full(size + 64, 0xAB, np.uint8)
        ends, needed = np.zeros(n, np.int64), C.c_int64()
        rc = m.lib.nemgpu_family_table_rtab(t._h, m._h, 0, n, buf.ctypes.data, size - 1, C.byref(needed), ends.ctypes.data)
        assert rc == E_ARG and needed.value == size and (buf == 0xAB).all() and "needs %d" % size in m.lib.nemgpu_last_error().decode()
        with pytest.raises(NemGpuError) as err:
            t.rtab_cells(0, n, out=np.zeros(size - 1, np.uint8))
        assert err.value.needed == size
        rc = m.lib.nemgpu_family_table_rtab(t._h, m._h, 0, n, buf.ctypes.data, size, C.byref(needed), ends.ctypes.data)
        assert rc == 0 and (buf[size:] == 0xAB).all() and buf[size - 1] == ord("\n") and ends[-1] == size
        for row0, rows in ((-1, 1), (0, 0), (n, 1), (1, n)):
            assert m.lib.nemgpu_family_table_rtab(t._h, m._h, row0, rows, buf.ctypes.data, size, C.byref(needed), ends.ctypes.data) == E_ARG
        t.close()
        same_master(m.arrays(), before, "after the refusals")
    finally:
        m.close()
