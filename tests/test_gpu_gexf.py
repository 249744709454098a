"""The edge table and the edges' organism <attvalue> text on the device (nemgpu_edge_table_*, csrc/nem_edges.hip) against
the numpy statement gexf.edge_table_arrays / gexf.attvalues_host -- which tests/test_gexf_host.py holds against the
reference's own export_to_GEXF() -- array for array and byte for byte: the recorded fixtures end to end
(Master.from_annotations -> family_table, edge_table -> write_gexf, both exports), and the smallest shapes where a
kernel takes another path: organism counts around a word of 32 and a wave's group of 64, edge counts around one, a wave
and a block, batches cut inside them, lines whose width changes, an edge of thousands of links next to edges of one, a
family of hundreds of neighbours, self-loops of both kinds, a family of thousands of genes; masters grown, made from
arrays, directed; what is refused, and the master left as it was."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.gexf import attvalues_host, edge_table_arrays, ushape_counts, write_gexf
from tests import master_shapes as ms
from tests.append_util import build_host
from tests.gexf_util import GEXF_FIXTURES, contigs_orders, path_contigs, same_edge_table, same_gexf_text, sizes_of
from tests.orders_util import load, same_master
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

E_ARG = 3


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def table_of(m, o):
    return m.edge_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]), starts=o["starts"], ends=o["ends"],
                        contig_sizes=o["contig_sizes"])


def device_equals_statement(m, o, what, attr_id=None, batches=(), bits_only=False):
    """the table of m and the orders o, its arrays and the text of all its edges, against the statement on m's own arrays;
    batches: (row0, rows) covering the edges, whose texts concatenated must be the one call's"""
    _, graph, eb, counts, order = m.arrays()
    want = edge_table_arrays(graph, eb, counts, order, o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"], o["contig_sizes"],
                             o["repeated"], d=m.d, bits_only=bits_only)
    attr_id = np.arange(m.d, dtype=np.int32) * 3 + 8 if attr_id is None else np.asarray(attr_id, np.int32)
    t = table_of(m, o)
    try:
        same_edge_table(t.arrays(), want, what)
        assert (t.n, t.d, t.n_edges) == (m.n, m.d, len(want["src"]))
        if t.n_edges:
            text, ends = t.attvalues(attr_id)
            want_text, want_ends = attvalues_host(graph, eb, counts, attr_id, m.d)
            assert np.array_equal(ends, want_ends), what + ": edge ends"
            assert text.tobytes() == want_text.tobytes(), what + ": text differs first at byte %d" % int(np.flatnonzero(text != want_text)[:1].sum())
            assert t.attvalues_size(attr_id, 0, t.n_edges) == len(want_text)
            parts, row = [], 0
            for row0, nrows in batches:
                assert row0 == row
                part, part_ends = t.attvalues(attr_id, row0, nrows)
                assert np.array_equal(part_ends, want_ends[row0:row0 + nrows] - (want_ends[row0 - 1] if row0 else 0)), (what, row0)
                parts.append(part.tobytes())
                row += nrows
            if batches:
                assert row == t.n_edges and b"".join(parts) == want_text.tobytes(), what + ": batches"
    finally:
        t.close()
    return want


@pytest.mark.parametrize("path", GEXF_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixtures_end_to_end(gpu_lib, path, tmp_path):
    rec = load(path)
    ann = annotations_of(rec)
    everyone = rec["organisms"] + rec["new_organisms"]
    m = Master.from_annotations(annotations_of(rec, rec["organisms"]), rec["organisms"], rec["circular"], rec["repeated"])
    try:
        if rec["new_organisms"]:
            grown = m.add_annotations(annotations_of(rec, rec["new_organisms"]), rec["new_organisms"],
                                      set(rec["circular"]) | set(rec["update_circular"]), set(rec["repeated"]) | set(rec["update_repeated"]))
            m.close()
            m = grown
        before = m.arrays()
        repeated = set(rec["repeated"]) | set(rec["update_repeated"])
        ft, et = m.family_table(ann, repeated), m.edge_table(ann, repeated, sizes_of(rec))
        try:
            write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann)
            write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False)
            same_gexf_text(open(str(tmp_path / "full.gexf"), newline="", encoding="utf-8").read(), rec["gexf"], everyone, rec["name"] + " full")
            same_gexf_text(open(str(tmp_path / "light.gexf"), newline="", encoding="utf-8").read(), rec["gexf_light"], everyone, rec["name"] + " light")
            write_gexf(str(tmp_path / "cut"), rec["labels"], ft, et, ann, budget=1)       # a device call per edge
            assert open(str(tmp_path / "cut.gexf"), "rb").read() == open(str(tmp_path / "full.gexf"), "rb").read()
            assert ushape_counts(rec["labels"], ft).T.tolist() == rec["ushape"]
        finally:
            ft.close()
            et.close()
        same_master(m.arrays(), before, rec["name"])
    finally:
        m.close()


@pytest.mark.parametrize("d", [1, 31, 32, 33, 63, 64, 65, 129])
def test_organisms_around_words_and_edges_around_waves_and_blocks(gpu_lib, d):
    rng = np.random.default_rng(300 + d)
    for ne in (1, 63, 64, 65, 256, 257):
        o = contigs_orders(path_contigs(rng, ne, d), d, rng)
        m = from_orders(o)
        try:
            cut = [(0, ne)] if ne == 1 else [(0, 1), (1, 30), (31, ne - 31)] if ne < 256 else [(0, 3), (3, 61), (64, 129), (193, ne - 193)]
            want = device_equals_statement(m, o, "edges %d d %d" % (ne, d), batches=cut)
            assert len(want["src"]) == ne
        finally:
            m.close()


def test_a_lines_width_changes_with_the_id_and_the_count(gpu_lib):
    counts = [1, 9, 10, 99, 100, 1]
    contigs = [(org, [0, 1], -1) for org, cnt in enumerate(counts) for _ in range(cnt)]
    contigs += [(0, [1, 2, 3], -1), (3, [3, 2], -1), (5, [2, 2], -1), (4, [3], 7)]
    o = contigs_orders(contigs, 6, np.random.default_rng(5))
    m = from_orders(o)
    try:
        ids = [0, 9, 10, 99, 100, 12345]
        for shift in range(6):
            device_equals_statement(m, o, "widths %d" % shift, attr_id=ids[shift:] + ids[:shift], batches=[(0, 1), (1, 2), (3, 2)])
        t = table_of(m, o)
        text, ends = t.attvalues(ids, 0, 1)
        t.close()
        assert bytes(text).decode() == "".join('          <attvalue for="%d" value="%d" />\n' % (a, b) for a, b in zip(ids, counts)) and ends.tolist() == [len(text)]
    finally:
        m.close()


@pytest.mark.parametrize("size, passes", [("pass", 1), ("pass+1", 2)])
def test_one_gene_past_a_single_pass_of_the_scans_tile_totals(gpu_lib, size, passes):
    """the table scans one item per gene, kept or not: at SCAN_PASS + 1 genes k_scan_partials carries from its first pass
    into a second, in the scans of the links' and of the genes' distinct lengths alike"""
    o = dict(ms.scan_orders(size))
    g, cptr = len(o["genes"]), o["contig_ptr"].astype(np.int64)
    assert ms.scan_passes(g) == passes and g == ms.SCAN_PASS + passes - 1
    assert (np.diff(o["contig_org"]) >= 0).all()
    rng = np.random.default_rng(29)
    length, gap = rng.integers(90, 3000, g), rng.integers(-20, 30, g)
    upto = np.concatenate([[0], np.cumsum(gap + length)])     # (the ENDs if all the genes were one contig, from 0)
    end = upto[1:] - np.repeat(upto[cptr[:-1]], np.diff(cptr))                        # (every contig starts over)
    o["starts"], o["ends"] = (end - length).astype(np.int32), end.astype(np.int32)
    o["contig_sizes"] = np.where(o["contig_circular"] != 0, upto[cptr[1:]] - upto[cptr[:-1]] + 1000, -1).astype(np.int32)
    m = from_orders(o)
    try:
        assert m.d == ms.SCAN_ORGANISMS and int((o["contig_sizes"] >= 0).sum()) > 0
        want = device_equals_statement(m, o, "scan " + size)
        assert int(want["weight"].max()) > 1 and int(want["len_distinct"].max()) > 2
    finally:
        m.close()


@pytest.mark.parametrize("lengths, links", [("equal", 3000), ("distinct", 2999), ("distinct", 3000), ("negative", 3000)])
def test_an_edge_of_thousands_of_links_next_to_edges_of_one(gpu_lib, lengths, links):
    hub = ([0, 1] * 1501)[:links + 1]
    contigs = [(0, [2, 3], -1), (1, hub, -1), (1, [3, 4], -1), (2, [4, 0], -1)] + [(2, [5], -1)] * 3000      # (family 5: 3000 genes, no link)
    o = contigs_orders(contigs, 3, np.random.default_rng(7), lengths=lengths)
    m = from_orders(o)
    try:
        want = device_equals_statement(m, o, "hub %s %d" % (lengths, links))
        at = np.argsort(m.order)                                  # (caller id -> master family)
        e = int(np.flatnonzero((want["src"] == min(at[0], at[1])) & (want["dst"] == max(at[0], at[1])))[0])
        assert want["weight"][e] == 1 and len(want["src"]) == 4
        if lengths == "equal":
            assert (want["len_distinct"] == 1).all() and want["len_mid_lo"][e] == want["len_mid_hi"][e] == want["len_min"][e]
        if lengths == "distinct":
            assert want["len_distinct"][e] == links and (want["len_mid_lo"][e] == want["len_mid_hi"][e]) == (links % 2 == 1)
            assert want["fam_mid_lo"][at[5]] < want["fam_mid_hi"][at[5]]
        if lengths == "negative":
            assert (want["len_max"] < 0).all() and (want["len_sum"] < 0).all()
    finally:
        m.close()


def test_a_family_of_hundreds_of_neighbours_and_self_loops_of_both_kinds(gpu_lib):
    rng = np.random.default_rng(9)
    contigs = [(int(rng.integers(0, 40)), [0, 1 + i] if i % 2 else [1 + i, 0], -1) for i in range(300)]
    contigs += [(3, [301, 301], -1), (4, [302], 50), (5, [0, 0], -1), (6, [0], 9), (7, [303, 304], 11)]
    o = contigs_orders(contigs, 40, rng)
    m = from_orders(o)
    try:
        want = device_equals_statement(m, o, "hub family", batches=[(0, 100), (100, 204)])
        assert len(want["src"]) == 304 and (want["src"] == want["dst"]).sum() == 3
        at = np.argsort(m.order)
        assert ((want["src"] == at[0]) | (want["dst"] == at[0])).sum() == 301
    finally:
        m.close()


def test_masters_grown_from_arrays_and_directed(gpu_lib):
    rng = np.random.default_rng(13)
    ne, d, d0 = 90, 40, 25
    o = contigs_orders(path_contigs(rng, ne, d), d, rng)
    c0 = int(np.searchsorted(o["contig_org"], d0))
    g0 = int(o["contig_ptr"][c0])
    base = dict(o, genes=o["genes"][:g0], contig_ptr=o["contig_ptr"][:c0 + 1], contig_org=o["contig_org"][:c0], contig_circular=o["contig_circular"][:c0], d=d0)
    m0 = from_orders(base)
    grown = m0.add_orders(o["genes"][g0:], o["contig_ptr"][c0:] - g0, o["contig_org"][c0:], o["contig_circular"][c0:], d - d0, repeated=o["repeated"])
    m0.close()
    host = build_host(o)
    assert np.array_equal(host[4], np.arange(ne + 1))         # (organism 0 walks the path in order: caller ids are the master's)
    counted = Master(host[0], host[1][0], host[1][1], host[2], edge_counts=host[3])
    bits = Master(host[0], host[1][0], host[1][1], host[2])
    directed = from_orders(o, directed=True)
    try:
        for m, what in ((grown, "grown"), (counted, "from arrays with counts"), (bits, "from arrays, bits only")):
            before = m.arrays()
            want = device_equals_statement(m, o, what, bits_only=m is bits)
            assert len(want["src"]) == ne
            same_master(m.arrays(), before, what)
        assert len(host[3][1]) > 0                            # (some pair has a count of 2: the bits-only master cannot know)
        before = directed.arrays()
        with pytest.raises(NemGpuError, match="directed"):
            table_of(directed, o)
        same_master(directed.arrays(), before, "directed")
    finally:
        for m in (grown, counted, bits, directed):
            m.close()


def raw_create(m, f, o, **kw):
    lib = m.lib
    h = C.c_void_p()
    a = {k: np.ascontiguousarray(kw.get(k, o[k]), np.int32) for k in ("genes", "starts", "ends", "contig_ptr", "contig_org", "contig_sizes")}
    rc = lib.nemgpu_edge_table_create(C.byref(h), m._h, f, a["genes"].ctypes.data, a["starts"].ctypes.data, a["ends"].ctypes.data, len(a["genes"]),
                                      a["contig_ptr"].ctypes.data, a["contig_org"].ctypes.data, a["contig_sizes"].ctypes.data, len(a["contig_org"]), None)
    assert (rc == 0) == bool(h.value)
    if h.value:
        lib.nemgpu_edge_table_destroy(h)
    return rc, lib.nemgpu_last_error().decode()


def test_refusals_leave_the_master_as_it_was(gpu_lib):
    rng = np.random.default_rng(17)
    ne, d = 12, 5
    contigs = path_contigs(rng, ne, d) + [(4, [3, 3], -1), (4, [7], 10)]
    o = contigs_orders(contigs, d, np.random.default_rng(1))
    m = from_orders(o)
    try:
        before = m.arrays()
        t = table_of(m, o)                                    # (binds the entry points)
        n = m.n
        assert raw_create(m, n, o)[0] == 0
        same_master(m.arrays(), before, "after a good call")
        # one gene's family changed: organism 0's path now runs 4 - 9 - 6, edges the master lacks
        changed = o["genes"].copy()
        changed[5] = 9
        rc, why = raw_create(m, n, o, genes=changed)
        assert rc == E_ARG and "not this master's" in why and "not an edge" in why
        with pytest.raises(NemGpuError, match="not this master's"):
            m.edge_table(orders=(changed, o["contig_ptr"], o["contig_org"]), starts=o["starts"], ends=o["ends"], contig_sizes=o["contig_sizes"])
        same_master(m.arrays(), before, "a family changed")
        # a family the master lacks
        rc, why = raw_create(m, n + 1, o, genes=np.where(np.arange(len(o["genes"])) == 5, n, o["genes"]))
        assert rc == E_ARG and "not in the master" in why
        # one adjacency duplicated: the same edges, the same organisms, one count differs
        twice = contigs_orders(contigs + [(0, [0, 1], -1)], d, np.random.default_rng(1))
        rc, why = raw_create(m, n, twice)
        assert rc == E_ARG and "not this master's" in why and "count" in why
        same_master(m.arrays(), before, "a count differs")
        # an adjacency dropped: the master has an edge bit the orders do not
        rc, why = raw_create(m, n, contigs_orders(contigs[:-2] + [(4, [3], -1), (4, [7], 10)], d, np.random.default_rng(1)))
        assert rc == E_ARG and "not this master's" in why and "no link" in why
        # a length outside int32
        far = o["starts"].copy()
        far[1] = 2 ** 31 - 1
        ends = o["ends"].copy()
        ends[0] = -5
        rc, why = raw_create(m, n, o, starts=far, ends=ends)
        assert rc == E_ARG and "outside int32" in why
        # malformed orders: refused on the host
        for bad, word in ((dict(contig_org=o["contig_org"][::-1].copy()), "non-decreasing"),
                          (dict(contig_ptr=o["contig_ptr"] + np.where(np.arange(len(o["contig_ptr"])) == len(o["contig_ptr"]) - 1, 1, 0)), "contig_ptr"),
                          (dict(contig_org=np.where(np.arange(len(o["contig_org"])) == len(o["contig_org"]) - 1, d, o["contig_org"])), "organism out of range"),
                          (dict(genes=np.where(np.arange(len(o["genes"])) == 1, n, o["genes"])), "family id out of range")):
            rc, why = raw_create(m, n, o, **bad)
            assert rc == E_ARG and word in why, (rc, why)
        same_master(m.arrays(), before, "malformed")
        # a buffer one byte too small: the size needed is reported, nothing is written, the guard behind it neither
        lib, rows = m.lib, t.n_edges
        ids = np.arange(d, dtype=np.int32) + 95
        size = t.attvalues_size(ids, 0, rows)
        buf = np.full(size + 64, 0xAB, np.uint8)
        ends, needed = np.zeros(rows, np.int64), C.c_int64()
        call = lambda row0, nrows, cap, a=ids: lib.nemgpu_edge_table_attvalues(t._h, m._h, a.ctypes.data, row0, nrows, buf.ctypes.data, cap,
                                                                                C.byref(needed), ends.ctypes.data)
        assert call(0, rows, size - 1) == E_ARG and needed.value == size and (buf == 0xAB).all() and "needs %d" % size in lib.nemgpu_last_error().decode()
        with pytest.raises(NemGpuError) as err:
            t.attvalues(ids, 0, rows, out=np.zeros(size - 1, np.uint8))
        assert err.value.needed == size
        assert call(0, rows, size) == 0 and (buf[size:] == 0xAB).all() and buf[size - 1] == ord("\n") and ends[-1] == size
        for row0, nrows in ((-1, 1), (0, 0), (rows, 1), (1, rows)):
            assert call(row0, nrows, size) == E_ARG and "rows outside" in lib.nemgpu_last_error().decode()
        negative = ids.copy()
        negative[2] = -1
        assert call(0, rows, size, negative) == E_ARG and "negative" in lib.nemgpu_last_error().decode()
        t.close()
        same_master(m.arrays(), before, "after the refusals")
    finally:
        m.close()
