"""The edges' metadata on the device (nemgpu_edge_table_metadata / _metamasks / _metavalues, csrc/nem_edge_meta.hip)
against the numpy statement gexf.edge_metadata_arrays / gexf.metavalues_host -- which tests/test_gexf_metadata_host.py
holds against the reference's own export_to_GEXF(metadata=) -- mask for mask and byte for byte: the recorded fixtures end
to end, both exports; random masters at the smallest shapes where a kernel takes another path (organism counts around a
word of 32 and a wave's group of 64, value counts around a mask word and a wave's 64 words, values of 0, 1 and more than
64 bytes, ids of 1 and 5 digits, an edge of all organisms next to edges of one, self-loops of both kinds); batches; what
is refused, and the master and the table left as they were."""
import ctypes as C

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.gexf import attvalues_host, edge_metadata_arrays, metavalues_host, write_gexf
from tests.gexf_bounds_util import EDGES, attributes, shape_orders
from tests.gexf_metadata_util import METADATA_FIXTURES, metadata_of, read_text
from tests.gexf_util import contigs_orders, path_contigs, same_gexf_text, sizes_of
from tests.orders_util import load, same_master
from tests.projection_util import annotations_of

pytestmark = pytest.mark.gpu

E_ARG = 3


def from_orders(o):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])


def table_of(m, o):
    return m.edge_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]), starts=o["starts"], ends=o["ends"],
                        contig_sizes=o["contig_sizes"])


def held_to_statement(m, t, meta, what, batches=()):
    _, graph, eb, _, _ = m.arrays()
    attr_id, rank, n_values, ptr, blob = meta
    t.set_metadata(*meta)
    want_masks = edge_metadata_arrays(graph, eb, rank, n_values, m.d)
    masks = t.metamasks()
    assert masks.shape == want_masks.shape and np.array_equal(masks, want_masks), "%s: masks differ at edges %s" % (
        what, np.flatnonzero((masks != want_masks).any(axis=1))[:5].tolist())
    want_text, want_ends = metavalues_host(graph, eb, attr_id, rank, n_values, ptr, blob, m.d)
    text, ends = t.metavalues()
    assert np.array_equal(ends, want_ends), what + ": edge ends"
    assert text.tobytes() == want_text.tobytes(), what + ": text"
    assert t.metavalues_size(0, t.n_edges) == len(want_text)
    parts, row = [], 0
    for row0, nrows in batches:
        assert row0 == row
        part, part_ends = t.metavalues(row0, nrows)
        assert np.array_equal(part_ends, want_ends[row0:row0 + nrows] - (want_ends[row0 - 1] if row0 else 0)), (what, row0)
        assert np.array_equal(t.metamasks(row0, nrows), want_masks[row0:row0 + nrows]), (what, row0)
        parts.append(part.tobytes())
        row += nrows
    if batches:
        assert row == t.n_edges and b"".join(parts) == want_text.tobytes(), what + ": batches"
    return want_masks, want_text


@pytest.mark.parametrize("path", METADATA_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
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
            meta = metadata_of(rec)
            write_gexf(str(tmp_path / "full"), rec["labels"], ft, et, ann, metadata=meta)
            write_gexf(str(tmp_path / "light"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, metadata=meta)
            same_gexf_text(read_text(str(tmp_path / "full.gexf")), rec["gexf"], everyone, rec["name"] + " full")
            same_gexf_text(read_text(str(tmp_path / "light.gexf")), rec["gexf_light"], everyone, rec["name"] + " light")
            for budget in (1, 400):                           # a device call per edge; per two or three edges
                assert len(list(et._batches(budget, metadata=True))) > 1
                write_gexf(str(tmp_path / "cut"), rec["labels"], ft, et, ann, metadata=meta, budget=budget)
                assert open(str(tmp_path / "cut.gexf"), "rb").read() == open(str(tmp_path / "full.gexf"), "rb").read()
                write_gexf(str(tmp_path / "cut"), rec["labels"], ft, et, ann, all_node_attributes=False, all_edge_attributes=False, metadata=meta,
                           budget=budget)
                assert open(str(tmp_path / "cut.gexf"), "rb").read() == open(str(tmp_path / "light.gexf"), "rb").read()
        finally:
            ft.close()
            et.close()
        same_master(m.arrays(), before, rec["name"])
    finally:
        m.close()


@pytest.mark.parametrize("d", [1, 33, 65, 129])
def test_the_device_equals_the_statement(gpu_lib, d):
    rng = np.random.default_rng(700 + d)
    o = shape_orders(rng, d)
    m = from_orders(o)
    try:
        before = m.arrays()
        t = table_of(m, o)
        try:
            ne = t.n_edges
            assert ne == EDGES + 5 and (t.src == t.dst).sum() == 2 and int(t.weight.max()) == d and (t.weight == 1).sum() >= 4
            cut = [(0, 1), (1, 3), (4, 1), (5, 64), (69, ne - 70), (ne - 1, 1)]
            for counts, ids in (((1,), (3,)), ((2, 65, 33), (9, 12345, 10)), ((d,), (99999,)), ((33, 1, d), (10000, 0, 7))):
                meta = attributes(rng, d, counts, ids)
                masks, text = held_to_statement(m, t, meta, "d %d values %s" % (d, counts), cut if len(counts) == 3 else ())
                lines = text.tobytes().decode().split("\n")
                assert len(lines) == ne * len(counts) + 1
                if d in counts and d > 64:                    # every organism another value: the widest line holds them all
                    first = sum((nv + 31) // 32 for nv in counts[:counts.index(d)])
                    everyone = masks[:, first:first + (d + 31) // 32]
                    assert max(int(sum(bin(int(w)).count("1") for w in row)) for row in everyone) == d
                    assert max(line.count("|") for line in lines) >= d - 1
            # the organism lines are what they were beside the metadata
            _, graph, eb, counts, _ = m.arrays()
            ids = np.arange(d, dtype=np.int32) + 5
            assert t.attvalues(ids)[0].tobytes() == attvalues_host(graph, eb, counts, ids, d)[0].tobytes()
        finally:
            t.close()
        same_master(m.arrays(), before, "d %d" % d)
    finally:
        m.close()


def test_refusals_leave_the_master_and_the_table_as_they_were(gpu_lib):
    rng = np.random.default_rng(23)
    d = 5
    o = contigs_orders(path_contigs(rng, 12, d) + [(4, [3, 3], -1), (4, [7], 10)], d, np.random.default_rng(1))
    m = from_orders(o)
    try:
        before = m.arrays()
        t = table_of(m, o)
        lib, rows = m.lib, t.n_edges
        with pytest.raises(NemGpuError, match="no metadata"):
            t.metavalues_size(0, rows)
        meta = attributes(rng, d, (3, 5), (8, 12345))
        _, want_text = held_to_statement(m, t, meta, "before")
        size = len(want_text)
        # a buffer one byte too small: the size needed is reported, nothing is written
        buf = np.full(size + 64, 0xAB, np.uint8)
        ends, needed = np.zeros(rows, np.int64), C.c_int64()
        call = lambda row0, nrows, cap: lib.nemgpu_edge_table_metavalues(t._h, m._h, row0, nrows, buf.ctypes.data, cap, C.byref(needed), ends.ctypes.data)
        assert call(0, rows, size - 1) == E_ARG and needed.value == size and (buf == 0xAB).all() and "needs %d" % size in lib.nemgpu_last_error().decode()
        with pytest.raises(NemGpuError) as err:
            t.metavalues(0, rows, out=np.zeros(size - 1, np.uint8))
        assert err.value.needed == size
        assert call(0, rows, size) == 0 and (buf[size:] == 0xAB).all() and buf[:size].tobytes() == want_text.tobytes() and ends[-1] == size
        for row0, nrows in ((-1, 1), (0, 0), (rows, 1), (1, rows)):
            assert call(row0, nrows, size) == E_ARG and "rows outside" in lib.nemgpu_last_error().decode()
        # bad ranks, bad offsets, a bad id, too many values: refused before any launch, the table keeps its metadata
        attr_id, rank, n_values, ptr, blob = meta

        def raw(attr_id=attr_id, rank=rank, n_values=n_values, ptr=ptr):
            a = [np.ascontiguousarray(x, np.int32) for x in (attr_id, rank, n_values)] + [np.ascontiguousarray(ptr, np.int64)]
            rc = lib.nemgpu_edge_table_metadata(t._h, len(a[0]), *(x.ctypes.data for x in a), blob.ctypes.data)
            return rc, lib.nemgpu_last_error().decode()

        high, low, back, off = rank.copy(), rank.copy(), ptr.copy(), ptr.copy()
        high[0, 2], low[1, 4], back[3], off[0] = 3, -1, ptr[4] + 1, 1
        for kw, word in ((dict(rank=high), "rank 3 outside"), (dict(rank=low), "rank -1 outside"), (dict(ptr=back), "ascend"), (dict(ptr=off), "start at 0"),
                         (dict(attr_id=np.asarray([8, -2])), "negative"), (dict(n_values=np.asarray([3, 0])), "values"),
                         (dict(n_values=np.asarray([3, 65537])), "values")):
            rc, why = raw(**kw)
            assert rc == E_ARG and word in why, (rc, why, word)
            with pytest.raises((ValueError, NemGpuError)):
                t.set_metadata(kw.get("attr_id", attr_id), kw.get("rank", rank), kw.get("n_values", n_values), kw.get("ptr", ptr), blob)
        assert lib.nemgpu_edge_table_metadata(t._h, 0, attr_id.ctypes.data, rank.ctypes.data, n_values.ctypes.data, ptr.ctypes.data, blob.ctypes.data) == E_ARG
        text, ends = t.metavalues()
        assert text.tobytes() == want_text.tobytes() and ends[-1] == size
        _, graph, eb, counts, _ = m.arrays()
        ids = np.arange(d, dtype=np.int32) + 95
        assert t.attvalues(ids)[0].tobytes() == attvalues_host(graph, eb, counts, ids, d)[0].tobytes()
        t.close()
        same_master(m.arrays(), before, "after the refusals")
    finally:
        m.close()
