"""The GEXF edge text on the device (csrc/nem_edges.hip, csrc/nem_edge_meta.hip) held to the bounds its kernels state,
against the numpy statements (gexf.edge_table_arrays, attvalues_host, edge_metadata_arrays, metavalues_host) byte for
byte and mask for mask -- which tests/test_gexf_bounds_host.py holds, at these very shapes, to the plain statement of
tests/gexf_bounds_util.py: more than 2 048 organisms (more than one trip of 64 words), ids of 1 to 10 digits, the
fullest LDS stage that can be built, attributes of up to 65 536 values (masks of up to 2 048 words), first edges on the
256-edge tile's boundary, the largest metadata that is accepted and the first that is refused."""
import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.gexf import HostEdgeTable
from tests import gexf_bounds_util as u
from tests.append_util import build_host
from tests.gexf_util import contigs_orders, path_contigs, same_edge_table

pytestmark = pytest.mark.gpu

E_ARG = 3


def from_orders(o):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"])


def table_of(m, o):
    return m.edge_table(orders=(o["genes"], o["contig_ptr"], o["contig_org"], o["repeated"]), starts=o["starts"], ends=o["ends"],
                        contig_sizes=o["contig_sizes"])


def text_equals(got, want, what):
    (text, ends), (want_text, want_ends) = got, want
    assert np.array_equal(ends, want_ends), what + ": edge ends"
    assert text.tobytes() == want_text.tobytes(), what + ": text differs first at byte %d" % int(
        np.flatnonzero(text[:len(want_text)] != want_text[:len(text)])[:1].sum())


def part_of(text, ends, row0, rows):
    """rows row0 .. row0 + rows - 1 of a whole text, as a batch call gives them"""
    base = int(ends[row0 - 1]) if row0 else 0
    return text[base:int(ends[row0 + rows - 1])], ends[row0:row0 + rows] - base


def organism_lines_equal(t, kind, d, cut, what):
    for run, (name, _) in enumerate(u.organism_ids(kind, d)):
        attr_id, want_text, want_ends = u.organism_text(kind, d, run)
        text_equals(t.attvalues(attr_id), (want_text, want_ends), "%s %s" % (what, name))
        assert t.attvalues_size(attr_id, 0, t.n_edges) == len(want_text)
        if run == 0:
            row = 0
            for row0, rows in cut:
                assert row0 == row
                text_equals(t.attvalues(attr_id, row0, rows), part_of(want_text, want_ends, row0, rows), "%s rows %d + %d" % (what, row0, rows))
                row += rows
            assert not cut or row == t.n_edges


def table_at(kind, d):
    """the shape's master and table on the device, both held to the numpy ones the reference texts were made from"""
    _, o, host, het = u.host_of(kind, d)
    m = from_orders(o)
    try:
        u.same_master_arrays(m, host, "%s d %d" % (kind, d))
        t = table_of(m, o)
    except BaseException:
        m.close()
        raise
    try:
        same_edge_table(t.arrays(), het.arrays(), "%s d %d" % (kind, d))
        assert (t.n, t.d, t.n_edges) == (m.n, d, het.n_edges)
    except BaseException:
        t.close()
        m.close()
        raise
    return m, t


@pytest.mark.parametrize("d", [2048, 2049, 4097])
def test_organism_lines_beyond_2048_organisms_and_at_every_id_width(gpu_lib, d):
    """wf = 64, 65, 129 words of 32 organisms: one trip of k_att_sizes' `for (w = lane; w < wf; w += 64)`, one lane in
    its second trip, a third trip -- a wrong stride or bound there moves every later edge's end; the edge table itself
    at that size (k_edges_popcount's words, k_edges_pairs' bd-bit organism keys, k_edges_first's grid of wf blocks) and
    k_att_text's 33 and more groups of 64 organisms, with an edge of the last organism alone and one of organism 2048
    alone (every earlier group skipped by the ballot).  Ids: all 2**31 - 1, then every digit count, every power of ten
    and its predecessor, shifted by one per run so the widths change inside the 8-byte words: digits_of's terms
    >= 100000 .. >= 1000000000 and put_digits' 6 to 10 digits each decide bytes that are compared."""
    m, t = table_at("organisms", d)
    try:
        ne = t.n_edges
        organism_lines_equal(t, "organisms", d, [(0, 1), (1, 63), (64, 192), (256, ne - 256)], "d %d" % d)
    finally:
        t.close()
        m.close()


def test_a_full_stage_of_64_lines_of_53_bytes_at_every_alignment(gpu_lib):
    """k_att_text's LDS stage (kStageWords: 64 lines of 59 bytes and the misalignment): one group of 64 organisms all on
    one edge, 1 000 links each, ids of 10 digits: 64 lines of 53 bytes fill 3 392 bytes of the stage, at each of the eight
    alignments of the edge's start (the eight edges in front have lines of 41 to 48 bytes; a batch begins at each; that
    all eight values of start & 7 occur is asserted).  A wrong stage offset, a wrong scan of the widths or a wrong
    partial first or last word shows in the bytes; the edge behind (organism 191 alone) must be intact although the
    stage is overwritten for it.  NOT covered: a line of 59 bytes needs a count of 10**9 links, which no test can
    build, so the stage's last 384 bytes are never written by any test."""
    d = u.STAGE_D
    m, t = table_at("stage", d)
    try:
        attr_id, want_text, want_ends = u.organism_text("stage", d, 0)
        organism_lines_equal(t, "stage", d, [(0, 1), (1, 8), (9, 1)], "stage")
        starts = set()
        for k in range(u.STAGE_FULL):
            text, ends = t.attvalues(attr_id, k, t.n_edges - k)
            text_equals((text, ends), part_of(want_text, want_ends, k, t.n_edges - k), "stage from edge %d" % k)
            starts.add(int(ends[u.STAGE_FULL - k - 1]) & 7)
            assert int(ends[u.STAGE_FULL - k]) - int(ends[u.STAGE_FULL - k - 1]) == 64 * 53
            assert text[int(ends[-2]):].tobytes() == (u.ATT % (attr_id[191], "1")).encode()
        assert starts == set(range(8))
    finally:
        t.close()
        m.close()


def metadata_equals(m, t, kind, d, counts, attr_id, batches):
    """set_metadata, then the masks and the text against the statements, whole and in batches; _metadata_bound and
    _batches against the device's own sizes.  Returns (meta, want_masks, want_text, want_ends)."""
    meta, want_masks, want_text, want_ends = u.metadata_text(kind, d, counts)
    what = "%s values %s" % (kind, counts)
    t.set_metadata(*meta)
    masks = t.metamasks()
    assert masks.shape == want_masks.shape and np.array_equal(masks, want_masks), "%s: masks differ at edges %s" % (
        what, np.flatnonzero((masks != want_masks).any(axis=1))[:5].tolist())
    text, ends = t.metavalues()
    text_equals((text, ends), (want_text, want_ends), what)
    assert t.metavalues_size(0, t.n_edges) == len(want_text)
    row = 0
    for row0, rows in batches:
        assert row0 == row
        text_equals(t.metavalues(row0, rows), part_of(want_text, want_ends, row0, rows), "%s rows %d + %d" % (what, row0, rows))
        assert np.array_equal(t.metamasks(row0, rows), want_masks[row0:row0 + rows]), (what, row0)
        row += rows
    assert row == t.n_edges
    words = sum((nv + 31) // 32 for nv in counts)
    true = np.diff(np.concatenate([[0], ends]))
    bound = t._metadata_bound()
    assert (bound >= true + 4 * words).all(), what + ": _metadata_bound below an edge's bytes at %s" % np.flatnonzero(bound < true + 4 * words)[:5]
    assert u.budget_held(t, lambda row0, rows: t.metavalues_size(row0, rows) + t.attvalues_size(attr_id, row0, rows), what) == words
    return meta, want_masks, want_text, want_ends


@pytest.mark.parametrize("counts", u.SPARSE_SETS, ids=lambda c: "-".join(map(str, c)))
def test_metadata_of_thousands_of_values_on_few_organisms(gpu_lib, counts):
    """masks of 64, 65, 129 and 2 048 words on d = 129 organisms; 65 536 values is the most nemgpu_edge_table_metadata
    accepts (65 537 is refused in tests/test_gpu_gexf_metadata.py) and is accepted and run here.  Would catch:
    k_meta_masks' zeroing loop and copy-out loop `k = lane; k < nw; k += 64` beyond their first trip -- in the sets of
    three the first attribute leaves bits in words >= 64 of the wave's LDS that the third must not have (zeroing only
    the first 64 words between attributes fails here); meta_line_width's same loop (a wrong width moves every later
    end); k_meta_text's `w0 += 64` loop with `first` carried across trips -- an organism alone at the last rank (every
    earlier trip empty: no leading `|`), two organisms at rank 5 and two trips further (the trip between skipped by the
    ballot: exactly one `|`; resetting `first` per trip fails here), ranks 0, 31, 32, 2047, 2048 and the last on the
    edge of all organisms; head_byte at 1, 5 and 10 digits (head = 44 lanes).  The conditions themselves are asserted on
    the plain statement in tests/test_gexf_bounds_host.py.  gexf._Edges._metadata_bound, which claims to lie above the
    bytes a metavalues call takes and which _batches relies on, is held to the device's own sizes (metavalues_size,
    attvalues_size) for budgets of 1 byte, 64 KiB and 4 MiB.  Afterwards the organism lines are what they were."""
    d = u.SPARSE_D
    m, t = table_at("sparse", d)
    try:
        ids = u.organism_text("sparse", d, 0)[0]
        meta, want_masks, _, _ = metadata_equals(m, t, "sparse", d, counts, ids, u.SPARSE_CUT)
        if len(counts) == 3:                                  # (the stale-LDS condition, on the statement's masks)
            first, third = want_masks[:, 64:(counts[0] + 31) // 32], want_masks[:, -((counts[2] + 31) // 32):][:, 64:]
            assert ((first[:, :third.shape[1]] & ~third) != 0).any()
        organism_lines_equal(t, "sparse", d, (), "beside the metadata")
    finally:
        t.close()
        m.close()


@pytest.mark.parametrize("counts", u.DENSE_SETS, ids=lambda c: "-".join(map(str, c)))
def test_metadata_of_4100_organisms_each_another_value(gpu_lib, counts):
    """d = 4 100, every organism a value of its own: k_meta_masks reads the edge's bit row in 65 groups of 64 organisms
    and ORs 4 100 bits into 129 words (all ones but the last); meta_line_width and k_meta_text walk three trips of 64
    words with no empty word, 4 100 values and 4 099 separators on the widest line (asserted on the statement's masks
    and text)"""
    d = u.DENSE_D
    m, t = table_at("dense", d)
    try:
        ne = t.n_edges
        ids = u.organism_text("dense", d, 0)[0]
        meta, want_masks, want_text, want_ends = metadata_equals(m, t, "dense", d, counts, ids, [(0, 1), (1, 63), (64, 192), (256, ne - 256)])
        set_bits = np.unpackbits(np.ascontiguousarray(want_masks[:, :129]).view(np.uint8), axis=1).sum(axis=1)
        widest = int(set_bits.argmax())
        assert int(set_bits[widest]) == d and (want_masks[widest, :128] == 0xFFFFFFFF).all() and want_masks[widest, 128] == 0xF
        line = part_of(want_text, want_ends, widest, 1)[0].tobytes().split(b"\n")[0]
        inside = meta[4][:int(meta[3][d])].tobytes().count(b"|")          # (a value may hold a | of its own)
        assert line.count(b"|") - inside == d - 1
    finally:
        t.close()
        m.close()


@pytest.mark.parametrize("d", [32, 33, 64, 65])
def test_first_edges_on_the_tiles_boundaries(gpu_lib, d):
    """k_edges_first: an organism's first edge exactly at 0, 255, 256, 257, 511, 512 and the last of 600 edges (a wrong
    tile base, a wrong exclusive OR-scan across the waves or a wrong carry shows at the 256-edge boundary); organisms on
    no edge (first == E, the word never full, the walk runs to the end); a word whose 32 organisms are all met in the
    first tile (the `carry != full` early stop); last words of exactly 32 and of exactly 1 organisms (word_mask), every
    word in turn.  org_first_edge against the plain statement's `first`, attribute_ids against the HostEdgeTable's."""
    seen = set()
    for what, contigs, edgeless in u.first_edge_cases(d):
        o = contigs_orders(contigs, d, np.random.default_rng(d))
        host = build_host(o)
        het = HostEdgeTable(host[1], host[2], host[3], host[4], o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"],
                            o["contig_sizes"], o["repeated"], d=d)
        m = from_orders(o)
        try:
            assert np.array_equal(m.order, np.arange(m.n))    # (organism 0 walks the path in order: edge p is (p, p + 1))
            plain = u.Plain(contigs, m.order, d)
            t = table_of(m, o)
            try:
                assert t.n_edges == u.FIRST_EDGES and t.org_first_edge.tolist() == plain.first, what
                assert [plain.first[k] for k in edgeless] == [u.FIRST_EDGES] * len(edgeless)
                same_edge_table(t.arrays(), het.arrays(), what)
                for args in ((0, True, 0), (7, True, 2), (7, False, 2)):
                    got, want = t.attribute_ids(*args), het.attribute_ids(*args)
                    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, args)
                seen |= set(t.org_first_edge.tolist())
            finally:
                t.close()
        finally:
            m.close()
    assert set(u.FIRST_AT) | {u.FIRST_EDGES} <= seen


def test_the_values_bytes_and_number_past_2_to_the_30_are_refused(gpu_lib):
    """nemgpu_edge_table_metadata's kMetaTextMax: value_ptr[-1] + values == 2**30 + 1 is refused with E_ARG and a message
    that names the limit, before anything is read or uploaded (value_text has the real size, so a missing check reads
    nothing it may not), and the table keeps the metadata it had.  NOT covered: attributes whose value COUNTS sum past
    2**30 (the refusal "too many values") cannot be built cheaply."""
    rng = np.random.default_rng(31)
    d = 5
    o = contigs_orders(path_contigs(rng, 12, d) + [(4, [3, 3], -1), (4, [7], 10)], d, np.random.default_rng(1))
    m = from_orders(o)
    try:
        t = table_of(m, o)
        try:
            t.set_metadata(*u.attributes(rng, d, (3, 5), (8, 12345)))
            before = t.metavalues()
            limit = 2 ** 30
            attr_id, rank, n_values = np.asarray([4], np.int32), np.zeros((1, d), np.int32), np.asarray([1], np.int32)
            ptr, blob = np.asarray([0, limit], np.int64), np.zeros(limit, np.uint8)
            assert int(ptr[-1]) + int(n_values.sum()) == limit + 1
            rc = m.lib.nemgpu_edge_table_metadata(t._h, 1, attr_id.ctypes.data, rank.ctypes.data, n_values.ctypes.data, ptr.ctypes.data, blob.ctypes.data)
            assert rc == E_ARG and str(limit) in m.lib.nemgpu_last_error().decode()
            with pytest.raises(NemGpuError, match=str(limit)):
                t.set_metadata(attr_id, rank, n_values, ptr, blob)
            text_equals(t.metavalues(), before, "after the refusal")
        finally:
            t.close()
    finally:
        m.close()
