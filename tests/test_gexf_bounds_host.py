"""The numpy statements of the GEXF edge text (gexf.edge_table_arrays through HostEdgeTable, attvalues_host,
edge_metadata_arrays, metavalues_host) against the PLAIN statement of tests/gexf_bounds_util.py, byte for byte and mask
for mask, at every shape at which tests/test_gpu_gexf_bounds.py holds the kernels to them: the recorded fixtures hold
the numpy statements to the reference only at small ids and few values.  Also here: _Edges._metadata_bound lies above an
edge's true bytes, as _Edges._batches relies on."""
import numpy as np
import pytest

from pangenomenem_amd.gexf import HostEdgeTable
from tests import gexf_bounds_util as u
from tests.append_util import build_host
from tests.gexf_util import contigs_orders

ORGANISM_CUT = lambda ne: [(0, 1), (1, 63), (64, 192), (256, ne - 256)]


def table_is_plain(et, plain, what):
    assert et.n_edges == plain.n_edges, what
    assert list(zip(et.src.tolist(), et.dst.tolist())) == plain.edges, what + ": the edges' order"
    assert et.weight.tolist() == [len(mine) for mine in plain.orgs], what + ": weight"
    assert et.org_first_edge.tolist() == plain.first, what + ": org_first_edge"


def text_is_plain(text, ends, lines, what):
    assert np.array_equal(ends, u.ends_of(lines)), what + ": edge ends"
    assert text.tobytes() == b"".join(lines), what + ": text"


def organism_lines_are_plain(kind, d, cut):
    contigs, _, host, et = u.host_of(kind, d)
    plain = u.Plain(contigs, host[4], d)
    table_is_plain(et, plain, "%s d %d" % (kind, d))
    for run, (what, _) in enumerate(u.organism_ids(kind, d)):
        attr_id, text, ends = u.organism_text(kind, d, run)
        lines = plain.organism_lines(attr_id.tolist())
        text_is_plain(text, ends, lines, "%s d %d %s" % (kind, d, what))
        if run == 0:
            for row0, rows in cut:                            # (the statement's own row0 / rows)
                part, part_ends = et.attvalues(attr_id, row0, rows)
                text_is_plain(part, part_ends, lines[row0:row0 + rows], "%s d %d rows %d + %d" % (kind, d, row0, rows))
    return plain, et


@pytest.mark.parametrize("d", [2048, 2049, 4097])
def test_organism_lines_beyond_2048_organisms_and_at_every_id_width(d):
    """attvalues_host and edge_table_arrays at 64, 65 and 129 words of 32 organisms, an edge of organism d - 1 alone and
    one of organism 2048 alone, ids of 1 to 10 digits (every power of ten, its predecessor, 2**31 - 1): what the device's
    k_att_sizes second trip, k_edges_popcount, k_edges_pairs' keys, k_edges_first's grid, k_att_text's 33 and more
    groups of 64 and digits_of / put_digits of 6 to 10 digits are then held to"""
    plain, et = organism_lines_are_plain("organisms", d, ORGANISM_CUT(u.EDGES + (7 if d > 2048 else 6)))
    assert et.n_edges == u.EDGES + (7 if d > 2048 else 6) and int(et.weight.max()) == d
    alone = [mine[0][0] for mine in plain.orgs if len(mine) == 1]
    assert d - 1 in alone and (d <= 2048 or 2048 in alone)
    widths = {len(str(v)) for v in u.ID_CYCLE}
    assert widths == set(range(1, 11)) and len(u.ID_CYCLE) == 20


def full_stage_starts(ends):
    """the full edge's start & 7 in the batches that begin at each of the eight edges in front of it"""
    return {int((ends[u.STAGE_FULL - 1] - (ends[k - 1] if k else 0)) & 7) for k in range(u.STAGE_FULL)}


def test_a_full_stage_of_64_lines_of_53_bytes_at_every_alignment():
    """the statement of k_att_text's fullest reachable LDS stage: 64 organisms of one group of 64 on one edge, each 1 000
    times, ids of 10 digits -- 64 lines of 53 bytes, 3 392 bytes of the stage.  (A line of 59 bytes needs a count of
    10**9 links and cannot be built: the stage's last 384 bytes are not covered by any test.)  The eight edges in front
    have lines of 41 to 48 bytes, so the batches that begin at them put the full edge at all eight alignments: asserted
    here and in the device test, not assumed."""
    plain, et = organism_lines_are_plain("stage", u.STAGE_D, [(0, 1), (1, 8), (9, 1)])
    lines = plain.organism_lines(u.stage_case()[2].tolist())
    assert et.n_edges == 10 and [o for o, _ in plain.orgs[u.STAGE_FULL]] == list(range(64, 128))
    assert {cnt for _, cnt in plain.orgs[u.STAGE_FULL]} == {u.STAGE_LINKS}
    assert len(lines[u.STAGE_FULL]) == 64 * 53 and all(len(line) + 1 == 53 for line in lines[u.STAGE_FULL].split(b"\n")[:-1])
    assert [len(line) for line in lines[:8]] == list(range(41, 49)) and plain.orgs[9] == [(191, 1)]
    assert full_stage_starts(u.organism_text("stage", u.STAGE_D, 0)[2]) == set(range(8))


def metadata_is_plain(kind, d, counts):
    contigs, _, host, et = u.host_of(kind, d)
    plain = u.Plain(contigs, host[4], d)
    meta, masks, text, ends = u.metadata_text(kind, d, counts)
    what = "%s values %s" % (kind, counts)
    want = plain.masks(meta[1])
    assert np.array_equal(masks, u.mask_words(want, counts)), what + ": masks"
    lines = plain.metadata_lines(meta[0].tolist(), meta[1], meta[2].tolist(), meta[3], meta[4])
    text_is_plain(text, ends, lines, what)
    et.set_metadata(*meta)
    assert np.array_equal(et.metamasks(5, 64), masks[5:69])
    part, part_ends = et.metavalues(5, 64)
    text_is_plain(part, part_ends, lines[5:69], what + ": rows 5 + 64")
    # the bound of a batch's budget
    words = sum((nv + 31) // 32 for nv in counts)
    bound = et._metadata_bound()
    true = np.asarray([len(line) for line in lines])
    assert (bound >= true + 4 * words).all(), what + ": _metadata_bound below an edge's bytes at %s" % np.flatnonzero(bound < true + 4 * words)[:5]
    organisms = np.asarray([len(line) for line in plain.organism_lines(list(range(d)))])
    assert u.budget_held(et, lambda row0, rows: int(true[row0:row0 + rows].sum() + organisms[row0:row0 + rows].sum()), what) == words
    return plain, want, lines


@pytest.mark.parametrize("counts", u.SPARSE_SETS, ids=lambda c: "-".join(map(str, c)))
def test_metadata_of_thousands_of_values_on_few_organisms(counts):
    """edge_metadata_arrays and metavalues_host at masks of 64, 65, 129 and 2 048 words (65 536 values, the most the
    device accepts) with the ranks that matter forced: on the edge of all organisms ranks 0, 31, 32, 2047, 2048 and the
    last; an organism alone on an edge at the last rank (k_meta_text: every earlier trip of 64 words empty, no leading
    `|`); two organisms on an edge of their own at rank 5 and two trips further (an empty trip between, exactly one
    `|`); in the sets of three, bits of the first attribute in words >= 64 that the third lacks (k_meta_masks' zeroing
    and copy-out loops, stale LDS from attribute to attribute).  These conditions are asserted on the plain statement;
    _metadata_bound and _batches are held to the true bytes."""
    d = u.SPARSE_D
    plain, masks, lines = metadata_is_plain("sparse", d, counts)
    meta = u.sparse_meta(counts)
    ids, values = meta[0].tolist(), lambda a, v: meta[4][meta[3][sum(counts[:a]) + v]:meta[3][sum(counts[:a]) + v + 1]].tobytes()
    of = {tuple(o for o, _ in mine): e for e, mine in enumerate(plain.orgs)}
    everyone, alone, pair, last = of[tuple(range(d))], of[(0,)], of[u.PAIR], of[(d - 1,)]
    for a, nv in enumerate(counts):
        if nv <= d:
            continue
        for v in u.EVERYONE_RANKS:
            v = nv - 1 if v < 0 else v
            assert v >= nv or masks[everyone][a] >> v & 1, (counts, a, v)
        assert masks[alone][a] == 1 << (nv - 1)
        head = (u.ATT_HEAD % ids[a]).encode()
        assert head + values(a, nv - 1) + u.ATT_TAIL.encode() in lines[alone] and values(a, nv - 1) == b"x"
        far = u.FAR_RANK if u.FAR_RANK < nv else nv - 1
        assert masks[pair][a] == 1 << 5 | 1 << far and (nv <= 4096 or far >> 11 >= 2)     # (a trip is 64 words: 2 048 ranks)
        assert head + values(a, 5) + b"|" + values(a, far) + u.ATT_TAIL.encode() in lines[pair]
    if len(counts) == 3:
        first, third = masks[last][0] >> 2048, masks[last][2] >> 2048
        assert first == 1 << 2 and third == 0 and masks[last][2] == 1 << 7      # (word 64: the first's bit, none of the third's)


@pytest.mark.parametrize("counts", u.DENSE_SETS, ids=lambda c: "-".join(map(str, c)))
def test_metadata_of_4100_organisms_each_another_value(counts):
    """edge_metadata_arrays and metavalues_host at d = 4 100, every organism a value of its own: the edge of all organisms
    has 129 mask words, all ones but the last, 4 100 values and 4 099 separators on one line -- k_meta_masks' 65 groups
    of 64 organisms, meta_line_width's and k_meta_text's third trip"""
    d = u.DENSE_D
    plain, masks, lines = metadata_is_plain("dense", d, counts)
    widest = max(range(plain.n_edges), key=lambda e: len(plain.orgs[e]))
    assert len(plain.orgs[widest]) == d and masks[widest][0] == (1 << d) - 1
    words = u.mask_words(masks, counts)[widest, :129]
    assert (words[:128] == 0xFFFFFFFF).all() and words[128] == 0xF
    meta = u.dense_meta(counts)
    rest = lines[widest].split(b"\n")[0]
    blob = meta[4].tobytes()
    assert int(meta[3][d]) + d - 1 + 39 + len(str(int(meta[0][0]))) == len(rest) + 1 and rest.count(b"|") >= d - 1
    assert b"|".join(blob[meta[3][v]:meta[3][v + 1]] for v in range(d)) in rest


@pytest.mark.parametrize("d", [32, 33, 64, 65])
def test_first_edges_on_the_tiles_boundaries(d):
    """edge_table_arrays' org_first_edge (and attribute_ids, which is made from it) where k_edges_first can go wrong: an
    organism's first edge at 0, 255, 256, 257, 511, 512 and the last of 600, organisms on no edge (first == E), in every
    word of 32 in turn -- words of exactly 32 and of exactly 1 organisms among them"""
    seen = set()
    for what, contigs, edgeless in u.first_edge_cases(d):
        o = contigs_orders(contigs, d, np.random.default_rng(d))
        host = build_host(o)
        assert np.array_equal(host[4], np.arange(len(host[4])))       # (organism 0 walks the path in order: edge p is (p, p + 1))
        plain = u.Plain(contigs, host[4], d)
        et = HostEdgeTable(host[1], host[2], host[3], host[4], o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"],
                           o["contig_sizes"], o["repeated"], d=d)
        table_is_plain(et, plain, what)
        assert plain.edges == [(p, p + 1) for p in range(u.FIRST_EDGES)]
        assert [plain.first[o] for o in edgeless] == [u.FIRST_EDGES] * len(edgeless)
        for org, fams, _ in contigs[1:]:
            assert plain.first[org] == (fams[0] if len(fams) == 2 else u.FIRST_EDGES)
        assert max(plain.first[:32]) < 256 if what.endswith("early") else edgeless
        seen |= set(plain.first)
    assert set(u.FIRST_AT) <= seen
