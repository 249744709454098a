"""What tests/test_gexf_host.py and tests/test_gpu_gexf.py share: the recorded exports of tests/golden/gexf/ (made by
tests/golden/make_gexf.py from the reference's own export_to_GEXF() and ushaped_plot), the comparison of a written file
with a recorded one, a fixture's host tables, and flat orders with gene positions for synthetic shapes."""
import glob
import os
import re

import numpy as np

from pangenomenem_amd.gexf import EDGE_FIELDS, HostEdgeTable, gexf_orders
from pangenomenem_amd.matrix import HostFamilyTable, table_orders
from tests.matrix_util import repeated_by_organism
from tests.projection_util import annotations_of, fixture_master_host

GEXF_FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gexf", "*.json")))
ATTRIBUTE = re.compile(r'^      <attribute id="(\d+)" title="(.*)" type="(\w+)" />$')
ATTVALUE = re.compile(r'^          <attvalue for="(\d+)" value="(.*)" />$')


def sizes_of(rec):
    return dict(rec["circular"], **rec["update_circular"])


def same_gexf_text(got, want, organisms, what):
    """byte for byte, except the two lines of <meta> (the date, the creator) and, inside <nodes>, the values the reference
    joins from a set in hash order -- name, product and an organism's genes -- which are compared as sets"""
    got_lines, want_lines = got.split("\n"), want.split("\n")
    assert len(got_lines) == len(want_lines), "%s: %d lines, %d wanted" % (what, len(got_lines), len(want_lines))
    joined, section = set(), None
    for k, (a, b) in enumerate(zip(got_lines, want_lines)):
        if b.startswith("  <meta ") or b.startswith("    <creator>"):
            assert a.lstrip()[:6] == b.lstrip()[:6], (what, k, a, b)                  # (the same element)
            continue
        if b.startswith("    <attributes ") or b in ("    <nodes>", "    <edges>"):
            section = b
        found = ATTRIBUTE.match(b)
        if found and 'class="node"' in section and found.group(2) in set(organisms) | {"name", "product"}:
            joined.add(found.group(1))
        value = ATTVALUE.match(b)
        if value and section == "    <nodes>" and value.group(1) in joined:
            mine = ATTVALUE.match(a)
            assert mine and mine.group(1) == value.group(1), (what, k, a, b)
            x, y = mine.group(2).split("|"), value.group(2).split("|")
            assert len(x) == len(y) and set(x) == set(y), (what, k, a, b)
        else:
            assert a == b, "%s: line %d: %r, wanted %r" % (what, k, a, b)


def host_tables(rec):
    """a fixture's family table, edge table (both from the numpy statements on the numpy master) and annotations"""
    m, ids, names = fixture_master_host(rec)
    everyone = rec["organisms"] + rec["new_organisms"]
    ann = annotations_of(rec)
    by_org = repeated_by_organism(rec)
    o = table_orders(ann, everyone, ids, by_org)
    ft = HostFamilyTable(m[0], m[4], o["genes"], o["lengths"], o["contig_ptr"], o["contig_org"], o["repeated"], names=names,
                         organism_names=everyone, repeated_names=by_org)
    o = gexf_orders(ann, everyone, ids, by_org, sizes_of(rec))
    et = HostEdgeTable(m[1], m[2], m[3], m[4], o["genes"], o["starts"], o["ends"], o["contig_ptr"], o["contig_org"], o["contig_sizes"],
                       o["repeated"], d=len(everyone))
    return ft, et, ann


def same_edge_table(got, want, what=""):
    for name in EDGE_FIELDS:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape, "%s: %s %s %s / %s %s" % (what, name, a.dtype, a.shape, b.dtype, b.shape)
        assert np.array_equal(a, b), "%s: %s differs at %s" % (what, name, np.flatnonzero(a != b)[:5].tolist())


def contigs_orders(contigs, d, rng=None, lengths="random", n=None):
    """flat orders of contigs given as (organism, [family, ...], circular size or -1), sorted by organism; every gene
    gets a START and an END: lengths "random" (genes of a few sizes, gaps of a few sizes, some overlapping), "equal"
    (every gap the same), "distinct" (every gap of the orders another one), "negative" (every gene overlaps the one
    before).  Returns a dict: genes, contig_ptr, contig_org, contig_circular, contig_sizes, starts, ends, d, repeated."""
    rng = np.random.default_rng(0) if rng is None else rng
    contigs = sorted(contigs, key=lambda c: c[0])
    genes, cptr, corg, sizes, starts, ends = [], [0], [], [], [], []
    k = 0
    for org, fams, size in contigs:
        at = 0
        for fam in fams:
            k += 1
            gap = dict(random=lambda: int(rng.integers(-2, 4)) * 25, equal=lambda: 40, distinct=lambda: k, negative=lambda: -1 - k % 7)[lengths]()
            glen = dict(random=lambda: int(rng.integers(1, 5)) * 150, equal=lambda: 300, distinct=lambda: 3 * k, negative=lambda: 200 + k % 3)[lengths]()
            starts.append(at + gap)
            ends.append(at + gap + glen)
            at = ends[-1]
            genes.append(fam)
        cptr.append(len(genes))
        corg.append(org)
        sizes.append(size if size < 0 else at + size)          # (a circular contig is `size` longer than its last gene's end)
    n = (max(genes) + 1 if genes else 1) if n is None else n
    return dict(genes=np.asarray(genes, np.int32), contig_ptr=np.asarray(cptr, np.int32), contig_org=np.asarray(corg, np.int32),
                contig_circular=(np.asarray(sizes) >= 0).astype(np.uint8), contig_sizes=np.asarray(sizes, np.int32),
                starts=np.asarray(starts, np.int32), ends=np.asarray(ends, np.int32), d=d, repeated=np.zeros(n, np.uint8))


def path_contigs(rng, ne, d, p_twice=0.2):
    """contigs whose graph is the path 0 - 1 - ... - ne (exactly ne edges): organism 0 walks the whole path, every other
    one a random stretch of it in either direction, now and then its first link once more (a count of 2)"""
    out = [(0, list(range(ne + 1)), -1)]
    for o in range(1, d):
        a = int(rng.integers(0, ne))
        b = int(rng.integers(a + 1, ne + 1))
        stretch = list(range(a, b + 1))
        out.append((o, stretch if rng.random() < 0.5 else stretch[::-1], -1))
        if rng.random() < p_twice:
            out.append((o, stretch[:2], -1))
    return out
