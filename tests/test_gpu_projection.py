"""A partition projected onto the organisms on the device (nemgpu_master_project, csrc/nem_project.hip) against the
numpy statement projection.projection_arrays -- which tests/test_projection_host.py holds against the reference's own
projection() -- array for array: the recorded fixtures end to end (Master.from_annotations -> projection -> write),
random annotation sets with random labels, and the shapes where the kernels take another path: organism counts around
a word of 32 and of 64, an organism spanning three blocks followed by many inside one wave, a hub's row longer than a
block next to empty rows, copies spread over contigs; what is refused, and the master left as it was."""
import random
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from pangenomenem_amd.projection import projection_arrays
from tests.append_util import append_host, build_host, slice_orders
from tests.orders_util import load, orders_from_annotations, random_genomes, same_master
from tests.projection_util import PROJECTION_FIXTURES, annotations_of, random_part, same_projection, written

pytestmark = pytest.mark.gpu

E_ARG = 3


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def flat(contigs, d, f, repeated=()):
    """contigs: [(organism, [family id, ...]), ...] -> flat orders"""
    genes = [x for _, fams in contigs for x in fams]
    rep = np.zeros(f, np.uint8)
    rep[list(repeated)] = 1
    return dict(genes=np.asarray(genes, np.int32), contig_ptr=np.cumsum([0] + [len(fams) for _, fams in contigs]).astype(np.int32),
                contig_org=np.asarray([o for o, _ in contigs], np.int32), contig_circular=np.zeros(len(contigs), np.uint8), d=d, repeated=rep)


def device_equals_host(m, host, part, p, what, f=None):
    """m.project_orders of the orders p against projection_arrays on the host master `host` (its order host[4])"""
    got = m.project_orders(part, p["genes"], p["contig_ptr"], p["contig_org"], p.get("repeated"), f)
    want = projection_arrays(host, host[4], part, p["genes"], p["contig_ptr"], p["contig_org"], p.get("repeated"), f,
                             d=None if np.asarray(host[0]).dtype != np.uint32 else m.d)
    same_projection(got, want, what)
    return want


@pytest.mark.parametrize("path", PROJECTION_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
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
        proj = m.projection(rec["labels"], ann, rec["project"], set(rec["repeated"]) | set(rec["update_repeated"]))
        got = written(proj, ann, tmp_path)
        assert sorted(got) == sorted(rec["files"])
        for name in rec["files"]:
            assert got[name] == rec["files"][name], name
        assert list(proj.means()) == rec["means"] and proj.organisms == rec["project"]
        if rec["project"] == rec["organisms"] + rec["new_organisms"]:
            again = m.projection(rec["labels"], ann, None, set(rec["repeated"]) | set(rec["update_repeated"]))      # (the default: all)
            same_projection((again.gene_family, again.gene_copies, again.nei_counts, again.org_counts),
                            (proj.gene_family, proj.gene_copies, proj.nei_counts, proj.org_counts), rec["name"])
    finally:
        m.close()


def test_random_annotations(gpu_lib):
    rng = np.random.default_rng(20261202)
    done = skipped = multi = undefined = subsets = 0
    for case in range(24):
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 40)), int(rng.integers(1, 70)), max_len=30)
        o = orders_from_annotations(ann, orgs, circular, repeated)
        if not len(o["genes"]) or o["repeated"][o["genes"]].all():
            continue
        host = build_host(o)
        part = random_part(rng, host[0].shape[0])
        project = list(ann)
        if case % 2:
            project = [project[i] for i in rng.permutation(len(project))[:max(1, len(project) // 2)]]
            subsets += 1
        p = orders_from_annotations(OrderedDict((name, ann[name]) for name in project), orgs, (), repeated, families=o["families"])
        m = from_orders(o)
        try:
            want = device_equals_host(m, host, part, p, "case %d" % case)
        finally:
            m.close()
        done += 1
        skipped += int((want[0] == -1).sum())
        multi += int((want[1] >= 2).sum())
        undefined += int(want[3][:, 3].sum())
    assert done >= 20 and skipped > 100 and multi > 100 and undefined > 100 and subsets >= 8, (done, skipped, multi, undefined, subsets)


def core_orders(n_fam, d, seed, n_core=12):
    """n_fam families x d organisms: the first n_core family ids in every organism, one more in all but the last (when
    d > 1), the others in about half; shuffled, so the master's numbering spreads the core over its 64-family words"""
    rng = np.random.default_rng(seed)
    contigs = []
    for o in range(d):
        have = [i for i in range(n_fam) if i < n_core or (i == n_core and o != d - 1) or (i > n_core and rng.random() < 0.5)]
        if o == 0:
            have = list(range(n_fam))                         # (every family has a gene: n = n_fam)
        have = [have[i] for i in rng.permutation(len(have))]
        cut = int(rng.integers(0, len(have) + 1))
        contigs += [(o, have[:cut]), (o, have[cut:])]
    return flat(contigs, d, n_fam)


@pytest.mark.parametrize("d", [1, 31, 32, 33, 64, 65])
def test_organism_counts_around_a_word(gpu_lib, d):
    """core_exact is a count over all d organisms: d at and around the words of the presence rows and of edge_bits"""
    o = core_orders(90, d, 500 + d)
    host = build_host(o)
    part = random_part(np.random.default_rng(d), 90)
    m = from_orders(o)
    try:
        want = device_equals_host(m, host, part, o, "d %d" % d)
    finally:
        m.close()
    core = want[3][:, 4].sum()
    assert host[0].shape == (90, d) and core >= 12 * d and (d == 1 or want[3][:, 5].sum() > 0)
    assert d == 1 or core < 14 * d                            # (the family missing from one organism alone is accessory)


def test_master_grown_and_master_from_arrays(gpu_lib):
    """the same projection from a master appended to (31 -> 33 organisms) and from one made of plain arrays (identity order)"""
    whole = core_orders(90, 33, 77)
    base, upd = slice_orders(whole, 0, 31), slice_orders(whole, 31, 33)
    base["d"] = 31
    host0 = build_host(base)
    host = append_host(host0, 90, upd, 2)
    part = random_part(np.random.default_rng(5), host[0].shape[0])
    m0 = from_orders(base)
    m = m0.add_orders(upd["genes"], upd["contig_ptr"], upd["contig_org"], upd["contig_circular"], 2, repeated=upd["repeated"])
    try:
        device_equals_host(m, host, part, whole, "appended")
        device_equals_host(m0, host0, part[:host0[0].shape[0]], base, "its base")
    finally:
        m.close()
        m0.close()
    plain = Master(host[0], host[1][0], host[1][1], host[2], edge_counts=host[3])
    try:
        # its family i is id i: the orders in the master's own numbering
        newid = np.full(90, -1, np.int64)
        newid[host[4]] = np.arange(len(host[4]))
        p = dict(whole, genes=newid[whole["genes"]].astype(np.int32))
        ident = tuple(host[:4]) + (np.arange(len(host[4]), dtype=np.int32),)
        want = device_equals_host(plain, ident, part, p, "from arrays")
        assert np.array_equal(want[0], newid[whole["genes"]])
    finally:
        plain.close()


def test_one_long_organism_then_many_short(gpu_lib):
    """700 genes of one organism in a single contig (three 256-lane blocks), then 130 organisms of one to three genes:
    many organisms inside one wave, runs crossing wave and block boundaries"""
    rng = np.random.default_rng(31)
    n_fam = 200
    contigs = [(0, list(rng.integers(0, n_fam, 700)))]
    contigs[0][1][:n_fam] = list(rng.permutation(n_fam))      # (every family has a gene)
    for o in range(1, 131):
        contigs.append((o, list(rng.integers(0, n_fam, int(rng.integers(1, 4))))))
    o = flat(contigs, 131, n_fam, repeated=[7, 150])
    assert o["contig_ptr"][1] == 700 and len(o["contig_org"]) == 131
    host = build_host(o)
    part = random_part(rng, host[0].shape[0])
    m = from_orders(o)
    try:
        want = device_equals_host(m, host, part, o, "long then short")
    finally:
        m.close()
    assert want[3][0, 6] == (want[0][:700] >= 0).sum() > 600 and (want[3][1:, 6] > 0).sum() > 100


def test_hub_row_next_to_empty_rows(gpu_lib):
    """a family with 300 distinct neighbours: its row is longer than a wave and than a block and, behind two families
    without a neighbour, crosses the entry-wise kernel's first block boundary; families with empty rows follow it too"""
    hub, n_nei = 2, 300
    contigs = [(0, [0]), (0, [1])] + [(i % 3, [hub, 3 + i]) for i in range(n_nei)] + [(1, [3 + n_nei]), (2, [4 + n_nei]), (1, [3, 4, 5])]
    o = flat(contigs, 3, 5 + n_nei)
    host = build_host(o)
    ptr = host[1][0]
    assert np.array_equal(host[4], np.arange(5 + n_nei)) and ptr[hub] == 0 and ptr[hub + 1] == n_nei > 256 and ptr[-1] - ptr[-3] == 0
    rng = np.random.default_rng(9)
    part = random_part(rng, 5 + n_nei)
    m = from_orders(o)
    try:
        want = device_equals_host(m, host, part, o, "hub")
    finally:
        m.close()
    assert want[2][hub].sum() == (part[3:3 + n_nei] < 3).sum() and want[2][hub].min() > 50
    assert not want[2][[0, 1, 3 + n_nei, 4 + n_nei]].any()


def crafted_master():
    """80 families x 4 organisms; family 0 five times in organism 0 over two contigs (one tandem pair) and once in organism 2"""
    rng = np.random.default_rng(4)
    rest = list(range(1, 80))
    contigs = [(0, [0, 0, 1, 0] + rest[:40]), (0, [2, 0, 3, 0] + rest[40:]), (1, list(rng.permutation(rest)[:50])), (2, [0] + list(rng.permutation(rest)[:30])),
               (3, list(rng.permutation(rest)[:60]))]
    return flat(contigs, 4, 80)


def test_copies_over_contigs_and_a_self_loop(gpu_lib):
    o = crafted_master()
    host = build_host(o)
    assert host[0].shape[0] == 80 and 0 in host[1][1][host[1][0][0]:host[1][0][1]], "family 0's tandem self-loop"
    part = random_part(np.random.default_rng(1), 80)
    m = from_orders(o)
    try:
        want = device_equals_host(m, host, part, o, "copies")
    finally:
        m.close()
    fam0 = np.flatnonzero(want[0] == 0)
    assert want[1][fam0].tolist() == [5, 5, 5, 5, 5, 1]


def test_contig_layouts_subsets_and_unknown_ids(gpu_lib):
    """empty contigs, an organism whose genes are all repeated, an organism whose contigs are not adjacent, a subset in
    reversed column order (the other rows of org_counts 0), ids the master has no family for (-2, counted nowhere),
    no gene at all, outputs not wanted"""
    o = crafted_master()
    host = build_host(o)
    part = random_part(np.random.default_rng(2), 80)
    m = from_orders(o)
    try:
        # organism 3's contigs around organism 1's; empty contigs at the start, in the middle and at the end; organism 1 all repeated
        p = flat([(3, []), (3, [5, 6, 5]), (1, [9, 9]), (2, []), (3, [6, 7, 80, 81]), (0, [79, 5, 80]), (0, [])], 4, 82, repeated=[9])
        want = device_equals_host(m, host, part, p, "layouts", f=82)
        assert want[0].tolist() == [5, 6, 5, -1, -1, 6, 7, -2, -2, 79, 5, -2] and want[1].tolist() == [2, 2, 2, 0, 0, 2, 1, 0, 0, 1, 1, 0]
        assert want[3][:, 6].tolist() == [2, 0, 0, 5]
        # a subset of the build's organisms in reversed column order
        parts = [slice_orders(o, c, c + 1) for c in (3, 1)]
        sub = dict(genes=np.concatenate([q["genes"] for q in parts]), contig_org=np.concatenate([q["contig_org"] for q in parts]),
                   contig_ptr=np.concatenate([parts[0]["contig_ptr"], parts[1]["contig_ptr"][1:] + parts[0]["contig_ptr"][-1]]).astype(np.int32),
                   repeated=o["repeated"])
        want = device_equals_host(m, host, part, sub, "reversed subset")
        assert not want[3][[0, 2]].any() and want[3][3, 6] == 60 and want[3][1, 6] == 50
        proj = m.projection(part, orders=(sub["genes"], sub["contig_ptr"], sub["contig_org"], sub["repeated"]))
        assert proj.columns == [3, 1] and proj.means() == tuple(float(want[3][[3, 1], k].sum()) / 2 for k in range(3))
        # no gene at all
        none = dict(genes=np.zeros(0, np.int32), contig_ptr=np.zeros(1, np.int32), contig_org=np.zeros(0, np.int32), repeated=o["repeated"])
        want = device_equals_host(m, host, part, none, "no gene")
        assert not want[3].any() and want[2].any()
        none = dict(none, contig_ptr=np.zeros(3, np.int32), contig_org=np.asarray([2, 0], np.int32))
        device_equals_host(m, host, part, none, "empty contigs only")
        # every output alone, the others NULL
        full = projection_arrays(host, host[4], part, p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"], 82)
        shapes = dict(org=(4, 7), nei=(80, 3), fam=(12,), cop=(12,))
        for k, name in enumerate(("org", "nei", "fam", "cop")):
            outs = {name: np.full(shapes[name], -7, np.int32)}
            rc, msg = raw(m, part, 82, p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"], **outs)
            assert rc == 0, msg
            assert np.array_equal(outs[name], full[(3, 2, 0, 1)[k]]), name
        assert raw(m, part, 82, p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"])[0] == 0
        # Master.projection names the id that no family has
        with pytest.raises(KeyError, match="80"):
            m.projection(part, orders=(p["genes"], p["contig_ptr"], p["contig_org"], p["repeated"]))
    finally:
        m.close()


def raw(m, part, f, genes, cptr, corg, rep=None, org=None, nei=None, fam=None, cop=None):
    """nemgpu_master_project as it is: (status, message)"""
    arrs = [np.ascontiguousarray(part, np.uint8), np.ascontiguousarray(genes, np.int32), np.ascontiguousarray(cptr, np.int32),
            np.ascontiguousarray(corg, np.int32), None if rep is None else np.ascontiguousarray(rep, np.uint8)]
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    rc = m.lib.nemgpu_master_project(m._h, ptr(arrs[0]), int(f), ptr(arrs[1]), len(arrs[1]), ptr(arrs[2]), ptr(arrs[3]), len(arrs[3]), ptr(arrs[4]),
                                     ptr(org), ptr(nei), ptr(fam), ptr(cop))
    return rc, m.lib.nemgpu_last_error().decode()


def test_refusals_leave_the_master_as_it_was(gpu_lib):
    o = crafted_master()
    part = random_part(np.random.default_rng(3), 80)
    good = dict(part=part, f=80, genes=[1, 2, 3, 0], cptr=[0, 2, 4], corg=[0, 3])
    m = from_orders(o)
    try:
        before = m.arrays()
        for change, word in ((dict(part=np.where(np.arange(80) == 17, 4, part)), "class 4"), (dict(part=np.where(np.arange(80) == 79, 255, part)), "class 255"),
                             (dict(cptr=[0, 3, 2, 4], corg=[0, 1, 3]), "monotone"), (dict(cptr=[0, 2, 3]), "contig_ptr"),
                             (dict(corg=[0, 4]), "organism out of range"), (dict(genes=[1, 2, 80, 0]), "family id out of range")):
            rc, msg = raw(m, **dict(good, **change))
            assert rc == E_ARG and word in msg, (change, rc, msg)
        after = m.arrays()
        same_master(after, before, "after the refusals")
        assert np.array_equal(after[4], before[4])
        rc, msg = raw(m, **good)
        assert rc == 0, msg
        after = m.arrays()
        same_master(after, before, "after a projection")
        assert np.array_equal(after[4], before[4])
        partitions, cnt, samples = m.partition(rng=random.Random(1))
        assert len(partitions) == 80
        names = ["fam%d" % (i + 1) for i in range(80)]
        codes = np.asarray(["PSCU".index(partitions[name]) for name in names], np.uint8)
        device_equals_host(m, build_host(o), codes, o, "the partition's own labels")
        with pytest.raises(NemGpuError, match="class 4"):
            m.project_orders(np.full(80, 4, np.uint8), good["genes"], good["cptr"], good["corg"])
    finally:
        m.close()
    d = from_orders(o, directed=True)
    try:
        n = d.shape()[0]
        rc, msg = raw(d, np.zeros(n, np.uint8), 80, good["genes"], good["cptr"], good["corg"])
        assert rc == E_ARG and "directed" in msg, (rc, msg)
        with pytest.raises(NemGpuError, match="directed"):
            d.projection(np.zeros(n, np.uint8), orders=(good["genes"], good["cptr"], good["corg"]))
    finally:
        d.close()


def test_projection_raises_keyerror_for_an_unknown_family(gpu_lib):
    rec = load([p for p in PROJECTION_FIXTURES if p.endswith("late.json")][0])
    ann = annotations_of(rec)
    m = Master.from_annotations(ann, rec["organisms"], rec["circular"], rec["repeated"])
    try:
        gene = next(iter(ann["o2"]["o2c1"]))
        ann["o2"]["o2c1"][gene][1] = "NEVER_SEEN"
        with pytest.raises(KeyError, match="NEVER_SEEN"):
            m.projection(rec["labels"], ann, ["o3", "o2"], rec["repeated"])
        with pytest.raises(KeyError):
            m.projection(rec["labels"], ann, ["o3", "nobody"], rec["repeated"])
        m.projection(rec["labels"], ann, ["o3", "o1"], rec["repeated"])
    finally:
        m.close()
