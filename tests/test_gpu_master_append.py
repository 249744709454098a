"""Organisms appended to a resident master on the device (nemgpu_master_append_orders, csrc/nem_orders.hip) against the
numpy statement chunks.master_arrays_append_orders -- which tests/test_master_append_host.py holds against the
reference's own add_organism -- on the recorded fixtures, on random annotation sets with one or two appends and at the
shapes where a stride changes or a path is first taken; the source master left as it was; partition() on an appended
master and on the master of everything; what is refused."""
import random
from collections import OrderedDict

import numpy as np
import pytest

from pangenomenem_amd.chunks import Master
from pangenomenem_amd.engine import NemGpuError
from tests import master_shapes as ms
from tests.append_util import (UPDATE_FIXTURES, append_host, build_host, fixture_parts, lists_to_annotations, part_orders, slice_orders,
                               split_annotations)
from tests.orders_util import load, random_genomes, same_master, synthetic_orders

pytestmark = pytest.mark.gpu


def from_orders(o, **kw):
    return Master.from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"], **kw)


def add_orders(m, u, d_new):
    return m.add_orders(u["genes"], u["contig_ptr"], u["contig_org"], u["contig_circular"], d_new, repeated=u["repeated"])


def device_equals_host(base, updates, what):
    """base orders, then updates [(orders, d_new), ...] appended one after the other: every device master equals the
    statement's, and the master appended to is afterwards what it was.  Returns the host masters, base first."""
    host = [build_host(base)]
    m = from_orders(base)
    f_old = len(base["repeated"])
    try:
        for step, (u, d_new) in enumerate(updates):
            before = m.arrays()
            want = append_host(host[-1], f_old, u, d_new)
            grown = add_orders(m, u, d_new)
            try:
                got = grown.arrays()
                tag = "%s, append %d" % (what, step)
                assert grown.shape() == (want[0].shape[0], want[0].shape[1], len(want[1][1]), len(want[3][1])), tag
                assert np.array_equal(got[4], want[4]) and np.array_equal(grown.order, want[4]), tag + ": family order"
                same_master(got, want, tag)
                after = m.arrays()
                same_master(after, before, tag + ": the source master")
                assert np.array_equal(after[4], before[4]) and m.shape()[1] == host[-1][0].shape[1]
            except BaseException:
                grown.close()
                raise
            m.close()
            m = grown
            host.append(want)
            f_old = len(u["repeated"])
    finally:
        m.close()
    return host


@pytest.mark.parametrize("path", UPDATE_FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_fixtures(gpu_lib, path):
    rec = load(path)
    base, upd = fixture_parts(rec)
    device_equals_host(base, [(upd, len(rec["new_organisms"]))], rec["name"])
    m = Master.from_annotations(lists_to_annotations(rec["annotations"]), rec["organisms"], rec["circular"], rec["repeated"])
    g = m.add_annotations(lists_to_annotations(rec["update_annotations"]), rec["new_organisms"],
                          set(rec["circular"]) | set(rec["update_circular"]), set(rec["repeated"]) | set(rec["update_repeated"]))
    assert g.names == [f for f, _ in rec["undirected"]["nodes"]] and g.organism_names == rec["organisms"] + rec["new_organisms"]
    assert m.names == g.names[:m.n] and m.organism_names == rec["organisms"]
    m.close()
    g.close()


def test_random_annotations(gpu_lib):
    rng = np.random.default_rng(20261104)
    done = twice = multi = fresh = 0
    for case in range(70):
        k = 2 + case % 2
        ann, orgs, circular, repeated = random_genomes(rng, int(rng.integers(2, 40)), int(rng.integers(k, 70)), max_len=30)
        cuts = np.sort(rng.choice(np.arange(1, len(orgs)), k - 1, replace=False))
        parts, cols = split_annotations(ann, orgs, cuts)
        os_, _ = part_orders(parts, cols, circular, repeated)
        if not len(os_[0]["genes"]) or os_[0]["repeated"][os_[0]["genes"]].all() or any(len(o["genes"]) == 0 for o in os_):
            continue
        host = device_equals_host(os_[0], [(o, len(p)) for o, p in zip(os_[1:], parts[1:])], "case %d" % case)
        done += 1
        twice += k == 3
        multi += len(host[-1][3][1]) - len(host[0][3][1])
        fresh += host[-1][0].shape[0] - host[0][0].shape[0]
    assert done >= 55 and twice >= 20 and multi > 300 and fresh > 20, (done, twice, multi, fresh)


def two_parts(nf0, d0, nf1, d1, seed, density=0.5):
    """a base of nf0 families x d0 organisms and an update of organisms d0 .. d1 - 1 over nf1 >= nf0 family ids"""
    base = synthetic_orders(nf0, d0, seed, density=density, p_repeat=0.0)
    base["repeated"] = np.zeros(nf0, np.uint8)
    upd = slice_orders(synthetic_orders(nf1, d1, seed + 1000, density=density, p_repeat=0.0), d0, d1)
    upd["repeated"] = np.zeros(nf1, np.uint8)
    return base, upd


@pytest.mark.parametrize("d0,d1", [(31, 33), (64, 65), (32, 64)])
def test_organism_word_boundaries(gpu_lib, d0, d1):
    """the edge_bits stride changes (31 -> 33, 64 -> 65) or does not (32 -> 64)"""
    base, upd = two_parts(40, d0, 50, d1, 300 + d0)
    host = device_equals_host(base, [(upd, d1 - d0)], "d %d -> %d" % (d0, d1))
    assert host[0][0].shape == (40, d0) and host[1][0].shape[1] == d1 and host[1][0].shape[0] > 40


@pytest.mark.parametrize("n0,n1", [(63, 65), (64, 64)])
def test_family_word_boundaries(gpu_lib, n0, n1):
    """the presence rows' stride changes (63 -> 65 families) or does not (64 -> 64: no new family)"""
    base, upd = two_parts(n0, 5, n1, 7, 400 + n0, density=1.0)
    host = device_equals_host(base, [(upd, 2)], "n %d -> %d" % (n0, n1))
    assert host[0][0].shape[0] == n0 and host[1][0].shape[0] == n1


def as_orders(contigs, orgs, f, d=None, repeated=()):
    """contigs: lists of family ids; orgs: their columns"""
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int32)
    rep = np.zeros(f, np.uint8)
    rep[list(repeated)] = 1
    return dict(genes=np.concatenate(contigs).astype(np.int32), contig_ptr=ptr, contig_org=np.asarray(orgs, np.int32),
                contig_circular=np.zeros(len(contigs), np.uint8), d=d, repeated=rep)


def test_an_update_without_a_kept_gene_only_adds_organisms(gpu_lib):
    base = synthetic_orders(30, 6, 51, density=0.5, p_repeat=0.0)
    base["repeated"] = np.zeros(30, np.uint8)
    upd = as_orders([[3, 3], [3]], [6, 7], 30, repeated=[3])
    host = device_equals_host(base, [(upd, 2)], "no kept gene")
    assert host[1][0].shape == (30, 8) and np.array_equal(host[1][1][1], host[0][1][1]) and not host[1][0][:, 6:].any()


def test_an_update_without_a_new_edge(gpu_lib):
    base = synthetic_orders(30, 6, 52, density=0.5, p_repeat=0.0)
    base["repeated"] = np.zeros(30, np.uint8)
    upd = slice_orders(base, 2, 4)                            # (organisms 2 and 3 once more, as 6 and 7)
    upd["contig_org"] = upd["contig_org"] + 4
    host = device_equals_host(base, [(upd, 2)], "no new edge")
    assert np.array_equal(host[1][1][0], host[0][1][0]) and np.array_equal(host[1][1][1], host[0][1][1])
    assert np.array_equal(host[1][0][:, 6:], host[0][0][:, 2:4])


def repeats(orgs, rng, f=30):
    """every organism: the adjacency 0-1 three times, then some of the other families"""
    return as_orders([[0, 1, 0, 1] + list(2 + rng.permutation(f - 2)[:12]) for _ in orgs], list(orgs), f)


def test_more_than_32_extras_only_after_the_append(gpu_lib):
    """entry (0, 1) has 20 extras, then 40: the chunk coverage walks them by wave (k_chunk_cov<true>) only on the grown
    master, whose chunks equal those of the master of everything"""
    rng = np.random.default_rng(53)
    base, upd = repeats(range(20), rng), repeats(range(20, 40), rng)
    base["d"] = 20
    host = device_equals_host(base, [(upd, 20)], "extras")
    assert np.diff(host[0][3][0]).max() == 20 and np.diff(host[1][3][0]).max() == 40
    whole = dict(genes=np.concatenate([base["genes"], upd["genes"]]), contig_ptr=np.concatenate([base["contig_ptr"], base["contig_ptr"][-1] + upd["contig_ptr"][1:]]),
                 contig_org=np.concatenate([base["contig_org"], upd["contig_org"]]), contig_circular=np.zeros(40, np.uint8), d=40,
                 repeated=base["repeated"])
    a, b = from_orders(base), from_orders(whole)
    g = add_orders(a, upd, 20)
    samples = [list(range(40)), list(range(5, 38)), [39, 0, 21, 20, 19]]
    for ra, rb in zip(g.solve_chunks(samples, tie="libc", seed=3), b.solve_chunks(samples, tie="libc", seed=3)):
        assert ra["n"] == rb["n"] and ra["nnz"] == rb["nnz"] and ra["iters"] == rb["iters"] and np.array_equal(ra["labels"], rb["labels"])
        assert np.array_equal(ra["center"], rb["center"])
    for m in (a, b, g):
        m.close()


def test_a_master_without_extras_gains_its_first(gpu_lib):
    rng = np.random.default_rng(54)
    base = as_orders([list(rng.permutation(30)[:15]) for _ in range(6)], list(range(6)), 30, d=6)
    upd = repeats([6], rng)
    host = device_equals_host(base, [(upd, 1)], "first extra")
    assert len(host[0][3][1]) == 0 and len(host[1][3][1]) > 0


def test_an_update_of_several_scan_tiles_and_sort_blocks(gpu_lib):
    o = synthetic_orders(5000, 40, 55)
    base = dict(slice_orders(o, 0, 32), d=32)
    upd = slice_orders(o, 32, 40)
    assert len(upd["genes"]) > 4 * 2048
    host = device_equals_host(base, [(upd, 8)], "5000 x 32 + 8")
    whole = build_host(o)
    assert np.array_equal(host[1][4], whole[4])
    same_master(host[1], whole, "one build")


def test_partition_on_an_appended_master(gpu_lib):
    """add_annotations(...).partition() is from_annotations(everything).partition(): labels, counts, samples and the
    generator's state, where the vote loop runs (40 organisms, chunks of 16)"""
    o = synthetic_orders(300, 40, 7, density=0.5, p_repeat=0.03)
    fams, orgs = ["fam%d" % i for i in range(300)], ["org%d" % i for i in range(40)]
    ann, circular = OrderedDict(), set()
    for j, org in enumerate(o["contig_org"]):
        contig = "c%d" % j
        ann.setdefault(orgs[org], OrderedDict())[contig] = OrderedDict(
            ("g%d" % p, ["CDS", fams[o["genes"][p]]]) for p in range(o["contig_ptr"][j], o["contig_ptr"][j + 1]))
        if o["contig_circular"][j]:
            circular.add(contig)
    repeated = [fams[i] for i in np.flatnonzero(o["repeated"])]
    first, rest = OrderedDict(list(ann.items())[:32]), OrderedDict(list(ann.items())[32:])
    a = Master.from_annotations(first, orgs[:32], circular, repeated)
    g = a.add_annotations(rest, orgs[32:], circular, repeated)
    b = Master.from_annotations(ann, orgs, circular, repeated)
    assert g.names == b.names and g.organism_names == b.organism_names
    same_master(g.arrays(), b.arrays(), "appended")
    r1, r2 = random.Random(5), random.Random(5)
    rg = g.partition(chunk_size=16, rng=r1, batch=8, tie="libc", seed=3)
    rb = b.partition(chunk_size=16, rng=r2, batch=8, tie="libc", seed=3)
    assert rg[0] == rb[0] and np.array_equal(rg[1], rb[1]) and rg[2] == rb[2] and rg[2] > 1 and r1.getstate() == r2.getstate()
    ra = a.partition(chunk_size=16, rng=random.Random(5), batch=8, tie="libc", seed=3)       # (the source master still works)
    assert ra[2] > 0 and len(ra[0]) == a.n
    for m in (a, b, g):
        m.close()


def test_refusals(gpu_lib):
    base = synthetic_orders(30, 6, 56, density=0.5, p_repeat=0.0)
    base["repeated"] = np.zeros(30, np.uint8)
    upd = as_orders([[0, 1, 2]], [6], 30)
    m = from_orders(base, directed=True)
    with pytest.raises(NemGpuError, match="directed"):
        add_orders(m, upd, 1)
    m.close()
    x, (ptr, idx), eb = ms.boundary_master(65, 33)
    m = Master(x, ptr, idx, eb)                               # bits only
    with pytest.raises(NemGpuError, match="bits-only"):
        add_orders(m, as_orders([[0, 1, 2]], [33], 65), 1)
    m.close()
    m = from_orders(base)
    with pytest.raises(NemGpuError, match="family ids"):
        add_orders(m, as_orders([[0, 1, 2]], [6], 29), 1)
    for col in (5, 7):
        with pytest.raises((NemGpuError, ValueError), match="organism"):
            add_orders(m, as_orders([[0, 1, 2]], [col], 30), 1)
    with pytest.raises(NemGpuError, match="organism out of range"):       # (past Python's own check: the library's)
        u = as_orders([[0, 1, 2]], [5], 30)
        arrs = [np.ascontiguousarray(u[k]) for k in ("genes", "contig_ptr", "contig_org", "contig_circular")]
        import ctypes as C
        h = C.c_void_p()
        rc = m.lib.nemgpu_master_append_orders(C.byref(h), m._h, 1, 30, arrs[0].ctypes.data, 3, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                               arrs[3].ctypes.data, 1, None)
        assert rc == 3 and not h.value
        raise NemGpuError(m.lib.nemgpu_last_error().decode())
    ok = add_orders(m, upd, 1)                                # (the master is as usable as before)
    assert ok.shape()[1] == 7
    ok.close()
    m.close()
