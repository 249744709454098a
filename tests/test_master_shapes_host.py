"""The masters of tests/master_shapes.py reach the kernel branches tests/test_gpu_master_shapes.py is there to run, so
that those tests cannot quietly stop covering them: asserted on the CPU from the fixtures and the kernels' launch
arithmetic.  And the master builders' default spectrum still gives every older fixture bit for bit.  The same for the
orders of tests/test_gpu_orders_shapes.py: the scans' item counts, the sorted keys' runs, the key widths and the rows
an append joins."""
import hashlib

import numpy as np
import pytest

from pangenomenem_amd import synth
from tests import master_shapes as ms


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def flat(out):
    return [a for v in out for a in (v if isinstance(v, tuple) else (v,))]


# recorded from the builders before they took a / b
@pytest.mark.parametrize("counts,args,kw,want", [
    (False, (3000, 300, 5), {}, "1e7537fff1a0b894"),
    (False, (2000, 40, 3), {}, "2c3095a467e19cae"),
    (True, (1500, 40, 8), dict(multi_frac=0.1, loops=0.02), "7be050c21c3a46ff"),
    (True, (2500, 320, 2), dict(multi_frac=0.05, dense_loops=2, directed=True), "a1bc8506edd1b1eb")])
def test_default_spectrum_keeps_the_old_fixtures(counts, args, kw, want):
    build = synth.master_pangenome_counts if counts else synth.master_pangenome
    assert digest(flat(build(*args, **kw))) == want
    assert digest(flat(build(*args, a=0.3, b=0.3, **kw))) == want
    assert digest(flat(build(*args, a=0.05, b=1.0, **kw))) != want


def test_spectrum_reaches_the_matrix():
    x0, _, _ = synth.master_pangenome(4000, 60, 1)
    x1, _, _ = synth.master_pangenome(4000, 60, 1, a=0.05, b=1.0)
    assert x1.mean() < 0.2 < x0.mean()


def test_launch_arithmetic():
    assert ms.index_passes(65536) == 1 and ms.index_passes(65537) == 2 and ms.index_passes(140000) == 3
    assert ms.core_y_blocks(4096) == 1 and ms.core_y_blocks(4097) == 2
    assert ms.tile_shape(1) == (0, 1, 256) and ms.tile_shape(255) == (0, 255, 256)
    assert ms.tile_shape(256) == (1, 256, 256) and ms.tile_shape(257) == (1, 1, 512)
    assert ms.organism_passes(256) == 1 and ms.organism_passes(257) == 2
    fam = np.arange(256) * 3
    assert ms.tile_staged(fam) == [True] and ms.tile_staged(fam * 4) == [False]
    assert ms.tile_staged(np.r_[0, np.arange(255) + 11 * 64 - 254]) == [True]      # first and last 11 words apart
    assert ms.tile_staged(np.r_[0, np.arange(255) + 12 * 64 - 254]) == [False]     # 12


def test_wide_masters_pass_2048_words():
    for x, _, _, *rest in (ms.wide_master(), ms.wide_counts_master()):
        n = x.shape[0]
        assert ms.nw64(n) > 2048 and ms.index_passes(n) >= 3
        assert ms.core_y_blocks(n) >= 2 and ms.vote_blocks(n) > 256


def test_cloud_master_mixes_staged_and_unstaged_samples():
    x, _, _ = ms.cloud_master()
    assert ms.core_y_blocks(x.shape[0]) >= 2
    staged = [ms.tile_staged(ms.kept(x, s)) for s in ms.cloud_samples()]
    assert any(not all(t) for t in staged) and any(all(t) for t in staged)
    assert any(all(not v for v in t) for t in staged)       # a sample of unstaged tiles only
    dcs = [len(s) for s in ms.cloud_samples()]
    assert 1 in dcs and 257 in dcs and 300 in dcs
    assert ms.organism_passes(257) == 2


@pytest.mark.parametrize("which", ["bits", "counts"])
def test_wide_groups_straddle_65536(which):
    x = (ms.wide_master() if which == "bits" else ms.wide_counts_master())[0]
    nc = [len(ms.kept(x, s)) for s in ms.wide_samples()]
    groups = [nc[g:g + ms.WIDE_GROUP] for g in range(0, len(nc), ms.WIDE_GROUP)]
    assert all(min(g) < ms.FUSED_LIMIT <= max(g) for g in groups), nc
    assert 1 in map(len, ms.wide_samples()) and 257 in map(len, ms.wide_samples())


def test_boundary_masters():
    for n, d in ms.BOUNDARY_SHAPES:
        x, (ptr, idx), eb = ms.boundary_master(n, d)
        assert x.shape == (n, d) and eb.shape == (len(idx), (d + 31) // 32)
    ns = {n for n, _ in ms.BOUNDARY_SHAPES}
    ds = {d for _, d in ms.BOUNDARY_SHAPES}
    assert {1, 63, 64, 65, 4097} <= ns and {1, 32, 33, 65} <= ds
    assert 64 * ms.nw64(63) - 63 == 1 and 64 * ms.nw64(64) == 64 and ms.nw64(65) == 2


def test_tile_master_keeps():
    x, (ptr, idx), eb = ms.tile_master()
    assert x.shape == (600, 6) and x.any(axis=1).all()
    for o, c in enumerate(ms.TILE_KEEPS):
        assert len(ms.kept(x, [o])) == c
    tails = {ms.tile_shape(len(ms.kept(x, s)))[1:] for s in ms.tile_samples()}
    assert {(1, 256), (255, 256), (256, 256), (1, 512)} <= tails
    # its edges are the organisms that hold both ends
    src = np.repeat(np.arange(600), np.diff(ptr))
    bits = np.unpackbits(eb.view(np.uint8), axis=1, bitorder="little")[:, :6]
    assert np.array_equal(bits, x[src] & x[idx]) and bits.any()


# ---- the build, the append and the projection (tests/test_gpu_orders_shapes.py)
def test_scan_arithmetic():
    assert ms.SCAN_TILE == 8 * ms.SCAN_THREADS and ms.SCAN_PASS == 524288
    assert ms.scan_tiles(1) == 1 and ms.scan_tiles(2048) == 1 and ms.scan_tiles(2049) == 2
    assert ms.scan_passes(ms.SCAN_PASS) == 1 and ms.scan_passes(ms.SCAN_PASS + 1) == 2 and ms.scan_passes(2 * ms.SCAN_PASS) == 2
    assert [ms.key_bits(c) for c in (1, 2, 3, 4, 5, 64, 65, 4096, 4097)] == [1, 1, 2, 2, 3, 6, 7, 12, 13]
    assert ms.key_bits(1 << 30) == 30 and ms.key_bits((1 << 30) + 1) == 31 and ms.key_bits((1 << 31) - 1) == 31


def test_scan_fixture_sizes():
    """the projection scans one item per gene: above a pass, exactly a pass, a pass and one, whole tiles"""
    want = {"all": None, "pass": ms.SCAN_PASS, "pass+1": ms.SCAN_PASS + 1, "tiles": 3 * ms.SCAN_TILE, "half": ms.SCAN_PASS // 2,
            "half+1": ms.SCAN_PASS // 2 + 1}
    for size, g in want.items():
        o = ms.scan_orders(size)
        assert o["contig_ptr"][-1] == len(o["genes"]) and (np.diff(o["contig_ptr"]) >= 0).all() and o["contig_org"].max() == o["d"] - 1
        assert g is None or len(o["genes"]) == g
    g = len(ms.scan_orders()["genes"])
    assert ms.SCAN_PASS + 1 < g < ms.SCAN_PASS + ms.SCAN_TILE and ms.scan_passes(g) == 2       # (the second pass: a single tile)
    assert ms.scan_passes(len(ms.scan_orders("pass")["genes"])) == 1 and ms.scan_passes(len(ms.scan_orders("pass+1")["genes"])) == 2
    assert len(ms.scan_orders("tiles")["genes"]) % ms.SCAN_TILE == 0 and ms.scan_tiles(len(ms.scan_orders("tiles")["genes"])) == 3
    # the projection sorts the genes not counted behind the kept ones, whose runs alone are numbered by the scan: the whole
    # fixture's kept genes end before the second pass, those of "more" fill tiles of it
    keys, others = ms.projection_keys(ms.scan_master(), ms.scan_orders(), ms.scan_orders()["repeated"])
    assert ms.SCAN_PASS - 8 * ms.SCAN_TILE < len(keys) < ms.SCAN_PASS and others > 1000
    more = ms.scan_orders("more")
    keys, others = ms.projection_keys(ms.scan_master(), more, more["repeated"])
    assert len(keys) > ms.SCAN_PASS + 2 * ms.SCAN_TILE and others > 1000 and len(keys) + others == len(more["genes"])
    runs = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    assert (runs > ms.SCAN_PASS).sum() > ms.SCAN_TILE and len(ms.straddling_runs(keys, ms.SCAN_TILE)) > 0      # (runs that start in the second pass)
    assert more["contig_org"][-1] == ms.SCAN_AGAIN - 1 and more["d"] == ms.SCAN_ORGANISMS


def test_scan_fixture_builds_pass_a_scan_pass():
    """a build's scans: one item per gene, per record (two per gene), per (entry, organism) pair, per entry"""
    o, m = ms.scan_orders(), ms.scan_master()
    scans = ms.plan_scans(o, m)
    assert scans["records"] == ms.orders_records(o) == 2 * scans["genes"]
    records, pairs = ms.half_edges(m)
    assert pairs <= records <= scans["records"] and records > pairs                 # (the statement's rows fill the slots they need)
    assert all(ms.scan_passes(scans[k]) >= 2 for k in ("genes", "records", "pairs")), scans
    assert ms.scan_tiles(scans["entries"]) > 32 and len(m[3][1]) > 200 and np.diff(m[3][0]).max() > 32
    # the record count on the boundary: exactly a pass, and one gene more
    assert ms.orders_records(ms.scan_orders("half")) == ms.SCAN_PASS and ms.orders_records(ms.scan_orders("half+1")) == ms.SCAN_PASS + 2
    assert ms.scan_passes(ms.SCAN_PASS + 2) == 2
    # and the last kept gene's scan on it
    assert len(ms.scan_orders("pass")["genes"]) == ms.SCAN_PASS


def test_wide_orders_pass_a_scan_pass():
    """test_gpu_orders.test_wide_shape's orders"""
    from tests.orders_util import synthetic_orders
    n, d = ms.wide_master()[0].shape
    o = synthetic_orders(n, d, 42, density=0.1, p_repeat=0.0)
    assert ms.scan_passes(len(o["genes"])) > 2 and ms.scan_passes(ms.orders_records(o)) > 4


def test_scan_fixture_as_an_append():
    base, upd = ms.scan_parts()
    m0, m1 = ms.scan_appended()
    assert m0[0].shape[1] == ms.SCAN_BASE and m1[0].shape[1] == ms.SCAN_ORGANISMS
    assert ms.scan_passes(ms.orders_records(upd)) >= 2 and ms.scan_passes(len(upd["genes"])) == 1
    alone = ms.host_master(dict(upd, d=ms.SCAN_ORGANISMS))
    records, pairs = ms.half_edges(alone)
    assert ms.scan_passes(pairs) >= 2 and records > ms.SCAN_PASS
    assert ms.scan_tiles(len(alone[1][1])) > 32 and ms.scan_tiles(len(m1[1][1])) > 32      # (the edges' scans: tens of tiles)
    # old entries with extras gain more, one of them past 32; entries and families are new
    assert len(m0[3][1]) > 0 and np.diff(m0[3][0]).max() < 32 < np.diff(m1[3][0]).max()
    assert len(m1[1][1]) > len(m0[1][1]) and m1[0].shape[0] >= m0[0].shape[0]


def test_copies_fixture_straddles_a_tile():
    o = ms.copies_orders()
    m = ms.host_master(o)
    assert np.array_equal(m[4], np.arange(ms.COPIES_FAMILIES))
    keys, others = ms.projection_keys(m, o)
    assert others == 0 and len(keys) == len(o["genes"]) > ms.SCAN_TILE           # every gene kept: no key behind the last kept one
    over_tile, over_block = ms.straddling_runs(keys, ms.SCAN_TILE), ms.straddling_runs(keys, ms.SCAN_THREADS)
    assert over_tile.tolist() == [ms.COPIES + 1] and ms.COPIES + 1 in over_block.tolist() and ms.COPIES > ms.SCAN_THREADS
    assert keys[-1] == keys[-2] == keys[-3]                                       # the last run ends with the last sorted item
    keys, others = ms.projection_keys(m, o, np.ones(ms.COPIES_FAMILIES, np.uint8))
    assert len(keys) == 0 and others == len(o["genes"])                           # no gene kept


def test_key_fixtures_sit_on_the_widths():
    bits = lambda counts: [ms.key_bits(c) for c in counts]
    assert bits(ms.KEY_FAMILIES) == [6, 7, 7, 8, 12, 13] and bits(ms.KEY_ORGANISMS) == [1, 1, 2, 5, 6, 6, 7]
    for n in ms.KEY_FAMILIES:
        for d in ms.KEY_ORGANISMS:
            o, rep = ms.key_orders(n, d)
            m = ms.host_master(o)
            assert m[0].shape == (n, d) and n < len(o["genes"]) < n + 70 * d
            # the keys that one bit less in a field would merge: the first and last families in the first two and last organisms
            inv = np.empty(n, np.int64)
            inv[m[4]] = np.arange(n)
            org = np.repeat(o["contig_org"], np.diff(o["contig_ptr"]))
            have = set(zip(org.tolist(), inv[o["genes"]].tolist()))
            assert all((c, i) in have for c in {0, min(1, d - 1), d - 1} for i in (0, 1, n - 2, n - 1))
            assert not rep[m[4][[0, 1, n - 2, n - 1]]].any() and (n < 100 or rep.any())
            keys, _ = ms.projection_keys(m, o, rep)
            assert (np.diff(np.flatnonzero(np.r_[True, keys[1:] != keys[:-1], True])) >= 2).any()      # (copies of 2 or more)


def test_wide_rows_fixture():
    o, hubs = ms.wide_rows_orders()
    m = ms.host_master(o)
    ptr = m[1][0].astype(np.int64)
    deg = np.diff(ptr)
    n = len(deg)
    assert n > 131072 and np.array_equal(m[4], np.arange(n))
    assert deg[list(hubs)].tolist() == [ms.WIDE_ROWS_HUB, ms.WIDE_ROWS_HUB + 200] and min(deg[list(hubs)]) > 3 * ms.SCAN_THREADS
    e0, e1, e2 = ms.WIDE_ROWS_EMPTY
    assert not deg[:hubs[0]].any() and hubs[0] == e0 and not deg[hubs[1] - e1:hubs[1]].any() and not deg[n - e2:].any()
    assert (deg == 0).sum() > 0.98 * n
    assert ptr[hubs[0]] // ms.SCAN_THREADS < (ptr[hubs[0] + 1] - 1) // ms.SCAN_THREADS - 2      # the hub's entries: four blocks or more


def test_hub_fixture_joins():
    base, upd = ms.hub_parts()
    m0 = ms.host_master(base)
    m1 = ms.host_append(m0, len(base["repeated"]), upd, 2)
    old, new = np.diff(m0[1][0])[ms.HUB], np.diff(m1[1][0])[ms.HUB]
    assert old == ms.HUB_OLD + 2 and new - old == ms.HUB_NEW + 22 > ms.SCAN_THREADS
    assert m1[0].shape[0] == m0[0].shape[0] + ms.HUB_NEW and np.array_equal(m1[4], np.arange(3000 + ms.HUB_NEW))
    rows = ms.update_rows(upd, 5, m1)
    at = np.concatenate([[0], np.cumsum(rows)])
    assert rows[ms.HUB] == new - old + 50                                          # (50 of its old neighbours once more)
    assert at[ms.HUB] < ms.SCAN_TILE < at[ms.HUB + 1] and at[ms.HUB] // ms.SCAN_THREADS < at[ms.HUB + 1] // ms.SCAN_THREADS - 1


def test_extras_fixture():
    base, upd = ms.extras_parts()
    m0 = ms.host_master(base)
    m1 = ms.host_append(m0, 30, upd, ms.EXTRAS_UPDATE)
    assert np.diff(m0[3][0]).max() == ms.EXTRAS_BASE > 32 and np.diff(m1[3][0]).max() == ms.EXTRAS_BASE + ms.EXTRAS_UPDATE
    assert upd["contig_org"].min() == ms.EXTRAS_BASE < 64 < upd["contig_org"].max() and m1[2].shape[1] == 3 and m0[2].shape[1] == 2


def test_key_bits_change_across_the_append():
    base, upd = ms.key_bits_parts()
    m0 = ms.host_master(base)
    m1 = ms.host_append(m0, len(base["repeated"]), upd, ms.KEY_BITS_PARTS[3] - ms.KEY_BITS_PARTS[1])
    assert m0[0].shape == ms.KEY_BITS_PARTS[:2] and m1[0].shape == ms.KEY_BITS_PARTS[2:]
    assert ms.key_bits(m0[0].shape[0]) == 12 and ms.key_bits(m1[0].shape[0]) == 13
    assert ms.key_bits(m0[0].shape[1]) == 5 and ms.key_bits(m1[0].shape[1]) == 6


def test_triple_append_stages():
    stages = ms.triple_masters()
    shapes = [m[0].shape for m in stages]
    assert [d for _, d in shapes] == list(ms.TRIPLE_STAGES)
    assert all(d % 32 for _, d in shapes) and all(n % 64 for n, _ in shapes)
    assert [(d + 31) // 32 for _, d in shapes] == [1, 2, 3, 4]                     # every append re-strides edge_bits
    ns = [n for n, _ in shapes]
    assert ns[0] < ns[1] < ns[2] < ns[3] and all(len(a[1][1]) < len(b[1][1]) for a, b in zip(stages[:-1], stages[1:]))
    # the old entries' last word has bits to mask in every stage that is appended to
    assert all(len(m[3][1]) > 0 for m in stages)


def test_count_bound_orders():
    half = ms.COUNT_BOUND // 2
    o = ms.alternating_orders(half, 0, 1)
    assert len(o["genes"]) == half + 1 and o["genes"][:4].tolist() == [0, 1, 0, 1]
    small = ms.host_master(ms.alternating_orders(6, 0, 1))
    assert small[3][2].tolist() == [6, 6] and small[1][1].tolist() == [1, 0]      # entry (0, 1) counts the links
