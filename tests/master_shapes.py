"""Masters at pangenome-scale shapes for the device chunk, vote and evolution paths (csrc/nem_chunks.hip, nem_vote.hip,
nem_resample.hip), and the host arithmetic that says which branch of those kernels a sample takes.

The small dense masters of the other tests (synth.master_pangenome's Beta(0.3, 0.3) spectrum, n <= 20 000) never reach
the branches below; tests/test_master_shapes_host.py asserts on the CPU that these fixtures do, and
tests/test_gpu_master_shapes.py runs them on the device against the host recipe.

Further down: gene orders for the device build, append and projection (csrc/nem_orders.hip, nem_project.hip,
nem_scan.hpp) at the shapes where those take another path, run by tests/test_gpu_orders_shapes.py."""
import functools

import numpy as np

from pangenomenem_amd import synth
from pangenomenem_amd.partitioning import vote_host, vote_map, vote_state

# ---- the kernels' constants and launch shapes, restated
CHUNK_TILE = 256            # k_chunk_rows: kept families per block
CHUNK_SPAN = 12             # k_chunk_rows: kChunkSpan, the 64-family words of a row one pass stages
CHUNK_ORGS = 256            # k_chunk_rows: kChunkOrgs, the organisms staged per pass
INDEX_WORDS = 1024          # k_chunk_index: 64-family words per pass of its 1024-thread block
CORE_WORDS = 64             # k_resample_core: kResampleCoreWave, words per y-block
VOTE_THREADS = 256          # k_vote_init: organisms per thread stride; k_vote_scan / k_vote_commit: families per block
FUSED_LIMIT = 65536         # density_verify_supported / launch_sweep_counts: fused kernels below this many families


def nw64(n):
    return (n + 63) // 64


def index_passes(n):
    """k_chunk_index's passes over the keep words (base is carried from one to the next)"""
    return -(-nw64(n) // INDEX_WORDS)


def core_y_blocks(n):
    """gridDim.y of k_resample_core"""
    return -(-nw64(n) // CORE_WORDS)


def vote_blocks(n):
    """blocks of k_vote_scan / k_vote_commit"""
    return -(-n // VOTE_THREADS)


def organism_passes(dc):
    """k_chunk_rows' passes over the sample's organisms"""
    return -(-dc // CHUNK_ORGS)


def tile_staged(families):
    """k_chunk_rows' staging decision per 256-family tile of a sample's kept families (master indices, ascending): a
    tile is staged through LDS when its first and last family lie fewer than kChunkSpan 64-family words apart, and
    read straight from the master's rows (the unstaged branch) otherwise"""
    fam = np.asarray(families, np.int64)
    return [bool((fam[min(t + CHUNK_TILE, len(fam)) - 1] >> 6) - (fam[t] >> 6) < CHUNK_SPAN) for t in range(0, len(fam), CHUNK_TILE)]


def tile_shape(nc):
    """(full tiles, families in the last started tile, npad) of a chunk with nc kept families"""
    npad = -(-nc // CHUNK_TILE) * CHUNK_TILE
    last = nc - (npad - CHUNK_TILE) if nc else 0
    return nc // CHUNK_TILE, last, npad


def kept(x, organisms):
    """the master indices of the families a sample keeps"""
    return np.flatnonzero(np.asarray(x)[:, np.asarray(organisms, np.int64)].any(axis=1))


# ---- the masters (cached: the host and the device tests of one session build each once)
@functools.lru_cache(maxsize=None)
def cloud_master():
    """mostly cloud (Beta(0.05, 1)): a sample of a few organisms keeps a small, sparse share of the families, so its
    tiles span more than kChunkSpan words (unstaged); 313 words, 5 core y-blocks"""
    return synth.master_pangenome(20000, 300, 41, a=0.05, b=1.0)


@functools.lru_cache(maxsize=None)
def wide_master():
    """more than 131 072 families (3 index passes, 2 188 words); a single organism keeps fewer than 65 536 of them,
    three or more organisms keep more"""
    return synth.master_pangenome(140000, 300, 42, a=0.3, b=0.6)


@functools.lru_cache(maxsize=None)
def wide_counts_master():
    """wide_master's shape with occurrence counts (nemgpu_master_create_counts), a directed graph's"""
    return synth.master_pangenome_counts(140000, 300, 43, multi_frac=0.05, dense_loops=2, directed=True, a=0.3, b=0.6)


BOUNDARY_SHAPES = ((1, 1), (1, 33), (63, 32), (64, 1), (64, 65), (65, 33), (4097, 32), (4097, 65))


@functools.lru_cache(maxsize=None)
def boundary_master(n, d):
    """n around one 64-family word (the last word partial or exactly full), d around one 32-organism word"""
    return synth.master_pangenome(n, d, 50 + n + d)


TILE_KEEPS = (1, 255, 256, 257)     # the kept families of tile_master's single-organism samples 0 .. 3


@functools.lru_cache(maxsize=None)
def tile_master():
    """600 families, 6 organisms: organism o < 4 alone keeps exactly TILE_KEEPS[o] families (a partial tile, one
    short of a tile, an exact tile, a tile and one), spread over the master; organisms 4 and 5 hold the rest and some
    of the same.  The graph: contiguity_graph's structure, an edge carried by the organisms that hold both ends."""
    n, d = 600, 6
    rng = np.random.default_rng(600)
    x = np.zeros((n, d), np.uint8)
    for o, c in enumerate(TILE_KEEPS):
        x[np.sort(rng.permutation(n)[:c]), o] = 1
    x[:, 4] = x[:, :4].sum(axis=1) == 0
    x[rng.permutation(n)[:200], 5] = 1
    ptr, idx, _ = synth.contiguity_graph(n, 600)
    src = np.repeat(np.arange(n), np.diff(ptr))
    both = x[src] & x[idx]
    eb = np.zeros((len(idx), 4), np.uint8)
    eb[:, :1] = np.packbits(both, axis=1, bitorder="little")
    return x, (ptr, idx), np.ascontiguousarray(eb.view(np.uint32))


# ---- the samples the tests draw
def cloud_samples():
    """single organisms and pairs (unstaged), 5 and 20 (some tiles staged), 100, 257 (a second organism pass with one
    organism in it) and the full set (staged)"""
    rng = np.random.default_rng(41)
    return [rng.permutation(300)[:dc] for dc in (1, 2, 100, 1, 5, 257, 20, 300, 2)]


WIDE_GROUP = 2


def wide_samples():
    """lock-step groups of WIDE_GROUP: every group has one member below 65 536 kept families and one above"""
    rng = np.random.default_rng(42)
    return [rng.permutation(300)[:dc] for dc in (1, 10, 3, 2, 257, 1)]


def boundary_samples(d):
    rng = np.random.default_rng(d)
    out = [[o] for o in sorted({0, d - 1, d // 2})] + [np.arange(d)]
    if d > 2:
        out += [rng.permutation(d)[:d // 2 + 1], rng.permutation(d)]
    return out


def tile_samples():
    return [[0], [1], [2], [3], [3, 0], [0, 1, 2, 3, 4, 5], [5, 1]]


# ---- partition()'s sequential loop on the host
def host_solve(x, ptr, idx, eb, counts, subs, **cfg):
    """the samples formed by form_chunk_host and solved by solve_many (PPanGGOLiN's default .m)"""
    from pangenomenem_amd.batch import solve_many
    from pangenomenem_amd.chunks import form_chunk_host
    host = [form_chunk_host(x, ptr, idx, eb, s, edge_counts=counts) for s in subs]
    probs = [(xc, nei, 3) + synth.default_init(xc.shape[1]) for xc, nei, _ in host]
    return host, solve_many(probs, workers=4, group=8, **cfg)


def host_partition(x, ptr, idx, eb, counts, organisms, chunk_size, rng, tie, seed, batch=16, max_samples=5000):
    """partition()'s sequential loop on the host: the samples formed by form_chunk_host, solved by solve_many, voted by
    vote_map and vote_host; the draws after the stop undone"""
    organisms = np.asarray(organisms)
    st = vote_state(x.shape[0], x[:, organisms].any(axis=1))
    cfg = dict(algo="ncem", beta=0.5, disper="sk_", it_max=100, tie=tie, seed=seed)
    while st["samples"] < max_samples:
        states, samples = [], []
        for _ in range(batch):
            states.append(rng.getstate())
            samples.append(organisms[rng.sample(range(len(organisms)), chunk_size)])
        host, res = host_solve(x, ptr, idx, eb, counts, samples, **cfg)
        votes = [(fam, r["c"].argmax(1), vote_map(r["status"], r["center"], r["disp"])) for (_, _, fam), r in zip(host, res)]
        stop = vote_host(st, votes, len(organisms), chunk_size)
        if stop >= 0:
            if stop + 1 < batch:
                rng.setstate(states[stop + 1])
            return st
    raise AssertionError("no end")


# ---- the units on sorted records: the master's build and append (csrc/nem_orders.hip), the projection
# (csrc/nem_project.hip) and the scans they share (csrc/nem_scan.hpp); tests/test_gpu_orders_shapes.py runs these
SCAN_THREADS = 256                   # seg::kThreads: every kernel of the three files runs 256-thread blocks
SCAN_TILE = 2048                     # seg::kScanTile: kThreads * kScanItems, the items of one block of k_scan_reduce / k_scan_apply
SCAN_PASS = SCAN_THREADS * SCAN_TILE   # the items whose tile totals one pass of k_scan_partials' single block takes: beyond, it carries


def scan_tiles(n):
    """blocks of k_scan_reduce / k_scan_apply, and the tile totals k_scan_partials scans"""
    return -(-n // SCAN_TILE)


def scan_passes(n):
    """k_scan_partials' passes over the tile totals (carry goes from one to the next)"""
    return -(-scan_tiles(n) // SCAN_THREADS)


def key_bits(count):
    """bits_for (nem_orders.hip, nem_project.hip): the bits of a key field holding 0 .. count - 1, at least 1"""
    b = 1
    while b < 31 and (1 << b) < count:
        b += 1
    return b


def orders_records(o):
    """the records a build or an update sorts and scans: k_orders_records fills two slots per gene (n2 = 2 g in
    orders_stage), the unused ones under the key that sorts behind all.  The statement's rows (chunks.py: a link per
    kept gene with a previous one or closing a circular contig, two half-edges per link, one for a self-loop) are the
    used ones: half_edges() of the master it returns, never more than this."""
    return 2 * len(o["genes"])


def half_edges(master):
    """(records, pairs) of a host master: the statement's half-edge rows (every (entry, organism) pair's count summed)
    and its distinct (entry, organism) pairs (orders_stage's tn: the items of the scan of the multi-copy flags)"""
    bits = np.ascontiguousarray(master[2], np.uint32)
    pairs = int(np.unpackbits(bits.view(np.uint8)).sum())
    return pairs + int(np.asarray(master[3][2], np.int64).sum()) - len(master[3][2]), pairs


def plan_scans(o, master):
    """the item counts of the scans a build of the orders o runs (master: its statement): last kept gene, record flags,
    multi-copy flags, extras per entry"""
    return dict(genes=len(o["genes"]), records=orders_records(o), pairs=half_edges(master)[1], entries=len(master[1][1]))


def concat_orders(parts, d):
    """orders of several parts (each with absolute organism columns) one after the other"""
    ptr, at = [np.zeros(1, np.int32)], 0
    for p in parts:
        ptr.append(p["contig_ptr"][1:] + at)
        at += int(p["contig_ptr"][-1])
    return dict(genes=np.concatenate([p["genes"] for p in parts]).astype(np.int32), contig_ptr=np.concatenate(ptr).astype(np.int32),
                contig_org=np.concatenate([p["contig_org"] for p in parts]).astype(np.int32),
                contig_circular=np.concatenate([p["contig_circular"] for p in parts]).astype(np.uint8), d=d, repeated=parts[-1]["repeated"])


def contigs_orders(contigs, d, f, repeated=(), circular=()):
    """contigs: [(organism, family ids), ...] -> flat orders; circular: the indices of the circular ones"""
    contigs = [(o, np.asarray(fams, np.int32)) for o, fams in contigs]
    rep, circ = np.zeros(f, np.uint8), np.zeros(len(contigs), np.uint8)
    rep[list(repeated)] = 1
    circ[list(circular)] = 1
    return dict(genes=np.concatenate([fams for _, fams in contigs]).astype(np.int32),
                contig_ptr=np.concatenate([[0], np.cumsum([len(fams) for _, fams in contigs])]).astype(np.int32),
                contig_org=np.asarray([o for o, _ in contigs], np.int32), contig_circular=circ, d=d, repeated=rep)


def trim_orders(o, g):
    """the first g genes of flat orders: the contigs behind them dropped, the one they end in cut"""
    c = int(np.searchsorted(o["contig_ptr"], g, side="left"))
    ptr = o["contig_ptr"][:c + 1].copy()
    ptr[-1] = g
    return dict(genes=o["genes"][:g], contig_ptr=ptr, contig_org=o["contig_org"][:c], contig_circular=o["contig_circular"][:c],
                d=int(o["contig_org"][:c].max()) + 1, repeated=o["repeated"])


def host_master(o, directed=False):
    from pangenomenem_amd.chunks import master_arrays_from_orders
    return master_arrays_from_orders(o["genes"], o["contig_ptr"], o["contig_org"], o["contig_circular"], o["d"], repeated=o["repeated"],
                                     directed=directed)


def host_append(master, f_old, u, d_new):
    from pangenomenem_amd.chunks import master_arrays_append_orders
    return master_arrays_append_orders(master, master[4], f_old, u["genes"], u["contig_ptr"], u["contig_org"], u["contig_circular"], d_new,
                                       repeated=u["repeated"])


def part_of(o, lo, hi):
    """organisms lo .. hi - 1 of orders walked in column order, their columns absolute (an update's orders)"""
    from tests.append_util import slice_orders
    return slice_orders(o, lo, hi)


def with_repeats(o, every=4, pairs=((10, 20), (11, 21), (12, 22))):
    """every `every`-th organism gets one more contig a b a b a of one of `pairs`: (a, b) counts 4 there, so the master
    has multi-copy pairs, some entries more than 32 of them (synthetic_orders alone has next to none)"""
    parts = []
    for org in range(o["d"]):
        parts.append(part_of(o, org, org + 1))
        if org % every == 0:
            a, b = pairs[(org // every) % len(pairs)]
            parts.append(dict(genes=np.asarray([a, b, a, b, a], np.int32), contig_ptr=np.asarray([0, 5], np.int32),
                              contig_org=np.asarray([org], np.int32), contig_circular=np.zeros(1, np.uint8), repeated=o["repeated"]))
    out = concat_orders(parts, o["d"])
    out["repeated"] = o["repeated"].copy()
    out["repeated"][np.asarray(pairs).ravel()] = 0
    return out


# the scan fixture: 3 000 families x 484 organisms at density 0.35, every fourth organism with a repeated adjacency:
# just over the genes whose tile totals one pass of k_scan_partials takes
SCAN_FAMILIES, SCAN_ORGANISMS, SCAN_BASE, SCAN_AGAIN = 3000, 484, 64, 14


@functools.lru_cache(maxsize=None)
def scan_orders(size="all"):
    """the scan fixture's orders, or their first SCAN_PASS ("pass"), SCAN_PASS + 1 ("pass+1"), 3 * SCAN_TILE ("tiles"),
    SCAN_PASS / 2 ("half") or SCAN_PASS / 2 + 1 ("half+1") genes; "more": all of them and the first SCAN_AGAIN
    organisms once more (orders to project: the kept genes alone, which sort before the others, pass SCAN_PASS)"""
    from tests.orders_util import synthetic_orders
    if size == "all":
        return with_repeats(synthetic_orders(SCAN_FAMILIES, SCAN_ORGANISMS, 61))
    if size == "more":
        return concat_orders([scan_orders(), part_of(scan_orders(), 0, SCAN_AGAIN)], SCAN_ORGANISMS)
    g = {"pass": SCAN_PASS, "pass+1": SCAN_PASS + 1, "tiles": 3 * SCAN_TILE, "half": SCAN_PASS // 2, "half+1": SCAN_PASS // 2 + 1}[size]
    return trim_orders(scan_orders(), g)


@functools.lru_cache(maxsize=None)
def scan_master(size="all"):
    """the statement's master of scan_orders(size)"""
    return host_master(scan_orders(size))


@functools.lru_cache(maxsize=None)
def scan_parts():
    """the scan fixture as an append: (base orders of the first SCAN_BASE organisms, the update of the others)"""
    o = scan_orders()
    return dict(part_of(o, 0, SCAN_BASE), d=SCAN_BASE), part_of(o, SCAN_BASE, SCAN_ORGANISMS)


@functools.lru_cache(maxsize=None)
def scan_appended():
    """the statement's masters of scan_parts(): (base, appended)"""
    base, upd = scan_parts()
    m0 = host_master(base)
    return m0, host_append(m0, SCAN_FAMILIES, upd, SCAN_ORGANISMS - SCAN_BASE)


# ---- the projection's keys: (organism << bits(n)) | family, the genes not counted under 1 << (bits(n) + bits(d))
def projection_keys(master, o, repeated=None):
    """the sorted keys of the kept genes of the orders o projected on the host master (o's family ids are the build's)"""
    n, d = np.asarray(master[0]).shape
    inv = np.full(len(o["repeated"]), -2, np.int64)
    inv[master[4]] = np.arange(n)
    fam = inv[o["genes"]]
    if repeated is not None:
        fam = np.where(np.asarray(repeated)[o["genes"]] != 0, -1, fam)
    org = np.repeat(o["contig_org"].astype(np.int64), np.diff(o["contig_ptr"]))
    kept = fam >= 0
    return np.sort((org[kept] << key_bits(n)) | fam[kept]), int((~kept).sum())


def straddling_runs(keys, boundary):
    """the lengths of the runs of equal sorted keys with items on both sides of a multiple of boundary"""
    keys = np.asarray(keys)
    if not len(keys):
        return np.zeros(0, np.int64)
    start = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    end = np.r_[start[1:], len(keys)]
    return (end - start)[(start // boundary) != ((end - 1) // boundary)]


COPIES_FAMILIES, COPIES_FAMILY, COPIES = 2500, 1900, 300


@functools.lru_cache(maxsize=None)
def copies_orders():
    """2 500 families x 3 organisms, no repeated family: organism 0 carries every family in id order (the master's
    numbering is the ids') and COPIES more genes of family COPIES_FAMILY in a second contig, so that its 301 sorted
    keys lie at 1 900 .. 2 200, over a scan tile's end and two blocks' ends; the last organism ends the sorted keys
    with a kept gene's"""
    f = COPIES_FAMILIES
    return contigs_orders([(0, np.arange(f)), (0, np.full(COPIES, COPIES_FAMILY)), (1, np.arange(100)), (1, [7, 7, 7]),
                           (2, np.arange(f - 100, f)), (2, [f - 1, f - 1])], 3, f)


# ---- the projection's key widths
KEY_FAMILIES = (64, 65, 128, 129, 4096, 4097)
KEY_ORGANISMS = (1, 2, 3, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def key_orders(n, d):
    """n families x d organisms, a few hundred genes beyond the n of organism 0, which carries every family (shuffled:
    master family i is id perm[i]); every other organism carries the master's first two and last two families -- the
    ones whose keys an organism or family field one bit short would merge with a neighbour's -- and some 60 more, a
    few of them twice.  Returns the orders and a repeated-family mask for the projection (not the build's)."""
    rng = np.random.default_rng(1000 * n + d)
    perm = rng.permutation(n)
    cut = int(rng.integers(1, n))
    ends = perm[[0, 1, n - 2, n - 1]]
    contigs = [(0, perm[:cut]), (0, perm[cut:]), (0, ends[[3, 0, 3]])]
    for o in range(1, d):
        some = rng.permutation(n)[:60]
        have = np.concatenate([ends, some, some[:5]])
        contigs.append((o, have[rng.permutation(len(have))]))
    rep = (rng.random(n) < 0.05).astype(np.uint8)
    rep[ends] = 0
    return contigs_orders(contigs, d, n), rep


# ---- rows far apart
WIDE_ROWS_EMPTY = (70000, 40000, 30000)      # families without a neighbour before, between and behind the two hubs
WIDE_ROWS_HUB = 1000


@functools.lru_cache(maxsize=None)
def wide_rows_orders():
    """more than 131 072 families over 3 organisms, nearly all alone in their contig (an empty row); two hubs of
    WIDE_ROWS_HUB and WIDE_ROWS_HUB + 200 neighbours, each its neighbour's only one, behind 70 000, between 40 000 and
    before 30 000 empty rows.  Ids in order of first gene: the master's numbering is the ids'.  Returns the orders and
    the two hubs."""
    e0, e1, e2 = WIDE_ROWS_EMPTY
    h = WIDE_ROWS_HUB
    hub_a, hub_b = e0, e0 + 1 + h + e1
    f = hub_b + 1 + h + e2
    single = lambda lo, hi: np.arange(lo, hi, dtype=np.int64).reshape(-1, 1)
    pairs = lambda hub, nb: np.stack([np.full(len(nb), hub, np.int64), nb], axis=1)
    blocks = [single(0, e0), pairs(hub_a, np.arange(hub_a + 1, hub_a + 1 + h)), single(hub_a + 1 + h, hub_b),
              pairs(hub_b, np.arange(hub_b + 1, hub_b + 1 + h)), pairs(hub_b, np.arange(hub_a + 1, hub_a + 201)), single(hub_b + 1 + h, f)]
    lens = np.concatenate([np.full(len(b), b.shape[1]) for b in blocks])
    c = len(lens)
    o = dict(genes=np.concatenate([b.ravel() for b in blocks]).astype(np.int32), contig_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
             contig_org=(np.arange(c) % 3).astype(np.int32), contig_circular=np.zeros(c, np.uint8), d=3, repeated=np.zeros(f, np.uint8))
    return o, (hub_a, hub_b)


# ---- appends at their joins
HUB, HUB_OLD, HUB_NEW = 1000, 400, 300


@functools.lru_cache(maxsize=None)
def hub_parts():
    """a base of 3 000 families in a chain (organism 0: the master's numbering is the ids') whose family HUB has HUB_OLD
    more neighbours in organisms 1 and 2; an update of two organisms: the chain's even families then its odd ones (two
    new edges in nearly every row: some 2 000 update edges sort before the hub's), and the hub next to HUB_NEW families
    the master does not have, to 20 it has but not as neighbours, and to 50 of its old neighbours again"""
    f = 3000 + HUB_NEW
    base = contigs_orders([(0, np.arange(3000))] + [(1 + i % 2, [HUB, 1500 + i]) for i in range(HUB_OLD)], 3, f)
    upd = contigs_orders([(3, np.r_[np.arange(0, 3000, 2), np.arange(1, 3000, 2)])] + [(4, [HUB, 3000 + j]) for j in range(HUB_NEW)]
                         + [(4, [HUB, 2000 + j]) for j in range(20)] + [(3 + j % 2, [HUB, 1500 + j]) for j in range(50)], 5, f)
    return base, upd


def update_rows(upd, d, grown):
    """the update's edges per row of the grown host master, old and new alike (its own build's rows, renumbered): the
    items of k_append_isnew's flags lie in this order"""
    alone = host_master(dict(upd, d=d))
    newid = np.full(len(upd["repeated"]), -1, np.int64)
    newid[grown[4]] = np.arange(len(grown[4]))
    rows = np.zeros(len(grown[4]), np.int64)
    rows[newid[alone[4]]] = np.diff(alone[1][0])
    return rows


EXTRAS_BASE, EXTRAS_UPDATE = 40, 30


@functools.lru_cache(maxsize=None)
def extras_parts():
    """every organism: the adjacency 0-1 three times, then 12 other families.  Entry (0, 1) has EXTRAS_BASE extras and
    gains EXTRAS_UPDATE, the update's organisms 40 .. 69 on both sides of the word that ends with organism 63"""
    rng = np.random.default_rng(57)
    f = 30
    make = lambda orgs, d: contigs_orders([(o, np.r_[[0, 1, 0, 1], 2 + rng.permutation(f - 2)[:12]]) for o in orgs], d, f)
    return make(range(EXTRAS_BASE), EXTRAS_BASE), make(range(EXTRAS_BASE, EXTRAS_BASE + EXTRAS_UPDATE), EXTRAS_BASE + EXTRAS_UPDATE)


KEY_BITS_PARTS = (4090, 31, 4100, 33)        # families and organisms of the base, then of base + update


@functools.lru_cache(maxsize=None)
def key_bits_parts():
    """an append that takes the families over 4 096 and the organisms over 32: the update's keys are wider in both
    fields than the ones the base was built with"""
    from tests.orders_util import synthetic_orders
    n0, d0, n1, d1 = KEY_BITS_PARTS
    base = synthetic_orders(n0, d0, 58, density=0.2, p_repeat=0.0)
    upd = part_of(synthetic_orders(n1, d1, 59, density=1.0, p_repeat=0.0), d0, d1)
    return base, upd


TRIPLE_STAGES = (30, 45, 70, 100)            # the organisms of the base and after each of three appends


@functools.lru_cache(maxsize=None)
def triple_parts():
    """300 families x 100 sparse organisms cut at TRIPLE_STAGES: every append brings new families and a wider
    edge_bits stride, and the last one starts from a master of 70 organisms that an append made"""
    from tests.orders_util import synthetic_orders
    o = synthetic_orders(300, TRIPLE_STAGES[-1], 60, density=0.05)
    cuts = (0,) + TRIPLE_STAGES
    parts = [part_of(o, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    parts[0] = dict(parts[0], d=TRIPLE_STAGES[0])
    return parts


@functools.lru_cache(maxsize=None)
def triple_masters():
    parts = triple_parts()
    out = [host_master(parts[0])]
    for u, lo, hi in zip(parts[1:], TRIPLE_STAGES[:-1], TRIPLE_STAGES[1:]):
        out.append(host_append(out[-1], 300, u, hi - lo))
    return out


COUNT_BOUND = 1 << 24                        # an entry's summed count may not pass it (a float weight would not be exact)


def alternating_orders(links, org, d):
    """one contig 0 1 0 1 ... of links + 1 genes in organism org: entry (0, 1) counts `links` there"""
    genes = np.zeros(links + 1, np.int32)
    genes[1::2] = 1
    return dict(genes=genes, contig_ptr=np.asarray([0, links + 1], np.int32), contig_org=np.asarray([org], np.int32),
                contig_circular=np.zeros(1, np.uint8), d=d, repeated=np.zeros(2, np.uint8))
