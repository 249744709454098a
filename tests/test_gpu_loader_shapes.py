"""The loader on the device (csrc/nem_gff.hip) at the sizes and bytes where its kernels take another path, against its
statement (loader._batch_host, families_table_host, number_host, load_arrays_host) or, where the statement is too slow,
against what tests/loader_util.py's constructed_batch expects by construction: rocPRIM's three sort paths by gene count,
the scans of marks(), ranks() and the families table beyond one pass of k_scan_partials, nemgpu_gff_number's sort and
its look lim places on, fuzzed files with every line end, padding, byte and error, the int32 edges and the bytes >= 0x80
through the whole load, probes that pass a table's last slot, and key widths at and past a power of two.
tests/test_loader_shapes_host.py asserts on the CPU that every fixture here reaches the branch it is named for.
Every comparison is exact."""
import numpy as np
import pytest

from pangenomenem_amd import loader
from tests import loader_util as lu
from tests.loader_util import cds_line, error_of, same_batch, same_loaded, write_set

pytestmark = pytest.mark.gpu

# The string hash of the colliding run at SORT_MERGE_LIMIT + 1 genes keeps this many bits.  With 3 bits, or with 16, the
# million distinct IDs form one cluster of a million slots and every insert walks half of it: about 5e11 probes, minutes.
# With 20 bits the IDs fall into the lowest quarter of the 2^22 slots at a load of 1 there: the probes are long (hundreds
# of slots on average) and the run still takes well under a second.
LARGE_HASH_BITS = 20


def run_batch(fam, hash_bits, text, fs, fe, infer):
    dev = loader._Device(fam, 0, hash_bits)
    try:
        return dev.batch(text, fs, fe, infer), dev.family_spans
    finally:
        dev.close()


def test_tile(gpu_lib):
    assert loader.gff_info()["tile"] == lu.LOADER_TILE


@pytest.mark.parametrize("g,contigs,files", lu.SORT_CASES)
def test_sort_paths(gpu_lib, g, contigs, files):
    """one block, merge sort and Onesweep of rocPRIM's radix sort; at the two largest sizes ranks() and marks() carry"""
    text, fs, fe, want = lu.constructed_batch(g, contigs, files, g)
    for bits in (0, 3) if g <= 4096 else (0, LARGE_HASH_BITS) if g > lu.SORT_MERGE_LIMIT else (0,):
        got, _ = run_batch(b"F x\n", bits, text, fs, fe, True)
        same_batch(got, want, "%d genes, hash bits %d" % (g, bits))
        assert got["error"] is None


@pytest.mark.parametrize("variant", ["plain", "edge", "crlf"])
def test_marks_across_a_pass(gpu_lib, variant):
    text, fs, fe, want = lu.fasta_batch(variant)
    stated = loader._batch_host(text, fs, fe, {}, True)
    got, _ = run_batch(b"", 0, text, fs, fe, True)
    same_batch(got, stated, variant)
    same_batch(got, want, variant + ", by construction")


@pytest.mark.parametrize("newline", [True, False], ids=["newline", "no_newline"])
def test_families_table_across_a_pass(gpu_lib, newline):
    table, first = lu.families_table(newline)
    gene_tf, spans = loader.families_table_host(table)
    text, fs, fe, _ = lu.constructed_batch(lu.TABLE_GENES, 11, 2, 9, first_id=first)
    want = loader._batch_host(text, fs, fe, gene_tf, False)
    assert want["error"] is None and len(np.unique(want["fam"])) == 1000
    got, got_spans = run_batch(table, 0, text, fs, fe, False)
    assert got_spans.dtype == spans.dtype and got_spans.shape == spans.shape and np.array_equal(got_spans, spans)
    same_batch(got, want, "newline %d" % newline)
    text, fs, fe, _ = lu.constructed_batch(3, 1, 1, 9, first_id=lu.TABLE_LINES - 2)      # the table's last gene, and one it does not have
    same_batch(run_batch(table, 0, text, fs, fe, True)[0], loader._batch_host(text, fs, fe, gene_tf, True), "the last token")
    same_batch(run_batch(table, 0, text, fs, fe, False)[0], loader._batch_host(text, fs, fe, gene_tf, False), "the last token", keys=["error"])


def number_combos(g):
    """(n_orgs, lim): all of them up to SCAN_TILE + 1 genes; beyond, where number_host takes a quarter of a second a
    call, every organism count and every lim once and the widest key with both small lims"""
    lims = (1, 3, g - 1, g)
    if g <= lu.SCAN_TILE + 1:
        return [(n, lim) for n in lu.NUMBER_ORGS for lim in lims]
    return [(1, 1), (2, 3), (3, g - 1), (256, g), (257, 3), (257, 1), (256, 3)]


@pytest.mark.parametrize("g", lu.NUMBER_SIZES)
def test_number_at_sizes(gpu_lib, g):
    dev = loader._Device(b"", 0, 0)
    try:
        for n_orgs, lim in number_combos(g):
            name, org, n_names, planted = lu.number_case(g, n_orgs, lim, g + n_orgs)
            want = loader.number_host(name, org, n_names, n_orgs, lim)
            got = dev.number(name, org, n_names, n_orgs, lim)
            for a, b, what in zip(got, want, ("genes", "order", "repeated")):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "%d genes, %d organisms, lim %d: %s" % (g, n_orgs, lim, what)
            ids = {int(n): k for k, n in enumerate(got[1])}
            assert all(got[2][ids[n]] == rep for n, rep in planted.items())
        for lim in (g - 1, g):                                               # one family, one organism: g occurrences
            name, org = np.full(g, 2, np.int32), np.zeros(g, np.int32)
            want, got = loader.number_host(name, org, 5, 1, lim), dev.number(name, org, 5, 1, lim)
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want)) and int(got[2][0]) == (1 if 0 < lim < g else 0)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def fuzz():
    """the fuzzed files, their families table, and the statement of every file alone"""
    files, table = lu.fuzz_set()
    gene_tf, _ = loader.families_table_host(table)
    alone = [loader._batch_host(*lu.joined([d]), gene_tf, False) for d in files]
    return files, table, gene_tf, alone


@pytest.mark.parametrize("hash_bits", [0, 2])
def test_fuzz_batches(gpu_lib, fuzz, hash_bits):
    files, table, gene_tf, _ = fuzz
    dev = loader._Device(table, 0, hash_bits)
    try:
        for k in range(len(files)):
            for n in (1, 2, 5):
                text, fs, fe = lu.joined([files[(k + j) % len(files)] for j in range(n)])
                want = loader._batch_host(text, fs, fe, gene_tf, False)
                got = dev.batch(text, fs, fe, False)
                what = "seed %d, %d files, hash bits %d" % (lu.FUZZ_SEEDS[k], n, hash_bits)
                # (a refused batch: the device keeps a duplicate's row, the statement does not, and the load raises either way)
                same_batch(got, want, what, keys=None if want["error"] is None else ["error"])
    finally:
        dev.close()


def test_fuzz_loads(gpu_lib, fuzz, tmp_path):
    files, table, _, alone = fuzz
    good = [k for k, r in enumerate(alone) if r["error"] is None][:10]
    bad = [k for k, r in enumerate(alone) if r["error"] is not None]
    bad = [next(k for k in bad if alone[k]["error"][2] == code) for code in (loader.E_FIELDS3, loader.E_ATTR, loader.E_UNKNOWN, loader.E_END, loader.E_DUP)]
    assert len(good) == 10
    orgs, fam = write_set(tmp_path / "good", [files[k] for k in good], table)
    want = loader.load_arrays_host(orgs, fam, lim_occurence=1)
    assert want.families_repeted
    for options in (dict(), dict(batch_bytes=1, _hash_bits=2)):
        same_loaded(loader.load_files(orgs, fam, lim_occurence=1, **options), want, repr(options))
    for k in bad:
        orgs, fam = write_set(tmp_path / ("bad%d" % k), [files[good[0]], files[k], files[good[1]]], table)
        want = error_of(lambda: loader.load_arrays_host(orgs, fam))
        assert want is not None and "o1.gff: line %d" % (alone[k]["error"][1] + 1) in want[1]
        for options in (dict(), dict(batch_bytes=1)):
            assert error_of(lambda: loader.load_files(orgs, fam, **options)) == want, (k, options)


def test_numbers_python_would_take_are_refused_on_the_device(gpu_lib, tmp_path):
    """the tokens of test_loader_host's test of that name, a number beyond int64, and 2^64 + 5, which an int64 that
    wraps takes for 5"""
    for k, tok in enumerate(lu.BAD_NUMBERS + (b"18446744073709551621", b"-18446744073709551621")):
        for field, word in ((b"\t1\t", "START"), (b"\t51\t", "END")):
            line = cds_line(b"c", 1, b"a").replace(field, b"\t" + tok + b"\t")
            orgs, fams = write_set(tmp_path / ("%d%s" % (k, word)), [line], b"F a\n")
            want = error_of(lambda: loader.load_arrays_host(orgs, fams))
            assert want is not None and want[0] is ValueError and "line 1" in want[1] and word in want[1], (tok, want)
            assert error_of(lambda: loader.load_files(orgs, fams)) == want, tok


def test_int32_edges_on_the_device(gpu_lib, tmp_path):
    """INT_MIN and INT_MAX through the sign-flipped sort key: one contig whose starts are the edges and their neighbours"""
    starts = [2147483647, -2147483648, 0, -1, 2147483646, -2147483647, 1, -2147483648, 2147483647]
    lines = [cds_line(b"c", 1, b"g%d" % k).replace(b"\t1\t51\t", b"\t%+d\t%d\t" % (s, -s - 1)) for k, s in enumerate(starts)]
    orgs, fams = write_set(tmp_path, [b"\n".join(lines)], b"F " + b" ".join(b"g%d" % k for k in range(len(starts))) + b"\n")
    want = loader.load_arrays_host(orgs, fams)
    assert want.orders["starts"].tolist() == sorted(starts) and list(want.gene_ids)[:2] == ["g1", "g7"]
    assert want.orders["ends"].tolist() == [-s - 1 for s in sorted(starts)]
    same_loaded(loader.load_files(orgs, fams), want, "edges")


def test_high_bytes_and_nul_on_the_device(gpu_lib, tmp_path):
    """NBSP, NEL, 0xff and NUL are token bytes: in IDs, contig names and the families table, ended by the text's end"""
    gene = "g\u00a0\u0085x".encode()
    genes = [gene, gene + b"\xff", gene + b"\xfe", b"\x00", b"\x00\x00", b"\xc2", b"\xa0"]
    gff = b"\n".join(cds_line(c, 1 + k % 2, g) for k, (g, c) in enumerate(zip(genes, [b"\xc2\x85", b"\xc2\x85\x00", b"\xc2\xa0"] * 3)))
    table = b"F\xff " + b" ".join(genes[:4]) + b"\nF\xfe\t" + b"\x1f".join(genes[4:])        # no newline: the last token ends the text
    orgs, fams = write_set(tmp_path, [gff, gff], table)
    want = loader.load_arrays_host(orgs, fams, lim_occurence=3)
    assert list(want.gene_ids)[0] == gene.decode() and len(want.families) == 2 and len(want.families_repeted) == 1
    assert np.diff(want.orders["contig_ptr"]).tolist() == [3, 2, 2] * 2
    for options in (dict(), dict(_hash_bits=1), dict(batch_bytes=1)):
        same_loaded(loader.load_files(orgs, fams, lim_occurence=3, **options), want, repr(options))


def test_wraparound_loads(gpu_lib, tmp_path):
    """200 batches of 7 genes on 7 contigs: 16-slot contig and ID tables, the full hash"""
    gffs, whole, _ = lu.wrap_set()
    orgs, fams = write_set(tmp_path, gffs, whole)
    want = loader.load_arrays_host(orgs, fams, lim_occurence=1)
    same_loaded(loader.load_files(orgs, fams, lim_occurence=1, batch_bytes=1), want, "a file a batch")


@pytest.mark.parametrize("which", ["most", "half"])
def test_wraparound_family_tables(gpu_lib, which):
    """per organism a families table of 7 tokens, a 16-slot gene table: it knows 6 of the 7 genes, or 3 of them and 3
    strangers, so that a lookup that misses walks past the last slot to the empty one behind it"""
    gffs, _, lines = lu.wrap_set()
    for o, data in enumerate(gffs):
        text, fs, fe = lu.joined([data])
        gene_tf, spans = loader.families_table_host(lines[which][o])
        got, got_spans = run_batch(lines[which][o], 0, text, fs, fe, True)
        same_batch(got, loader._batch_host(text, fs, fe, gene_tf, True), "%s %d" % (which, o))
        assert np.array_equal(got_spans, spans) and (got["fam"] >= 0).sum() == (6 if which == "most" else 3)


@pytest.mark.parametrize("contigs", [1024, 1025])
def test_contig_counts_at_a_power_of_two(gpu_lib, contigs):
    rng = np.random.RandomState(contigs)
    lines = [cds_line(b"k%d" % c, int(rng.randint(-3, 3)), b"g%d_%d" % (c, j)) for c in rng.permutation(contigs) for j in range(2)]
    text, fs, fe = lu.joined([b"\n".join(lines[j] for j in rng.permutation(len(lines))) + b"\n"])
    want = loader._batch_host(text, fs, fe, {}, True)
    assert want["n_contigs"] == contigs and np.bincount(want["contig"]).tolist() == [2] * contigs
    for bits in (0, 4):
        same_batch(run_batch(b"", bits, text, fs, fe, True)[0], want, "%d contigs, hash bits %d" % (contigs, bits))
