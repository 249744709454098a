"""The fixtures of tests/test_gpu_loader_shapes.py reach the branches that file is there to run, so that it cannot
quietly stop covering them: asserted on the CPU from the builders of tests/loader_util.py, the statement
(loader._batch_host, families_table_host, number_host) and the launch arithmetic of csrc/nem_gff.hip and csrc/nem_scan.hpp
-- the counts of marks, lines, genes and tokens against the scans' tile and pass and against rocPRIM's sort switches, the
key widths, what the fuzzed files hold, and the probes that pass a table's last slot."""
import collections

import numpy as np
import pytest

from pangenomenem_amd import loader
from tests import loader_util as lu
from tests import master_shapes as ms


def test_constants_are_the_shared_ones():
    assert lu.SCAN_TILE is ms.SCAN_TILE and lu.SCAN_PASS is ms.SCAN_PASS and lu.SCAN_PASS == 524288
    assert lu.LOADER_TILE == 256 * lu.MARK_BYTES and lu.SORT_ONE_BLOCK == 1024 and lu.SORT_MERGE_LIMIT == 1 << 20
    assert lu.table_slots(7) == 16 and lu.table_slots(8) == 32 and lu.table_slots(0) == 16
    assert lu.mark_counts(16 * lu.SCAN_PASS) == lu.SCAN_PASS and lu.mark_counts(16 * lu.SCAN_PASS + 1) == lu.SCAN_PASS + 1
    assert len(lu.constructed_batch(1, 1, 1, 0)[0]) >= lu.MIN_LINE


def test_construction_equals_the_statement():
    """what constructed_batch expects by construction is what _batch_host makes of its text: the million-line batches
    are too long for the statement (about 18 us a line), so they stand on this"""
    for args, kw in (((3000, 70, 3, 1), {}), ((500, 500, 2, 2), {}), ((700, 3, (1, 600, 99), 3), dict(eol=b"\r\n", first_id=12345)),
                     ((40, 5, 2, 4), dict(tail=b"##FASTA\n>c0\nACGT\nc0\tt\tCDS\t1\t2\t.\t+\t0\tID=late\n"))):
        text, fs, fe, want = lu.constructed_batch(*args, **kw)
        lu.same_batch(loader._batch_host(text, fs, fe, {}, True), want, repr(args))
        assert want["error"] is None and len(np.unique(want["start"])) < len(want["start"]) and want["start"].min() < 0      # ties, negatives
        per_file = [np.flatnonzero(want["file"] == f) for f in range(len(fs))]
        assert all(len(p) for p in per_file)
    text, fs, fe, want = lu.constructed_batch(3000, 70, 3, 1)
    order = np.argsort(want["span_off"][lu.loader.SPAN_ID])                  # line order: the contigs are interleaved
    assert (np.diff(want["contig"][order]) != 0).mean() > 0.5


@pytest.mark.parametrize("g,contigs,files", lu.SORT_CASES)
def test_sort_cases_reach_their_paths(g, contigs, files):
    """rocPRIM sorts up to SORT_ONE_BLOCK items in one block, up to SORT_MERGE_LIMIT by merging, more by Onesweep; the
    scans carry beyond SCAN_PASS items; the sort's key has 32 + bits_for(contigs) bits"""
    assert contigs <= g
    sizes = [c[0] for c in lu.SORT_CASES]
    assert sizes == [lu.SORT_ONE_BLOCK, lu.SORT_ONE_BLOCK + 1, 4096, lu.SORT_MERGE_LIMIT, lu.SORT_MERGE_LIMIT + 1]
    assert lu.SORT_ONE_BLOCK < 4096 < lu.SORT_MERGE_LIMIT
    # lines = genes here, and a line is at least MIN_LINE bytes: the counts marks() scans, from the text's length
    counts = lu.mark_counts(lu.MIN_LINE * g)
    if g >= lu.SORT_MERGE_LIMIT:
        assert ms.scan_passes(g) >= 2                                        # ranks() of the lines' and of the genes' flags carries
        assert ms.scan_passes(counts) >= 3                                   # marks() carries more than once
        assert lu.table_slots(g) == 1 << 22
    else:
        assert ms.scan_passes(g) == 1 and ms.scan_tiles(g) in (1, 2)
    assert [lu.key_bits(c[1]) for c in lu.SORT_CASES[-2:]] == [12, 13] and 1 << 12 == lu.SORT_CASES[-2][1] == lu.SORT_CASES[-1][1] - 1
    if g <= 4096:                                                            # (the large ones: by the arithmetic above)
        text, fs, fe, want = lu.constructed_batch(g, contigs, files, g)
        assert len(want["file"]) == g and want["n_contigs"] == contigs and len(text) >= lu.MIN_LINE * g


def test_contig_counts_at_a_power_of_two():
    assert lu.key_bits(1024) == 10 and lu.key_bits(1025) == 11


@pytest.mark.parametrize("variant", ["plain", "edge", "crlf"])
def test_fasta_batches_cross_a_pass_of_marks(variant):
    text, fs, fe, want = lu.fasta_batch(variant)
    counts = lu.mark_counts(len(text))
    assert lu.SCAN_PASS < counts < 2 * lu.SCAN_PASS and ms.scan_passes(counts) == 2
    assert len(want["file"]) == sum(lu.FASTA_CDS) and np.bincount(want["file"]).tolist() == list(lu.FASTA_CDS)
    assert fs[1] > lu.MARK_BYTES * lu.SCAN_PASS                              # every line of file 1 lies behind the carry
    eol = b"\r\n" if variant == "crlf" else b"\n"
    at = int(want["fasta_off"][0])
    assert text[at:at + 7 + len(eol)] == b"##FASTA" + eol and text[at - len(eol):at] == eol and want["fasta_off"][1] == fe[1]
    if variant == "edge":
        assert 0 <= at - lu.MARK_BYTES * lu.SCAN_PASS < lu.MARK_BYTES and at == lu.FASTA_AT      # the first count of the second pass
    else:
        assert at < lu.LOADER_TILE * 16 and text.count(eol, at) > 100000      # the sequence lines are lines to marks()
    assert (b"\r" in text) == (variant == "crlf")


@pytest.mark.parametrize("newline", [True, False])
def test_families_table_crosses_a_pass_of_tokens(newline):
    table, first = lu.families_table(newline)
    tokens = table.split()
    assert len(tokens) == 2 * lu.TABLE_LINES + 2 > lu.SCAN_PASS and ms.scan_passes(len(tokens)) == 2
    assert table.endswith(tokens[-1]) != newline
    mid = lu.SCAN_PASS // 2
    # one token more before the pass than two a line: the family of line mid is token SCAN_PASS + 1, its gene the next
    assert tokens[lu.SCAN_PASS - 1:lu.SCAN_PASS + 3] == [b"F%d" % ((mid - 1) % 1000), b"g%d" % (mid - 1), b"F%d" % (mid % 1000), b"g%d" % mid]
    assert first < mid - 2000 and mid + 2000 < first + lu.TABLE_GENES         # the batch has genes on either side, and the two listed twice
    gene_tf, spans = loader.families_table_host(table)
    assert len(spans) == 1000
    assert gene_tf[b"g%d" % (mid + 2000)] == (mid + 2000) % 1000 != (mid - 1003) % 1000      # the later line wins, either way round
    assert gene_tf[b"g%d" % (mid - 2000)] == (mid + 1001) % 1000 != (mid - 2000) % 1000


def test_number_cases_plant_what_they_say():
    assert lu.NUMBER_SIZES == (1, 1023, 1024, 1025, lu.SCAN_TILE - 1, lu.SCAN_TILE + 1, lu.SCAN_PASS, lu.SCAN_PASS + 1, lu.SORT_MERGE_LIMIT + 1)
    assert lu.NUMBER_ORGS == (1, 2, 3, 256, 257) and [lu.key_bits(n) for n in lu.NUMBER_ORGS] == [1, 1, 2, 8, 9]
    # the sort of the pairs: one block, merging, Onesweep; ranks() of the first genes: one tile, two, one pass, two
    assert [g <= lu.SORT_ONE_BLOCK for g in lu.NUMBER_SIZES] == [True] * 3 + [False] * 6
    assert [g <= lu.SORT_MERGE_LIMIT for g in lu.NUMBER_SIZES] == [True] * 8 + [False]
    assert [ms.scan_tiles(g) for g in lu.NUMBER_SIZES[:6]] == [1, 1, 1, 1, 1, 2]
    assert [ms.scan_passes(g) for g in lu.NUMBER_SIZES] == [1] * 7 + [2, 3]
    for g in (lu.SCAN_TILE + 1, lu.SCAN_PASS + 1):
        for n_orgs in (1, 257):
            for lim in (1, 3):
                name, org, n_names, planted = lu.number_case(g, n_orgs, lim, 7)
                assert len(name) == len(org) == g and np.all(np.diff(org) >= 0) and org.max() < n_orgs and 0 <= name.min() and name.max() < n_names
                genes, order, rep = loader.number_host(name, org, n_names, n_orgs, lim)
                ids = {int(n): k for k, n in enumerate(order)}
                assert all(rep[ids[n]] == want for n, want in planted.items()) and sum(planted.values()) >= 1
                key = org.astype(np.int64) << 32 | genes                     # the sorted pairs: a planted run across 255 | 256
                key.sort()
                fam = genes[255]
                run = np.flatnonzero(key == fam)
                assert run.tolist() == list(range(255, 256 + lim)) and rep[fam] == 1
                if g > lu.SCAN_PASS:
                    run = np.flatnonzero(key == key[lu.SCAN_TILE - 1])
                    assert run.tolist() == list(range(lu.SCAN_TILE - 1, lu.SCAN_TILE + lim)) and len(planted) >= 4
                    if n_orgs > 1:                                           # lim + 1 occurrences over two organisms: not repeated
                        split = [n for n, want in planted.items() if not want and (name == n).sum() == lim + 1]
                        assert len(split) == 1 and sorted(org[name == split[0]].tolist()) == [0] * lim + [1]


def test_fuzzed_files_hold_what_the_tests_need():
    """by the statement alone: 40 files, between a quarter and a half of them with an error, every code the first error
    of some file, ten error-free files of more than 50 genes; every line end, and bytes >= 0x80 and NUL, occur"""
    files, table = lu.fuzz_set()
    assert len(files) == len(lu.FUZZ_SEEDS) == 40
    gene_tf, _ = loader.families_table_host(table)
    codes, clean = collections.Counter(), 0
    for data in files:
        r = loader._batch_host(*lu.joined([data]), gene_tf, False)
        if r["error"] is not None:
            codes[r["error"][2]] += 1
        elif len(r["file"]) > 50:
            clean += 1
            assert (r["fam"] >= 0).all()
    assert 10 <= sum(codes.values()) <= 20 and sorted(codes) == list(range(1, 9)) and clean >= 10, (codes, clean)
    whole = b"\n".join(files)
    for piece in (b"\r\n", b"\xc2\x85", b"\xc2\xa0", b"\xff", b"\x00", b";;", b"-2147483648", b"+2147483647", b"007", b"-0", b"\x1c"):
        assert piece in whole, piece
    assert any(b"\r" in d.replace(b"\r\n", b"") for d in files)              # a lone \r
    assert sum(1 for d in files if d[-1:] not in b"\r\n") >= 5               # a last line without a terminator
    assert set(lu.fuzz_file(np.random.RandomState(1), p_error=0.0)[0]) >= set(b"\t\n=;")


def test_hash_restatement_and_probe_wraps():
    assert lu.py_hash_bytes(b"") == lu.py_hash_bytes(b"", 0) != lu.py_hash_bytes(b"", 1) and lu.py_hash_bytes(b"\xff", 0, 7) < 8
    assert lu.py_hash_bytes(b"a\x00") != lu.py_hash_bytes(b"a")
    # keys made to collide in slot 14 of 16: the third passes the last slot; looking for a fourth does too
    at14 = [b"k%d" % k for k in range(2000) if lu.py_hash_bytes(b"k%d" % k) & 15 == 14][:4]
    assert not lu.probe_wraps(at14[:2], 16) and lu.probe_wraps(at14[:3], 16) and lu.probe_wraps(at14[:2] + at14[:2], 16) is False
    assert lu.probe_wraps(at14[:2], 16, finds=at14[3:]) and not lu.probe_wraps(at14[:2], 16, finds=at14[:2])
    assert not lu.probe_wraps([(at14[0], 0), (at14[0], 0)], 16)


def test_wrap_set_wraps():
    """Whether a probe of the device passes its table's last slot is read off the restated hash: no output of the device
    can confirm the restatement.  That is why the set is 200 batches of 7 items in 16-slot tables: a wrap somewhere is
    near certain even if the restatement were off."""
    gffs, whole, lines = lu.wrap_set()
    slots = lu.table_slots(lu.WRAP_GENES)
    assert len(gffs) == lu.WRAP_BATCHES == 200 and slots == 16
    gene_tf, _ = loader.families_table_host(whole)
    wraps = collections.Counter()
    for o, data in enumerate(gffs):
        text, fs, fe = lu.joined([data])
        r = loader._batch_host(text, fs, fe, gene_tf, False)
        assert r["error"] is None and len(r["file"]) == lu.WRAP_GENES
        in_line = np.argsort(r["span_off"][loader.SPAN_ID])
        span = lambda j: [text[r["span_off"][j, i]:r["span_off"][j, i] + r["span_len"][j, i]] for i in in_line]
        ids, contigs = span(loader.SPAN_ID), span(loader.SPAN_CONTIG)
        wraps["contig"] += lu.probe_wraps(contigs, slots)                    # (one file a batch: every salt is 0)
        wraps["id"] += lu.probe_wraps(ids, slots)
        for which in ("most", "half"):
            tokens = lines[which][o].split()
            assert len(tokens) == 7 and lu.table_slots(len(tokens)) == slots
            known = [i for i in ids if i in tokens[1:]]
            assert len(known) == (6 if which == "most" else 3)
            wraps[which] += lu.probe_wraps(tokens[1:], slots, finds=ids)
            wraps[which + "_miss"] += lu.probe_wraps(tokens[1:], slots, finds=[i for i in ids if i not in known]) and \
                not lu.probe_wraps(tokens[1:], slots)
    assert wraps["contig"] >= 10 and wraps["id"] >= 10 and wraps["most"] >= 10 and wraps["half"] >= 10 and wraps["half_miss"] >= 10, wraps
