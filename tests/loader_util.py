"""What tests/test_loader_host.py and tests/test_gpu_loader.py share: the recorded loader fixtures
(tests/golden/loader/, written by tests/golden/make_loader.py), the comparison of a Loaded with a recording and of two
Loaded with each other, and the sets of files the device tests are sized around.  Then what
tests/test_gpu_loader_shapes.py and tests/test_loader_shapes_host.py share: the sizes at which the loader's kernels take
another path, batches whose result is known by construction, the large families table, fuzzed files, the wrap-around
set with the restated string hash, and genes to number."""
import glob
import json
import os
from collections import OrderedDict

import numpy as np

from pangenomenem_amd import loader
from pangenomenem_amd.chunks import orders_from_annotations
from tests.master_shapes import SCAN_PASS, SCAN_TILE, key_bits, scan_passes       # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(os.path.dirname(p) for p in glob.glob(os.path.join(HERE, "golden", "loader", "*", "expected.json")))
ORDER_KEYS = ("genes", "contig_ptr", "contig_org", "contig_circular", "repeated")
# the reference's exception -> ours (an IndexError or an exit() of the reference is a ValueError that names the place)
RAISES = {"KeyError": KeyError, "IndexError": ValueError, "ValueError": ValueError, "SystemExit": ValueError}


def case_id(path):
    return os.path.basename(path)


def recorded(path):
    with open(os.path.join(path, "expected.json")) as f:
        return json.load(f)


def paths(path):
    return os.path.join(path, "organisms.tsv"), os.path.join(path, "families.tsv")


def annotations_of(rec):
    return OrderedDict((org, OrderedDict((contig, OrderedDict((gene, info) for gene, info in genes)) for contig, genes in contigs))
                       for org, contigs in rec["annotations"])


def nested_lists(ann):
    """annotations with their dict orders made explicit"""
    return [[org, [[contig, [[gene, list(info)] for gene, info in annot.items()]] for contig, annot in contigs.items()]] for org, contigs in ann.items()]


def equals_recording(ld, rec, what):
    """the contract: annotations (dict orders included), circular sizes, repeated families and organisms are the
    reference's, and orders is orders_from_annotations of the reference's output, array for array"""
    assert list(ld.organisms) == rec["organisms"], what
    assert nested_lists(ld.annotations()) == rec["annotations"], what + ": annotations"
    assert ld.circular_contig_size == rec["circular_contig_size"], what + ": circular_contig_size"
    assert list(ld.circular_contig_size) == list(rec["circular_contig_size"]), what + ": circular_contig_size order"
    assert sorted(ld.families_repeted) == rec["families_repeted"], what + ": families_repeted"
    want = orders_from_annotations(annotations_of(rec), rec["organisms"], rec["circular_contig_size"], rec["families_repeted"])
    for k in ORDER_KEYS:
        assert ld.orders[k].dtype == want[k].dtype and np.array_equal(ld.orders[k], want[k]), what + ": orders[%s]" % k
    assert ld.orders["d"] == want["d"] and ld.orders["families"] == want["families"] and ld.orders["organisms"] == want["organisms"], what
    assert ld.families == want["families"], what
    infos = [info for _, contigs in rec["annotations"] for _, genes in contigs for _, info in genes]
    assert ld.orders["starts"].tolist() == [i[2] for i in infos] and ld.orders["ends"].tolist() == [i[3] for i in infos], what
    assert ld.orders["lengths"].tolist() == [i[3] - i[2] for i in infos], what
    assert ld.orders["strand"].tolist() == [ord(i[4][0]) if i[4] else 0 for i in infos] and ld.orders["strand"].dtype == np.uint8, what
    cnames = [contig for _, contigs in rec["annotations"] for contig, _ in contigs]
    assert list(ld.contig_names) == cnames, what
    assert ld.orders["contig_sizes"].tolist() == [rec["circular_contig_size"].get(c, -1) for c in cnames], what
    for k in ("starts", "ends", "lengths", "contig_sizes"):
        assert ld.orders[k].dtype == np.int32, what
    assert list(ld.gene_ids) == [gene for _, contigs in rec["annotations"] for _, genes in contigs for gene, _ in genes], what
    assert list(ld.gene_names) == [i[5] for i in infos] and list(ld.products) == [i[6] for i in infos], what


def same_loaded(got, want, what):
    """two loads, array for array and span for span"""
    a, b = got.arrays(), want.arrays()
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), what + ": " + k
    assert got.organisms == want.organisms and got.families == want.families, what
    assert got.families_repeted == want.families_repeted and got.circular_contig_size == want.circular_contig_size, what
    assert list(got.circular_contig_size) == list(want.circular_contig_size), what


def error_of(call):
    """(type, message) of what the call raises, None if it returns"""
    try:
        call()
    except Exception as e:                                # noqa: BLE001
        return type(e), str(e)
    return None


def write_set(directory, gffs, families, circular=None):
    """files of given bytes: gffs = [bytes per organism]; returns (organisms file, families file)"""
    os.makedirs(str(directory), exist_ok=True)
    lines = []
    for o, data in enumerate(gffs):
        with open(os.path.join(str(directory), "o%d.gff" % o), "wb") as f:
            f.write(data)
        lines.append("\t".join(["o%d" % o, "o%d.gff" % o] + list((circular or {}).get(o, ()))))
    orgs, fams = os.path.join(str(directory), "organisms.tsv"), os.path.join(str(directory), "families.tsv")
    with open(orgs, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(fams, "wb") as f:
        f.write(families)
    return orgs, fams


def cds_line(contig, start, gene, pad=b""):
    return b"\t".join([contig, b"t", b"CDS", b"%d" % start, b"%d" % (start + 50), b".", b"+", b"0", b"ID=" + gene + b";Name=n" + pad])


# ---- the shapes of tests/test_gpu_loader_shapes.py (tests/test_loader_shapes_host.py holds them to their branches) ------
LOADER_TILE = 4096                   # kGffTile: the bytes a block of k_mark_count / k_mark_emit marks (gff_info()["tile"])
MARK_BYTES = 16                      # kGffBytes: the bytes a thread marks; marks() scans one count per MARK_BYTES of text
# rocPRIM's dispatch limits, read from the installed rocprim/device/device_radix_sort.hpp: up to SORT_ONE_BLOCK items
# are sorted in one block, up to SORT_MERGE_LIMIT by the merge sort, more by Onesweep.  With another rocPRIM the sizes
# below are still valid inputs and merely no longer straddle a switch.
SORT_ONE_BLOCK = 1024
SORT_MERGE_LIMIT = 1 << 20
MIN_LINE = 26                        # the shortest line of constructed_batch: c0 t CDS 0 90 . + 0 ID=g0 and its '\n'

# (genes, contigs, files) of the sort-path batches: the contigs of the two largest put bits_for at and past a power of two
SORT_CASES = ((SORT_ONE_BLOCK, 37, 2), (SORT_ONE_BLOCK + 1, 37, 2), (4096, 70, 3), (SORT_MERGE_LIMIT, 4096, 3),
              (SORT_MERGE_LIMIT + 1, 4097, 3))
FASTA_CDS = (2000, 20000)            # the CDS lines of the two files of the marks-across-a-pass batches
FASTA_AT = MARK_BYTES * SCAN_PASS + 5            # where the ##FASTA line of the "edge" variant starts
TABLE_LINES = 300000                 # the lines of the large families table: two tokens each
TABLE_GENES = 5000                   # the genes of its batch, around the line whose family is token SCAN_PASS
NUMBER_SIZES = (1, SORT_ONE_BLOCK - 1, SORT_ONE_BLOCK, SORT_ONE_BLOCK + 1, SCAN_TILE - 1, SCAN_TILE + 1, SCAN_PASS, SCAN_PASS + 1,
                SORT_MERGE_LIMIT + 1)
NUMBER_ORGS = (1, 2, 3, 256, 257)
FUZZ_SEEDS = tuple(range(40))
FUZZ_ERROR = 0.4                     # the probability that a fuzzed file carries an error line
WRAP_BATCHES, WRAP_GENES = 200, 7    # the wrap-around set: table_slots(7) = 16


def mark_counts(n_bytes):
    """the counts marks() scans over a text of n_bytes"""
    return -(-n_bytes // MARK_BYTES)


def table_slots(items):
    """table_slots (nem_gff.hip): a power of two, at least 16 and more than twice the items"""
    s = 16
    while s < 2 * items + 1:
        s <<= 1
    return s


def _dlen(v):
    """the bytes of %d of every v"""
    v = np.asarray(v, np.int64)
    a = np.abs(v)
    return (v < 0).astype(np.int64) + 1 + sum((a >= 10 ** k).astype(np.int64) for k in range(1, 11))


def constructed_batch(n_genes, n_contigs, n_files, seed, tail=b"", eol=b"\n", first_id=0):
    """A batch of CDS lines ``c%d\\tt\\tCDS\\t%d\\t%d\\t.\\t+\\t0\\tID=g%d`` with what _batch_host makes of it (the IDs in no
    families table, infer_singletons), the latter from the construction alone: n_files an int (the lines spread evenly)
    or every file's line count; n_contigs over the batch, every one present, interleaved within its file, the same names
    in every file; starts from a small range, some negative; the IDs g<first_id> onwards in line order; `tail` (empty, or
    lines of which one starts with ##FASTA) appended to file 0.  Returns (text, file_start, file_end, expected)."""
    rng = np.random.RandomState(seed)
    per_file = np.asarray([n_genes // n_files + (f < n_genes % n_files) for f in range(n_files)] if isinstance(n_files, int) else n_files, np.int64)
    nf = len(per_file)
    assert per_file.sum() == n_genes and n_contigs <= n_genes
    lo = np.concatenate([[0], np.cumsum(per_file)])
    # the contigs of a file: a share of n_contigs by its lines, at least one and at most its lines
    share = np.maximum(1, np.minimum(per_file, per_file * n_contigs // max(n_genes, 1)))
    f = 0
    while share.sum() != n_contigs:                       # (move the remainder to where there is room)
        step = 1 if share.sum() < n_contigs else -1
        if 1 <= share[f] + step <= per_file[f]:
            share[f] += step
        f = (f + 1) % nf
    file = np.repeat(np.arange(nf), per_file)
    name = np.zeros(n_genes, np.int64)
    for f in range(nf):
        n, c = int(per_file[f]), int(share[f])
        names = np.concatenate([rng.permutation(c), rng.randint(0, c, n - c)])     # every contig once, then any
        name[lo[f]:lo[f + 1]] = names[rng.permutation(n)]
    start = rng.randint(-40, 160, n_genes).astype(np.int64)
    end = start + 90
    ident = np.arange(n_genes, dtype=np.int64) + first_id
    line = b"c%d\tt\tCDS\t%d\t%d\t.\t+\t0\tID=g%d" + eol
    lines = [line % t for t in zip(name.tolist(), start.tolist(), end.tolist(), ident.tolist())]
    files = [b"".join(lines[lo[f]:lo[f + 1]]) + (tail if f == 0 else b"") for f in range(nf)]
    text = b"\n".join(files)
    file_start = np.cumsum([0] + [len(d) + 1 for d in files[:-1]]).astype(np.int32)
    file_end = file_start + np.asarray([len(d) for d in files], np.int32)
    # the spans from the line layout
    len_contig, len_start, len_end, len_id = 1 + _dlen(name), _dlen(start), _dlen(end), 1 + _dlen(ident)
    at_strand = len_contig + 7 + len_start + 1 + len_end + 3
    at_id = at_strand + 7
    length = at_id + len_id + len(eol)
    assert int(length.sum()) + len(tail) + nf - 1 == len(text)
    off = np.cumsum(length) - length + file + (len(tail) if nf > 1 else 0) * (file > 0)
    uniq, first, inverse = np.unique(file * (n_contigs + 1) + name, return_index=True, return_inverse=True)
    dense = np.zeros(len(uniq), np.int64)
    dense[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    contig = dense[inverse]
    by = np.lexsort((np.arange(n_genes), start, contig, file))
    span_off = np.stack([off + at_id, off + at_id, off + at_id, off + at_strand, off])[:, by].astype(np.int32)
    span_len = np.stack([len_id, 0 * len_id, 0 * len_id, 0 * len_id + 1, len_contig])[:, by].astype(np.int32)
    fasta_off = file_end.copy()
    if tail:
        k = 0 if tail.startswith(b"##FASTA") else tail.index(eol + b"##FASTA") + len(eol)
        fasta_off[0] = file_end[0] - len(tail) + k
    expected = dict(file=file[by].astype(np.int32), contig=contig[by].astype(np.int32), start=start[by].astype(np.int32), end=end[by].astype(np.int32),
                    fam=np.full(n_genes, -1, np.int32), span_off=span_off, span_len=span_len, n_contigs=len(uniq), fasta_off=fasta_off, error=None)
    assert len(uniq) == n_contigs
    return text, file_start, file_end, expected


def same_batch(got, want, what, keys=None):
    """two results of one batch, key for key (dtype, shape and values)"""
    assert sorted(got) == sorted(want), what
    for k in keys or sorted(want):
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "%s: %s" % (what, k)
        else:
            assert got[k] == want[k], "%s: %s: %r != %r" % (what, k, got[k], want[k])


def fasta_tail(variant, head_bytes):
    """What follows file 0's CDS lines (head_bytes of them) in the marks-across-a-pass batches, and its line end.
    "plain": ##FASTA, then more than 8 MiB of 60-byte sequence lines; "crlf": the same with \\r\\n ends; "edge": pragma
    lines up to byte FASTA_AT, where the ##FASTA line starts, then a few sequence lines."""
    eol = b"\r\n" if variant == "crlf" else b"\n"
    seq = b"ACGTTGCA" * 7 + b"ACGT" + eol
    if variant != "edge":
        return b"##FASTA" + eol + b">c0" + eol + seq * (MARK_BYTES * SCAN_PASS // len(seq) + 1000), eol
    pad = b"##" + b"x" * 58 + eol
    room = FASTA_AT - head_bytes
    q = room // len(pad) - 1
    last = b"##" + b"y" * (room - q * len(pad) - 2 - len(eol)) + eol
    return pad * q + last + b"##FASTA" + eol + b">c0" + eol + seq * 2000, eol


def fasta_batch(variant):
    """(text, file_start, file_end, expected) of a marks-across-a-pass batch: see fasta_tail"""
    head = constructed_batch(sum(FASTA_CDS), 31, FASTA_CDS, 5, eol=fasta_tail(variant, 0)[1])[2][0]       # (file 0's end without a tail)
    tail, eol = fasta_tail(variant, int(head))
    return constructed_batch(sum(FASTA_CDS), 31, FASTA_CDS, 5, tail=tail, eol=eol)


def families_table(newline):
    """The large families table, TABLE_LINES lines of F<k % 1000> g<k>, so that the family of line SCAN_PASS / 2 is token
    SCAN_PASS; two genes listed twice, once on either side of that token (the later family wins); its last token at the
    text's end where `newline` is false.  Returns (table, the first gene of its batch)."""
    mid = SCAN_PASS // 2
    lines = [b"F%d g%d" % (k % 1000, k) for k in range(TABLE_LINES)]
    lines[mid - 1003] += b" g%d" % (mid + 2000)           # g<mid + 2000> first in F<.. - 1003>, then in its own line behind the pass
    lines[mid + 1001] += b"\tg%d" % (mid - 2000)          # g<mid - 2000> in its own line before the pass, then in F<.. + 1001>
    return b"\n".join(lines) + (b"\n" if newline else b""), mid - TABLE_GENES // 2


# ---- the fuzzed files ---------------------------------------------------------------------------------------------------
_PAD = bytes(b for b in loader.WS if b not in b"\t\n\r")
_CONTIGS = (b"c", b"c1", b"c10", b"c11", b"c1\xff", b"c1\xfe", b"k\xc2\x85", b"k\xc2\xa0", b"c\x00", b"c\x00\x00")
_ID_ENDS = (b"", b"", b"a", b"b", b"\xff", b"\xfe", b"\x00", b"\xc2\x85", b"\xc2\xa0")
_VALUES = (b"n1", b"a b", b"\xc2\x85x", b"x\xc2\xa0y", b"\xff", b"a\x00b", b"", b"hypothetical protein")
_NUMBERS = (b"-2147483648", b"+2147483647", b"007", b"-0")
BAD_NUMBERS = (b"1_000", "١".encode(), b"+", b"1 2", b"2147483648", b"-2147483649", b"99999999999999999999")
_OTHER = (b"##gff-version 3", b"#\ta comment\t", b"##sequence-region c1 1 5000", b"##", b"c1\tt\tgene\t1\t99\t.\t+\t.\tID=gene1",
          b"c\tt\tregion", b"c1\tt\tcds\t1\t2\t.\t+\t0\tnothing", b"##FASTQ")


def fuzz_file(rng, p_error=FUZZ_ERROR):
    """One GFF file from a grammar of pieces, for the device to be held to the statement on: the three line ends and a last
    line without one; comments, pragmas and non-CDS lines; fields padded with whitespace bytes; CDS lines of 9, 10 and 12
    fields; attributes with empty parts, repeated and mixed-case keys, gene= without Name=, no product, values with
    bytes >= 0x80 and NUL; IDs and contig names that are prefixes of one another or differ in their last byte; START and
    END at the int32 edges, with signs and leading zeros.  With probability p_error one line of the file is an error
    (the codes 1 .. 8 equally likely).  Returns (the file's bytes, the IDs its families table must have)."""
    pick = lambda seq: seq[rng.randint(len(seq))]
    pad = lambda tok: (bytes(pick(_PAD) for _ in range(rng.randint(3))) + tok + bytes(pick(_PAD) for _ in range(rng.randint(3)))
                       if rng.rand() < 0.3 else tok)
    key = lambda word: word if rng.rand() < 0.5 else bytes(c ^ 32 if rng.rand() < 0.5 else c for c in word)
    number = lambda: pick(_NUMBERS) if rng.rand() < 0.15 else b"%d" % rng.randint(0, 30)
    base = rng.randint(1, 20)
    n = int(rng.choice([rng.randint(3, 40), rng.randint(55, 140)]))
    ids = [b"g%d" % (base + k) + pick(_ID_ENDS) for k in range(n)]

    def attributes(ident):
        parts = [pad(key(b"ID") + b"=" + ident)]
        if rng.rand() < 0.2:
            parts.insert(0, key(b"ID") + b"=elsewhere")                      # (the last of a key wins)
        if rng.rand() < 0.5:
            parts.append(pad(key(b"Name") + b"=" + pick(_VALUES)))
        if rng.rand() < 0.5:
            parts.insert(rng.randint(len(parts) + 1), key(b"gene") + b"=" + pick(_VALUES))
        if rng.rand() < 0.6:
            parts.append(pad(key(b"product") + b"=" + pick(_VALUES)))
        if rng.rand() < 0.3:
            parts.insert(rng.randint(len(parts) + 1), b"Note=" + pick(_VALUES))
        for _ in range(rng.randint(3)):
            parts.insert(rng.randint(len(parts) + 1), b"")                   # (;; and a ; at either end)
        return b";".join(parts)

    def cds(ident, start=None, end=None, attrs=None, fields=None):
        f = [pad(pick(_CONTIGS)), b"t", pad(b"CDS"), pad(start or number()), pad(end or number()), b".", pad(pick((b"+", b"-", b""))), b"0",
             pad(attributes(ident)) if attrs is None else attrs]
        f += [b"x", b"", b"ID=late"][:(fields or pick((9, 9, 10, 12))) - 9]
        return b"\t".join(f[:fields or len(f)])

    lines = [cds(i) for i in ids]
    for _ in range(rng.randint(1, 6)):
        lines.insert(rng.randint(len(lines) + 1), pick(_OTHER))
    known = list(ids)
    if rng.rand() < p_error:
        code, at = rng.randint(1, 9), rng.randint(1, len(lines) + 1)
        if code == loader.E_FIELDS3:
            bad = pick((b"", b"c1\tt", b"CDS"))
        elif code == loader.E_FIELDS9:
            bad = cds(b"short", fields=8)
        elif code == loader.E_ATTR:
            bad = cds(b"x", attrs=pick((b"ID=x;a=b=c", b"ID=x;flag", b"flag;ID=x", b"ID=x; ;Name=y")))
        elif code == loader.E_NOID:
            bad = cds(b"x", attrs=pick((b"Name=x;product=y", b"ID =x", b"")))
        elif code == loader.E_UNKNOWN:
            bad = cds(b"nobody" + pick(_ID_ENDS))
        elif code == loader.E_START:
            bad = cds(b"g0", start=pick(BAD_NUMBERS))
            known.append(b"g0")
        elif code == loader.E_END:
            bad = cds(b"g0", end=pick(BAD_NUMBERS))
            known.append(b"g0")
        else:
            at = rng.randint(len(lines) // 2, len(lines)) + 1                # (behind the line it repeats)
            bad = cds(pick(ids[:max(len(ids) // 3, 1)]))
        lines.insert(at, bad)
    ends = [pick((b"\n", b"\n", b"\r\n", b"\r")) for _ in lines]
    if rng.rand() < 0.3:
        ends[-1] = b""
    return b"".join(l + e for l, e in zip(lines, ends)), known


def fuzz_set():
    """the FUZZ_SEEDS' files and the families table that knows their IDs (of a few families, several IDs a line)"""
    files, lines = [], []
    for seed in FUZZ_SEEDS:
        data, known = fuzz_file(np.random.RandomState(1500 + seed))
        files.append(data)
        lines += [b"Fam%d\t" % ((seed + k) % 23) + b" ".join(known[k:k + 5]) for k in range(0, len(known), 5)]
    return files, b"\n".join(lines) + b"\n"


def joined(files):
    """a batch of whole files: (text, file_start, file_end)"""
    fs = np.cumsum([0] + [len(d) + 1 for d in files[:-1]]).astype(np.int32)
    return b"\n".join(files), fs, fs + np.asarray([len(d) for d in files], np.int32)


# ---- the tables' probes ----------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def py_hash_bytes(data, salt=0, keep=_M64):
    """hash_bytes (nem_gff.hip), restated"""
    h = 0xcbf29ce484222325 ^ (((salt & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & _M64)
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & _M64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & _M64
    h ^= h >> 33
    return h & keep


def probe_wraps(keys, slots, finds=()):
    """Whether inserting the keys (bytes, or (bytes, salt)) in order into a table of `slots` slots, equal keys sharing
    one, makes a linear probe pass the table's last slot -- or a later lookup of one of `finds` does.  (Which slots end
    up taken, and so whether some probe wraps, does not depend on the order in which the device's threads insert.)"""
    tbl, wraps = [None] * slots, False
    for insert, k in [(True, k) for k in keys] + [(False, k) for k in finds]:
        item = k if isinstance(k, tuple) else (k, 0)
        slot = py_hash_bytes(*item) & (slots - 1)
        while tbl[slot] is not None and tbl[slot] != item:
            wraps = wraps or slot == slots - 1
            slot = (slot + 1) & (slots - 1)
        if insert:
            tbl[slot] = item
    return wraps


def wrap_set(seed=3):
    """The wrap-around set: WRAP_BATCHES organisms of WRAP_GENES genes, every gene on a contig of its own name, and per
    organism a families line of 7 tokens that knows 6 of its genes ("most") or 3 of them and 3 strangers ("half").
    Returns (gffs, the table of all genes, {"most": lines, "half": lines})."""
    rng = np.random.RandomState(seed)
    gffs, whole, most, half = [], [], [], []
    for o in range(WRAP_BATCHES):
        genes = [b"w%dg%d" % (o, rng.randint(10 ** 6)) + b"abc"[j % 3:j % 3 + 1] * (j % 4) for j in range(WRAP_GENES)]
        assert len(set(genes)) == WRAP_GENES
        gffs.append(b"".join(cds_line(b"q%d_%d" % (rng.randint(1000), j), int(rng.randint(0, 4)), g) + b"\n" for j, g in enumerate(genes)))
        whole.append(b"W%d " % (o % 13) + b" ".join(genes))
        most.append(b"M%d " % o + b" ".join(genes[:6]) + b"\n")
        half.append(b"H%d " % o + b" ".join(genes[:3] + [b"stranger%d" % rng.randint(10 ** 6) for _ in range(3)]) + b"\n")
    return gffs, b"\n".join(whole) + b"\n", dict(most=most, half=half)


# ---- genes to number -----------------------------------------------------------------------------------------------------
def number_case(g, n_orgs, lim, seed):
    """(name, org, n_names, planted) for number_host / nemgpu_gff_number: g genes, org non-decreasing, as in a walk.  Organism
    0 starts with 255 families met once, then a family met lim + 1 times (its sorted run straddles positions 255 | 256)
    and one met lim times, single families up to position SCAN_TILE - 1, there a family met lim + 1 times and one met
    lim times, then a family met lim + 1 times of which organism 0 has all but one and organism 1 the last.  The other
    genes draw from names of their own.  planted: {name: whether it is repeated} for the families that g had room for."""
    rng = np.random.RandomState(seed)
    plan, planted, fresh = [], [], iter(range(1 << 30))
    single = lambda count: [next(fresh) for _ in range(max(count, 0))]
    split = None
    if 0 < lim <= 8:
        plan += single(255)
        for _ in range(2):
            for times in (lim + 1, lim):
                fam = next(fresh)
                plan += [fam] * times
                planted.append((fam, len(plan), times > lim))
            plan += single(SCAN_TILE - 1 - len(plan))
        if n_orgs > 1:
            split = next(fresh)
            plan += [split] * lim
    plan = plan[:g]
    rest = g - len(plan)
    org = np.zeros(g, np.int32)
    if n_orgs > 1 and rest:
        org[len(plan):] = np.sort(rng.randint(1, n_orgs, rest))
    names0 = next(fresh)
    pool = max(rest // 3, 1)
    name = np.concatenate([np.asarray(plan, np.int64), names0 + rng.randint(0, pool, rest)])
    want = {fam: rep for fam, end, rep in planted if end <= len(plan)}
    if split is not None and rest:
        name[len(plan)], org[len(plan)] = split, 1
        want[split] = False
    n_names = names0 + pool + 3
    perm = rng.permutation(n_names)
    return perm[name].astype(np.int32), org, n_names, {int(perm[k]): v for k, v in want.items()}
