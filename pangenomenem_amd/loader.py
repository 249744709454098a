"""From the files: the organisms' GFFs and the families table (``PPanGGOLiN("file", organisms_file, families_tsv,
lim_occurence, infer_singletons)``: ``__initialize_from_files`` and ``__load_gff``, ppanggolin.py:180-315) as the flat
gene orders every ``orders=`` entry point takes, without the nested dict.

``load_files`` reads (and gunzips) the files on the host into batches of whole files and hands each batch to the device
(csrc/nem_gff.hip); ``load_arrays_host`` is the same computation in plain Python on bytes, the statement the device is
held to array for array and span for span.  Both return a ``Loaded``.

The text of a load is the files of the organisms in order, joined by one ``\\n``; a span is (offset, length) in it.  A
batch is a run of whole files of that text, so nothing depends on where the batches are cut.

What one batch gives (``_batch_host`` states it, ``nemgpu_gff_batch`` computes it), for the CDS lines before a file's
``##FASTA``, ordered by (file, contig by first appearance in the file, START, line):

  file, start, end      int32 [g]
  span_off, span_len    int32 [5][g]: ID, NAME (else GENE), PRODUCT, strand and contig name, stripped; an absent NAME
                        or PRODUCT is the empty span at the ID's offset
  fam                   int32 [g]: the gene's family among the table's distinct family names (numbered by their first
                        line), -1 for an ID the table does not have
  contig                int32 [g]: the contig, dense over the batch
  fasta_off             int32 [files]: where the file's ``##FASTA`` line starts (its end if it has none)
  error                 the smallest (file, line, code) of a refused line, or None

After the batches, two small things on the host for both: the ``##sequence-region`` pragmas (found by a byte search
before ``fasta_off``) and the names of the inferred singletons, numbered after the table's families by their bytes.
Then the dense family ids by first occurrence in the walk and the per-organism occurrence counts against
``lim_occurence``: ``number_host`` states them, ``nemgpu_gff_number`` computes them.

Two departures from the reference, and one note: bytes >= 0x80 are ordinary token bytes (Unicode-only whitespace does
not separate); an ID that occurs twice within one organism is refused; ``region`` features are not read, as the
reference does not read them either (ppanggolin.py:264 compares a constant).  START and END are an optional sign and
ASCII digits within int32: Python's ``1_000`` and non-ASCII digits are refused.
"""
import ctypes as C
import gzip
import os
import re
from collections import OrderedDict

import numpy as np

WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"            # str.isspace() below 0x80
_WS_TO_SPACE = bytes(32 if b in WS else b for b in range(256))
_LINE = re.compile(rb"\r\n|\r|\n")
_INT = re.compile(rb"[+-]?[0-9]+\Z")
SPAN_ID, SPAN_NAME, SPAN_PRODUCT, SPAN_STRAND, SPAN_CONTIG = range(5)

# why a line is refused, in the order the reference meets them within one line; the numbers are the device's
(E_FIELDS3, E_FIELDS9, E_ATTR, E_NOID, E_UNKNOWN, E_START, E_END, E_DUP) = range(1, 9)
_WHY = {E_FIELDS3: "fewer than 3 tab-separated fields", E_FIELDS9: "a CDS line with fewer than 9 tab-separated fields",
        E_ATTR: "an attribute that is not key=value", E_NOID: "a CDS without an ID attribute",
        E_START: "START is not an int32 written as an optional sign and ASCII digits",
        E_END: "END is not an int32 written as an optional sign and ASCII digits"}
PRAGMA = b"##sequence-region"
MAX_BATCH = (1 << 31) - 2


# ---- reading ------------------------------------------------------------------------------------------------------
def read_bytes(file_or_path):
    """the bytes of a path or an open file, gunzipped where they start with the gzip magic"""
    if isinstance(file_or_path, (str, bytes, os.PathLike)):
        with open(file_or_path, "rb") as f:
            data = f.read()
    else:
        name = getattr(file_or_path, "name", None)
        if isinstance(name, str) and os.path.isfile(name):
            with open(name, "rb") as f:
                data = f.read()
        else:
            data = file_or_path.read()
            if isinstance(data, str):
                data = data.encode()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def _name_of(file_or_path):
    if isinstance(file_or_path, (str, bytes, os.PathLike)):
        return os.fsdecode(file_or_path)
    return str(getattr(file_or_path, "name", "<file>"))


def split_lines(data):
    """universal newlines: the (start, end) of every line without its terminator; a last line may have none"""
    out, at = [], 0
    for m in _LINE.finditer(data):
        out.append((at, m.start()))
        at = m.end()
    if at < len(data):
        out.append((at, len(data)))
    return out


def strip_span(data, a, b):
    """[a, b) without the whitespace at either end; an all-whitespace run is the empty span at b"""
    while a < b and data[a] in WS:
        a += 1
    while b > a and data[b - 1] in WS:
        b -= 1
    return a, b


def parse_int32(tok):
    """an optional sign and ASCII digits within int32, else None"""
    if not _INT.match(tok):
        return None
    v = int(tok)
    return v if -(1 << 31) <= v < (1 << 31) else None


def read_organisms(organisms_file):
    """The organisms file: per line the id, the GFF path and the circular contigs' names, tab-split and stripped.
    Returns (ids, paths, circular name lists, the index of the first duplicate id or None)."""
    name = _name_of(organisms_file)
    data = read_bytes(organisms_file)
    ids, paths, circ, dup, seen = [], [], [], None, set()
    for k, (a, b) in enumerate(split_lines(data)):
        el = [e.strip(WS).decode("utf-8", "surrogateescape") for e in data[a:b].split(b"\t")]
        if len(el) < 2:
            raise ValueError("%s: line %d: an organism line is its id, a tab and its GFF file" % (name, k + 1))
        if el[0] in seen and dup is None:
            dup = len(ids)
        seen.add(el[0])
        ids.append(el[0]); paths.append(el[1]); circ.append(el[2:])
    base = os.path.dirname(os.path.abspath(name)) if os.path.isfile(name) else None
    for i, p in enumerate(paths):
        if not os.path.exists(p) and base is not None and os.path.exists(os.path.join(base, p)):
            paths[i] = os.path.join(base, p)              # (a relative path that the working directory does not have)
    return ids, paths, circ, dup


def families_table_host(fam):
    """The families table on bytes: tokens split as str.split() splits, the first of a line the family, every later one
    a gene; a gene assigned twice keeps the later family.  Returns (gene -> family index, the distinct family names'
    (offset, length) in order of their first line)."""
    tf, spans, gene_tf = {}, [], {}
    for a, b in split_lines(fam):
        line = fam[a:b].translate(_WS_TO_SPACE)
        toks = line.split()
        if not toks:
            continue
        if toks[0] not in tf:
            a0, _ = strip_span(fam, a, b)
            tf[toks[0]] = len(spans)
            spans.append((a0, len(toks[0])))
        t = tf[toks[0]]
        for gene in toks[1:]:
            gene_tf[gene] = t
    return gene_tf, np.asarray(spans, np.int32).reshape(-1, 2)


# ---- one batch, stated ----------------------------------------------------------------------------------------------
def _cds_attributes(text, a, b):
    """the spans of ID, NAME (else GENE) and PRODUCT among the attributes [a, b), or an error code"""
    a, b = strip_span(text, a, b)
    found = {}
    at = a
    while at <= b:
        semi = text.find(b";", at, b)
        stop = b if semi < 0 else semi
        if stop > at:                                     # (the empty parts are dropped before the strip)
            pa, pb = strip_span(text, at, stop)
            eq = text.find(b"=", pa, pb)
            if eq < 0 or text.find(b"=", eq + 1, pb) >= 0:
                return None, E_ATTR
            found[text[pa:eq].upper()] = (eq + 1, pb)      # (bytes.upper(): ASCII only; the last of a key wins)
        at = stop + 1
    if b"ID" not in found:
        return None, E_NOID
    ident = found[b"ID"]
    name = found.get(b"NAME", found.get(b"GENE", (ident[0], ident[0])))
    product = found.get(b"PRODUCT", (ident[0], ident[0]))
    return (ident, name, product), 0


def _batch_host(text, file_start, file_end, gene_tf, infer_singletons):
    """One batch in plain Python: see the module's docstring for what it returns."""
    rows, fasta_off, error = [], [], None
    n_contigs = 0

    def refuse(f, line, code):
        nonlocal error
        if error is None or (f, line, code) < error:
            error = (f, line, code)

    for f, (fs, fe) in enumerate(zip(file_start, file_end)):
        data = text[fs:fe]
        contig_of, seen, fasta = {}, {}, fe
        for ln, (a, b) in enumerate(split_lines(data)):
            a, b = a + fs, b + fs
            if text[a:a + 2] == b"##":
                if text[a + 2:min(a + 7, b)] == b"FASTA":
                    fasta = a
                    break
                continue
            cuts = _tabs(text, a, b)
            nf = len(cuts) - 1                            # fields, counted up to 10
            if nf < 3:
                refuse(f, ln, E_FIELDS3)
                continue
            field = lambda j: strip_span(text, cuts[j] + 1, cuts[j + 1])
            ta, tb = field(2)
            if text[ta:tb] != b"CDS":
                continue
            if nf < 9:
                refuse(f, ln, E_FIELDS9)
                continue
            spans, code = _cds_attributes(text, cuts[8] + 1, cuts[9])
            if code:
                refuse(f, ln, code)
                continue
            ident, name, product = spans
            gene = text[ident[0]:ident[1]]
            fam = gene_tf.get(gene, -1)
            if fam < 0 and not infer_singletons:
                refuse(f, ln, E_UNKNOWN)
                continue
            start, end = parse_int32(text[slice(*field(3))]), parse_int32(text[slice(*field(4))])
            if start is None or end is None:
                refuse(f, ln, E_START if start is None else E_END)
                continue
            if gene in seen:
                refuse(f, ln, E_DUP)
                continue
            seen[gene] = ln
            ca, cb = field(0)
            cname = text[ca:cb]
            if cname not in contig_of:
                contig_of[cname] = n_contigs
                n_contigs += 1
            rows.append((f, contig_of[cname], start, ln, end, ident, name, product, field(6), (ca, cb), fam))
        fasta_off.append(fasta)
    rows.sort(key=lambda r: r[:4])
    g = len(rows)
    out = dict(file=np.asarray([r[0] for r in rows], np.int32), contig=np.asarray([r[1] for r in rows], np.int32),
               start=np.asarray([r[2] for r in rows], np.int32), end=np.asarray([r[4] for r in rows], np.int32),
               fam=np.asarray([r[10] for r in rows], np.int32), span_off=np.zeros((5, g), np.int32), span_len=np.zeros((5, g), np.int32),
               n_contigs=n_contigs, fasta_off=np.asarray(fasta_off, np.int32).reshape(-1), error=error)
    for k, r in enumerate(rows):
        for j in range(5):
            out["span_off"][j, k], out["span_len"][j, k] = r[5 + j][0], r[5 + j][1] - r[5 + j][0]
    return out


# ---- the device -------------------------------------------------------------------------------------------------------
_P, _I = C.c_void_p, C.c_int


def _bind(lib):
    if getattr(lib, "_gff_bound", False):
        return lib
    lib.nemgpu_gff_info.argtypes = [_P, _P, _P]
    lib.nemgpu_gff_create.argtypes = [_P, _I, _P, C.c_longlong, _I, _P]
    lib.nemgpu_gff_family_spans.argtypes = [_P, _P]
    lib.nemgpu_gff_batch.argtypes = [_P, _P, C.c_longlong, _P, _P, _I, _I, _P, _P, _P]
    lib.nemgpu_gff_fetch.argtypes = [_P] * 9
    lib.nemgpu_gff_number.argtypes = [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P]
    lib.nemgpu_gff_stage_ms.argtypes = [_P, _P]
    lib.nemgpu_gff_destroy.argtypes = [_P]
    lib.nemgpu_gff_destroy.restype = None
    for f in ("info", "create", "family_spans", "batch", "fetch", "number", "stage_ms"):
        getattr(lib, "nemgpu_gff_" + f).restype = _I
    lib._gff_bound = True
    return lib


STAGES = ("upload", "lines", "parse", "contigs_ids", "sort", "gather_download")


def gff_info():
    """{'tile': the byte kernels' tile in bytes, 'sort_thresholds': the contig sizes at which the sort changes its path}.
    The sort is one device-wide stable radix sort on (contig, START) whatever the contigs' sizes: no thresholds."""
    from .engine import load_library
    lib = _bind(load_library())
    tile, nth = C.c_int(), C.c_int()
    th = (C.c_int * 8)()
    if lib.nemgpu_gff_info(C.byref(tile), C.byref(nth), th) != 0:
        raise RuntimeError("nemgpu_gff_info failed")
    return dict(tile=tile.value, sort_thresholds=[th[i] for i in range(nth.value)])


class _Device:
    """the loader's handle on the device: the families table, then batch after batch"""

    def __init__(self, fam, device, hash_bits):
        from .engine import NemGpuError, load_library
        self.lib, self._err = _bind(load_library()), NemGpuError
        self._h = C.c_void_p()
        nfam = C.c_int()
        self._check(self.lib.nemgpu_gff_create(C.byref(self._h), int(device), fam, len(fam), int(hash_bits), C.byref(nfam)), "nemgpu_gff_create")
        self.family_spans = np.zeros((nfam.value, 2), np.int32)
        self._check(self.lib.nemgpu_gff_family_spans(self._h, self.family_spans.ctypes.data), "nemgpu_gff_family_spans")
        self.stage_ms = np.zeros(len(STAGES))

    def _check(self, rc, what):
        if rc != 0:
            raise self._err("%s failed (status %d): %s" % (what, rc, self.lib.nemgpu_last_error().decode()))

    def batch(self, text, file_start, file_end, infer_singletons):
        fs, fe = np.ascontiguousarray(file_start, np.int32), np.ascontiguousarray(file_end, np.int32)
        g, c, err = C.c_int(), C.c_int(), C.c_ulonglong()
        self._check(self.lib.nemgpu_gff_batch(self._h, text, len(text), fs.ctypes.data, fe.ctypes.data, len(fs), 1 if infer_singletons else 0,
                                              C.byref(g), C.byref(c), C.byref(err)), "nemgpu_gff_batch")
        g = g.value
        out = dict(file=np.zeros(g, np.int32), contig=np.zeros(g, np.int32), start=np.zeros(g, np.int32), end=np.zeros(g, np.int32),
                   fam=np.zeros(g, np.int32), span_off=np.zeros((5, g), np.int32), span_len=np.zeros((5, g), np.int32), n_contigs=c.value,
                   fasta_off=np.zeros(len(fs), np.int32))
        self._check(self.lib.nemgpu_gff_fetch(self._h, *(out[k].ctypes.data for k in ("file", "start", "end", "span_off", "span_len", "fam", "contig",
                                                                                      "fasta_off"))), "nemgpu_gff_fetch")
        ms = np.zeros(len(STAGES), np.float32)
        self._check(self.lib.nemgpu_gff_stage_ms(self._h, ms.ctypes.data), "nemgpu_gff_stage_ms")
        self.stage_ms += ms
        e = err.value
        out["error"] = None if e == (1 << 64) - 1 else (int(e >> 40), int((e >> 8) & 0xFFFFFFFF), int(e & 0xFF))
        return out

    def number(self, name, org, n_names, n_orgs, lim_occurence):
        name, org = np.ascontiguousarray(name, np.int32), np.ascontiguousarray(org, np.int32)
        genes, order, rep = np.zeros(len(name), np.int32), np.zeros(max(n_names, 1), np.int32), np.zeros(max(n_names, 1), np.uint8)
        used = C.c_int()
        self._check(self.lib.nemgpu_gff_number(self._h, name.ctypes.data, org.ctypes.data, len(name), int(n_names), int(n_orgs), int(lim_occurence),
                                               genes.ctypes.data, order.ctypes.data, rep.ctypes.data, C.byref(used)), "nemgpu_gff_number")
        return genes, order[:used.value].copy(), rep[:max(used.value, 1)].copy()

    def close(self):
        if self._h:
            self.lib.nemgpu_gff_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the result ---------------------------------------------------------------------------------------------------------
class _Spans:
    """strings kept as (offset, length) in the load's text, decoded when asked for"""

    def __init__(self, loaded, off, length):
        self._ld, self.off, self.len = loaded, off, length

    def __len__(self):
        return len(self.off)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        return self._ld.text_at(int(self.off[i]), int(self.len[i]))

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def __eq__(self, other):
        return list(self) == list(other)


class Loaded:
    """What the reference has after ``__initialize_from_files``, flat.  organisms, families, families_repeted,
    circular_contig_size, orders (orders_from_annotations' keys and starts, ends, lengths, contig_sizes, strand),
    gene_ids / gene_names / products / contig_names (lazy), annotations()."""

    def __init__(self, organisms, files, file_base, orders, families, families_repeted, circular_contig_size, spans, contig_span, timing=None):
        self.organisms, self.orders, self.families = organisms, orders, families
        self.families_repeted, self.circular_contig_size = families_repeted, circular_contig_size
        self._files, self._base = files, file_base
        self.span_off, self.span_len = spans              # int64 / int32 [4][G]: ID, NAME, PRODUCT, strand
        self.contig_off, self.contig_len = contig_span    # [C]
        self.gene_ids = _Spans(self, self.span_off[SPAN_ID], self.span_len[SPAN_ID])
        self.gene_names = _Spans(self, self.span_off[SPAN_NAME], self.span_len[SPAN_NAME])
        self.products = _Spans(self, self.span_off[SPAN_PRODUCT], self.span_len[SPAN_PRODUCT])
        self.strands = _Spans(self, self.span_off[SPAN_STRAND], self.span_len[SPAN_STRAND])
        self.contig_names = _Spans(self, self.contig_off, self.contig_len)
        self.timing = timing or {}

    def text_at(self, off, length):
        if length == 0:
            return ""
        f = int(np.searchsorted(self._base, off, side="right")) - 1
        a = off - int(self._base[f])
        return self._files[f][a:a + length].decode("utf-8", "surrogateescape")

    def arrays(self):
        """every array of the load, for comparing two loads"""
        out = {k: v for k, v in self.orders.items() if isinstance(v, np.ndarray)}
        out.update(span_off=self.span_off, span_len=self.span_len, contig_off=self.contig_off, contig_len=self.contig_len)
        return out

    def annotations(self):
        """the reference's {organism: {contig: OrderedDict(gene -> [TYPE, FAMILY, START, END, STRAND, NAME, PRODUCT])}}"""
        o = self.orders
        ann = OrderedDict((org, OrderedDict()) for org in self.organisms)
        ptr, fams = o["contig_ptr"], self.families
        for c in range(len(o["contig_org"])):
            genes = OrderedDict()
            for k in range(int(ptr[c]), int(ptr[c + 1])):
                genes[self.gene_ids[k]] = ["CDS", fams[int(o["genes"][k])], int(o["starts"][k]), int(o["ends"][k]), self.strands[k],
                                           self.gene_names[k], self.products[k]]
            ann[self.organisms[int(o["contig_org"][c])]][self.contig_names[c]] = genes
        return ann


# ---- the load -------------------------------------------------------------------------------------------------------------
def _line_of(data, off):
    """the 0-based line of byte `off` of a file"""
    return sum(1 for a, _ in split_lines(data[:off + 1]) if a <= off) - 1


def _pragmas(data, fasta, known, sizes):
    """apply a file's ##sequence-region lines before `fasta` to sizes (the names in `known`); the (offset, why) of a
    refused one, or None"""
    at = data.find(PRAGMA, 0, fasta)
    while at >= 0:
        if at == 0 or data[at - 1:at] in (b"\n", b"\r"):
            m = _LINE.search(data, at)
            fields = data[at:m.start() if m else len(data)].translate(_WS_TO_SPACE).split()
            if len(fields) < 2:
                return at, "a ##sequence-region line without a name"
            name = fields[1].decode("utf-8", "surrogateescape")
            if name in known:
                size = parse_int32(fields[3]) if len(fields) >= 4 else None
                if size is None:
                    return at, "a ##sequence-region line of a circular contig without an int32 size"
                sizes[name] = size
        at = data.find(PRAGMA, at + 1, fasta)
    return None


def _raise_line(path, data, line, code):
    lines = split_lines(data)
    a, b = lines[line] if line < len(lines) else (0, 0)
    where = "%s: line %d: " % (path, line + 1)
    if code in (E_UNKNOWN, E_DUP):
        cuts = _tabs(data, a, b)
        spans, _ = _cds_attributes(data, cuts[8] + 1, cuts[9])
        gene = data[spans[0][0]:spans[0][1]].decode("utf-8", "surrogateescape")
        if code == E_UNKNOWN:
            raise KeyError(where + "unknown families: gene %r is not in the families table (infer_singletons makes it a family of its own)" % gene)
        raise ValueError(where + "the ID %r occurs twice in this organism" % gene)
    raise ValueError(where + _WHY[code])


def _tabs(data, a, b):
    """the tabs of the line [a, b), at most nine, between a - 1 and b: field j is (cuts[j] + 1, cuts[j + 1])"""
    cuts = [a - 1]
    at = a
    while len(cuts) < 10:
        t = data.find(b"\t", at, b)
        if t < 0:
            break
        cuts.append(t)
        at = t + 1
    return cuts + [b]


def number_host(name, org, n_names, n_orgs, lim_occurence):
    """The families' ids and the repeated ones, in numpy (nemgpu_gff_number computes the same): name[g] every gene's
    family name as a number below n_names, org[g] its organism, in the walk's order.  Returns genes int32 [g] (ids dense
    by first occurrence), order (the name of every id) and repeated uint8 [max(ids, 1)]: the families that occur more
    than lim_occurence > 0 times in ONE organism."""
    used, first = np.unique(name, return_index=True)
    order = used[np.argsort(first, kind="stable")].astype(np.int32)
    dense = np.zeros(n_names + 1, np.int64)
    dense[order] = np.arange(len(order))
    genes = dense[name].astype(np.int32)
    rep = np.zeros(max(len(order), 1), np.uint8)
    if lim_occurence > 0 and len(name):
        pair, count = np.unique(org.astype(np.int64) * len(order) + genes, return_counts=True)
        rep[(pair[count > lim_occurence] % len(order)).astype(np.int64)] = 1
    return genes, order, rep


def _load(organisms_file, families_file, lim_occurence, infer_singletons, batch_bytes, run_batch, family_spans, number, timing):
    """what load_files and load_arrays_host share: reading, batching, and the small host steps after the batches"""
    import time
    t0 = time.perf_counter()
    ids, paths, circ, dup = read_organisms(organisms_file)
    fam = read_bytes(families_file)
    fam_spans = family_spans(fam)
    names = [fam[a:a + n] for a, n in fam_spans]          # the table's distinct family names, then the inferred singletons
    name_id = {n: i for i, n in enumerate(names)}
    n_org = len(ids) if dup is None else dup
    timing["host_read_s"] = time.perf_counter() - t0

    files, base, sizes, known = [], [], OrderedDict(), set()
    parts = []                                            # per batch: its result with global offsets
    at, i = 0, 0
    while i < n_org:
        t0 = time.perf_counter()
        j, total, batch = i, 0, []
        while j < n_org and (not batch or total + len(batch[-1]) + 1 <= batch_bytes):
            try:
                data = read_bytes(paths[j])
            except OSError:
                if not batch:
                    raise
                break                                     # (the files before it first: an error in them precedes this one)
            if batch and total + len(data) + 1 > batch_bytes:
                break
            batch.append(data)
            total += len(data) + 1
            j += 1
        text = b"\n".join(batch)
        if len(text) > MAX_BATCH:
            raise ValueError("%s: a batch of %d bytes: offsets within a batch are int32" % (paths[i], len(text)))
        fs = np.cumsum([0] + [len(b) + 1 for b in batch[:-1]]).astype(np.int32)
        fe = fs + np.asarray([len(b) for b in batch], np.int32)
        timing["host_read_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        r = run_batch(text, fs, fe)
        timing["batch_s"] = timing.get("batch_s", 0.0) + time.perf_counter() - t0
        t0 = time.perf_counter()
        error = None if r["error"] is None else (r["error"][0], r["error"][1], r["error"][2], None)
        for k, data in enumerate(batch):                  # the pragmas, organism by organism as the reference meets them
            for name in circ[i + k]:
                sizes[name] = None
                known.add(name)
            if error is not None and error[0] < k:
                break
            bad = _pragmas(data, int(r["fasta_off"][k] - fs[k]), known, sizes)
            if bad is not None:
                cand = (k, _line_of(data, bad[0]), 0, bad[1])
                if error is None or cand[:2] < error[:2]:
                    error = cand
                break
        if error is not None:
            k, line, code, why = error
            if why is not None:
                raise ValueError("%s: line %d: %s" % (paths[i + k], line + 1, why))
            _raise_line(paths[i + k], batch[k], line, code)
        r["org"] = r["file"] + np.int32(i)
        sb = np.frombuffer(text, np.uint8)[np.minimum(r["span_off"][SPAN_STRAND], max(len(text) - 1, 0))] if len(text) else np.zeros(0, np.uint8)
        r["strand"] = np.where(r["span_len"][SPAN_STRAND] > 0, sb, 0).astype(np.uint8)
        r["goff"] = r["span_off"].astype(np.int64) + at
        parts.append(r)
        for k, data in enumerate(batch):
            files.append(data)
            base.append(at + int(fs[k]))
        at += len(text) + 1
        i = j
        timing["host_finish_s"] = timing.get("host_finish_s", 0.0) + time.perf_counter() - t0
    if dup is not None:
        raise KeyError("Redondant organism names was found (" + ids[dup] + ")")
    missing = [n for n, s in sizes.items() if s is None]
    if missing:
        raise ValueError("circular contigs named in the organisms file have no ##sequence-region size in any GFF file: " + ", ".join(missing))

    t0 = time.perf_counter()
    cat = lambda key, dt: np.concatenate([p[key] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    org, start, end, fam_of = cat("org", np.int32), cat("start", np.int32), cat("end", np.int32), cat("fam", np.int64)
    goff = np.concatenate([p["goff"] for p in parts], axis=1) if parts else np.zeros((5, 0), np.int64)
    glen = np.concatenate([p["span_len"] for p in parts], axis=1).astype(np.int32) if parts else np.zeros((5, 0), np.int32)
    shift, contig = 0, []
    for p in parts:
        contig.append(p["contig"].astype(np.int64) + shift)
        shift += p["n_contigs"]
    contig = np.concatenate(contig) if contig else np.zeros(0, np.int64)
    g, c = len(org), shift
    ld = Loaded(ids, files, np.asarray(base, np.int64), None, None, None, None, (goff[:4], glen[:4]), (None, None), timing)
    for k in np.flatnonzero(fam_of < 0):                  # an inferred singleton is the family named by its ID's bytes
        name = ld.text_at(int(goff[SPAN_ID, k]), int(glen[SPAN_ID, k])).encode("utf-8", "surrogateescape")
        fam_of[k] = name_id.setdefault(name, len(name_id))
        if fam_of[k] == len(names):
            names.append(name)
    # dense ids by first occurrence in the walk; the occurrences of a family in one organism against the threshold
    t1 = time.perf_counter()
    genes, order, rep = number(fam_of.astype(np.int32), org, len(names), len(ids), lim_occurence)
    timing["number_s"] = time.perf_counter() - t1
    families = [names[k].decode("utf-8", "surrogateescape") for k in order]
    contig_ptr = np.zeros(c + 1, np.int32)
    contig_ptr[1:] = np.cumsum(np.bincount(contig, minlength=c))
    head = contig_ptr[:-1].astype(np.int64)
    ld.contig_off, ld.contig_len = goff[SPAN_CONTIG, head], glen[SPAN_CONTIG, head]
    ld.contig_names = _Spans(ld, ld.contig_off, ld.contig_len)
    cnames = list(ld.contig_names)
    strand = cat("strand", np.uint8)                      # a gene's strand: the first byte of the stripped field, 0 where it is empty
    ld.orders = dict(genes=genes, contig_ptr=contig_ptr, contig_org=org[head].astype(np.int32),
                     contig_circular=np.asarray([1 if n in sizes else 0 for n in cnames], np.uint8), repeated=rep, d=len(ids),
                     families=families, organisms=list(ids), starts=start, ends=end, lengths=(end.astype(np.int64) - start).astype(np.int32),
                     contig_sizes=np.asarray([sizes.get(n, -1) for n in cnames], np.int32).reshape(-1), strand=strand)
    ld.families = families
    ld.families_repeted = {families[k] for k in np.flatnonzero(rep[:len(order)])}
    ld.circular_contig_size = dict(sizes)
    timing["host_finish_s"] = timing.get("host_finish_s", 0.0) + time.perf_counter() - t0
    return ld


def load_arrays_host(organisms_file, families_file, lim_occurence=0, infer_singletons=False, batch_bytes=256 << 20):
    """The load in plain Python on bytes: the statement of what load_files computes on the device."""
    gene_tf = {}

    def family_spans(fam):
        table, spans = families_table_host(fam)
        gene_tf.update(table)
        return spans

    return _load(organisms_file, families_file, int(lim_occurence), bool(infer_singletons), int(batch_bytes),
                 lambda text, fs, fe: _batch_host(text, fs, fe, gene_tf, infer_singletons), family_spans, number_host, {})


def load_files(organisms_file, families_file, lim_occurence=0, infer_singletons=False, device=0, batch_bytes=256 << 20, *, _hash_bits=0):
    """PPanGGOLiN("file", ...)'s loading, on the device: see the module's docstring.  _hash_bits (tests): keep only that
    many bits of the string hash, so that the tables' probes collide."""
    dev = []

    def family_spans(fam):
        dev.append(_Device(fam, device, _hash_bits))
        return dev[0].family_spans

    timing = {}
    try:
        ld = _load(organisms_file, families_file, int(lim_occurence), bool(infer_singletons), int(batch_bytes),
                   lambda text, fs, fe: dev[0].batch(text, fs, fe, infer_singletons), family_spans, lambda *a: dev[0].number(*a), timing)
        timing["device_stage_ms"] = dict(zip(STAGES, dev[0].stage_ms.tolist()))
        return ld
    finally:
        for d in dev:
            d.close()


# ---- a small GFF generator (tests, profiles) ------------------------------------------------------------------------------
def synth_files(directory, contig_genes, n_families=50, seed=0, shuffle_starts=True, gene_prefix="g"):
    """Write a synthetic set under `directory`: contig_genes[o] = the gene counts of organism o's contigs.  Genes are
    drawn from n_families families; starts are shuffled within a contig (with ties) unless told otherwise.
    Returns (organisms file, families file, bytes of GFF text)."""
    rng = np.random.RandomState(seed)
    os.makedirs(directory, exist_ok=True)
    fam_genes = [[] for _ in range(n_families)]
    org_lines, total = [], 0
    for o, contigs in enumerate(contig_genes):
        lines = ["##gff-version 3"]
        k = 0
        for ci, ng in enumerate(contigs):
            starts = (rng.randint(0, max(ng // 2, 1), ng) * 100 + 1) if shuffle_starts else np.arange(ng) * 100 + 1
            fams = rng.randint(0, n_families, ng)
            for s, fm in zip(starts.tolist(), fams.tolist()):
                gid = "%s%d_%d" % (gene_prefix, o, k)
                k += 1
                fam_genes[fm].append(gid)
                lines.append("o%dc%d\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=%s;Name=n%d;product=family %d protein" %
                             (o, ci, s, s + 90, "+-"[k & 1], gid, fm, fm))
        data = ("\n".join(lines) + "\n").encode()
        total += len(data)
        path = os.path.join(directory, "o%d.gff" % o)
        with open(path, "wb") as f:
            f.write(data)
        org_lines.append("o%d\t%s" % (o, os.path.basename(path)))
    orgs, fams = os.path.join(directory, "organisms.tsv"), os.path.join(directory, "families.tsv")
    with open(orgs, "w") as f:
        f.write("\n".join(org_lines) + "\n")
    with open(fams, "w") as f:
        for fm, genes in enumerate(fam_genes):
            f.write("F%d\t%s\n" % (fm, "\t".join(genes)))
    return orgs, fams, total
