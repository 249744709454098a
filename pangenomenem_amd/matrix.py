"""The pangenome matrix and the partition lists (PPanGGOLiN.write_matrix, ppanggolin.py:1400-1452: the Roary-style
``.csv`` and ``.Rtab``; the CLI's ``partitions/<name>.txt``, ``pangenome.txt`` and summary statistics,
command_line.py:549-556, 580-582; ``__str__``, ppanggolin.py:319-340), from a resident master: no graph is walked.

``write_matrix`` writes one line per node of the graph: the family, its partition, its products, how many organisms
and genes it has, the min / max / mean of the SET of its genes' lengths (``node["length"]``, :426-430) and, per
organism, the genes of the family there (``.csv``) or their number (``.Rtab``, ``len(node[org])``, :1429).  All the
numbers are a function of the master (its presence rows, its numbering) and the flat gene orders of all its organisms
with every gene's length:

``family_table_arrays`` states them in numpy and ``rtab_cells_host`` the ``.Rtab``'s cell text;
``nemgpu_family_table_create`` / ``nemgpu_family_table_rtab`` (csrc/nem_matrix.hip) compute both on the device,
``Master.family_table`` (chunks.py) is their Python surface; ``FamilyTable`` holds the result and writes the files;
``write_partitions`` and ``summary`` write what the CLI writes next to them.

Where the reference's bytes are not determined -- ``"|".join(set)`` of a cell's genes (:1429) and of the products
(:1434) follows string hash order -- the fields are joined in walk order here.
"""
import ctypes as C
import os

import numpy as np

from .engine import NemGpuError
from .projection import FAMILY, START, END, PRODUCT, LONG, check_projection_orders, part_codes

HEADER = ("Gene", "Non-unique Gene name", "Annotation", "No. isolates", "No. sequences", "Avg sequences per isolate",
          "Accessory Fragment", "Genome Fragment", "Order within Fragment", "Accessory Order with Fragment", "QC",
          "Min group size nuc", "Max group size nuc", "Avg group size nuc")                       # ppanggolin.py:1412-1425
LISTS = ("undefined", "persistent", "shell", "cloud", "core_exact", "accessory")            # pan.partitions' keys, in order
TEXT_BUDGET = 64 << 20                                                                      # bytes of .Rtab cells per device call
FIELDS = ("nb_genes", "nb_org", "len_min", "len_max", "len_distinct", "len_sum", "multi_ptr", "multi_org", "multi_cnt")


def lengths_from_annotations(annotations):
    """END - START of every gene (what __add_gene receives, ppanggolin.py:497, :511) in the walk order of
    chunks.orders_from_annotations: int32 [G]"""
    return np.asarray([info[END] - info[START] for contigs in annotations.values() for annot in contigs.values() for info in annot.values()],
                      np.int64).astype(np.int32)


def table_orders(annotations, organisms, families, repeated, family=FAMILY, lengths=None):
    """The flat orders a family table is made from: chunks.orders_from_annotations of ALL the organisms with the ids of
    `families` (a master's .id_names), every gene's length in the same walk, and the genes to skip.  repeated: the
    repeated family names, or {organism: names} where they differ (a grown master: a family declared repeated by an update
    keeps the genes its node got before).  A skipped gene gets one extra id, the only one flagged in `repeated`.
    Returns a dict: genes, lengths, contig_ptr, contig_org, repeated uint8 [f], f."""
    from .chunks import orders_from_annotations
    o = orders_from_annotations(annotations, organisms, (), (), family, families=families)
    by_org = repeated if isinstance(repeated, dict) else {org: frozenset(repeated) for org in organisms}
    skip = np.asarray([info[family] in by_org[org] for org, contigs in annotations.items() for annot in contigs.values() for info in annot.values()], bool)
    f0 = len(o["families"])
    genes = o["genes"].copy()
    genes[skip] = f0
    rep = np.zeros(f0 + 1, np.uint8)
    rep[f0] = 1
    return dict(genes=genes, lengths=lengths_from_annotations(annotations) if lengths is None else np.ascontiguousarray(lengths, np.int32),
                contig_ptr=o["contig_ptr"], contig_org=o["contig_org"], repeated=rep, f=f0 + 1)


def _presence(x, d):
    """a master's matrix (uint8 [n][d], or packed rows uint32 [n][ceil(d/32)] with d) as bool [n][d]"""
    x = np.asarray(x)
    if x.dtype == np.uint32:
        if d is None:
            raise ValueError("packed rows do not say how many organisms there are (d=)")
        bits = np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1), axis=1, bitorder="little")
        return bits[:, :d].astype(bool)
    if d is not None and d != x.shape[1]:
        raise ValueError("d is not the matrix's")
    return x != 0


def family_table_arrays(x, order, genes, gene_len, contig_ptr, contig_org, repeated=None, f=None, d=None):
    """What nemgpu_family_table_create computes, in numpy.
    x: the master's matrix (uint8 [n][d] or packed rows with d=); order int32 [n]: master family i is caller id order[i];
    genes / contig_ptr / contig_org / repeated / f: the flat orders of ALL the master's organisms (the layout of
    nemgpu_master_project); gene_len int32 [g]: END - START of every gene, negatives allowed.
      * a gene of a repeated family is skipped; every other gene is KEPT and must have a master family;
      * nb_genes[i] the kept genes of family i; nb_org[i] the organisms with at least one;
      * len_min, len_max, len_distinct, len_sum (int64) over the DISTINCT lengths of the family's kept genes;
      * multi_ptr [n + 1], multi_org, multi_cnt: the (family, organism) cells of 2 or more kept genes, CSR over the
        families, organisms increasing; every other cell's count is its presence bit;
      * the cells derived from the orders must be exactly the master's presence bits: ValueError otherwise (the orders
        are not this master's), also for a kept gene whose family the master does not have.
    Returns a dict of those arrays."""
    present = _presence(x, d)
    n, d = present.shape
    order = np.asarray(order, np.int64)
    if order.shape != (n,):
        raise ValueError("family_table_arrays: order [n]")
    if f is None:
        f = len(repeated) if repeated is not None else max(int(order.max()) + 1 if n else 1, int(np.max(genes)) + 1 if len(genes) else 1)
    genes, contig_ptr, contig_org, repeated = check_projection_orders(genes, contig_ptr, contig_org, repeated, d, int(f))
    gene_len = np.ascontiguousarray(gene_len, np.int32)
    if gene_len.shape != genes.shape:
        raise ValueError("family_table_arrays: gene_len [G]")
    inv = np.full(int(f), -2, np.int64)
    inside = order < f
    inv[order[inside]] = np.flatnonzero(inside)
    fam = inv[genes] if len(genes) else np.zeros(0, np.int64)
    kept = np.ones(len(genes), bool) if repeated is None else repeated[genes] == 0
    if (fam[kept] < 0).any():
        raise ValueError("these orders are not this master's: a kept gene's family is not in the master")
    org = np.repeat(contig_org.astype(np.int64), np.diff(contig_ptr))
    kf, ko, kl = fam[kept], org[kept], gene_len[kept].astype(np.int64)
    cell, copies = np.unique(kf * d + ko, return_counts=True)
    derived = np.zeros(n * d, bool)
    derived[cell] = True
    if not np.array_equal(derived.reshape(n, d), present):
        raise ValueError("these orders are not this master's: their cells are not its presence bits")
    big = copies >= 2
    multi_ptr = np.zeros(n + 1, np.int32)
    multi_ptr[1:] = np.cumsum(np.bincount(cell[big] // d, minlength=n))
    low = int(kl.min()) if len(kl) else 0
    span = (int(kl.max()) - low + 1) if len(kl) else 1
    pair = np.unique(kf * span + (kl - low))                  # the distinct (family, length), sorted by family, then length
    pf, pl = pair // span, pair % span + low
    len_distinct = np.bincount(pf, minlength=n)
    len_sum = np.zeros(n, np.int64)
    np.add.at(len_sum, pf, pl)
    first = np.concatenate([[0], np.cumsum(len_distinct)[:-1]]) if n else np.zeros(0, np.int64)
    has = len_distinct > 0
    len_min, len_max = np.zeros(n, np.int32), np.zeros(n, np.int32)
    len_min[has] = pl[first[has]]                             # (the pairs are sorted by family, then length)
    len_max[has] = pl[first[has] + len_distinct[has] - 1]
    return dict(nb_genes=np.bincount(kf, minlength=n).astype(np.int32), nb_org=np.bincount(cell // d, minlength=n).astype(np.int32),
                len_min=len_min, len_max=len_max, len_distinct=len_distinct.astype(np.int32), len_sum=len_sum,
                multi_ptr=multi_ptr, multi_org=(cell[big] % d).astype(np.int32), multi_cnt=copies[big].astype(np.int32))


def copy_counts(present, multi_ptr, multi_org, multi_cnt, row0=0, rows=None):
    """the copy count of every cell of families row0 .. row0 + rows - 1: int64 [rows][d]"""
    rows = present.shape[0] - row0 if rows is None else rows
    counts = np.asarray(present[row0:row0 + rows]).astype(np.int64)
    a, b = int(multi_ptr[row0]), int(multi_ptr[row0 + rows])
    fam = np.repeat(np.arange(rows), np.diff(np.asarray(multi_ptr[row0:row0 + rows + 1], np.int64)))
    counts[fam, np.asarray(multi_org[a:b], np.int64)] = np.asarray(multi_cnt[a:b], np.int64)
    return counts


def rtab_cells_host(x, multi_ptr, multi_org, multi_cnt, row0=0, rows=None, d=None):
    """What nemgpu_family_table_rtab writes, in numpy: for families row0 .. row0 + rows - 1 the text the reference
    writes after column 14 of a line of the .Rtab -- the d copy counts in decimal joined by a tab, then a newline.
    Returns (text uint8 [bytes], line_end int64 [rows]: every line's end offset)."""
    present = _presence(x, d)
    counts = copy_counts(present, multi_ptr, multi_org, multi_cnt, row0, rows)
    rows, d = counts.shape
    digits = np.ones(counts.shape, np.int64)
    for k in range(1, 19):
        digits += counts >= 10 ** k
    end = np.cumsum((digits + 1).ravel())                     # a cell: its digits and its separator
    text = np.empty(int(end[-1]) if end.size else 0, np.uint8)
    sep = np.full(counts.shape, ord("\t"), np.uint8)
    sep[:, -1] = ord("\n")
    text[end - 1] = sep.ravel()
    flat, nd = counts.ravel(), digits.ravel()
    for k in range(int(nd.max()) if nd.size else 0):          # the k-th digit from the right of every cell that has one
        has = nd > k
        text[end[has] - 2 - k] = ord("0") + (flat[has] // 10 ** k) % 10
    return text, end.reshape(rows, d)[:, -1].copy()


def _bind_matrix(lib):
    lib.nemgpu_family_table_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p]
    lib.nemgpu_family_table_shape.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 3
    lib.nemgpu_family_table_fetch.argtypes = [C.c_void_p] * 10
    lib.nemgpu_family_table_rtab_size.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.nemgpu_family_table_rtab.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    lib.nemgpu_family_table_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_family_table_destroy.restype = None
    return lib


def _long_names(partitions, names, n):
    """every family's long partition name: partitions is {family name: 'P' | 'S' | 'C' | 'U'} (a family it does not
    name is undefined) or uint8 [n] in the same codes"""
    if isinstance(partitions, dict):
        if names is None:
            raise ValueError("this master carries no names (give the classes as uint8 [n])")
        part = part_codes(partitions, names)
    else:
        part = np.ascontiguousarray(partitions, np.uint8)
    if part.shape != (n,) or (n and part.max() > 3):
        raise ValueError("partitions: a class per family, P 0, S 1, C 2, U 3")
    return [LONG[k] for k in part]


class _Table:
    """what a family table writes, from its arrays, its names (.names, .organism_names; .repeated_names: the repeated
    families' names, or {organism: names}, table_orders), rtab_size() and
    rtab_cells(): FamilyTable on the device, HostFamilyTable in numpy"""

    def arrays(self):
        return {name: getattr(self, name) for name in FIELDS}

    def _batches(self, budget):
        """(row0, rows) covering the table, each batch's text within the budget (one line where a line alone is above it)"""
        row0 = 0
        while row0 < self.n:
            rows = max(1, min(self.n - row0, budget // (2 * self.d)))
            size = self.rtab_size(row0, rows)
            while size > budget and rows > 1:
                rows = max(1, min(rows - 1, rows * budget // size))
                size = self.rtab_size(row0, rows)
            yield row0, rows
            row0 += rows

    def write_matrix(self, path, partitions, annotations, header=True, csv=True, Rtab=True, budget=TEXT_BUDGET):
        """<path>.csv and <path>.Rtab as PPanGGOLiN.write_matrix writes them (ppanggolin.py:1400-1452), families in master
        order.  partitions: what Master.partition returned, or uint8 [n]; annotations: the ones the table was made from
        (the .csv's gene ids and both files' products are read from them, in walk order).  The .Rtab's cells are the
        device's bytes, a slice per line."""
        names, orgs = self.names, self.organism_names
        if names is None or orgs is None:
            raise ValueError("write_matrix: a master that carries names (from_annotations, from_graph, add_annotations)")
        if (self.nb_org == 0).any():
            raise ZeroDivisionError("write_matrix: a family without an organism")
        longs = _long_names(partitions, names, self.n)
        index = {name: i for i, name in enumerate(names)}
        products = [dict() for _ in names]                    # (insertion-ordered sets)
        cells = [dict() for _ in names] if csv else None      # family -> organism -> its genes
        by_org = self.repeated_names if isinstance(self.repeated_names, dict) else None
        for org, contigs in annotations.items():
            skipped = by_org[org] if by_org is not None else self.repeated_names
            for annot in contigs.values():
                for gene, info in annot.items():
                    if info[FAMILY] in skipped:
                        continue
                    i = index[info[FAMILY]]
                    products[i][info[PRODUCT]] = None
                    if csv:
                        cells[i].setdefault(org, dict())[gene] = None

        def prefix(i, sep):
            nb_org, nb_genes = int(self.nb_org[i]), int(self.nb_genes[i])
            return sep.join(['"' + names[i] + '"', '"' + longs[i] + '"', '"' + "|".join(products[i]) + '"', str(nb_org), str(nb_genes),
                             str(round(nb_genes / nb_org, 2)), '""', '""', '""', '""', '""', str(int(self.len_min[i])), str(int(self.len_max[i])),
                             str(round(float(int(self.len_sum[i])) / max(int(self.len_distinct[i]), 1), 2))])

        def head(sep):
            return sep.join(['"' + h + '"' for h in HEADER] + ['"' + org + '"' for org in orgs]) + "\n"

        if csv:
            with open(path + ".csv", "w") as out:
                if header:
                    out.write(head(","))
                for i in range(self.n):
                    row = cells[i]
                    out.write(",".join([prefix(i, ",")] + ['"' + "|".join(row[org]) + '"' if org in row else '""' for org in orgs]) + "\n")
        if Rtab:
            with open(path + ".Rtab", "wb") as out:
                if header:
                    out.write(head("\t").encode())
                for row0, rows in self._batches(budget):
                    text, ends = self.rtab_cells(row0, rows)
                    view, start = memoryview(text), 0
                    for r in range(rows):
                        out.write((prefix(row0 + r, "\t") + "\t").encode())
                        out.write(view[start:int(ends[r])])
                        start = int(ends[r])


class DeviceTable:
    """A table of a master on the device behind a C handle (nemgpu_<KIND>_create / _shape / _fetch / _destroy), its arrays
    (ARRAYS) read back.  A subclass names KIND, ARRAYS, the attribute of its third shape number (COUNT), gives _sizes() and
    sets self.lib (the bound library) before it calls _create().
    The master must stay open as long as the table writes."""

    def _call(self, name, *args):
        name = "nemgpu_%s_%s" % (self.KIND, name)
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise NemGpuError("%s failed (status %d): %s" % (name, rc, self.lib.nemgpu_last_error().decode()))

    def _orders(self, master, genes, contig_ptr, contig_org, repeated, f):
        """the orders checked, f defaulted: (f, genes, contig_ptr, contig_org, repeated)"""
        if f is None:
            f = len(repeated) if repeated is not None else max(master.f, int(np.max(genes)) + 1 if len(genes) else 1)
        return (int(f),) + check_projection_orders(genes, contig_ptr, contig_org, repeated, master.d, int(f))

    def _create(self, master, f, genes, per_gene, contig_ptr, contig_org, per_contig, repeated):
        """the table made from the orders and what it adds per gene and per contig (int32 arrays), its arrays fetched"""
        self.master, self._h = master, C.c_void_p()
        self._call("create", C.byref(self._h), master._h, f, genes.ctypes.data, *(a.ctypes.data for a in per_gene), len(genes),
                   contig_ptr.ctypes.data, contig_org.ctypes.data, *(a.ctypes.data for a in per_contig), len(contig_org),
                   repeated.ctypes.data if repeated is not None else None)
        v = [C.c_int() for _ in range(3)]
        self._call("shape", self._h, *(C.byref(a) for a in v))
        self.n, self.d, count = (a.value for a in v)
        setattr(self, self.COUNT, count)
        for name, size in zip(self.ARRAYS, self._sizes()):
            setattr(self, name, np.zeros(size, np.int64 if name == "len_sum" else np.int32))
        self._call("fetch", self._h, *(getattr(self, name).ctypes.data if getattr(self, name).size else None for name in self.ARRAYS))

    def _text(self, name, out, needed, *args):
        """a text call into `out`; too small: the NemGpuError carries the size needed"""
        try:
            self._call(name, *args)
        except NemGpuError as err:
            err.needed = needed.value
            raise
        return out[:needed.value]

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self.lib, "nemgpu_%s_destroy" % self.KIND)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FamilyTable(DeviceTable, _Table):
    """The family table of a master on the device (nemgpu_family_table_create) with its arrays read back: nb_genes,
    nb_org, len_min, len_max, len_distinct int32 [n], len_sum int64 [n], multi_ptr int32 [n + 1], multi_org, multi_cnt.
    The master must stay open as long as the table writes."""
    KIND, ARRAYS, COUNT = "family_table", FIELDS, "n_multi"

    def __init__(self, master, genes, gene_len, contig_ptr, contig_org, repeated=None, f=None, repeated_names=()):
        self.lib = _bind_matrix(master.lib)
        f, genes, contig_ptr, contig_org, repeated = self._orders(master, genes, contig_ptr, contig_org, repeated, f)
        gene_len = np.ascontiguousarray(gene_len, np.int32)
        if gene_len.shape != genes.shape or not len(genes):
            raise ValueError("family table: genes [G] and gene_len [G], G > 0")
        self.repeated_names = repeated_names
        self.names, self.organism_names = getattr(master, "names", None), getattr(master, "organism_names", None)
        self._create(master, f, genes, (gene_len,), contig_ptr, contig_org, (), repeated)

    def _sizes(self):
        return (self.n,) * 6 + (self.n + 1, self.n_multi, self.n_multi)

    def copies(self, i):
        """the copy count of family i in every organism (len(node[org]), 0 where it is absent): int64 [d]"""
        present = _presence(self.master._rows[i:i + 1], self.d)
        a, b = self.multi_ptr[i], self.multi_ptr[i + 1]
        return copy_counts(present, np.asarray([0, b - a]), self.multi_org[a:b], self.multi_cnt[a:b])[0]

    def rtab_size(self, row0, rows):
        size = C.c_int64()
        self._call("rtab_size", self._h, int(row0), int(rows), C.byref(size))
        return size.value

    def rtab_cells(self, row0=0, rows=None, out=None):
        """The .Rtab cell text of families row0 .. row0 + rows - 1, formatted on the device (nemgpu_family_table_rtab;
        rtab_cells_host states it): (text uint8 [bytes], line_end int64 [rows]).  out: a uint8 buffer to write into (too
        small: NemGpuError that says the size needed, nothing written)."""
        rows = self.n - row0 if rows is None else rows
        if out is None:
            out = np.empty(self.rtab_size(row0, rows), np.uint8)
        ends, needed = np.zeros(rows, np.int64), C.c_int64()
        return self._text("rtab", out, needed, self._h, self.master._h, int(row0), int(rows), out.ctypes.data, out.size, C.byref(needed),
                          ends.ctypes.data), ends


class HostFamilyTable(_Table):
    """The same table from the numpy statement (family_table_arrays, rtab_cells_host): what the device is held against,
    and a table for a caller who has the master's arrays on the host.  x, order, d: the master's (family_table_arrays)."""

    def __init__(self, x, order, genes, gene_len, contig_ptr, contig_org, repeated=None, f=None, d=None, names=None, organism_names=None,
                 repeated_names=()):
        self.present = _presence(x, d)
        self.n, self.d = self.present.shape
        for name, a in family_table_arrays(self.present.astype(np.uint8), order, genes, gene_len, contig_ptr, contig_org, repeated, f).items():
            setattr(self, name, a)
        self.n_multi = len(self.multi_org)
        self.names, self.organism_names, self.repeated_names = names, organism_names, repeated_names

    def copies(self, i):
        return copy_counts(self.present, self.multi_ptr, self.multi_org, self.multi_cnt, i, 1)[0]

    def rtab_cells(self, row0=0, rows=None):
        return rtab_cells_host(self.present, self.multi_ptr, self.multi_org, self.multi_cnt, row0, rows)

    def rtab_size(self, row0, rows):
        return len(self.rtab_cells(row0, rows)[0])


def partition_lists(partitions, names, nb_org, d):
    """pan.partitions as partition() fills it (ppanggolin.py:1131-1148) for families walked in master order: {list name:
    family names}, the six lists in the CLI's order; core_exact: a family in all d organisms"""
    longs = _long_names(partitions, names, len(names))
    lists = {name: [] for name in LISTS}
    for name, long_name, orgs in zip(names, longs, nb_org):
        lists[long_name].append(name)
        lists["core_exact" if int(orgs) == d else "accessory"].append(name)
    return lists


def _names_of(table):
    names = table.names
    if names is None:
        raise ValueError("a master that carries names (from_annotations, from_graph, add_annotations)")
    return names


def write_partitions(out_dir, partitions, table):
    """partitions/<name>.txt for the six lists and pangenome.txt (core_exact's lines, then accessory's), as
    command_line.py:549-555 writes them: "\\n".join(families) + "\\n", an empty list one newline"""
    lists = partition_lists(partitions, _names_of(table), table.nb_org, table.d)
    os.makedirs(os.path.join(out_dir, "partitions"), exist_ok=True)
    with open(os.path.join(out_dir, "pangenome.txt"), "w") as pan:
        for name, families in lists.items():
            with open(os.path.join(out_dir, "partitions", name + ".txt"), "w") as out:
                out.write("\n".join(families) + "\n")
            if name in ("core_exact", "accessory"):
                pan.write("\n".join(families) + "\n")
    return lists


def summary(partitions, table):
    """the text of str(pan) (ppanggolin.py:319-340) for a partitioned pangenome"""
    lists = partition_lists(partitions, _names_of(table), table.nb_org, table.d)
    size = {name: len(families) for name, families in lists.items()}
    return ("\n----------- Statistics -----------\n"
            "Number of organisms: %d\nPangenome size:%d\n\n"
            "Exact core-genome size:%d\nExact variable-genome size:%d\n\n"
            "Persistent genome size:%d\nShell genome size:%d\nCloud genome cloud:%d\n\n"
            "Gene families with undefined partition:%d\n"
            "----------------------------------" % (table.d, table.n, size["core_exact"], table.n - size["core_exact"], size["persistent"],
                                                    size["shell"], size["cloud"], size["undefined"]))
