"""A partition projected onto the organisms (PPanGGOLiN.projection, ppanggolin.py:1698-1755; the CLI's -pr,
command_line.py:557-560; the first thing partition_shell(Q="auto") does, :1190-1192), from a resident master.

``projection()`` walks every gene of the organisms to project and, for a gene whose family is not repeated (:1719),
counts it under its family's ``partition``, its ``partition_exact`` and "pangenome" (:1720-1722), and writes a line with
how many genes of that family the organism carries (``len(node[family][organism])``, :1731) and how many of the family's
neighbours (``nx.all_neighbors``, :1723) are persistent / shell / cloud (:1733-1735).  All of that is a function of the
master (its CSR, its presence rows, its numbering), the partition and the flat gene orders of the organisms to project:

``projection_arrays`` states it in numpy; ``nemgpu_master_project`` (csrc/nem_project.hip) computes it on the device,
``Master.projection`` (chunks.py) is its Python surface; ``Projection`` holds the result and writes the reference's
files; ``shell_q_auto`` is the Q that partition_shell(Q="auto") derives from the projection's mean.
"""
import os

import numpy as np

from .partitioning import CODES

LONG = ("persistent", "shell", "cloud", "undefined")          # the node attribute `partition` of each of CODES
(TYPE, FAMILY, START, END, STRAND, NAME, PRODUCT) = range(7)  # a gene's annotation record (ppanggolin.py:25)
# the columns of org_counts
(PERSISTENT, SHELL, CLOUD, UNDEFINED, CORE_EXACT, ACCESSORY, PANGENOME) = range(7)
REPEATED, UNKNOWN = -1, -2                                    # gene_family of a gene that is not counted


def _popcount_rows(rows):
    ones = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1)
    return ones[np.ascontiguousarray(rows, np.uint32).view(np.uint8)].reshape(len(rows), -1).sum(axis=1)


def check_orders(genes, contig_ptr, contig_org, repeated, d, f, circular=None, allow_empty=False):
    """The gene orders as contiguous arrays, or ValueError.  circular: contig_circular [C], which the build and the append
    need (chunks._check_orders; they also infer an f of None); allow_empty: the projection's rules
    (check_projection_orders): no gene at all is allowed, genes + contigs stay below 2^30."""
    genes = np.ascontiguousarray(genes, np.int32)
    contig_ptr = np.ascontiguousarray(contig_ptr, np.int32)
    contig_org = np.ascontiguousarray(contig_org, np.int32)
    c = len(contig_org)
    layout = "orders: genes [G], contig_ptr [C + 1], contig_org [C]"
    if circular is not None:
        circular = np.ascontiguousarray(circular, np.uint8)
        layout += ", contig_circular [C]"
    if genes.ndim != 1 or contig_ptr.shape != (c + 1,) or (circular is not None and circular.shape != (c,)):
        raise ValueError(layout)
    if f is None and circular is not None:
        f = len(repeated) if repeated is not None else (int(genes.max()) + 1 if len(genes) else 1)
    if repeated is not None:
        repeated = np.ascontiguousarray(repeated, np.uint8)
        if repeated.shape != (f,):
            raise ValueError("orders: repeated [F]")
    if f <= 0 or (d <= 0 and not allow_empty):
        raise ValueError("orders: F must be positive" if allow_empty else "orders: D and F must be positive")
    if allow_empty and len(genes) + c >= 1 << 30:
        raise ValueError("orders: genes + contigs must stay below 2^30")
    if (c == 0 and not allow_empty) or contig_ptr[0] != 0 or contig_ptr[-1] != len(genes) or (np.diff(contig_ptr) < 0).any():
        raise ValueError("orders: contig_ptr must run from 0 to the number of genes, monotone")
    if len(genes) and (genes.min() < 0 or genes.max() >= f):
        raise ValueError("orders: family id out of range")
    if c and (contig_org.min() < 0 or contig_org.max() >= d):
        raise ValueError("orders: contig organism out of range")
    return genes, contig_ptr, contig_org, circular, repeated, int(d), int(f)


def check_projection_orders(genes, contig_ptr, contig_org, repeated, d, f):
    """the rules nemgpu_master_project refuses by (the build's, without contig_circular; no gene at all is allowed)"""
    genes, contig_ptr, contig_org, _, repeated, _, _ = check_orders(genes, contig_ptr, contig_org, repeated, d, f, allow_empty=True)
    return genes, contig_ptr, contig_org, repeated


def projection_arrays(master_arrays, order, part, genes, contig_ptr, contig_org, repeated=None, f=None, d=None):
    """What nemgpu_master_project computes, in numpy.
    master_arrays: (x uint8 [n][d] or its packed rows uint32 [n][ceil(d/32)], (ptr, idx), ...) of an undirected master,
    as master_arrays_from_orders or Master.arrays() return them (packed rows do not say d: give it); order int32 [n]:
    master family i is caller id order[i]; part uint8 [n]: every family's class in partitioning.CODES (P 0, S 1, C 2,
    U 3); genes / contig_ptr / contig_org / repeated / f: the gene orders of the organisms to project in the layout of
    nemgpu_master_create_orders (contig_org: master columns; any subset of the organisms, in any order).
      * a gene of a repeated family is skipped (ppanggolin.py:1719): gene_family -1; an id no master family has: -2 (the
        reference would raise KeyError); every other gene is KEPT and has its master family;
      * gene_copies of a kept gene: the kept genes of its family in its organism among the contigs given
        (len(node[family][organism]), :1731); 0 for the others;
      * nei_counts[i] = how many entries of family i's CSR row are of class P, S, C (nx.all_neighbors of an nx.Graph,
        :1723: a self-loop is one entry); class U counts nowhere;
      * org_counts[o] over organism o's kept genes: persistent, shell, cloud, undefined (by the family's class),
        core_exact (the family is present in all d organisms of the master) or accessory (partition_exact,
        :1143-1148), pangenome (every kept gene); the rows of organisms not given stay 0.
    Returns gene_family int32 [g], gene_copies int32 [g], nei_counts int32 [n][3], org_counts int32 [d][7]."""
    x = np.asarray(master_arrays[0])
    ptr, idx = (np.asarray(a, np.int64) for a in master_arrays[1])
    n = x.shape[0]
    if x.dtype == np.uint32:
        if d is None:
            raise ValueError("projection_arrays: packed rows do not say how many organisms there are (d=)")
        present = _popcount_rows(x.reshape(n, -1)) if n else np.zeros(0, np.int64)
    else:
        if d is not None and d != x.shape[1]:
            raise ValueError("projection_arrays: d is not the matrix's")
        d = x.shape[1]
        present = (x != 0).sum(axis=1)
    d = int(d)
    order = np.asarray(order, np.int64)
    part = np.ascontiguousarray(part, np.uint8)
    if order.shape != (n,) or part.shape != (n,) or ptr.shape != (n + 1,):
        raise ValueError("projection_arrays: the master's arrays, its order [n] and part [n]")
    if n and part.max() > 3:
        raise ValueError("projection_arrays: a class above 3")
    if f is None:
        f = len(repeated) if repeated is not None else max(int(order.max()) + 1 if n else 1, int(np.max(genes)) + 1 if len(genes) else 1)
    f = int(f)
    genes, contig_ptr, contig_org, repeated = check_projection_orders(genes, contig_ptr, contig_org, repeated, d, f)
    g, c = len(genes), len(contig_org)
    # the neighbours' classes, per CSR row
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    cls = part[idx] if len(idx) else np.zeros(0, np.uint8)
    nei_counts = np.stack([np.bincount(row[cls == k], minlength=n) for k in range(3)], axis=1).astype(np.int32) if n else np.zeros((0, 3), np.int32)
    # every gene's master family
    inv = np.full(f, UNKNOWN, np.int64)
    inside = order < f                                        # (an id space smaller than the master's: those families have no gene here)
    inv[order[inside]] = np.flatnonzero(inside)
    fam = inv[genes] if g else np.zeros(0, np.int64)
    if repeated is not None and g:
        fam = np.where(repeated[genes] != 0, REPEATED, fam)
    kept = fam >= 0
    org = np.repeat(contig_org.astype(np.int64), np.diff(contig_ptr))
    # the organisms' counts
    ko, kf = org[kept], fam[kept]
    org_counts = sum(np.bincount(ko * 7 + column, minlength=d * 7) for column in
                     (part[kf].astype(np.int64), np.where(present[kf] == d, CORE_EXACT, ACCESSORY), PANGENOME)).reshape(d, 7)
    # the copies: runs of equal (organism, family)
    gene_copies = np.zeros(g, np.int32)
    if kept.any():
        _, back, count = np.unique(ko * max(n, 1) + kf, return_inverse=True, return_counts=True)
        gene_copies[kept] = count[back]
    return fam.astype(np.int32), gene_copies, nei_counts, org_counts.astype(np.int32)


def part_codes(partitions, names):
    """{family name: 'P' | 'S' | 'C' | 'U'} (what Master.partition returns) as uint8 [n] by the master's names; a family
    the dict does not name (not in the pangenome that was partitioned) is undefined"""
    code = {ch: k for k, ch in enumerate(CODES)}
    return np.asarray([code[partitions.get(name, "U")] for name in names], np.uint8)


def shell_q_auto(n_shell_families, mean_shell):
    """the Q of partition_shell(Q="auto") (ppanggolin.py:1190-1192): the shell families over the mean number of shell
    genes per organism, rounded, + 1 for the unexclusive families"""
    return int(round(float(n_shell_families) / mean_shell, 0)) + 1


class Projection:
    """What projection() computes, as arrays (projection_arrays' four), with what names them: the master's family
    names (or None), its organism names (or None), the projected organisms' columns in the caller's order, part."""

    def __init__(self, gene_family, gene_copies, nei_counts, org_counts, part, columns, family_names=None, organism_names=None):
        self.gene_family, self.gene_copies, self.nei_counts, self.org_counts = gene_family, gene_copies, nei_counts, org_counts
        self.part = np.ascontiguousarray(part, np.uint8)
        self.columns = [int(c) for c in columns]
        self.family_names = list(family_names) if family_names is not None else None
        self.organism_names = list(organism_names) if organism_names is not None else None

    @property
    def organisms(self):
        """the projected organisms' names, in the caller's order"""
        if self.organism_names is None:
            return ["org%d" % (c + 1) for c in self.columns]
        return [self.organism_names[c] for c in self.columns]

    def means(self):
        """(mean persistent, mean shell, mean cloud) over the projected organisms, as projection() returns it
        (ppanggolin.py:1746-1755; utils.mean: the sum over max(count, 1))"""
        rows = self.org_counts[self.columns] if self.columns else np.zeros((0, 7), np.int64)
        return tuple(float(int(rows[:, k].sum())) / max(len(self.columns), 1) for k in (PERSISTENT, SHELL, CLOUD))

    def write(self, out_dir, annotations):
        """nb_genes.csv and one <organism>.csv per projected organism, byte for byte as ppanggolin.py:1711-1743 writes
        them; annotations: the ones Master.projection was given (the same walk: gene p of the arrays is the p-th gene
        of the projected organisms' contigs)."""
        names = self.organisms
        p = 0
        with open(os.path.join(out_dir, "nb_genes.csv"), "w") as nb:
            nb.write("org\tpersistent\tshell\tcloud\tcore_exact\taccessory\tpangenome\n")
            for org, col in zip(names, self.columns):
                with open(os.path.join(out_dir, org + ".csv"), "w") as out:
                    out.write(",".join(["gene", "contig", "coord_start", "coord_end", "strand", "ori", "family", "nb_copy_in_org", "partition",
                                        "persistent", "shell", "cloud"]) + "\n")
                    for contig, annot in annotations[org].items():
                        for gene, info in annot.items():
                            fam = int(self.gene_family[p])
                            if fam >= 0:
                                ori = "T" if (info[NAME].upper() == "DNAA" or info[PRODUCT].upper() == "DNAA") else "F"
                                nei = self.nei_counts[fam]
                                out.write(",".join([gene, contig, str(info[START]), str(info[END]), info[STRAND], ori, info[FAMILY],
                                                    str(int(self.gene_copies[p])), LONG[self.part[fam]], str(int(nei[0])), str(int(nei[1])),
                                                    str(int(nei[2]))]) + "\n")
                            elif fam == UNKNOWN:
                                raise KeyError(info[FAMILY])
                            p += 1
                row = self.org_counts[col]
                nb.write("\t".join([org] + [str(int(row[k])) for k in (PERSISTENT, SHELL, CLOUD, CORE_EXACT, ACCESSORY, PANGENOME)]) + "\n")
        if p != len(self.gene_family):
            raise ValueError("Projection.write: these are not the annotations that were projected")
