"""The shell subpartitioned on the device: PPanGGOLiN.partition_shell (ppanggolin.py:1175-1248, the CLI's ``-ss``) on a
resident master.

``partition_shell`` solves the NEM problem of the shell families alone.  Its writer call,
``__write_nem_input_files(dir, self.organisms, init=init_using_qual, filter_by_partition="shell")``, keeps the nodes
whose ``partition`` is ``"shell"`` in node order (:844) and all organisms as columns.  For the neighbours (:859) the test
is INVERTED: a neighbour that *is* shell is skipped, one that is *not* reaches ``index_fam[neighbor]`` (:879) where it has
no entry, and only ``NetworkXError`` is caught.  As written the reference therefore raises ``KeyError`` as soon as one
shell family has a non-shell neighbour, and writes a ``.nei`` in which every family has 0 neighbours when the shell is
closed under adjacency.  The evident intent is the induced subgraph (what the same writer writes, unfiltered, for
``neighbors_graph.subgraph(shell)``): ``edges="induced"``, the default here; ``edges="reference"`` is the code as written.

``form_subproblem_host`` states the formation in numpy (``chunks.form_chunk_host`` with a selection and the two edge
rules); ``nemgpu_master_subproblem`` (csrc/nem_chunks.hip, csrc/nem_engine.hip) does it on the device, into an engine on
which the 50 random starts of INIT_RANDOM (no ``init_using_qual``) or a parameter file (``shell_init_params``) run.
``shell_labels`` is what partition_shell makes of the run (:1208-1247), from parameters that went through the ``.mf``'s
print formats (``mf_parameters``), as the reference reads them.
"""
import ctypes as C
import time
from collections import defaultdict

import numpy as np

from .chunks import form_chunk_host
from .engine import NemEngine, NemGpuError
from .projection import shell_q_auto

LONG = {"P": "persistent", "S": "shell", "C": "cloud", "U": "undefined"}
EDGE_RULES = {"induced": 0, "reference": 1}
MAX_Q = 32                                                    # kMaxKernelK


def outside_entry_host(x, ptr, idx, edge_bits, organisms, select, edge_counts=None):
    """The smallest CSR entry of the master that the writer as written has no index for: row a kept family (selected and
    present in `organisms`), neighbour NOT selected, coverage over `organisms` positive.  -1: none."""
    x = np.asarray(x, np.uint8)
    select = np.asarray(select, bool)
    n = x.shape[0]
    if len(idx) == 0:
        return -1
    # the coverage of every entry: the unselected chunk of all families holds it for the entries it keeps
    organisms = np.asarray(organisms, np.int64)
    mask = np.zeros(np.asarray(edge_bits).shape[1] * 32, np.uint8)
    mask[organisms] = 1
    words = np.packbits(mask, bitorder="little").view(np.uint32)
    cov = np.unpackbits(np.bitwise_and(np.asarray(edge_bits, np.uint32), words[None, :]).view(np.uint8), axis=1).sum(axis=1).astype(np.int64)
    if edge_counts is not None:
        xptr, xorg, xcnt = (np.asarray(a, np.int64) for a in edge_counts)
        np.add.at(cov, np.repeat(np.arange(len(idx)), np.diff(xptr)), (xcnt - 1) * mask[xorg])
    kept = select & x[:, organisms].any(axis=1)
    src = np.repeat(np.arange(n), np.diff(ptr))
    bad = np.flatnonzero(kept[src] & (cov > 0) & ~select[np.asarray(idx, np.int64)])
    return int(bad[0]) if len(bad) else -1


def form_subproblem_host(x, ptr, idx, edge_bits, organisms, select, edge_counts=None, edges="induced"):
    """The NEM problem of the selected families the way `__write_nem_input_files(..., filter_by_partition=)` makes it
    (ppanggolin.py:821-930), in numpy: form_chunk_host's arguments and its tuple (x_sub uint8 [n_s][d_s], (ptr_s, idx_s,
    w_s), families int64 [n_s]), with select bool [n] (:844).  A family is kept iff it is selected and present in one of
    `organisms`; the numbering stays the master's order.  edges="induced": an edge is kept iff its coverage is positive
    and both ends are kept.  edges="reference": the inverted test of :859 as written -- KeyError(master index of the
    neighbour) when a kept family has a neighbour of positive coverage that is not selected (the first such CSR entry),
    else no edge at all."""
    if edges not in EDGE_RULES:
        raise ValueError("edges: 'induced' or 'reference'")
    x = np.asarray(x, np.uint8)
    select = np.asarray(select, bool)
    if select.shape != (x.shape[0],):
        raise ValueError("select: bool [n]")
    if edges == "reference":
        e = outside_entry_host(x, ptr, idx, edge_bits, organisms, select, edge_counts)
        if e >= 0:
            raise KeyError(int(np.asarray(idx)[e]))
    # a family that is not selected is a family without organisms: form_chunk_host drops it and its edges
    xs, (ptr_s, idx_s, w_s), families = form_chunk_host(x * select[:, None].astype(np.uint8), ptr, idx, edge_bits, organisms, edge_counts)
    if edges == "reference":
        ptr_s, idx_s, w_s = np.zeros(len(families) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    return xs, (ptr_s, idx_s, w_s), families


def remainder_proportion(head):
    """the last class's proportion as ReadParamFile computes it (nem_exe.c:1022-1034): 1 minus the others, one float32
    subtraction after the other"""
    rem = np.float32(1.0)
    for v in head:
        rem = np.float32(rem - np.float32(v))
    return rem


def shell_init_params(init, organism_names, low_disp=0.1):
    """The `.m` that __write_nem_input_files writes for partition_shell's init_using_qual (ppanggolin.py:902-927), as
    arrays: init a dict {group: set(organisms)} (Q = len + 1 classes: one per group, then one of centre 0.5 and
    dispersion 0.5; every proportion round(1 / len, 4)) or a list (positive, negative) (Q = 3).  Returns (prop float32
    [Q] with the last one ReadParamFile's remainder, center float32 [Q][d], disp float32 [Q][d]).  A remainder <= 0 (a
    dict of 2, 4, 6, 7, 8, ... groups; 5 leave 2.98e-08, which ReadParamFile accepts) raises ValueError: nem() refuses that file (nem_io.cpp:401) and the reference's caller
    then dies on a KeyError."""
    organism_names = list(organism_names)
    half = [0.5] * len(organism_names)
    if isinstance(init, dict):
        every = set(org for orgs in init.values() for org in orgs)
        head = [round(float(1) / len(init), 4)] * len(init)
        center = [[1.0 if org in orgs else 0.0 if org in every else 0.5 for org in organism_names] for orgs in init.values()] + [half]
        disp = [[low_disp if org in every else 0.5 for org in organism_names] for _ in init] + [half]
    elif isinstance(init, (list, tuple)):
        positive, negative = init
        head = [0.33333, 0.33333]
        center = [[1.0 if org in positive else 0.0 if org in negative else 0.5 for org in organism_names],
                  [0.0 if org in positive else 1.0 if org in negative else 0.5 for org in organism_names], half]
        row = [low_disp if org in positive or org in negative else 0.5 for org in organism_names]
        disp = [row, row, half]
    else:
        raise ValueError("init_using_qual: a dict {group: organisms} or a list (positive, negative)")
    rem = remainder_proportion(head)
    if not rem > 0:
        raise ValueError("init_using_qual: the last class's proportion, 1 - %d x %s, is %s: nem() refuses this parameter file"
                         % (len(head), head[0], rem))
    prop = np.asarray(head + [rem], np.float32)
    return prop, np.asarray(center, np.float32), np.asarray(disp, np.float32)


def mf_value(v, fmt):
    """a float32 as run_partitioning reads it back from the `.mf` (nem_io.cpp:523-526): printed with fmt, parsed by float()"""
    return float(fmt % float(v))


def mf_parameters(res, Q):
    """all_parameters of run_partitioning (ppanggolin.py:1907-1923) from a finished run's arrays, through the `.mf`'s
    print formats: {k: (mu bool list: centres through "%10.3g" and then their truth, epsilon float list through "%10g",
    proportion through "%5.3g")}.  A run that emptied a class wrote no `.mf`: {}."""
    if res["status"] != 0:
        return {}
    return {k: ([bool(mf_value(v, "%10.3g")) for v in res["center"][k]], [mf_value(v, "%10g") for v in res["disp"][k]],
                mf_value(res["prop"][k], "%5.3g")) for k in range(Q)}


def uf_classes(c):
    """the class of every family as run_partitioning reads the `.uf` (ppanggolin.py:1959-1972, init != default): the LAST
    maximum of the posteriors after their " %5.3f\""""
    c3 = np.round(np.asarray(c, np.float64), 3)
    k = c3.shape[1]
    return (k - 1 - np.argmax(c3[:, ::-1], axis=1)).astype(np.int64)


def mean(numbers):
    """ppanggolin/utils.py:81"""
    return float(sum(numbers)) / max(len(numbers), 1)


def shell_labels(parameters, classes, family_names, organism_names, exclusity_th=0.1, init_using_qual=None):
    """What partition_shell makes of run_partitioning's result (ppanggolin.py:1208-1247).  parameters: mf_parameters';
    classes: the class of every family of the sub-problem; family_names: theirs; organism_names: the columns'.
    Returns (subpartitions_shell_parameters {label: ([organisms with mu true], mean(eps), proportion)},
    organisms_subpartitions_shell {organism: {labels}}, subpartition_shell {label: [families]}, {class: label}).
    A class without parameters (a run that emptied a class gives none at all) is the reference's KeyError."""
    labels, params, by_org = {}, {}, defaultdict(set)
    for k, (mu, eps, proportion) in parameters.items():
        m = mean(eps)
        label = str(k) + ("_exclusive:" if m < exclusity_th else "_shared:") + str(round(m, 2))
        k_orgs = [org for org, b in zip(organism_names, mu) if b]
        if isinstance(init_using_qual, dict):
            coverages = {}
            k_set = set(k_orgs)
            for group, set_org in init_using_qual.items():
                set_org = set(set_org)
                if len(k_set) > 0:
                    coverage = float(len(k_set & set_org)) / float(len(set_org))
                    if coverage >= 0.5:
                        coverages[group] = coverage
            if coverages:
                label = label + "_" + "|".join(sorted(coverages, key=coverages.get))
        params[label] = (k_orgs, m, proportion)
        for org in k_orgs:
            by_org[org].add(label)
        labels[k] = label
    families = defaultdict(list)
    for name, k in zip(family_names, classes):
        families[labels[k if isinstance(k, str) else int(k)]].append(name)
    return params, dict(by_org), dict(families), labels


class ShellSubpartition:
    """partition_shell's outcome: Q (its return value), parameters (subpartitions_shell_parameters), organisms
    (organisms_subpartitions_shell), families (subpartition_shell), node_attribute ({family: its label, or its
    partition's long name for a family outside the shell}: the node attribute subpart_name), and what they were made of:
    family_index int64 [n_s] (the sub-problem's families in the master), classes int64 [n_s], run (the engine's
    full-precision results)."""

    def __init__(self, Q, parameters, organisms, families, node_attribute, subpart_name, family_index, classes, run):
        self.Q, self.parameters, self.organisms, self.families = Q, parameters, organisms, families
        self.node_attribute, self.subpart_name = node_attribute, subpart_name
        self.family_index, self.classes, self.run = family_index, classes, run


def _bind(lib):
    if not getattr(lib, "_subproblem_bound", False):
        lib.nemgpu_master_subproblem.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                 C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.nemgpu_subproblem_fetch.argtypes = [C.c_void_p] * 5
        lib._subproblem_bound = True
    return lib


class Subproblem:
    """nemgpu_master_subproblem: the engine that holds the device-formed problem of a master's selected families.
    .engine (a NemEngine; None when edges="reference" met an outside neighbour), .families int64 [n] (master indices),
    .n, .nnz, .outside_entry (-1: none).  The master is only read."""

    def __init__(self, master, select, k, organisms=None, edges="induced"):
        if edges not in EDGE_RULES:
            raise ValueError("edges: 'induced' or 'reference'")
        lib = _bind(master.lib)
        sel = np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
        if sel.shape != (master.n,):
            raise ValueError("select: one value per family of the master")
        org = np.ascontiguousarray(np.arange(master.d) if organisms is None else organisms, np.int32)
        fam = np.zeros(master.n, np.int32)
        h, n, nnz, outside = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        rc = lib.nemgpu_master_subproblem(master._h, org.ctypes.data, len(org), sel.ctypes.data, EDGE_RULES[edges], int(k), C.byref(h),
                                          fam.ctypes.data, C.byref(n), C.byref(nnz), C.byref(outside))
        if rc != 0:
            raise NemGpuError("nemgpu_master_subproblem failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
        self.lib, self.n, self.nnz, self.d, self.outside_entry = lib, n.value, nnz.value, len(org), outside.value
        self.families = fam[:self.n].astype(np.int64)
        self.engine = None
        if h.value:
            eng = NemEngine.__new__(NemEngine)
            eng.lib, eng._h = lib, h
            eng.n_total, eng.d, eng.k, eng.lo, eng.hi, eng.n = self.n, self.d, int(k), 0, self.n, self.n
            self.engine = eng

    def fetch(self):
        """the formed problem read back: rows uint32 [n][ceil(d/32)], (ptr int32 [n + 1], idx int32 [nnz], w float32 [nnz])"""
        rows = np.zeros((self.n, (self.d + 31) // 32), np.uint32)
        ptr, idx, w = np.zeros(self.n + 1, np.int32), np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.float32)
        rc = self.lib.nemgpu_subproblem_fetch(self.engine._h, rows.ctypes.data, ptr.ctypes.data, idx.ctypes.data if self.nnz else None,
                                              w.ctypes.data if self.nnz else None)
        if rc != 0:
            raise NemGpuError("nemgpu_subproblem_fetch failed (status %d): %s" % (rc, self.lib.nemgpu_last_error().decode()))
        return rows, (ptr, idx, w)

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None


def resolve_q(Q, init_using_qual, n_shell, mean_shell):
    """step 1 of partition_shell (ppanggolin.py:1188-1202)"""
    if isinstance(Q, str):
        if Q != "auto":
            raise ValueError('Q must be above 1 or equals to "auto"')
        if init_using_qual is None:
            if mean_shell is None:
                raise ValueError('Q="auto" needs mean_shell (Projection.means()[1]) or annotations=')
            Q = shell_q_auto(n_shell, mean_shell)
        elif isinstance(init_using_qual, dict):
            Q = len(init_using_qual) + 1
        elif isinstance(init_using_qual, (list, tuple)):
            Q = 3
        else:
            raise ValueError("init_using_qual: a dict {group: organisms} or a list (positive, negative)")
    Q = int(Q)
    if Q <= 1:
        raise ValueError('Q must be above 1 or equals to "auto"')
    if Q > MAX_Q:
        raise ValueError("Q = %d: at most %d classes" % (Q, MAX_Q))
    return Q


def partition_shell(master, partitions=None, Q="auto", mean_shell=None, beta=0.5, free_dispersion=False, exclusity_th=0.1,
                    init_using_qual=None, edges="induced", seed=None, subpart_name="subpartition_shell", select=None,
                    annotations=None, repeated=(), low_disp=0.1):
    """Master.partition_shell (its docstring)."""
    names = getattr(master, "names", None)
    names = list(names) if names is not None else ["fam%d" % (i + 1) for i in range(master.n)]
    org_names = getattr(master, "organism_names", None)
    org_names = list(org_names) if org_names is not None else list(range(master.d))
    if (partitions is None) == (select is None):
        raise ValueError("partition_shell: partitions (what Master.partition returned) or select= (bool [n]), one of them")
    if partitions is not None:
        sel = np.asarray([partitions.get(f) == "S" for f in names], bool)
    else:
        sel = np.asarray(select) != 0
        if sel.shape != (master.n,):
            raise ValueError("select: one value per family of the master")
    if master.directed:
        raise NemGpuError("partition_shell: the master was built directed (nx.all_neighbors of a DiGraph lists a family that is both "
                          "predecessor and successor twice, the master's row once)")
    if Q == "auto" and init_using_qual is None and mean_shell is None and annotations is not None:
        mean_shell = master.projection(partitions, annotations, repeated=repeated).means()[1]
    Q = resolve_q(Q, init_using_qual, int(sel.sum()), mean_shell)
    params = shell_init_params(init_using_qual, org_names, low_disp) if init_using_qual is not None else None
    if params is not None and len(params[0]) != Q:
        raise ValueError("init_using_qual describes %d classes, Q is %d" % (len(params[0]), Q))
    seed = int(time.time()) & 0xFFFFFFFF if seed is None else int(seed)
    attr = {f: LONG.get(partitions.get(f, "U"), "undefined") if partitions is not None else None for f in names}
    if not sel.any():                                         # empty files, no `.uf`: nothing is labelled (ppanggolin.py:1975, :1208-1248)
        return ShellSubpartition(Q, {}, {}, {}, attr, subpart_name, np.zeros(0, np.int64), np.zeros(0, np.int64), None)
    sub = Subproblem(master, sel, Q, edges=edges)
    try:
        if sub.engine is None:                                # the writer's KeyError (ppanggolin.py:879)
            midx = np.zeros(master.shape()[2], np.int32)
            master._fetch(idx=midx)
            raise KeyError(names[int(midx[sub.outside_entry])])
        eng = sub.engine
        eng.configure(algo="ncem", beta=beta, disper="skd" if free_dispersion else "sk_", propor="pk", cvtest="clas", cvthres=1e-8,
                      it_max=100, tie="libc", seed=seed)
        if params is None:
            res = eng.run_random(50, seed)
        else:
            eng.set_params(*params)
            res = eng.run()
        families = sub.families
    finally:
        sub.close()
    parameters = mf_parameters(res, Q)
    classes = uf_classes(res["c"]) if res["status"] == 0 else ["U"] * len(families)
    p, by_org, fams, _ = shell_labels(parameters, classes, [names[i] for i in families], org_names, exclusity_th, init_using_qual)
    for label, members in fams.items():
        for f in members:
            attr[f] = label
    return ShellSubpartition(Q, p, by_org, fams, attr, subpart_name, families, np.asarray(classes), res)
