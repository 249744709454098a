"""`run_partitioning` without the files.

PPanGGOLiN's ``run_partitioning(nem_dir_path, nb_org, beta, free_dispersion, Q, init)``
(ppanggolin/ppanggolin.py:1761-1984) writes nothing itself: it calls ``nem()`` on the five ASCII files
``__write_nem_input_files`` produced (ppanggolin.py:821-930) and parses ``nem_file.uf`` / ``.mf`` back.
``run_partitioning_arrays`` takes the same problem as arrays, runs it through the in-memory C ABI and returns the
same two dicts.  What the text files did to the numbers is kept so that both routes give the same answer: the
posteriors are compared after rounding to the three decimals of ``.uf`` (nem_exe.c:1677) and the parameters after
the ``%g``-style precision of ``.mf`` is NOT needed (mu is only tested for truthiness, epsilon and pi are floats).
"""
import numpy as np

from . import synth
from .engine import NemEngine


def run_partitioning_arrays(x, nei, beta, free_dispersion=False, Q=3, init="param_file_default", names=None,
                            low_disp=0.1, params=None, rng_seed=1, device=0, tie="hash"):
    """x uint8 [families, organisms]; nei = CSR (ptr, idx, w) or None; names = family identifiers (default
    fam1..famN).  init: "param_file_default" (PPanGGOLiN's default .m, ppanggolin.py:893-901), "param_file" (give
    params = (prop, center, disp)) or "random" (init_mode INIT_RANDOM, 50 starts, ppanggolin.py:1207).
    tie: the tie rule ("libc" with init="random": the starts and the ties draw from one random() stream, as in nem()).
    Returns ({family: 'P'|'S'|'C'|'U' or class index}, {k: (mu bool list, epsilon list, proportion)})."""
    x = np.ascontiguousarray(x, np.uint8)
    n, d = x.shape
    names = list(names) if names is not None else ["fam%d" % (i + 1) for i in range(n)]
    eng = NemEngine(n, d, Q, device=device)
    try:
        eng.set_matrix(x)
        eng.set_graph(nei)
        eng.configure(algo="ncem", beta=beta, disper="skd" if free_dispersion else "sk_", propor="pk", cvtest="clas",
                      cvthres=1e-8, it_max=100, tie=tie, seed=rng_seed)
        if init.startswith("param_file"):
            if init == "param_file_default":
                if Q != 3:
                    raise ValueError("the default parameter file describes 3 classes")
                prop, center, disp = synth.default_init(d, low_disp)
            else:
                prop, center, disp = params
            eng.set_params(prop, center, disp)
            res = eng.run()
        else:
            res = eng.run_random(50, rng_seed)
    finally:
        eng.close()
    return partition_dicts(res, names, Q, init)


def partition_dicts(res, names, Q=3, init="param_file_default"):
    """What run_partitioning makes of a finished NEM run (ppanggolin.py:1886-1980), from the run's full-precision
    results instead of the `.uf` / `.mf` text: res = dict(status, c [n, Q], center [Q, d], disp [Q, d], prop [Q])."""
    n = len(names)
    partitions = ["U"] * n
    all_parameters = {}
    if res["status"] != 0:                                    # empty class: nem() writes no files, everything stays 'U'
        return dict(zip(names, partitions)), all_parameters
    mus, epss = class_sums(res["center"], res["disp"], Q)
    for k in range(Q):
        all_parameters[k] = (mus[k], epss[k], float(res["prop"][k]))
    partition = None
    if init == "param_file_default":
        partition = class_partition([sum(m) for m in mus], [sum(e) for e in epss])
        if partition is None:
            return dict(zip(names, partitions)), all_parameters       # the reference's ValueError branch: all 'U'
    c3 = np.round(res["c"].astype(np.float64), 3)             # what survives the " %5.3f" of .uf
    top = c3.max(axis=1, keepdims=True)
    for i in range(n):                                        # ppanggolin.py:1959-1972
        pos = np.flatnonzero(c3[i] == top[i])
        if init == "param_file_default":
            partitions[i] = "S" if len(pos) > 1 else partition[int(pos[-1])]
        else:
            partitions[i] = int(pos[-1])
    return dict(zip(names, partitions)), all_parameters


CODES = "PSCU"                                                # the vote's codes: P = 0, S = 1, C = 2, U = 3


def class_sums(center, disp, Q=3):
    """Per class the truth of every centre and every dispersion as Python floats (ppanggolin.py:1907-1923): what
    sum_mu / sum_eps add up -- Python's sum, left to right, in float64 (a NaN centre is true)."""
    mus = [[bool(float(v)) for v in center[k]] for k in range(Q)]
    epss = [[float(v) for v in disp[k]] for k in range(Q)]
    return mus, epss


def class_partition(sum_mu, sum_eps):
    """{class: 'P'|'S'|'C'} of run_partitioning (ppanggolin.py:1925-1957), or None where the reference raises its
    ValueError and everything is 'U'.  max() keeps the first of equal values, .index() finds it."""
    persistent_k = sum_mu.index(max(sum_mu))
    shell_k = sum_eps.index(max(sum_eps))
    cloud = list(set([0, 1, 2]) - set([persistent_k, shell_k]))
    partition = {persistent_k: "P", shell_k: "S"}
    if cloud:
        partition[cloud[0]] = "C"
    if partition.get(0) != "P" or partition.get(1) != "S" or partition.get(2) != "C":
        return None
    return partition


def vote_map(status, center, disp):
    """The codes a run's labels 0, 1, 2 vote with (uint8 [3]): P/S/C, or U for all three when the run emptied a class
    (no .uf) or the class map is the ValueError branch.  NCEM posteriors are 0/1, so the .uf rule 'ties go to S'
    never fires: a run's label is its vote's class."""
    if status != 0:
        return np.full(3, 3, np.uint8)
    mus, epss = class_sums(center, disp, 3)
    part = class_partition([sum(m) for m in mus], [sum(e) for e in epss])
    if part is None:
        return np.full(3, 3, np.uint8)
    return np.array([CODES.index(part[k]) for k in range(3)], np.uint8)


def vote_state(n, pan):
    """An empty vote over n families of which `pan` (bool [n]) are the pangenome."""
    return dict(cnt=np.zeros((n, 4), np.int64), pan=np.asarray(pan, bool).copy(), validated=np.zeros(n, bool),
                forced=np.zeros(n, bool), first=np.full(n, -1, np.int64), samples=0)


def vote_host(state, samples, n_sel, chunk_size):
    """validate_family and partition()'s loop (ppanggolin.py:1015-1037, 1045-1098) over a stream of samples, in numpy:
    family-parallel, sample after sample.  samples: (families, labels, codes) -- the master indices of the families a
    sample keeps, their labels 0..2, the codes (vote_map) the labels vote with.  Every vote counts, validated or not;
    an unvalidated family is validated by the vote that makes its total exceed n_sel / chunk_size (a float64
    quotient) with an absolute majority, or exceed n_sel -- U is forced if it has none then.  Stops after the sample
    that validates the last family of the pangenome: returns its index in `samples`, or -1 (all counted).  `state`
    (vote_state) is updated in place."""
    cnt, validated, forced, first, pan = state["cnt"], state["validated"], state["forced"], state["first"], state["pan"]
    quotient = n_sel / chunk_size
    unval = int(np.count_nonzero(pan & ~validated))
    for s, (fam, lab, codes) in enumerate(samples):
        state["samples"] += 1
        fam = np.asarray(fam, np.int64)
        if len(fam) == 0:
            continue
        code = np.asarray(codes, np.uint8)[np.asarray(lab, np.int64)]
        cnt[fam, code] += 1                                   # (a family appears once per sample)
        open_ = fam[~validated[fam]]
        c = cnt[open_]
        tot, mx = c.sum(axis=1), c.max(axis=1)
        ok = ((tot > quotient) & (2 * mx >= tot)) | (tot > n_sel)
        newly = open_[ok]
        validated[newly] = True
        first[newly] = state["samples"] - 1
        forced[newly[2 * mx[ok] < tot[ok]]] = True
        unval -= len(newly)
        if unval == 0:
            return s
    return -1


def vote_final(state):
    """max(cnt, key=cnt.get) per family in the order P, S, C, U (ppanggolin.py:1104-1105), U where it was forced;
    0xFF outside the pangenome."""
    out = np.argmax(state["cnt"], axis=1).astype(np.uint8)     # (argmax: the first of equal counts)
    out[state["forced"]] = 3
    out[~state["pan"]] = 0xFF
    return out
