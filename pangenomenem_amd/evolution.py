"""PPanGGOLiN's evolution curves (the CLI's ``--evolution``) from one master on the device.

``--evolution`` draws resamples of the organisms, partitions every one of them and writes one line of
``evolutions/evol_stats.txt`` per resample (ppanggolin/command_line.py:262-281 and 591-625):

  * the draws (``utils.samplingCombinations``, ppanggolin/utils.py:54-78): for every size k = 1 .. D - 1 (D organisms;
    k never reaches D), ``sample_min`` draws capped at ``sample_max``.  The intended count, comb(D, k) / sample_ratio,
    never applies: the call is ``comb_k_n(item_size, k)`` with its arguments swapped, which is 0 for k < D, so
    ``sample_ratio`` changes nothing.  Each draw is ``random.sample(items, k)`` on the global ``random``; a draw equal
    (as a list, so in order) to an earlier one of its size is dropped but still counts towards the size's draws;
  * the driver flattens them, sizes ascending and draws in draw order, keeps ``k % STEP == 0 and k <= LIMIT`` and
    shuffles the list with the same global ``random``; a resample's column order is its draw order;
  * every resample is ``partition(organisms=subset, inplace=False, just_stats=True)``: with at most ``chunk_size``
    organisms one NCEM run, which draws nothing from ``random``; with more, partition()'s vote loop, which draws its
    samples from that same stream;
  * the line is ``nb_org,persistent,shell,cloud,core_exact,accessory,pangenome``, with ``NA`` for the three NEM counts
    whenever a family is undefined; the file starts with a header and a line for the full pangenome.

With ``--cpu 1`` one worker runs the resamples in shuffled order on one continuing stream: that run is what
``Master.evolution`` reproduces.  The small resamples touch no stream, so all of them are solved in ONE library call
(``nemgpu_resamples_solve``: the chunk pipeline, each run reduced on the device to its six counts); the large ones run
one after another through ``Master.partition``, each from the stream state the previous one left.

Draws are made by position (``rng.sample(range(D), k)`` picks the same positions as sampling the organisms
themselves), so a resample is a list of the master's organism indices; the master's columns must be in the order of
the pangenome's organisms.
"""
import ctypes as C
import random

import numpy as np

from .chunks import Chunk
from .engine import STATUS_OK, Config, NemGpuError

STATS = ("persistent", "shell", "cloud", "undefined", "core_exact", "accessory")    # a resample's row of counts
HEADER = ("nb_org", "persistent", "shell", "cloud", "core_exact", "accessory", "pangenome")


def sampling_combinations(n_items, sample_ratio, sample_min, sample_max=100, step=1, rng=None):
    """utils.samplingCombinations over positions 0 .. n_items - 1: {k: [draw, ...]} for the sizes that kept a draw,
    in ascending order.  The number of draws of a size is ceil(comb_k_n(n_items, k) / sample_ratio), raised to
    sample_min, then capped at sample_max (None: no cap).  comb_k_n(n_items, k) is 0 for every k < n_items (its
    arguments are the wrong way round), so the count is sample_min capped at sample_max whatever sample_ratio is."""
    rng = random if rng is None else rng
    out = {}
    for k in range(1, n_items, step):
        draws = 0                                             # ceil(0 / sample_ratio)
        if draws < sample_min:
            draws = sample_min
        if sample_max is not None and draws > sample_max:
            draws = sample_max
        kept, seen = [], set()
        for _ in range(draws):
            comb = rng.sample(range(n_items), k)
            key = tuple(comb)
            if key not in seen:                               # sampling without replacement (the draw is still made)
                seen.add(key)
                kept.append(comb)
        if kept:
            out[k] = kept
    return out


def evolution_resamples(n_items, ratio=0.1, rmin=10, rmax=30, step=1, limit=None, rng=None):
    """The driver's list of resamples (command_line.py:599-604): the draws of sampling_combinations flattened (sizes
    ascending, draws in draw order), those with k % step == 0 and k <= limit kept (None: no limit), then shuffled with
    rng.shuffle.  Each resample is a list of organism positions in draw order."""
    rng = random if rng is None else rng
    comb = sampling_combinations(n_items, ratio, rmin, rmax, 1, rng)
    out = [c for k, draws in comb.items() for c in draws if k % step == 0 and (limit is None or k <= limit)]
    rng.shuffle(out)
    return out


def resample_stats_host(x, organisms, labels, codes):
    """One resample's counts in numpy (partition(just_stats=True), ppanggolin.py:982-993 and 1166-1170): int64 [6] =
    persistent, shell, cloud, undefined (labels: the run's labels 0 .. 2 of the families the resample keeps, in master
    order; codes: the codes 0 .. 3 they stand for, partitioning.vote_map), core_exact (the families in every one of
    `organisms`), accessory (the other kept ones)."""
    sub = np.asarray(x, np.uint8)[:, np.asarray(organisms, np.int64)]
    kept = sub.any(axis=1)
    core = kept & sub.all(axis=1)
    out = np.zeros(6, np.int64)
    lab = np.asarray(labels, np.int64)
    if len(lab):
        out[:4] = np.bincount(np.asarray(codes, np.int64)[lab], minlength=4)[:4]
    out[4] = np.count_nonzero(core)
    out[5] = np.count_nonzero(kept) - out[4]
    return out


def resample_stats(master, samples, beta=0.5, free_dispersion=False, tie="libc", seed=0, workers=8, group=32):
    """nemgpu_resamples_solve: the samples (lists of organism indices, each at most chunk_size long as the reference
    solves them) as single NCEM runs from PPanGGOLiN's default .m, in one call.  Returns int32 [count][6] (STATS)."""
    lib = master.lib
    _bind(lib)
    stats = np.zeros((len(samples), 6), np.int32)
    if not len(samples):
        return stats
    prop, center_k, disp_k, cfg = master._config(3, (0.33333, 0.33333, None), (1.0, 0.5, 0.0), (0.1, 0.5, 0.1), "ncem", beta,
                                                 "skd" if free_dispersion else "sk_", "pk", "clas", 1e-8, 100, False, tie, seed)
    arr = (Chunk * len(samples))()
    hold = [np.ascontiguousarray(s, np.int32) for s in samples]
    for q, org in zip(arr, hold):
        q.organisms, q.dc = org.ctypes.data, len(org)
    rc = lib.nemgpu_resamples_solve(master._h, arr, len(samples), 3, prop.ctypes.data, center_k.ctypes.data, disp_k.ctypes.data,
                                    C.byref(cfg), int(workers), int(group), stats.ctypes.data)
    if rc != STATUS_OK:
        err = NemGpuError("nemgpu_resamples_solve failed (status %d): %s" % (rc, lib.nemgpu_last_error().decode()))
        err.status = rc
        raise err
    return stats


def evolution_rows(resamples, rng, chunk_size, solve_small, solve_large):
    """The rows of the --cpu 1 run, in the resamples' (shuffled) order: int64 [count][7] = nb_org, then STATS.
    solve_small(list of resamples) -> [m][6] solves every resample of at most chunk_size organisms at once (they draw
    nothing); solve_large(resample, rng) -> [6] runs one larger resample's vote loop on rng, one after another in
    order, so rng ends where the reference's sequential loop leaves it."""
    rows = np.zeros((len(resamples), 7), np.int64)
    rows[:, 0] = [len(r) for r in resamples]
    small = [i for i, r in enumerate(resamples) if len(r) <= chunk_size]
    if small:
        rows[small, 1:] = np.asarray(solve_small([resamples[i] for i in small]), np.int64).reshape(len(small), 6)
    for i, r in enumerate(resamples):
        if len(r) > chunk_size:
            rows[i, 1:] = solve_large(r, rng)
    return rows


def partition_stats_row(stats):
    """Master.partition(just_stats=True)'s dict (or the tuple it returns) as a row of STATS"""
    if isinstance(stats, tuple):
        stats = stats[0]
    return np.array([stats.get(s, 0) for s in STATS], np.int64)


def evol_stats_text(full_stats, rows, nb_organisms):
    """evol_stats.txt as the reference writes it (command_line.py:273-279, 606-617): the header, the full pangenome's
    line (full_stats: what Master.partition(just_stats=True) returned for all nb_organisms organisms; no NA rule there),
    then one line per row of evolution_rows, NA for persistent / shell / cloud when a family is undefined."""
    p, s, c, _, core, acc = (int(v) for v in partition_stats_row(full_stats))
    lines = [",".join(HEADER), ",".join(str(v) for v in (int(nb_organisms), p, s, c, core, acc, acc + core))]
    for r in np.asarray(rows, np.int64).reshape(-1, 7):
        nb, p, s, c, u, core, acc = (int(v) for v in r)
        nem = [str(p), str(s), str(c)] if u == 0 else ["NA"] * 3
        lines.append(",".join([str(nb)] + nem + [str(core), str(acc), str(core + acc)]))
    return "".join(line + "\n" for line in lines)


def write_evol_stats(path, full_stats, rows, nb_organisms):
    """evol_stats_text into `path`"""
    with open(path, "w") as f:
        f.write(evol_stats_text(full_stats, rows, nb_organisms))


def _bind(lib):
    if getattr(lib, "_resamples_bound", False):
        return
    lib.nemgpu_resamples_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(Config), C.c_int, C.c_int, C.c_void_p]
    lib._resamples_bound = True
