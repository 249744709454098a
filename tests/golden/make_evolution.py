#!/usr/bin/env python3
"""Record the resamples of PPanGGOLiN's --evolution under tests/golden/evolution/ (what tests/test_evolution_host.py
holds pangenomenem_amd.evolution against).

Each case seeds the global `random`, calls the reference's own `utils.samplingCombinations` on positions
0 .. D - 1, then does what the driver does with it (ppanggolin/command_line.py:599-604: flatten in dict order, keep
nb_org % STEP == 0 and nb_org <= LIMIT, `shuffle` on the global `random`; a combination's OrderedSet keeps its draw
order, so a list stands for it), and stores the result with the next `random.random()`.  Large results are stored
as a sha256 of their JSON text.  The reference is read only here, while recording:

    python tests/golden/make_evolution.py PATH_TO_PPANGGOLIN_SOURCE_TREE
"""
import hashlib
import importlib.util
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "evolution")
FULL_LIMIT = 60            # D up to this: the draws themselves are stored

# name, D, ratio, min, max (None: no cap), STEP, LIMIT (None: Inf), seed, step of samplingCombinations itself
CASES = [
    ("d3", 3, 0.1, 10, 30, 1, None, 1, 1),
    ("d4", 4, 0.1, 10, 30, 1, None, 2, 1),
    ("d6_seed1", 6, 0.1, 10, 30, 1, None, 1, 1),
    ("d6_seed7", 6, 0.1, 10, 30, 1, None, 7, 1),
    ("d40", 40, 0.1, 10, 30, 1, None, 3, 1),
    ("d40_step3", 40, 0.1, 10, 30, 3, None, 5, 1),
    ("d40_limit12", 40, 0.1, 10, 30, 1, 12, 6, 1),
    ("d20_max_below_min", 20, 0.1, 10, 4, 1, None, 8, 1),
    ("d12_ratio_tiny", 12, 0.001, 10, 30, 1, None, 9, 1),
    ("d12_ratio_big_no_max", 12, 5.0, 3, None, 1, None, 10, 1),
    ("d15_combinations_step2", 15, 0.1, 10, 30, 1, None, 11, 2),
    ("d300", 300, 0.1, 10, 30, 1, None, 4, 1),
]


def digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(",", ":")).encode()).hexdigest()


def load_utils(src):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ppanggolin_utils", os.path.join(src, "ppanggolin", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record(utils, name, d, ratio, rmin, rmax, step, limit, seed, sc_step):
    random.seed(seed)
    combinations = utils.samplingCombinations(list(range(d)), sample_ratio=ratio, sample_min=rmin, sample_max=rmax, step=sc_step)
    comb = [[k, [list(c) for c in cs]] for k, cs in combinations.items()]
    lim = sys.maxsize if limit is None else limit
    shuffled = [list(c) for nb_org, cs in combinations.items() for c in cs if nb_org % step == 0 and nb_org <= lim]
    random.shuffle(shuffled)
    out = dict(name=name, n_items=d, ratio=ratio, rmin=rmin, rmax=rmax, step=step, limit=limit, seed=seed, sc_step=sc_step,
               sizes=[[k, len(cs)] for k, cs in combinations.items()], combinations_sha256=digest(comb),
               resamples_sha256=digest(shuffled), n_resamples=len(shuffled), next_random=repr(random.random()))
    if d <= FULL_LIMIT:
        out["combinations"] = comb
        out["resamples"] = shuffled
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    utils = load_utils(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        rec = record(utils, *case)
        with open(os.path.join(OUT, case[0] + ".json"), "w") as f:
            json.dump(rec, f, separators=(",", ":"))
            f.write("\n")
        print(case[0], rec["n_resamples"], "resamples")


if __name__ == "__main__":
    main()
