#!/usr/bin/env python3
"""Record the UNMODIFIED reference's nem() on matrices with missing cells -> tests/golden/missing/.

Runs only where the reference sources exist: oracle/Makefile compiles them where they lie (oracle/_ref/libnem_ref.so)
and this script calls nem() through oracle.pyoracle.Reference on the five ASCII input files, the unobserved cells of
the .dat written as `nan` / `NaN`.  A fixture is data only: the inputs (matrix and observed mask as packed bits, CSR
graph, the .m parameters, the call's configuration) and the text of the reference's .uf, .mf and .log, gzipped.

A case is kept only if
  (a) two runs at least one second apart give byte-identical files (nem() seeds its tie stream with time(NULL): a
      case that ties is not a fixture), and
  (b) in the reference's final partition every (class, organism) has at least 2 observed families -- a (class,
      organism) without one makes the reference call ComputeMedian with total weight 0, which reads out of bounds.

    python tests/golden/make_missing.py
"""
import gzip
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402
from pangenomenem_amd import synth  # noqa: E402
from tests import missing_util  # noqa: E402

OUT = missing_util.MISSING_DIR


def mask_for(n, d, seed, frac=0.15):
    """frac of the cells missing at random, plus: one family without an observed cell, a fully missing 32-organism
    word in one row, the last cell of the last row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    obs = rng.random((n, d)) >= frac
    obs[n // 3, :] = False
    obs[n // 2, 0:min(32, d)] = False
    obs[n - 1, d - 1] = False
    return obs


def case_list():
    cases = []

    def add(name, n, d, k, seed, **cfg):
        base = dict(algo="ncem", beta=0.5, disper="sk_", propor="pk", cvtest="clas", cvthres=1e-8, it_max=100)
        base.update(cfg)
        x, _ = synth.bernoulli_pa_matrix(n, d, seed)
        nei = synth.contiguity_graph(n, seed, weights="coverage", d=d)      # chain + chords, integer weights 1..d
        prop, center, disp = synth.default_init(d) if k == 3 else synth.kclass_init(x, k)
        if k == 2:
            # unequal proportions: the family without an observed cell has the same density in every class and would
            # tie under kclass_init's equal ones (the last one as ReadParamFile takes it, nem_exe.c:1022-1034)
            prop = np.array([np.float32(0.4), np.float32(1.0) - np.float32(0.4)], np.float32)
        cases.append(dict(name=name, x=x, obs=mask_for(n, d, seed + 100), nei=nei, k=k, prop=prop, center=center,
                          disp=disp, cfg=base))

    for disper in missing_util.DISPERSIONS:
        add("m300x40_" + disper, 300, 40, 3, 31, disper=disper)
        if disper != missing_util.DISPERSIONS[0]:           # the same inputs four times: stored with the first
            cases[-1]["inputs_of"] = "m300x40_" + missing_util.DISPERSIONS[0]
    add("m600x520_skd", 600, 520, 3, 32, disper="skd")
    add("m257x33_k2", 257, 33, 2, 33)
    add("m300x40_beta0", 300, 40, 3, 34, beta=0.0)
    return cases


def run_reference(ref, case, tmp):
    cfg = case["cfg"]
    base = missing_util.write_masked_inputs(tmp, case["x"], case["obs"], case["nei"], case["prop"], case["center"],
                                            case["disp"])
    rc = ref.nem(base, case["k"], algo=cfg["algo"].encode(), beta=cfg["beta"], convergence=cfg["cvtest"].encode(),
                 convergence_th=cfg["cvthres"], format=b"fuzzy", it_max=cfg["it_max"], dolog=1,
                 proportion=cfg["propor"].encode(), dispersion=cfg["disper"].encode(), init_mode=2)
    out = {ext: open(base + "." + ext, "rb").read() if os.path.isfile(base + "." + ext) else None
           for ext in ("uf", "mf", "log", "stderr")}
    return rc, out


def generate(ref, case):
    name, k = case["name"], case["k"]
    n, d = case["x"].shape
    runs = []
    for _ in range(2):
        tmp = tempfile.mkdtemp(prefix="nemmiss_")
        runs.append(run_reference(ref, case, tmp))
        shutil.rmtree(tmp)
        time.sleep(1.1)
    (rc, a), (rc2, b) = runs
    if rc != 0 or rc2 != 0 or any(a[e] is None for e in ("uf", "mf", "log")):
        print("%-16s DROPPED: nem() returned %d / %d" % (name, rc, rc2))
        return None
    same = a["uf"] == b["uf"] and a["mf"] == b["mf"] and a["log"].split(b"\n")[1:] == b["log"].split(b"\n")[1:]
    if not same:
        print("%-16s DROPPED: two runs differ (a tie: the reference's stream is seeded with the time)" % name)
        return None
    labels = missing_util.parse_uf(a["uf"], k)
    least = min(int((case["obs"][labels == h]).sum(axis=0).min()) if (labels == h).any() else 0 for h in range(k))
    if least < 2:
        print("%-16s DROPPED: a (class, organism) with %d observed families" % (name, least))
        return None
    text = (a["stderr"] or b"").decode("latin1")
    m = re.search(r"NEM (converged|did not converge) after (\d+) iterations", text)
    out = os.path.join(OUT, name)
    if os.path.isdir(out):
        shutil.rmtree(out)
    os.makedirs(out)
    nei = case["nei"]
    if "inputs_of" not in case:
        np.savez_compressed(os.path.join(out, "inputs.npz"), n=n, d=d, k=k, has_graph=True,
                            xbits=np.packbits(np.where(case["obs"], case["x"], 0).astype(np.uint8), axis=1, bitorder="little"),
                            obits=np.packbits(case["obs"], axis=1, bitorder="little"),
                            nei_ptr=nei[0], nei_idx=nei[1], nei_w=nei[2], prop=case["prop"], center=case["center"],
                            disp=case["disp"])
    for ext in ("uf", "mf", "log"):
        with open(os.path.join(out, "ref_%s.txt.gz" % ext), "wb") as raw:
            with gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as g:
                g.write(a[ext])
    meta = dict(name=name, n=n, d=d, k=k, cfg=case["cfg"], nem_rc=int(rc), iters=int(m.group(2)) if m else None,
                converged=bool(m and m.group(1) == "converged"), n_missing=int((~case["obs"]).sum()),
                least_observed=least)
    if "inputs_of" in case:
        meta["inputs_of"] = case["inputs_of"]
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("%-16s n=%4d d=%4d k=%d iters=%s converged=%s missing=%d least observed per (class, organism)=%d" %
          (name, n, d, k, meta["iters"], meta["converged"], meta["n_missing"], least), flush=True)
    return meta


def main():
    pyoracle.build(ref=True)
    ref = pyoracle.Reference()
    os.makedirs(OUT, exist_ok=True)
    manifest = [m for m in (generate(ref, c) for c in case_list()) if m is not None]
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
