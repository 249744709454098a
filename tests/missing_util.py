"""Host statement of NCEM on a matrix with missing cells, in plain numpy -- what the reference's NEM computes when a
cell of the .dat is `nan` (DensBernoulli nem_mod.c:654, EstimSizes :1310, ComputeMedian :1455, EstimLaplaceIner :1682,
InerToDisp* in their MISSING_IGNORE branches :988-1170, forced for Bernoulli :446-448).

density_masked_host and mstep_masked_host restate the two steps that see the matrix; run_masked_host is NemAlgo
(nem_alg.c:1789-1852) around them, with Oracle.sweep and Oracle.crit for the parts that do not.  With an all-ones mask
the two steps equal Oracle.density / Oracle.mstep bit for bit (tests/test_missing_host.py), and the run reproduces the
recorded reference on every fixture under tests/golden/missing/.

x: (n, d) 0/1 (the value of an unobserved cell is never read), obs: (n, d) bool.
"""
import gzip
import json
import math
import os

import numpy as np

EPSILON = 1e-20                                              # nem_typ.h:63
F32 = np.float32
MISSING_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "missing")
DISPERSIONS = ("s__", "sk_", "s_d", "skd")


# ---- E1 -----------------------------------------------------------------------------------------------------------
def _exp(v):
    """the C library's exp of a double (numpy's vector exp need not round as libm does)"""
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def density_masked_host(x, obs, prop, center, disp):
    """ComputePkFkiM (nem_alg.c:2234-2289) over DensBernoulli with the unobserved cells skipped.
    Returns (PkFki float64 (n, k), LogPkFki float32 (n, k), status: 2 when a proportion is <= EPSILON)."""
    x = np.asarray(x).astype(bool)
    obs = np.asarray(obs, bool)
    n, d = x.shape
    prop = np.asarray(prop, F32)
    k = len(prop)
    center = np.asarray(center, F32).reshape(k, d)
    disp = np.asarray(disp, F32).reshape(k, d)
    pkfki = np.zeros((n, k), np.float64)
    logpkfki = np.zeros((n, k), F32)
    sts = 0
    for h in range(k):
        dk = np.zeros(n, F32)
        nul = np.zeros(n, bool)
        for j in range(d):
            o = obs[:, j]
            if not o.any():
                continue
            eps, mu = disp[h, j], center[h, j]
            ad0 = abs(int(F32(0.0) - mu))                    # abs((int)(x - mu)), :658
            ad1 = abs(int(F32(1.0) - mu))
            if float(eps) > EPSILON:                         # :660-661
                l1 = math.log(float((F32(1.0) - eps) / eps))
                l0 = math.log(float(F32(1.0) - eps))
                add = np.where(x[:, j], ad1 * l1, ad0 * l1)
                with np.errstate(invalid="ignore", over="ignore"):
                    step = ((dk.astype(np.float64) + add) - l0).astype(F32)
                dk = np.where(o, step, dk)
            else:                                            # :662-669
                nul |= o & np.where(x[:, j], ad1 != 0, ad0 != 0)
        logfk = np.where(nul, -F32(np.finfo(F32).max), -dk).astype(F32)
        fk = np.array([0.0 if z else _exp(float(v)) for v, z in zip(logfk, nul)], np.float64)   # :676-688
        pk = float(prop[h])
        if pk > EPSILON:
            logpk = F32(math.log(pk))
        else:
            logpk = F32(-np.inf)
            sts = 2
        pkfki[:, h] = pk * fk
        with np.errstate(invalid="ignore"):
            logpkfki[:, h] = logpk + logfk
    return pkfki, logpkfki, sts


# ---- M ------------------------------------------------------------------------------------------------------------
def _median_walk(xj, oj, ch, totwei):
    """ComputeMedian (nem_mod.c:1439-1477) for one (class, variable): the observations in ascending order -- the observed
    zeros, then the observed ones (NaN sorts last, CompSortValue nem_alg.c:1557-1568) -- cumulated weight against
    totwei / 2, and the midway rule when the two are equal.  ch: the class's memberships (0/1 floats)."""
    order = np.concatenate([np.flatnonzero(oj & ~xj), np.flatnonzero(oj & xj)])
    vals = np.concatenate([np.zeros(int((oj & ~xj).sum()), F32), np.ones(int((oj & xj).sum()), F32)])
    halfwei = F32(totwei) / F32(2)
    cum = F32(0.0)
    i = 0
    while i < len(order) and cum < halfwei:
        cum = F32(cum + ch[order[i]])
        i += 1
    imed = i - 1
    if float(cum) > float(halfwei) + EPSILON:
        return vals[imed]
    i = imed + 1
    while ch[order[i]] < EPSILON:
        i += 1
    return F32(0.5) * (vals[imed] + vals[i])


def mstep_masked_host(x, obs, c, disper, propor, prop, center, disp):
    """EstimPara for FAMILY_BERNOULLI (MISSING_IGNORE) on a hard partition c (n, k) of 0/1 floats.  Returns the keys
    of Oracle.mstep.  A (class, variable) without an observed member keeps its centre (:1399-1401) and, under skd, its
    dispersion (:1166); the reference itself reads out of bounds there (ComputeMedian with total weight 0), so that
    branch is stated here and never recorded."""
    x = np.asarray(x).astype(bool)
    obs = np.asarray(obs, bool)
    c = np.asarray(c, F32)
    assert np.all((c == 0) | (c == 1)), "the masked statement is for hard (NCEM) partitions"
    n, d = x.shape
    k = c.shape[1]
    prop = np.array(prop, F32)
    center = np.array(center, F32).reshape(k, d)
    disp = np.array(disp, F32).reshape(k, d)
    nk = np.zeros(k, F32)
    nkd = np.zeros((k, d), F32)
    iner = np.zeros((k, d), F32)
    emptyk = 0
    # EstimSizes :1293-1315 (0/1 memberships: the float sums are exact counts below 2^24)
    for h in range(k):
        nk[h] = F32(c[:, h].sum(dtype=np.float64))
        nkd[h] = (c[:, h][:, None] * obs).sum(axis=0, dtype=np.float64).astype(F32)
    # EstimLaplaceCenters :1358-1412
    for h in range(k):
        if not float(nk[h]) > EPSILON:
            emptyk = h + 1
            continue
        for j in range(d):
            if float(nkd[h, j]) >= EPSILON:
                center[h, j] = _median_walk(x[:, j], obs[:, j], c[:, h], nkd[h, j])
    # EstimLaplaceIner :1669-1686: i-ordered float sum of cih * |xij - centre| over the observed cells
    for h in range(k):
        member = c[:, h] > 0
        for j in range(d):
            sel = member & obs[:, j]
            terms = np.abs(x[sel, j].astype(F32) - center[h, j]).astype(F32)
            iner[h, j] = np.add.accumulate(terms, dtype=F32)[-1] if len(terms) else F32(0.0)
    # InerToDisp*, MISSING_IGNORE
    if disper == "s__":                                      # :988-1015
        vol, nobs = F32(0.0), F32(0.0)
        for h in range(k):
            if nk[h] > 0:
                for j in range(d):
                    vol = F32(vol + iner[h, j])
                    nobs = F32(nobs + nkd[h, j])
        with np.errstate(invalid="ignore", divide="ignore"):
            disp[:, :] = F32(vol) / F32(nobs)
    elif disper == "sk_":                                    # :1043-1073
        for h in range(k):
            if nk[h] > 0:
                sn = np.add.accumulate(nkd[h], dtype=F32)[-1]
                si = np.add.accumulate(iner[h], dtype=F32)[-1]
                with np.errstate(invalid="ignore", divide="ignore"):
                    disp[h, :] = F32(si) / F32(sn)
    elif disper == "s_d":                                    # :1104-1126
        for j in range(d):
            sn = np.add.accumulate(nkd[:, j], dtype=F32)[-1]
            si = np.add.accumulate(iner[:, j], dtype=F32)[-1]
            with np.errstate(invalid="ignore", divide="ignore"):
                disp[:, j] = F32(si) / F32(sn)
    elif disper == "skd":                                    # :1152-1170
        for h in range(k):
            for j in range(d):
                if float(nkd[h, j]) > EPSILON:
                    disp[h, j] = iner[h, j] / nkd[h, j]
    else:
        raise ValueError(disper)
    if propor == "pk":                                       # EstimPara :456-465
        prop = (nk / F32(n)).astype(F32)
    else:
        prop = np.full(k, F32(1.0 / k), F32)
    return dict(status=2 if emptyk else 0, prop=prop, center=center, disp=disp, nbobs_k=nk, nbobs_kd=nkd, iner=iner,
                emptyk=emptyk)


# ---- the run --------------------------------------------------------------------------------------------------------
def run_masked_host(oracle, x, obs, nei, k, prop, center, disp, beta=0.5, disper="sk_", propor="pk", cvtest="clas",
                    cvthres=1e-8, it_max=100, tie="first", seed=0):
    """ClassifyByNem, INIT_PARAM_FILE + NemAlgo (nem_alg.c:1151-1169, 1746-1879), NCEM.  Keys as Oracle.run."""
    n, d = np.asarray(x).shape
    prop = np.array(prop, F32)
    center = np.array(center, F32).reshape(k, d)
    disp = np.array(disp, F32).reshape(k, d)
    c = np.zeros((n, k), F32)
    sweep = 0
    nzero = 0
    pk, lp, _ = density_masked_host(x, obs, prop, center, disp)
    for b in (0.0, beta):                                    # the blind sweep, then the sweep with the real beta
        c, nz = oracle.sweep(c, nei, b, pk, True, tie=tie, seed=seed, sweep_id=sweep)
        sweep += 1
        nzero += nz
    status, emptyk, converged, iters = 0, 0, False, 0
    nbobs_k = np.zeros(k, F32)
    it = 1
    while it <= it_max and not converged and status == 0:
        cold = c.copy()
        m = mstep_masked_host(x, obs, c, disper, propor, prop, center, disp)
        prop, center, disp, nbobs_k = m["prop"], m["center"], m["disp"], m["nbobs_k"]
        status, emptyk = m["status"], m["emptyk"]
        if status == 0:
            pk, lp, _ = density_masked_host(x, obs, prop, center, disp)
            c, nz = oracle.sweep(c, nei, beta, pk, True, tie=tie, seed=seed, sweep_id=sweep)
            sweep += 1
            nzero += nz
            if cvtest == "clas":                             # HasConverged :2075-2089
                converged = bool(float(np.max(np.abs(c - cold))) < cvthres)
        it += 1
    iters = it - 1
    if iters == 0:                                           # :1845-1851
        m = mstep_masked_host(x, obs, c, disper, propor, prop, center, disp)
        prop, center, disp, nbobs_k, emptyk = m["prop"], m["center"], m["disp"], m["nbobs_k"], m["emptyk"]
        pk, lp, _ = density_masked_host(x, obs, prop, center, disp)
    crit = oracle.crit(c, nei, beta, pk, lp)
    return dict(status=status, c=c, prop=prop, center=center, disp=disp, nbobs_k=nbobs_k, crit=crit, iters=iters,
                converged=converged, emptyk=emptyk, n_zero_density=nzero, pkfki=pk, logpkfki=lp)


# ---- files and fixtures ---------------------------------------------------------------------------------------------
NAN_TOKENS = ("nan", "NaN", "nan(0)")


def write_masked_inputs(nem_dir, x, obs, nei, prop, center, disp, tokens=("nan", "NaN")):
    """The five input files of nem() with the unobserved cells of the .dat written as nan tokens (cycling through
    `tokens`).  Returns the base name."""
    from pangenomenem_amd import nemfiles
    x = np.asarray(x, np.uint8)
    obs = np.asarray(obs, bool)
    base = nemfiles.write_nem_inputs(nem_dir, np.where(obs, x, 0), nei, prop, center, disp)
    t = 0
    lut = np.array(["0", "1"], dtype=object)
    with open(base + ".dat", "w") as f:
        for row, orow in zip(x, obs):
            cells = lut[row]
            for j in np.flatnonzero(~orow):
                cells[j] = tokens[t % len(tokens)]
                t += 1
            f.write("\t".join(cells) + "\n")
    return base


def fixture_names():
    with open(os.path.join(MISSING_DIR, "manifest.json")) as f:
        return [m["name"] for m in json.load(f)]


def load_fixture(name):
    d = os.path.join(MISSING_DIR, name)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    inp = np.load(os.path.join(MISSING_DIR, meta.get("inputs_of", name), "inputs.npz"))   # (cases that share their inputs)
    n, dd = int(inp["n"]), int(inp["d"])
    x = np.unpackbits(inp["xbits"], axis=1, bitorder="little")[:, :dd].astype(np.uint8)
    obs = np.unpackbits(inp["obits"], axis=1, bitorder="little")[:, :dd].astype(bool)
    nei = (inp["nei_ptr"], inp["nei_idx"], inp["nei_w"]) if bool(inp["has_graph"]) else None
    case = dict(name=name, meta=meta, cfg=meta["cfg"], x=x, obs=obs, nei=nei, k=int(inp["k"]), prop=inp["prop"],
                center=inp["center"], disp=inp["disp"])
    for ext in ("uf", "mf", "log"):
        case["ref_" + ext] = gzip.open(os.path.join(d, "ref_%s.txt.gz" % ext), "rb").read()
    return case


def parse_uf(text, k):
    """labels (n,) from the .uf text of an NCEM run (one-hot rows of ' %5.3f ')."""
    rows = np.array([[float(t) for t in ln.split()] for ln in text.decode().split("\n") if ln.strip()], np.float64)
    assert rows.shape[1] == k and np.all((rows == 0) | (rows == 1)) and np.all(rows.sum(axis=1) == 1)
    return rows.argmax(axis=1)


def parse_mf(text, k, d):
    """(prop (k,), center (k, d), disp (k, d)) as printed in the .mf (nem_exe.c:1708-1774)."""
    lines = text.decode().split("\n")
    at = next(i for i, ln in enumerate(lines) if ln.startswith("Mu (")) + 2
    prop, center, disp = np.zeros(k), np.zeros((k, d)), np.zeros((k, d))
    for h in range(k):
        t = [float(v) for v in lines[at + h].split()]
        assert len(t) == 2 * d + 1
        center[h], prop[h], disp[h] = t[:d], t[d], t[d + 1:]
    return prop, center, disp
