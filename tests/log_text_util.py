"""The text of the reference's <Fname>.log put together in Python from a list of per-iteration events (the oracle's
trace, oracle/pyoracle.py, or the engine's log events): the formats of StartLogFile, WriteLogHeader, WriteLogCrit and
WriteLogClasses as pangenomenem_amd/csrc/nem_capi.cpp restates them.  Test infrastructure only."""
import math

import numpy as np


def _f(v, width, dec):
    """" %<width>.<dec>f" of a float as C's printf prints it (Python's % prints "nan" for a NaN of either sign)."""
    v = float(v)
    if math.isnan(v):
        return " " + ("-nan" if math.copysign(1.0, v) < 0 else "nan").rjust(width)
    return " %*.*f" % (width, dec, v)


def log_mult(n):
    """what the criteria are multiplied by (nem_alg.c:1495, 2638)"""
    return np.float32(math.exp(-(int(math.log(n / 1000.) / math.log(10))) * math.log(10)))


def crit_text(crit6, mult):
    """WriteLogCrit: U, M and the error rate (no reference partition: NaN)"""
    c = np.asarray(crit6, np.float32)
    return _f(np.float32(c[2] * mult), 5, 0) + _f(np.float32(c[3] * mult), 5, 0) + _f(float("nan"), 5, 3)


def header_text(k, d):
    """WriteLogHeader (NbEIters = 1)"""
    out = "%4s  %5s %5s %5s" % ("It", "UM", "PM", "Er")
    out += " %3s%-2d %3s%-2d %3s%-2d" % ("UE", 1, "PE", 1, "Er", 1)
    out += " " + " %5s" % "Beta" + " "
    out += "".join(" %3s%02d" % ("P", h + 1) for h in range(k)) + " "

    def names(letter):
        return "".join(" %3s%02d_%1d" % (letter, h + 1, j + 1) for h in range(k) for j in range(d))

    return out + names("M") + " " + names("D") + " " + names("n") + "\n"


def classes_text(beta, prop, center, disp, sizes):
    """WriteLogClasses: beta, the proportions, the centres, the dispersions, NbObs_KD (a class's size for every
    organism: no missing data)"""
    k, d = np.asarray(center).shape
    out = " " + _f(np.float32(beta), 5, 3) + " "
    out += "".join(_f(v, 5, 3) for v in np.asarray(prop, np.float32)) + " "
    out += "".join(_f(v, 7, 3) for v in np.asarray(center, np.float32).ravel()) + " "
    out += "".join(_f(v, 7, 3) for v in np.asarray(disp, np.float32).ravel()) + " "
    out += "".join(_f(sizes[h], 7, 1) * d for h in range(k))
    return out + "\n"


def _preamble(n, mult):
    return "NEM log file  -  (date)\n\n" + "  Criteria are multiplied by %f\n\n" % float(mult)


def _empty_text(ev):
    return "%4d  Class %d empty at iteration %d\n" % (ev["iter"], ev["emptyk"], ev["iter"])


def run_log_text(events, n, k, d, beta, param_fix=False):
    """The log of an INIT_PARAM_FILE run.  NbObs_KD is zero until the first EstimPara (and for good with fixed
    parameters: it never runs)."""
    mult = log_mult(n)
    out = [_preamble(n, mult), "Initializing parameters from given value :\n"]
    for ev in events:
        if ev["kind"] == "empty":
            out.append(_empty_text(ev))
            continue
        assert ev["kind"] == "line"
        known = ev["iter"] > 0 and not param_fix and ev["nbobs_k"] is not None
        sizes = ev["nbobs_k"] if known else np.zeros(k, np.float32)
        out.append("%4d " % ev["iter"] + crit_text(ev["crit_before"], mult) + crit_text(ev["crit_after"], mult)
                   + classes_text(beta, ev["prop"], ev["center"], ev["disp"], sizes))
        if ev["iter"] == 0:
            out.append("\n" + header_text(k, d))
    return "".join(out)


def random_log_text(events, n, k, d, beta, best_start, crit_m):
    """The log of an INIT_RANDOM run.  A start's line 0 prints whatever NbObs the run so far left: NaN before the first
    EstimPara, then the sizes of the last one -- an emptied class's included; nothing resets them between starts."""
    mult = log_mult(n)
    out = [_preamble(n, mult)]
    left = np.full(k, np.nan, np.float32)
    for ev in events:
        if ev["kind"] == "start":
            out.append("\nRandom initialization %d :\n%4d " % (ev["start"] + 1, 0))
            continue
        if ev["kind"] == "empty":
            out.append(_empty_text(ev))
            left = ev["nbobs_k"]
            continue
        if ev["iter"] > 0:
            left = ev["nbobs_k"]
            out.append("%4d " % ev["iter"])
        out.append(crit_text(ev["crit_before"], mult) + crit_text(ev["crit_after"], mult)
                   + classes_text(beta, ev["prop"], ev["center"], ev["disp"], left))
        if ev["iter"] == 0:
            out.append("\n" + header_text(k, d))
    if best_start >= 0:
        out.append("Best start was %d (U = %g)\n" % (best_start + 1, float(crit_m)))
    return "".join(out)
