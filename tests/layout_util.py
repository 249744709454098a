"""What tests/test_layout_host.py and tests/test_gpu_layout.py share: the recorded exports of tests/golden/layout/ (made
by tests/golden/make_layout.py from the reference's own compute_layout loop and export_to_GEXF()), small symmetric
masters as arrays, and the tolerances a device step is held to, derived from the statement's own bound."""
import glob
import math
import os

import numpy as np

from pangenomenem_amd.layout import layout_arrays
from tests.orders_util import load

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT_FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "layout", "*.json")))
U = 2.0 ** -53                                                # the unit roundoff of float64
MARGIN = 1e-9                                                 # a comparison of the speed control closer than this could flip


def base_record(rec):
    """the GEXF fixture (annotations, organisms, ...) a layout fixture was made on"""
    return load(os.path.join(HERE, "golden", "gexf", rec["name"] + ".json"))


def positions_in_master_order(rec, names):
    at = {fam: k for k, fam in enumerate(rec["families"])}
    assert sorted(at) == sorted(names)
    return np.asarray([rec["positions"][at[name]] for name in names], np.float64)


def arrays_of(n, edges, d):
    """a symmetric master as arrays from edges [(a, b, [organisms])] (a == b: a self-loop, one entry, at the row's end):
    x uint8 [n][d] (a family is present where an edge of it is carried, and in organism 0), (ptr, idx), edge_bits"""
    wf = (d + 31) // 32
    rows = [[] for _ in range(n)]
    for a, b, orgs in edges:
        bits = np.zeros(wf, np.uint32)
        for o in orgs:
            bits[o // 32] |= np.uint32(1 << (o % 32))
        rows[a].append((b, bits))
        if a != b:
            rows[b].append((a, bits))
    x = np.zeros((n, d), np.uint8)
    x[:, 0] = 1
    for a, b, orgs in edges:
        x[a, orgs] = 1
        x[b, orgs] = 1
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.asarray([j for r in rows for j, _ in r], np.int32)
    eb = np.asarray([bits for r in rows for _, bits in r], np.uint32).reshape(-1, wf) if len(idx) else np.zeros((0, wf), np.uint32)
    return x, (ptr, idx), eb


def ring_with_chords(n, d, seed, chords=0.2):
    """a ring of n families with about n * chords chords; every edge carried by 1 .. d organisms"""
    rng = np.random.default_rng(seed)
    pairs = {tuple(sorted((i, (i + 1) % n))) for i in range(n)} if n > 2 else {(0, 1)}
    for _ in range(int(n * chords)):
        a, b = sorted(int(v) for v in rng.integers(0, n, 2))
        if a != b:
            pairs.add((a, b))
    return arrays_of(n, [(a, b, sorted(rng.choice(d, int(rng.integers(1, d + 1)), replace=False).tolist())) for a, b in sorted(pairs)], d)


def branches(result):
    """which way every comparison of every iteration went"""
    return [[(name, left > right) for name, left, right in made] for made in result["comparisons"]]


def check_margins(made, old_is_zero, what):
    """no comparison of one speed control is within MARGIN (relative) of flipping.  From old = 0 swinging and traction
    are the same numbers (|0 - f| and |0 + f|), so S = 2 T exactly in whatever order both are summed and `S / T > 2` is
    decided by an equality that holds bit for bit: that one comparison is asserted to BE the equality instead."""
    for name, left, right in made:
        if name == "ratio" and old_is_zero:
            assert left == right == 2.0, (what, name, left, right)
            continue
        if math.isinf(left) or math.isinf(right):
            continue
        assert abs(left - right) > MARGIN * max(abs(left), abs(right)), (what, name, left, right)


def step_tolerances(n, mass, want, prev_old, prev_speed, order="fsum"):
    """For one iteration from identical inputs: the statement `want` (order="fsum": every sum exactly rounded) against
    any device order.  Every term is bit-equal; a sum of m terms taken in any order is within (m - 1) u of sum |terms|,
    the fsum one within u: a component has at most 2 n - 1 terms (n - 1 pairs, gravity, at most n - 1 entries), so
      forces  E = 2 n u B; for a statement in order="extended" (layout_arrays: the terms accumulated in 64 significant
              bits, off the exact sum by at most n 2^-64 B before the one rounding) that error of the yardstick is added:
              E = 2 n u B + n 2^-64 B;
      sw, tr  (the norm of old -/+ f) inherit |E| and a few roundings: dsw = |E| + 8 u sw;
      S, T    2 n u S for the order, sum mass dsw for the terms;
      speed   exact where the step is half the speed; where it is target - speed, the relative error of jt eff T / S;
      pos     f speed / (1 + sqrt(speed mass sw)) with all of the above.
    Returns a dict of absolute tolerances."""
    f = want["forces"]
    if order not in ("fsum", "extended"):
        raise ValueError("step_tolerances: the statement in order fsum or extended")
    E = 2.0 * n * U * want["bound"]
    if order == "extended":
        E = E + n * 2.0 ** -64 * want["bound"]
    En = np.sqrt(E[:, 0] ** 2 + E[:, 1] ** 2)
    sw = np.sqrt(((prev_old - f) ** 2).sum(axis=1))
    tr = np.sqrt(((prev_old + f) ** 2).sum(axis=1))
    dsw, dtr = En + 8 * U * sw, En + 8 * U * tr
    tol_S = 2.0 * n * U * want["S"] + float((mass * dsw).sum()) + 4 * U * want["S"]
    tol_T = 2.0 * n * U * want["T"] + 0.5 * float((mass * dtr).sum()) + 4 * U * want["T"]
    out = dict(forces=E, S=tol_S, T=tol_T, speed=0.0, pos=np.zeros((n, 2)))
    if not want["moved"]:
        return out
    step = [c for c in want["comparisons"][-1] if c[0] == "step"][0]
    if not step[1] > step[2]:                                 # (the step is target - speed)
        rel = tol_S / want["S"] + 2.0 * tol_T / want["T"] + 16 * U
        out["speed"] = rel * (abs(want["speed"]) + abs(prev_speed))
    speed = want["speed"]
    q = np.sqrt(speed * mass * sw)
    factor = speed / (1.0 + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        dq = np.minimum(np.where(sw > 0, np.sqrt(speed * mass) * dsw / (2.0 * np.sqrt(sw)), np.inf), np.sqrt(speed * mass * dsw)) + 4 * U * q
    dfactor = out["speed"] + speed * dq / (1.0 + q) ** 2 + 8 * U * factor
    out["pos"] = E * factor[:, None] + np.abs(f) * dfactor[:, None] + 8 * U * (np.abs(want["pos"]) + np.abs(f) * factor[:, None])
    return out


def statement_step(graph, eb, d, pos, old, speed, eff, order="fsum", block_rows=None, **params):
    return layout_arrays(graph, eb, d, iterations=1, pos=pos, old=old, speed=speed, eff=eff, order=order, block_rows=block_rows, **params)
