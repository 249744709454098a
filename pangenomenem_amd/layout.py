"""The pangenome graph laid out (PPanGGOLiN.compute_layout, ppanggolin.py:1250-1292) from a resident master: ForceAtlas2
(Jacomy, Venturini, Heymann, Bastian 2014) over the family graph, 500 iterations by default, the positions then put on
every node of the GEXF as ``viz:position`` with ``z`` from the partition (:1286-1291).

``compute_layout`` delegates the layout to the external package ``fa2``: a single-threaded Barnes-Hut approximation at
theta 1.2, started from ``random.random()`` positions.  What the reference itself determines is which graph, masses and
weights go in (the family graph; ``data["weight"]``, :453-457, the organisms on an edge; fa2's mass is degree + 1),
``z``, and the ``<viz:position>`` element networkx writes.  Those are reproduced.  The rest is defined here:

``layout_arrays`` states the iteration in numpy, float64 -- an EXACT all-pairs repulsion instead of Barnes-Hut, strong
gravity, the attraction, the swinging / traction speed control of the paper; ``nemgpu_layout_*`` (csrc/nem_layout.hip)
runs it on the device and is held to the statement: every term is bit-equal, only the order of the sums is the
device's; ``Master.layout`` (chunks.py) is the Python surface and ``Layout`` the handle; ``positions_3d`` gives ``z``.
No equality with fa2's output is claimed, and the start stream (x then y from ``random.random()`` per node, in node order,
what fa2 is understood to do for ``pos=None``) could not be checked against fa2: the package is not part of the reference.
The cost grows as n^2 per iteration.  ``repulsion="barnes_hut"`` (``layout_bh.py``: its own statement, tree and walk; this
project's tree, not fa2's) is the opt-in that grows as n log n; ``layout_arrays`` and the default stay the exact sum.
"""
import ctypes as C
import math
import random

import numpy as np

from .engine import NemGpuError
from .projection import part_codes

TILE = 256                                                    # csrc/nem_layout.hpp: kLayoutTile, the repulsion kernel's tile width
SLICE_GRAIN = 64                                              # kLayoutSliceGrain: a graph above it has more than one slice
BLOCKS_TARGET, SLICES_MAX = 1024, 64
DEFAULTS = dict(scaling_ratio=50000.0, gravity=1.0, strong_gravity=True, outbound_attraction_distribution=True, edge_weight_influence=1.0,
                jitter_tolerance=1.0, lin_log=False, adjust_sizes=False)
ORDERS = ("numpy", "left", "perm", "fsum", "extended")
REPULSIONS = ("exact", "barnes_hut")                          # Layout's repulsion=: the all-pairs sum, or layout_bh.py's tree


def slices_of(n):
    """the slices the device cuts every node's j range into (nem_layout.hpp's layout_slices): a function of n alone"""
    if n <= 0:
        return 1
    nb = -(-n // TILE)
    return max(1, min(-(-n // SLICE_GRAIN), -(-BLOCKS_TARGET // nb), SLICES_MAX))


def check_params(params):
    """compute_layout's parameters over the defaults; what is not supported raises ValueError"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError("layout: unknown parameter %s" % sorted(unknown))
    p = dict(DEFAULTS, **params)
    if p["lin_log"]:
        raise ValueError("layout: the LinLog mode is not supported")
    if p["adjust_sizes"]:
        raise ValueError("layout: adjust_sizes (the anti-collision forces) is not supported")
    if not p["strong_gravity"]:
        raise ValueError("layout: only the strong gravity mode is supported")
    for name in ("scaling_ratio", "gravity", "edge_weight_influence", "jitter_tolerance"):
        p[name] = float(p[name])
        if not math.isfinite(p[name]):
            raise ValueError("layout: %s is not finite" % name)
    return p


def start_positions(n, pos=None, rng=None):
    """pos as float64 [n][2] (finite), or drawn: for each family in master order x = rng.random(), then y = rng.random()
    (rng: the `random` module by default)"""
    if pos is not None:
        if rng is not None:
            raise ValueError("layout: pos= or rng=, not both")
        pos = np.array(pos, np.float64).reshape(-1, 2) if n else np.zeros((0, 2))
        if pos.shape != (n, 2):
            raise ValueError("layout: pos float64 [n][2]")
        if not np.isfinite(pos).all():
            raise ValueError("layout: a start position is not finite")
        return np.ascontiguousarray(pos)
    rng = random if rng is None else rng
    out = np.zeros((n, 2), np.float64)
    for i in range(n):
        out[i, 0] = rng.random()
        out[i, 1] = rng.random()
    return out


def layout_graph(graph, edge_bits, d):
    """What the layout reads of a master's arrays (Master.arrays()): mass float64 [n] = 1 + the entries of the row (a
    self-loop entry included); per CSR entry its row, its neighbour and its weight, the popcount of its bit row
    (int64 [nnz] each); the edges src < dst with their weight, in CSR order (the entries with idx > row)."""
    ptr, idx = (np.asarray(a, np.int64) for a in graph)
    n, nnz = len(ptr) - 1, len(idx)
    wf = (d + 31) // 32
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    if nnz:
        eb = np.ascontiguousarray(edge_bits, np.uint32).reshape(-1, wf)[:nnz]
        weight = np.unpackbits(eb.view(np.uint8).reshape(nnz, -1), axis=1, bitorder="little")[:, :d].sum(axis=1).astype(np.int64)
    else:
        weight = np.zeros(0, np.int64)
    mass = (1 + np.diff(ptr)).astype(np.float64)
    up = idx > row
    return dict(n=n, mass=mass, row=row, col=idx, weight=weight, src=row[up], dst=idx[up], edge_weight=weight[up])


def _edge_value(weight, influence):
    """step 3's e of every entry"""
    if influence == 0.0:
        return np.ones(len(weight), np.float64)
    if influence == 1.0:
        return weight.astype(np.float64)
    table = {int(w): math.pow(float(w), influence) for w in np.unique(weight)}        # (libm's pow, as the C side calls it)
    return np.asarray([table[int(w)] for w in weight], np.float64)


def _ordered_sum(terms, order, perm):
    """the rows of terms [n][m] summed in the given order"""
    if terms.shape[1] == 0:
        return np.zeros(terms.shape[0])
    if order == "numpy":
        return terms.sum(axis=1)
    if order == "perm":
        terms = terms[:, perm]
    return np.cumsum(terms, axis=1)[:, -1]                    # (accumulate is strictly left to right)


def extended_type():
    """np.longdouble where it carries at least 64 significant bits (x87's extended format, or wider), else None: the
    "extended" order then takes math.fsum per row"""
    return np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None


def _total(values, order):
    if order in ("fsum", "extended"):
        return math.fsum(values.tolist())
    if order == "numpy":
        return float(values.sum())
    return float(np.cumsum(values)[-1]) if len(values) else 0.0


def speed_control(n, S, T, speed, eff, jitter_tolerance):
    """Step 5 for T != 0: (speed, eff, the comparisons made as (name, left, right) in order).  A comparison whose two
    sides are close is one that another order of the sums could decide the other way."""
    est = 0.05 * math.sqrt(n)
    jt = jitter_tolerance * max(math.sqrt(est), min(10.0, est * T / (float(n) * float(n))))
    made = [("ratio", S / T, 2.0)]
    if S / T > 2.0:
        if eff > 0.05:
            eff *= 0.5
        jt = max(jt, jitter_tolerance)
    target = jt * eff * T / S if S > 0.0 else math.inf
    made.append(("swing", S, jt * T))
    if S > jt * T:
        if eff > 0.05:
            eff *= 0.7
    else:
        made.append(("fast", speed, 1000.0))
        if speed < 1000.0:
            eff *= 1.3
    made.append(("step", target - speed, 0.5 * speed))
    speed += min(target - speed, 0.5 * speed)
    return speed, eff, made


def layout_arrays(graph, edge_bits, d, iterations=500, pos=None, rng=None, order="numpy", perm=None, attraction="gather", old=None,
                  speed=1.0, eff=1.0, block_rows=None, **params):
    """What nemgpu_layout_create / _run compute, in numpy, float64.
    graph (ptr, idx), edge_bits uint32 [nnz][ceil(d/32)], d: the master as Master.arrays() gives it (a symmetric CSR);
    pos / rng: start_positions; params: compute_layout's (DEFAULTS).  State: old = 0 (the previous forces), speed = 1,
    eff = 1, or given (a run taken up where another stopped).  One iteration:
      1. repulsion: f[i] = sum over j with d2 > 0 of (p_i - p_j) * ((scaling_ratio * mass_i) * mass_j / d2), d2 = dx * dx + dy * dy:
         j = i and a coincident pair contribute nothing;
      2. strong gravity: f[i] -= (gravity * mass_i) * p_i;
      3. attraction, per edge src < dst (a self-loop: none): comp = mean(mass) if outbound_attraction_distribution else 1;
         e = 1 / weight / weight ** influence for edge_weight_influence 0 / 1 / else; fac = (-comp) * e, divided by mass[src]
         when distributed; f[src] += (p_src - p_dst) * fac, f[dst] -= (p_src - p_dst) * fac (attraction="scatter") -- the
         same terms as, for every CSR entry (i, j) with j != i, f[i] += (p_i - p_j) * fac(edge) (attraction="gather");
      4. sw_i = |old_i - f_i|, tr_i = |old_i + f_i| (Euclidean), S = sum mass_i sw_i, T = sum mass_i tr_i / 2;
      5. speed_control; T == 0: nothing moves, speed, eff and old stay, the iteration ends here;
      6. p_i += f_i * speed / (1 + sqrt(speed * mass_i * sw_i)), old = f.
    order: how the sums of steps 1 - 4 are taken: "numpy" (np.sum), "left" (j ascending, then gravity, then the row's
    entries), "perm" (the repulsion's j in the order perm, int [n]), "fsum" (math.fsum over all of a component's terms:
    the exactly rounded sum, the yardstick), "extended" (the yardstick for a large n: the same float64 terms accumulated
    in np.longdouble, 64 significant bits, and rounded once -- within n 2^-64 B of the exact sum before that rounding, B
    the bound below; S and T by math.fsum; where np.longdouble is no wider than float64, math.fsum per row).
    block_rows: None, or the rows of the [n][n] arrays of step 1 that are held at a time (memory O(block_rows * n)
    instead of O(n * n)): a row's sum is taken along that row alone, so every returned bit is the unblocked form's.
    Returns a dict: pos [n][2], forces [n][2], speed, eff, S, T of the last iteration, iterations, bound [n][2] (per node
    and component the sum of the absolute values of the last iteration's terms of steps 1 - 3), old [n][2], moved (the
    last iteration's T != 0), comparisons (per iteration speed_control's list, [] where T == 0), wide (order="extended":
    the last iteration's forces before their one rounding, np.longdouble [n][2]; else, and for iterations=0, None)."""
    p = check_params(params)
    if order not in ORDERS or attraction not in ("gather", "scatter"):
        raise ValueError("layout_arrays: order one of %s, attraction gather or scatter" % (ORDERS,))
    if iterations < 0:
        raise ValueError("layout_arrays: iterations < 0")
    if block_rows is not None and (int(block_rows) != block_rows or block_rows < 1):
        raise ValueError("layout_arrays: block_rows is None or a whole number >= 1")
    g = layout_graph(graph, edge_bits, d)
    n, mass = g["n"], g["mass"]
    if order == "perm":
        perm = np.asarray(perm, np.int64)
        if sorted(perm.tolist()) != list(range(n)):
            raise ValueError("layout_arrays: perm is a permutation of the families")
    xy = start_positions(n, pos, rng).copy()
    old = np.zeros((n, 2)) if old is None else np.array(old, np.float64).reshape(n, 2)
    speed, eff = float(speed), float(eff)
    comp = float(mass.mean()) if p["outbound_attraction_distribution"] and n else 1.0
    # per CSR entry off the diagonal: the factor of its edge
    off = g["col"] != g["row"]
    ei, ej = g["row"][off], g["col"][off]
    fac = (-comp) * _edge_value(g["weight"][off], p["edge_weight_influence"])
    if p["outbound_attraction_distribution"]:
        fac = fac / mass[np.minimum(ei, ej)]
    up = ei < ej                                              # (the edges: the scatter form walks them)
    sm = p["scaling_ratio"] * mass
    forces, bound = np.zeros((n, 2)), np.zeros((n, 2))
    by_row = order == "fsum" or (order == "extended" and extended_type() is None)
    wide = np.zeros((n, 2), extended_type()) if order == "extended" and not by_row else None
    entries = [None, None]                                    # per component: step 3's (node, term) of every entry
    S = T = 0.0
    moved, comparisons = False, []
    for _ in range(iterations):
        grav = (p["gravity"] * mass)[:, None] * xy
        for c in (0, 1):
            if attraction == "gather":
                at_node, at_term = ei, (xy[ei, c] - xy[ej, c]) * fac
            else:
                t = (xy[ei[up], c] - xy[ej[up], c]) * fac[up]
                at_node, at_term = np.concatenate([ei[up], ej[up]]), np.concatenate([t, -t])
            entries[c] = (at_node, at_term)
            if by_row:
                rows = [[] for _ in range(n)]
                for node, term in zip(at_node.tolist(), at_term.tolist()):
                    rows[node].append(term)
                entries[c] += (rows,)
        for r0 in range(0, n, block_rows or max(n, 1)):
            r1 = min(n, r0 + (block_rows or n))
            dx = xy[r0:r1, 0][:, None] - xy[:, 0][None, :]    # [rows][n]
            dy = xy[r0:r1, 1][:, None] - xy[:, 1][None, :]
            d2 = dx * dx + dy * dy
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = (sm[r0:r1, None] * mass[None, :]) / d2
            coef[~(d2 > 0.0)] = 0.0
            for c, delta in ((0, dx), (1, dy)):
                rep = delta * coef
                if by_row:
                    rows = entries[c][2]
                    forces[r0:r1, c] = [math.fsum(rep[i - r0].tolist() + [-grav[i, c]] + rows[i]) for i in range(r0, r1)]
                elif order == "extended":
                    wide[r0:r1, c] = rep.sum(axis=1, dtype=wide.dtype)
                else:
                    forces[r0:r1, c] = _ordered_sum(rep, order, perm)
                bound[r0:r1, c] = np.abs(rep).sum(axis=1)
        for c in (0, 1):
            at_node, at_term = entries[c][:2]
            if not by_row:
                f = (wide[:, c] if order == "extended" else forces[:, c]) - grav[:, c]
                np.add.at(f, at_node, at_term)                # (unbuffered: the entries in order)
                forces[:, c] = f                              # (the extended sum: rounded here, once)
                if order == "extended":
                    wide[:, c] = f
            b = bound[:, c] + np.abs(grav[:, c])
            np.add.at(b, at_node, np.abs(at_term))
            bound[:, c] = b
        sx, sy = old[:, 0] - forces[:, 0], old[:, 1] - forces[:, 1]
        tx, ty = old[:, 0] + forces[:, 0], old[:, 1] + forces[:, 1]
        sw, tr = np.sqrt(sx * sx + sy * sy), np.sqrt(tx * tx + ty * ty)
        S, T = _total(mass * sw, order), 0.5 * _total(mass * tr, order)
        moved = T != 0.0
        if not moved:
            comparisons.append([])
            continue
        speed, eff, made = speed_control(n, S, T, speed, eff, p["jitter_tolerance"])
        comparisons.append(made)
        xy = xy + forces * speed / (1.0 + np.sqrt(speed * mass * sw))[:, None]
        old = forces.copy()
    return dict(pos=xy, forces=forces.copy(), speed=speed, eff=eff, S=S, T=T, iterations=iterations, bound=bound, old=old, moved=moved,
                comparisons=comparisons, wide=wide if iterations else None)


def positions_3d(partitions, names, pos):
    """compute_layout's viz position of every family (ppanggolin.py:1286-1292): (x, y, z) with z = 2 for a persistent
    family, 1 for a shell one, 0 otherwise; partitions: {family name: 'P' | 'S' | 'C' | 'U'} or uint8 [n] in the vote's
    codes, or None (a pangenome that is not partitioned: z = 0).  Returns (float64 [n][2], int64 [n])."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    if pos.shape != (n, 2):
        raise ValueError("positions_3d: pos float64 [n][2]")
    if partitions is None:
        return pos, np.zeros(n, np.int64)
    part = part_codes(partitions, names) if isinstance(partitions, dict) else np.ascontiguousarray(partitions, np.uint8)
    if part.shape != (n,):
        raise ValueError("positions_3d: a class per family")
    return pos, np.where(part == 0, 2, np.where(part == 1, 1, 0)).astype(np.int64)


class LayoutConfig(C.Structure):
    _fields_ = [("scaling_ratio", C.c_double), ("gravity", C.c_double), ("edge_weight_influence", C.c_double), ("jitter_tolerance", C.c_double),
                ("strong_gravity", C.c_int), ("outbound_attraction_distribution", C.c_int), ("lin_log", C.c_int), ("adjust_sizes", C.c_int)]


def _bind_layout(lib):
    lib.nemgpu_layout_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(LayoutConfig), C.c_void_p]
    lib.nemgpu_layout_run.argtypes = [C.c_void_p, C.c_int]
    lib.nemgpu_layout_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nemgpu_layout_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_layout_destroy.restype = None
    lib.nemgpu_layout_slices.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.nemgpu_layout_create_bh.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(LayoutConfig), C.c_void_p, C.c_double]
    lib.nemgpu_layout_bh_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.nemgpu_layout_bh_tree.argtypes = [C.c_void_p, C.POINTER(C.c_int)] + [C.c_void_p] * 11
    return lib


def config_of(p):
    return LayoutConfig(p["scaling_ratio"], p["gravity"], p["edge_weight_influence"], p["jitter_tolerance"], int(bool(p["strong_gravity"])),
                        int(bool(p["outbound_attraction_distribution"])), int(bool(p["lin_log"])), int(bool(p["adjust_sizes"])))


class Layout:
    """A layout on the device (nemgpu_layout_create): positions, forces and the speed control's state stay there between
    run() calls.  The master is read at creation only.  repulsion: "exact" (the all-pairs sum, the default) or
    "barnes_hut" (nemgpu_layout_create_bh: layout_bh.py states the tree and the walk; theta is read for it alone)."""

    def __init__(self, master, pos=None, rng=None, repulsion="exact", theta=1.2, **params):
        p = check_params(params)
        if repulsion not in REPULSIONS:
            raise ValueError("layout: repulsion one of %s" % (REPULSIONS,))
        self.repulsion = repulsion
        if repulsion == "barnes_hut":
            from .layout_bh import check_theta
            self.theta = check_theta(theta)
        if getattr(master, "directed", False):
            raise ValueError("layout: a directed master (a DiGraph's weight is per direction, the master holds only the sum)")
        self.lib = _bind_layout(master.lib)
        self.n = master.n
        start = start_positions(self.n, pos, rng)
        self.names = getattr(master, "names", None)
        self._h = C.c_void_p()
        cfg = config_of(p)
        if repulsion == "barnes_hut":
            self._call("create_bh", C.byref(self._h), master._h, C.byref(cfg), start.ctypes.data if self.n else None, self.theta)
        else:
            self._call("create", C.byref(self._h), master._h, C.byref(cfg), start.ctypes.data if self.n else None)

    def _call(self, name, *args):
        rc = getattr(self.lib, "nemgpu_layout_" + name)(*args)
        if rc != 0:
            raise NemGpuError("nemgpu_layout_%s failed (status %d): %s" % (name, rc, self.lib.nemgpu_last_error().decode()))

    def run(self, iterations):
        """`iterations` more iterations, enqueued: positions(), forces() and state() wait for them"""
        if iterations < 0:
            raise ValueError("layout: iterations < 0")
        self._call("run", self._h, int(iterations))
        return self

    def _fetch(self, pos=None, forces=None, state=None):
        self._call("fetch", self._h, *(a.ctypes.data if a is not None and a.size else None for a in (pos, forces, state)))

    def positions(self):
        """float64 [n][2], in master order"""
        pos = np.zeros((self.n, 2), np.float64)
        self._fetch(pos=pos)
        return pos

    def forces(self):
        """the last iteration's forces, float64 [n][2]"""
        forces = np.zeros((self.n, 2), np.float64)
        self._fetch(forces=forces)
        return forces

    def state(self):
        """dict: speed, eff, S, T (the last iteration's), iterations done"""
        v = np.zeros(5, np.float64)
        self._fetch(state=v)
        return dict(speed=float(v[0]), eff=float(v[1]), S=float(v[2]), T=float(v[3]), iterations=int(v[4]))

    def tree(self):
        """The Barnes-Hut tree of the current positions as the device builds it (nemgpu_layout_bh_tree): what
        layout_bh.tree_arrays returns, and accepted, visited int64 [n] (the walk's counters per family).  It changes no
        state.  A layout with the exact repulsion has no tree: NemGpuError."""
        from . import layout_bh as bh
        n, cap = self.n, bh.cell_bound(self.n)
        cells, box = C.c_int(), np.zeros(3, np.float64)
        skey, order = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        level, lo, hi = (np.zeros(cap, np.int32) for _ in range(3))
        M, Sx, Sy = (np.zeros(cap, np.float64) for _ in range(3))
        accepted, visited = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._call("bh_tree", self._h, C.byref(cells), *(a.ctypes.data if a.size else None for a in (box, skey, order, level, lo, hi, M, Sx, Sy, accepted, visited)))
        nc = cells.value
        order = order.astype(np.int64)
        key = np.zeros(n, np.uint32)
        key[order] = skey
        level, lo, hi = (a[:nc].astype(np.int64) for a in (level, lo, hi))
        child, rope = bh.links(skey, level, lo, hi) if nc else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        return dict(n=n, x0=float(box[0]), y0=float(box[1]), side=float(box[2]), key=key, order=order, cells=nc, level=level, lo=lo, hi=hi, M=M[:nc].copy(),
                    Sx=Sx[:nc].copy(), Sy=Sy[:nc].copy(), child=child, rope=rope, bound=cap, accepted=accepted.astype(np.int64),
                    visited=visited.astype(np.int64))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nemgpu_layout_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
