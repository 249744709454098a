"""The layout's repulsion as a Barnes-Hut sum (Barnes, Hut 1986), the option ``compute_layout`` asks its external package
for (``barnesHutOptimize=True, barnesHutTheta=1.2``, ppanggolin.py:1250-1292): O(n log n) per iteration instead of n^2.

``tree_arrays`` states the tree in numpy, float64, and ``layout_bh_arrays`` the iteration: step 1 of ``layout_arrays``
replaced by the walk of that tree, steps 2 - 6 its own.  ``nemgpu_layout_create_bh`` (csrc/nem_layout_bh.hip) runs it on
the device and is held to this statement bit for bit: keys, order, cells, moments and every force; only the order of the
two global sums S and T is the device's.  The tree is THIS project's: how ``fa2`` splits its regions, what it takes for
a region's size and what start stream it draws could not be checked (the package is not part of the reference), so no
equality with ``fa2``'s output is claimed here either.  The exact repulsion stays the default.

The rules (every one is what the device does as well):
  square   x0 = min x, y0 = min y, side = max(max x - x0, max y - y0); side == 0 (n <= 1, all bodies coincident): no tree,
           no repulsion -- what the exact sum gives, every pair having d2 == 0;
  grid     G = 2 ** DEPTH; per axis t = (x - x0) / side, c = int(t * G) clamped into [0, G - 1] (a NaN: 0; the far edge
           gives G before the clamp); key = the 32-bit Morton interleave, x in the even bits, y in the odd ones;
  order    the bodies sorted by (key, index);
  cells    at level l in 0 .. DEPTH a cell is a maximal run of sorted bodies with equal key >> 2 (DEPTH - l); level 0 is
           the root; a cell at level l > 0 exists iff the level l - 1 run around it holds more than LEAF bodies; a cell is
           a leaf iff it holds <= LEAF bodies or l == DEPTH; single-child cells are kept; cells are numbered by level,
           then by run order, and there are at most cell_bound(n) of them;
  moments  a leaf's (M, Sx, Sy): the sums of m, m x, m y over its bodies, left to right in sorted order; an inner cell's:
           the sums of its children's, left to right; the centre is (Sx / M, Sy / M); a level-l cell's size is
           s = side / 2 ** l;
  walk     for body i, depth first from the root, children in key order: an inner cell that does not contain i is
           ACCEPTED iff (theta * theta) * d2 > s * s, d2 the squared distance from i to the centre, and contributes
           (p_i - c) * ((scaling_ratio * mass_i) * M / d2); a cell that contains i is always opened; a leaf contributes
           the exact pair term of each of its bodies in sorted order under the d2 > 0 test; all of it accumulates left to
           right in walk order.
"""
import math

import numpy as np

from .layout import _edge_value, _total, check_params, layout_graph, speed_control, start_positions

DEPTH = 16                                                    # csrc/nem_layout_bh.hpp: kBhDepth, the levels below the root
LEAF = 8                                                      # kBhLeaf: a run of at most this many bodies is not split
SUM_ORDERS = ("left", "numpy", "fsum", "perm")


def cell_bound(n):
    """the cells a tree of n bodies can have: the root, and per further level at most four under every run above LEAF"""
    return 1 + DEPTH * min(n, 4 * (n // (LEAF + 1)))


def check_theta(theta):
    theta = float(theta)
    if not math.isfinite(theta) or theta < 0.0:
        raise ValueError("layout: theta is finite and not negative")
    return theta


def _spread(c):
    """the low 16 bits of c on the even bits of a uint32"""
    c = c.astype(np.uint32)
    c = (c | (c << np.uint32(8))) & np.uint32(0x00FF00FF)
    c = (c | (c << np.uint32(4))) & np.uint32(0x0F0F0F0F)
    c = (c | (c << np.uint32(2))) & np.uint32(0x33333333)
    c = (c | (c << np.uint32(1))) & np.uint32(0x55555555)
    return c


def morton_keys(pos, x0, y0, side):
    """uint32 [n]: the key of every body in the square (x0, y0, side), side > 0"""
    G = float(1 << DEPTH)

    def cell(v, v0):
        with np.errstate(invalid="ignore", over="ignore"):
            g = ((v - v0) / side) * G
            inside = np.where(g >= G, G - 1.0, np.trunc(g))
            return np.where(g >= 0.0, inside, 0.0).astype(np.int64)

    return _spread(cell(pos[:, 0], x0)) | (_spread(cell(pos[:, 1], y0)) << np.uint32(1))


def links(skey, level, lo, hi):
    """What makes the walk stackless, from the cells alone: child int64 [cells] (the first child, -1 for a leaf) and rope
    (the next cell in depth-first order when this one is skipped: the next sibling, else an ancestor's; -1: the walk
    ends).  The cell that follows one ending at `hi` is the shallowest cell that starts there, and that is at the first
    level at which the keys on both sides of `hi` differ."""
    level, lo, hi = (np.asarray(a, np.int64) for a in (level, lo, hi))
    n = len(skey)
    code = level * (n + 1) + lo                               # ascending: by level, then by run order
    find = lambda lv, at: np.searchsorted(code, lv * (n + 1) + at)
    leaf = (hi - lo <= LEAF) | (level == DEPTH)
    child = np.where(leaf, -1, find(level + 1, lo))
    rope = np.full(len(level), -1, np.int64)
    inner = hi < n
    if inner.any():
        h = hi[inner]
        diff = (skey[h - 1] ^ skey[h]).astype(np.int64)
        top = np.floor(np.log2(diff)).astype(np.int64)        # (exact: diff < 2^32 is a float64's integer)
        rope[inner] = find(DEPTH - (top >> 1), h)
    return child, rope


def tree_arrays(pos, mass):
    """The tree of the bodies pos float64 [n][2], mass float64 [n] (small integers).  Returns a dict: n, x0, y0, side;
    key uint32 [n] (per body), order int64 [n] (sorted position -> body); cells, and per cell level, lo, hi (its sorted
    bodies [lo, hi)), M, Sx, Sy, child, rope (links); bound = cell_bound(n).  side == 0: no cell, keys 0, order 0 .. n - 1."""
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    mass = np.asarray(mass, np.float64)
    n = len(pos)
    x0, y0 = (float(pos[:, 0].min()), float(pos[:, 1].min())) if n else (0.0, 0.0)
    side = max(float(pos[:, 0].max()) - x0, float(pos[:, 1].max()) - y0) if n else 0.0
    none_i, none_f = np.zeros(0, np.int64), np.zeros(0, np.float64)
    out = dict(n=n, x0=x0, y0=y0, side=side, key=np.zeros(n, np.uint32), order=np.arange(n, dtype=np.int64), cells=0, level=none_i, lo=none_i,
               hi=none_i, M=none_f, Sx=none_f, Sy=none_f, child=none_i, rope=none_i, bound=cell_bound(n))
    if not side > 0.0:
        return out
    key = morton_keys(pos, x0, y0, side)
    order = np.argsort(key, kind="stable").astype(np.int64)   # (key, index): stable over the indices in order
    skey = key[order]
    wide = skey.astype(np.uint64)
    level, lo, hi = [], [], []
    parent_count = np.full(n, n + LEAF + 1, np.int64)         # per sorted body: the bodies of the run one level up (the root: exists)
    for l in range(DEPTH + 1):
        pre = wide >> np.uint64(2 * (DEPTH - l))
        head = np.ones(n, bool)
        head[1:] = pre[1:] != pre[:-1]
        starts = np.nonzero(head)[0]
        ends = np.append(starts[1:], n)
        exists = parent_count[starts] > LEAF
        level.append(np.full(int(exists.sum()), l, np.int64))
        lo.append(starts[exists])
        hi.append(ends[exists])
        parent_count = np.repeat(ends - starts, ends - starts)
    level, lo, hi = (np.concatenate(a) for a in (level, lo, hi))
    cells = len(level)
    child, rope = links(skey, level, lo, hi)
    sx, sy, sm = pos[order, 0], pos[order, 1], mass[order]
    M, Sx, Sy = np.zeros(cells), np.zeros(cells), np.zeros(cells)
    for l in range(DEPTH, -1, -1):
        at = np.nonzero(level == l)[0]
        leaf = at[child[at] < 0]
        count = hi[leaf] - lo[leaf]
        for k in range(int(count.max()) if len(leaf) else 0):
            c = leaf[count > k]
            j = lo[c] + k
            M[c] += sm[j]
            Sx[c] += sm[j] * sx[j]
            Sy[c] += sm[j] * sy[j]
        inner = at[child[at] >= 0]
        kid = child[inner].copy()
        done = lo[inner].copy()                               # the children partition their parent, in key order
        while len(inner):
            M[inner] += M[kid]
            Sx[inner] += Sx[kid]
            Sy[inner] += Sy[kid]
            done = hi[kid]
            more = done < hi[inner]
            inner, kid, done = inner[more], kid[more] + 1, done[more]
    out.update(key=key, order=order, cells=cells, level=level, lo=lo, hi=hi, M=M, Sx=Sx, Sy=Sy, child=child, rope=rope)
    return out


def walk(tree, pos, mass, scaling_ratio, theta, ranges=False):
    """Step 1 for every body at once, each in its own walk order.  Returns (repulsion float64 [n][2], the sums of the
    terms' absolute values [n][2], accepted int64 [n]: the cells accepted per body, visited int64 [n]: the bodies of the
    leaves it opened), per body in the caller's order; ranges=True adds per body the list of the sorted ranges (lo, hi)
    its accepted cells and visited leaves cover, in walk order."""
    pos = np.asarray(pos, np.float64).reshape(-1, 2)
    n = len(pos)
    theta2 = theta * theta
    rep, ab = np.zeros((n, 2)), np.zeros((n, 2))
    accepted, visited = np.zeros(n, np.int64), np.zeros(n, np.int64)
    covered = [[] for _ in range(n)]
    if tree["cells"] == 0:
        return (rep, ab, accepted, visited) + ((covered,) if ranges else ())
    order, lo, hi, child, rope, M = (tree[k] for k in ("order", "lo", "hi", "child", "rope", "M"))
    sx, sy, sm = pos[order, 0], pos[order, 1], np.asarray(mass, np.float64)[order]
    smi = scaling_ratio * sm
    cx, cy = tree["Sx"] / M, tree["Sy"] / M
    s = tree["side"] / 2.0 ** tree["level"].astype(np.float64)
    s2 = s * s
    ax, ay, bx, by = (np.zeros(n) for _ in range(4))
    na, nv = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cur = np.zeros(n, np.int64)
    while True:
        act = np.nonzero(cur >= 0)[0]                         # (sorted positions: every body is its own lane)
        if not len(act):
            break
        c = cur[act]
        leaf = child[c] < 0
        contains = (lo[c] <= act) & (act < hi[c])
        dx, dy = sx[act] - cx[c], sy[act] - cy[c]
        d2 = dx * dx + dy * dy
        take = ~leaf & ~contains & (theta2 * d2 > s2[c])
        i, ct = act[take], c[take]
        coef = (smi[i] * M[ct]) / d2[take]
        tx, ty = dx[take] * coef, dy[take] * coef
        ax[i] += tx
        ay[i] += ty
        bx[i] += np.abs(tx)
        by[i] += np.abs(ty)
        na[i] += 1
        body, cl = act[leaf], c[leaf]
        count = hi[cl] - lo[cl]
        nv[body] += count
        if ranges:
            for b, a, z in zip(np.concatenate([i, body]).tolist(), np.concatenate([lo[ct], lo[cl]]).tolist(), np.concatenate([hi[ct], hi[cl]]).tolist()):
                covered[order[b]].append((a, z))
        for k in range(int(count.max()) if len(body) else 0):
            sel = count > k
            i, j = body[sel], lo[cl[sel]] + k
            ex, ey = sx[i] - sx[j], sy[i] - sy[j]
            e2 = ex * ex + ey * ey
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where(e2 > 0.0, (smi[i] * sm[j]) / e2, 0.0)     # j = i and a coincident pair: nothing
            tx, ty = ex * coef, ey * coef
            ax[i] += tx
            ay[i] += ty
            bx[i] += np.abs(tx)
            by[i] += np.abs(ty)
        cur[act] = np.where(leaf | take, rope[c], child[c])
    rep[order, 0], rep[order, 1] = ax, ay
    ab[order, 0], ab[order, 1] = bx, by
    accepted[order], visited[order] = na, nv
    return (rep, ab, accepted, visited) + ((covered,) if ranges else ())


def layout_bh_arrays(graph, edge_bits, d, iterations=500, pos=None, rng=None, theta=1.2, order="left", perm=None, old=None, speed=1.0, eff=1.0,
                     **params):
    """What nemgpu_layout_create_bh / _run compute, in numpy, float64: layout_arrays' iteration with step 1 replaced by
    the walk (this module's docstring) and the forces summed in the device's order -- the repulsion, then gravity, then
    the row's entries in CSR order -- so that every force is the device's bit for bit.  order: how S and T are summed
    ("left", "numpy", "perm": left to right over the families in the order perm, int [n], "fsum": the exactly rounded sum,
    the yardstick).  Returns layout_arrays' dict, and: tree (of the
    last iteration's positions before the move; of the start for iterations=0), accepted, visited int64 [n] (walk),
    bound [n][2] (the term bound B: the sum of the absolute values of the last iteration's terms), repulsion [n][2]."""
    p = check_params(params)
    theta = check_theta(theta)
    if order not in SUM_ORDERS:
        raise ValueError("layout_bh_arrays: order one of %s" % (SUM_ORDERS,))
    if iterations < 0:
        raise ValueError("layout_bh_arrays: iterations < 0")
    g = layout_graph(graph, edge_bits, d)
    n, mass = g["n"], g["mass"]
    if order == "perm":
        perm = np.asarray(perm, np.int64)
        if sorted(perm.tolist()) != list(range(n)):
            raise ValueError("layout_bh_arrays: perm is a permutation of the families")
    total = (lambda v: _total(v[perm], "left")) if order == "perm" else (lambda v: _total(v, order))
    xy = start_positions(n, pos, rng).copy()
    old = np.zeros((n, 2)) if old is None else np.array(old, np.float64).reshape(n, 2)
    speed, eff = float(speed), float(eff)
    comp = float(mass.mean()) if p["outbound_attraction_distribution"] and n else 1.0
    off = g["col"] != g["row"]
    ei, ej = g["row"][off], g["col"][off]
    fac = (-comp) * _edge_value(g["weight"][off], p["edge_weight_influence"])
    if p["outbound_attraction_distribution"]:
        fac = fac / mass[np.minimum(ei, ej)]
    forces, bound, rep = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    accepted, visited = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tree = tree_arrays(xy, mass)
    S = T = 0.0
    moved, comparisons = False, []
    for _ in range(iterations):
        tree = tree_arrays(xy, mass)
        rep, ab, accepted, visited = walk(tree, xy, mass, p["scaling_ratio"], theta)
        grav = (p["gravity"] * mass)[:, None] * xy
        for c in (0, 1):
            f = (0.0 + rep[:, c]) - grav[:, c]
            term = (xy[ei, c] - xy[ej, c]) * fac
            np.add.at(f, ei, term)                            # (unbuffered: a row's entries in CSR order)
            forces[:, c] = f
            b = ab[:, c] + np.abs(grav[:, c])
            np.add.at(b, ei, np.abs(term))
            bound[:, c] = b
        sx, sy = old[:, 0] - forces[:, 0], old[:, 1] - forces[:, 1]
        tx, ty = old[:, 0] + forces[:, 0], old[:, 1] + forces[:, 1]
        sw, tr = np.sqrt(sx * sx + sy * sy), np.sqrt(tx * tx + ty * ty)
        S, T = total(mass * sw), 0.5 * total(mass * tr)
        moved = T != 0.0
        if not moved:
            comparisons.append([])
            continue
        speed, eff, made = speed_control(n, S, T, speed, eff, p["jitter_tolerance"])
        comparisons.append(made)
        xy = xy + forces * speed / (1.0 + np.sqrt(speed * mass * sw))[:, None]
        old = forces.copy()
    return dict(pos=xy, forces=forces.copy(), speed=speed, eff=eff, S=S, T=T, iterations=iterations, bound=bound, old=old, moved=moved,
                comparisons=comparisons, tree=tree, accepted=accepted, visited=visited, repulsion=rep)
