"""The presence/absence plot of the R script that PPanGGOLiN's CLI writes (``plot_Rscript``, command_line.py:40-252; the
tile plot is :75-101), from a resident master: the organisms clustered, the families ordered, the raster's cells.

The script reads the ``.Rtab``, sets every cell above 1 to 1 (:57) and computes::

    binary_matrix_hclust <- hclust(dist(t(binary_matrix), method="binary"))                       # :79
    binary_matrix = binary_matrix[order(match(NEM partitions, c("persistent","shell","cloud")),
                                        match(Former partitions, c("core_exact","accessory")),
                                        -occurences),
                                  c(binary_matrix_hclust$label[binary_matrix_hclust$order], ...)]  # :84-87

``dist(..., "binary")`` is the Jaccard distance between every pair of organisms over all families, ``hclust`` with its
default method ``"complete"`` is Murtagh's nearest-neighbour algorithm (``hclust.f``) followed by ``hcass2``, which turns
the merges into R's ``merge`` matrix and the leaf ``order``.  Here:

``organism_distances_host``, ``hclust_complete_host``, ``r_merge``, ``hclust_order``, ``family_plot_order`` and
``tile_cells_host`` state every step in numpy; ``nemgpu_orgclust_*`` (csrc/nem_orgdist.hip) computes the distances, the
merges and the cells on the device and is held to the statements bit for bit, ties included: the counts are integers, a
distance is one IEEE double division of two of them, and a merge only compares and copies stored doubles.
``Master.organism_clustering`` and ``Master.tile_plot`` (chunks.py) are the Python surface.

The distances equal R's and ``scipy.spatial.distance.pdist(x.T, "jaccard")`` bit for bit, and on data without tied
distances the tree is the complete-linkage tree, which is unique (the tests hold it to ``scipy.cluster.hierarchy.
linkage``).  The tie rule and the leaf order are ``hclust.f`` / ``hcass2`` as understood: they could not be run against
R.  Not here: the PDF and ggplot.
"""
import ctypes as C

import numpy as np

from .engine import NemGpuError
from .projection import part_codes, _popcount_rows


# ---- the statements --------------------------------------------------------------------------------------------------
def organism_distances_host(x):
    """What nemgpu_orgclust_create computes, in numpy: x uint8 [n][d] (families x organisms, non-zero: present) ->
    float64 [d][d], dist[i][j] = (uni - inter) / uni with inter = |A & B|, uni = |A| + |B| - inter over the families
    of organisms i and j, 0 where uni == 0 (R_dist_binary; scipy's "jaccard")."""
    b = (np.asarray(x) != 0).astype(np.float64)                # (counts below 2^53 are exact in a float64 product)
    inter = np.rint(b.T @ b).astype(np.int64)
    pop = np.diag(inter)
    uni = pop[:, None] + pop[None, :] - inter
    out = np.zeros(inter.shape, np.float64)
    np.divide((uni - inter).astype(np.float64), uni.astype(np.float64), out=out, where=uni > 0)
    return out


def hclust_complete_host(dist):
    """What nemgpu_orgclust_run computes, in numpy: R's hclust(method="complete") as hclust.f runs it.  dist: float64
    [d][d], symmetric.  Returns (i2 int32 [d - 1], j2 int32 [d - 1], height float64 [d - 1]).
      * NN(i), for i < d - 1: the nearest live j > i, found with a strict <: the lowest j wins a tie; DISNN(i) its distance;
      * d - 1 times: the live i of least DISNN, strict <: the lowest i wins a tie; I2 = min(i, NN(i)), J2 = max;
        (I2, J2, DISNN) is the merge; J2 is retired; for every live k != I2: d(I2, k) = max(d(I2, k), d(J2, k)), and
        NN(I2) is found anew among the k > I2; every live i < d - 1 whose NN was I2 or J2 searches its row again.
    A row with no live j above it has NN -1 and DISNN inf (hclust.f leaves a stale NN there, which nothing reads)."""
    w = np.array(dist, np.float64)
    d = len(w)
    if w.shape != (d, d):
        raise ValueError("hclust_complete_host: the full square float64 [d][d]")
    live = np.ones(d, bool)
    nn, disnn = np.full(d, -1, np.int64), np.full(d, np.inf)

    def search(i):
        js = np.flatnonzero(live[i + 1:]) + i + 1
        if not len(js):
            return -1, np.inf
        j = js[int(np.argmin(w[i, js]))]                       # (argmin: the first of equal minima)
        return int(j), w[i, j]

    for i in range(d - 1):
        nn[i], disnn[i] = search(i)
    i2, j2, height = np.zeros(max(d - 1, 0), np.int32), np.zeros(max(d - 1, 0), np.int32), np.zeros(max(d - 1, 0), np.float64)
    for s in range(d - 1):
        im = int(np.argmin(np.where(live[:d - 1], disnn[:d - 1], np.inf)))
        a, b = min(im, int(nn[im])), max(im, int(nn[im]))
        i2[s], j2[s], height[s] = a, b, disnn[im]
        live[b] = False
        ks = np.flatnonzero(live)
        ks = ks[ks != a]
        v = np.maximum(w[a, ks], w[b, ks])
        w[a, ks] = v
        w[ks, a] = v
        nn[a], disnn[a] = search(a)
        for i in np.flatnonzero(live[:d - 1] & ((nn[:d - 1] == a) | (nn[:d - 1] == b))):
            nn[i], disnn[i] = search(int(i))
    return i2, j2, height


def r_merge(i2, j2):
    """R's `merge` matrix (hcass2) of the merges (i2, j2): int32 [d - 1][2].  A singleton is -(index + 1), a cluster the
    1-based step that made it; within a row a singleton comes before a cluster, two singletons in increasing index, two
    clusters in increasing step."""
    i2, j2 = np.asarray(i2, np.int64), np.asarray(j2, np.int64)
    d = len(i2) + 1
    name = -(np.arange(d, dtype=np.int64) + 1)                 # what the cluster kept under an index is called now
    merge = np.zeros((d - 1, 2), np.int32)
    for s in range(d - 1):
        a, b = int(name[i2[s]]), int(name[j2[s]])
        if a > 0 and b > 0:
            a, b = min(a, b), max(a, b)
        elif a > 0:                                            # (b < 0: the singleton first)
            a, b = b, a
        merge[s] = a, b
        name[i2[s]] = s + 1
    return merge


def hclust_order(merge):
    """R's `order` (hcass2) of a merge matrix: from the last merge, every cluster expanded in place into its row's
    left, then right member.  int32 [d], 0-based organisms; d == 1 (no merge): [0]."""
    merge = np.asarray(merge).reshape(-1, 2)
    if not len(merge):
        return np.zeros(1, np.int32)
    out, stack = [], [len(merge)]
    while stack:
        v = stack.pop()
        if v < 0:
            out.append(-v - 1)
        else:
            stack.append(int(merge[v - 1, 1]))
            stack.append(int(merge[v - 1, 0]))
    return np.asarray(out, np.int32)


def family_plot_order(partitions, nb_org, d):
    """The plot's rows (command_line.py:84-86): the families in the stable order (R's order() is stable: ties stay in
    master order) by persistent < shell < cloud < anything else (match() gives NA for "undefined", NA sorts last), then
    core_exact (nb_org == d) < accessory, then nb_org descending.  partitions: uint8 [n] in P 0, S 1, C 2, U 3;
    nb_org int [n]: the organisms of every family (the row popcount).  int32 [n]."""
    part = np.ascontiguousarray(partitions, np.uint8)
    nb_org = np.ascontiguousarray(nb_org, np.int64)
    if part.shape != nb_org.shape or part.ndim != 1:
        raise ValueError("family_plot_order: partitions [n] and nb_org [n]")
    return np.lexsort((-nb_org, nb_org != int(d), np.minimum(part, 3))).astype(np.int32)      # (lexsort is stable)


def tile_cells_host(x, family_order, organism_order, row0=0, rows=None):
    """What nemgpu_orgclust_cells writes, in numpy: uint8 [rows][d], cell (r, c) = family family_order[row0 + r]
    present in organism organism_order[c]."""
    present = np.asarray(x) != 0
    fam = np.asarray(family_order)[row0:None if rows is None else row0 + rows]
    return present[fam][:, np.asarray(organism_order)].astype(np.uint8)


# ---- the device --------------------------------------------------------------------------------------------------------
CELLS_BUDGET = 64 << 20                                        # bytes of raster per device call (TilePlot.all_cells)


def _bind_orgclust(lib):
    lib.nemgpu_orgclust_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
    lib.nemgpu_orgclust_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.nemgpu_orgclust_distances.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.nemgpu_orgclust_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.nemgpu_orgclust_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.nemgpu_orgclust_destroy.argtypes = [C.c_void_p]
    lib.nemgpu_orgclust_destroy.restype = None
    lib.nemgpu_orgdist_tile_info.argtypes = [C.POINTER(C.c_int)] * 3
    return lib


def tile_info(lib=None):
    """(tile, chunk_words, max_organisms) of the distance kernel (nemgpu_orgdist_tile_info): the organisms per side of
    a block's tile, the 64-bit words of a row staged per step, the most organisms a clustering takes.  Host only."""
    if lib is None:
        from .engine import load_library
        lib = load_library()
    v = [C.c_int() for _ in range(3)]
    _bind_orgclust(lib).nemgpu_orgdist_tile_info(*(C.byref(a) for a in v))
    return tuple(a.value for a in v)


class OrganismClustering:
    """The organisms of a master clustered on the device (nemgpu_orgclust_create + _run): .i2, .j2 int32 [d - 1] and
    .height float64 [d - 1] as hclust_complete_host states them, .merge (r_merge) and .order (hclust_order) derived on
    the host, .labels (the master's organism names, else 0 .. d - 1); distances(i0, rows): rows of the resident square.
    The master is only read and must stay open as long as this is."""

    def __init__(self, master):
        self.lib, self.master, self._h = _bind_orgclust(master.lib), master, C.c_void_p()
        self._call("create", C.byref(self._h), master._h)
        n, d = C.c_int(), C.c_int()
        self._call("shape", self._h, C.byref(n), C.byref(d))
        self.n, self.d = n.value, d.value
        m = max(self.d - 1, 0)
        self.i2, self.j2, self.height = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.float64)
        self._call("run", self._h, *(a.ctypes.data if m else None for a in (self.i2, self.j2, self.height)))
        self.merge = r_merge(self.i2, self.j2)
        self.order = hclust_order(self.merge)
        names = getattr(master, "organism_names", None)
        self.labels = list(names) if names is not None else list(range(self.d))

    def _call(self, name, *args):
        name = "nemgpu_orgclust_" + name
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise NemGpuError("%s failed (status %d): %s" % (name, rc, self.lib.nemgpu_last_error().decode()))

    def distances(self, i0=0, rows=None):
        """rows i0 .. i0 + rows - 1 of the distance square: float64 [rows][d]"""
        rows = self.d - i0 if rows is None else rows
        out = np.zeros((max(int(rows), 0), self.d), np.float64)
        self._call("distances", self._h, int(i0), int(rows), out.ctypes.data)
        return out

    def cells(self, family_order, organism_order, row0=0, rows=None):
        """the raster's rows (nemgpu_orgclust_cells; tile_cells_host states them): uint8 [rows][d]"""
        fam = np.ascontiguousarray(family_order, np.int32)
        org = np.ascontiguousarray(organism_order, np.int32)
        if fam.shape != (self.n,) or org.shape != (self.d,):
            raise ValueError("cells: family_order [n] and organism_order [d]")
        rows = self.n - row0 if rows is None else rows
        out = np.zeros((max(int(rows), 0), self.d), np.uint8)
        self._call("cells", self._h, fam.ctypes.data, org.ctypes.data, int(row0), int(rows), out.ctypes.data)
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nemgpu_orgclust_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TilePlot:
    """What the tile plot draws (Master.tile_plot): .organism_order int32 [d] (the clustering's leaf order; the columns),
    .organism_labels (the labels in that order: R's label[order]), .family_order int32 [n] (family_plot_order; the rows),
    .clustering (the OrganismClustering), cells(row0, rows): the raster's rows uint8 [rows][d], gathered on the device."""

    def __init__(self, master, partitions):
        if isinstance(partitions, dict):
            if getattr(master, "names", None) is None:
                raise ValueError("tile_plot: this master carries no names (give the classes as uint8 [n])")
            partitions = part_codes(partitions, master.names)
        part = np.ascontiguousarray(partitions, np.uint8)
        if part.shape != (master.n,):
            raise ValueError("tile_plot: a class per family, P 0, S 1, C 2, U 3")
        self.family_order = family_plot_order(part, _popcount_rows(master._rows), master.d)
        self.clustering = OrganismClustering(master)
        self.organism_order = self.clustering.order
        self.organism_labels = [self.clustering.labels[o] for o in self.organism_order]
        self.n, self.d = self.clustering.n, self.clustering.d

    def cells(self, row0=0, rows=None):
        return self.clustering.cells(self.family_order, self.organism_order, row0, rows)

    def all_cells(self, budget=CELLS_BUDGET):
        """(row0, cells) batches covering the raster, each within the budget"""
        step = max(1, budget // max(self.d, 1))
        for row0 in range(0, self.n, step):
            yield row0, self.cells(row0, min(step, self.n - row0))

    def close(self):
        self.clustering.close()
