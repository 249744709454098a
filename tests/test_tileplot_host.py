"""The numpy statements of the presence/absence plot (pangenomenem_amd/tileplot.py), which the device is held to in
tests/test_gpu_tileplot.py: the distances bit for bit against scipy's "jaccard", the merges against scipy's complete
linkage on tie-free data (heights bit for bit, merged sets equal: with pairwise distinct distances the tree is unique),
the tie rule on hand-made inputs, R's merge matrix and leaf order, the family order against a plain sorted()."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import pdist

from pangenomenem_amd import tileplot as tp
from tests.tileplot_util import LARGE, LARGE_SEEDS, SMALL, SMALL_SEEDS, condensed, distinct, hub_matrix, merged_sets, random_matrix


def linkage_sets(z, d):
    members = {i: frozenset([i]) for i in range(d)}
    out = []
    for k, row in enumerate(z):
        members[d + k] = members[int(row[0])] | members[int(row[1])]
        out.append(members[d + k])
    return out


@pytest.mark.parametrize("n,d,seed", [(3000, 12, 0), (500, 9, 1), (64, 5, 2), (1, 4, 3)])
def test_distances_are_scipys_jaccard_bit_for_bit(n, d, seed):
    x = random_matrix(n, d, seed)
    x[:, 0] = 0                                               # an organism with no family
    x[:, 2] = x[:, 1]                                         # two identical organisms
    x[::3] *= 3                                               # (a cell above 1 counts as 1)
    got = tp.organism_distances_host(x)
    assert got.dtype == np.float64 and got.shape == (d, d)
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    assert got[1, 2] == 0.0 and (got[0, 1] == 1.0 or not x[:, 1].any())
    assert condensed(got).tobytes() == pdist(x.T != 0, "jaccard").tobytes()


def test_two_empty_organisms_are_at_distance_zero():
    assert not tp.organism_distances_host(np.zeros((7, 3), np.uint8)).any()


@pytest.mark.parametrize("shape,seed", [(SMALL, s) for s in SMALL_SEEDS] + [(LARGE, s) for s in LARGE_SEEDS])
def test_merges_are_scipys_complete_linkage_on_tie_free_data(shape, seed):
    dist = tp.organism_distances_host(random_matrix(*shape, seed))
    cond = condensed(dist)
    assert distinct(cond), "the input must have pairwise distinct distances: pick another seed"
    i2, j2, height = tp.hclust_complete_host(dist)
    z = linkage(cond, "complete")
    assert (i2 < j2).all()
    assert height.tobytes() == z[:, 2].tobytes()
    assert merged_sets(i2, j2) == linkage_sets(z, shape[1])


def test_the_lowest_indices_win_every_tie():
    i2, j2, height = tp.hclust_complete_host(1.0 - np.eye(4))
    assert i2.tolist() == [0, 0, 0] and j2.tolist() == [1, 2, 3] and height.tolist() == [1.0, 1.0, 1.0]
    # two pairs at the same least distance: the lower row first; then a tie between a row's candidates: the lower column
    dist = np.array([[0.0, 0.5, 0.9, 0.9],
                     [0.5, 0.0, 0.9, 0.9],
                     [0.9, 0.9, 0.0, 0.5],
                     [0.9, 0.9, 0.5, 0.0]])
    i2, j2, height = tp.hclust_complete_host(dist)
    assert list(zip(i2.tolist(), j2.tolist(), height.tolist())) == [(0, 1, 0.5), (2, 3, 0.5), (0, 2, 0.9)]


def test_a_row_searched_again_changes_its_nearest_neighbour():
    # row 0 names 2 (0.2) until 2 is merged into 1: then d(0, {1, 2}) = 0.9 and its nearest is 3 (0.5)
    dist = np.zeros((4, 4))
    for (a, b), v in {(1, 2): 0.1, (0, 2): 0.2, (0, 1): 0.9, (0, 3): 0.5, (1, 3): 0.6, (2, 3): 0.7}.items():
        dist[a, b] = dist[b, a] = v
    i2, j2, height = tp.hclust_complete_host(dist)
    assert list(zip(i2.tolist(), j2.tolist(), height.tolist())) == [(1, 2, 0.1), (0, 3, 0.5), (0, 1, 0.9)]
    assert np.array_equal(dist, dist.T)                       # (the input is not changed)
    merge = tp.r_merge(i2, j2)
    assert merge.tolist() == [[-2, -3], [-1, -4], [1, 2]]
    assert tp.hclust_order(merge).tolist() == [1, 2, 0, 3]


def test_every_row_naming_the_retired_organism_is_searched_again():
    x = hub_matrix()
    d = x.shape[1]
    dist = tp.organism_distances_host(x)
    assert (np.argmin(dist[:d - 1] + np.tril(np.full((d, d), 2.0))[:d - 1], axis=1) == d - 1).all()
    i2, j2, height = tp.hclust_complete_host(dist)
    assert (i2[0], j2[0], height[0]) == (d - 2, d - 1, dist[d - 2, d - 1])
    # (complete linkage: the heights ascend and the last is the largest distance of all)
    assert (np.diff(height) >= 0).all() and height[-1] == dist.max()


def test_r_merge_signs_and_order_within_a_row():
    # singletons by increasing index; a singleton before a cluster; two clusters by increasing step
    i2, j2 = [4, 0, 0, 2, 0], [5, 1, 4, 3, 2]
    merge = tp.r_merge(i2, j2)
    assert merge.tolist() == [[-5, -6], [-1, -2], [1, 2], [-3, -4], [3, 4]]
    assert tp.hclust_order(merge).tolist() == [4, 5, 0, 1, 2, 3]
    merge = tp.r_merge([0, 0, 0], [1, 2, 3])
    assert merge.tolist() == [[-1, -2], [-3, 1], [-4, 2]]
    assert tp.hclust_order(merge).tolist() == [3, 2, 0, 1]
    assert tp.r_merge([], []).shape == (0, 2) and tp.hclust_order(tp.r_merge([], [])).tolist() == [0]


@pytest.mark.parametrize("seed", range(4))
def test_order_is_a_permutation_with_every_cluster_contiguous(seed):
    d = 37
    x = random_matrix(150, d, seed)
    x[:, 5] = x[:, 6]                                         # (ties too)
    i2, j2, _ = tp.hclust_complete_host(tp.organism_distances_host(x))
    order = tp.hclust_order(tp.r_merge(i2, j2))
    assert sorted(order.tolist()) == list(range(d))
    where = np.argsort(order)
    for members in merged_sets(i2, j2):
        at = where[sorted(members)]
        assert at.max() - at.min() + 1 == len(members)


def test_family_order_is_the_stable_sort_by_the_three_keys():
    rng = np.random.default_rng(5)
    n, d = 400, 9
    part = rng.integers(0, 4, n).astype(np.uint8)             # P S C U
    nb_org = rng.integers(1, d + 1, n)                        # few values: ties in all three keys, nb_org == d among them
    want = sorted(range(n), key=lambda i: ({0: 0, 1: 1, 2: 2}.get(int(part[i]), 3), 0 if nb_org[i] == d else 1, -int(nb_org[i])))
    got = tp.family_plot_order(part, nb_org, d)
    assert got.dtype == np.int32 and got.tolist() == want
    assert (part == 3).any() and (nb_org == d).any() and part[got[-1]] == 3
    with pytest.raises(ValueError):
        tp.family_plot_order(part, nb_org[:-1], d)


def test_cells_are_the_reordered_presence():
    x = random_matrix(30, 7, 1) * 2
    fam, org = np.arange(30)[::-1], np.asarray([3, 0, 6, 1, 2, 5, 4])
    cells = tp.tile_cells_host(x, fam, org, 4, 10)
    assert cells.dtype == np.uint8 and cells.shape == (10, 7) and cells.max() == 1
    for r in range(10):
        for c in range(7):
            assert cells[r, c] == (x[fam[4 + r], org[c]] != 0)
