"""An NCEM site's label from the unnormalised row (pangenomenem_amd/csrc/nem_map.hpp): wherever the decision says
"clear", the first maximum of the unnormalised row is the label ComputeLocalProba + ComputeMAP give, and no later entry
equals the maximum as a float (nequal = 0, no draw) -- in both normalisation branches.  The library's host hook runs
the header's own functions (the decision, and the normalisation and ComputeMAP the device code calls); a numpy
restatement of the reference's arithmetic and of the decision stands next to it.  No GPU needed.

Inputs: random rows for K = 2 .. 7 over the whole double range and within a few binades at every scale; rows whose
two largest entries differ by 1 + 2^-t, t = 10 .. 30, with their quotients either side of 1 / K (a power of two for
K = 2, 4, 8, 16, 32); exact ties, zeros, all-zero rows; subnormal entries and sums; sums just above and below EPSILON; inf and
NaN entries; sums that overflow."""
import numpy as np
import pytest

from tests import map_margin_rows as mm


@pytest.fixture(scope="module")
def lib():
    from pangenomenem_amd import build, engine
    build.build()
    return mm.declare(engine.load_library())


def hold(lib, rows):
    """the C hook equals the numpy restatement, row by row; clear rows have the full path's label and nequal = 0"""
    out = mm.host_rows(lib, rows)
    kmax, nequal = mm.numpy_full(rows)
    assert np.array_equal(out[:, 0], kmax) and np.array_equal(out[:, 1], nequal)
    assert np.array_equal(out[:, 3] != 0, mm.numpy_clear(rows))
    clear = out[:, 3] != 0
    bad = clear & ((out[:, 2] != out[:, 0]) | (out[:, 1] != 0))
    assert not bad.any(), (rows[bad][:5], out[bad][:5])
    return out


@pytest.mark.parametrize("K", [2, 3, 4, 5, 6, 7])
def test_random_rows_and_coverage(lib, K):
    rng = np.random.Generator(np.random.PCG64(1100 + K))
    rows = mm.whole_range_rows(rng, K, 40000)
    out = hold(lib, rows)
    # the shortcut must fire: at least 99 % of the random rows with a gap of at least 2^-10
    v1, v2 = mm.top_two(rows)
    with np.errstate(all="ignore"):
        gap = v1 >= v2 * (1.0 + 2.0 ** -10)
    assert gap.sum() > 30000
    assert (out[gap, 3] != 0).mean() >= 0.99, (out[gap, 3] != 0).mean()
    rows = mm.narrow_rows(rng, K, 40000)
    out = hold(lib, rows)
    v1, v2 = mm.top_two(rows)
    with np.errstate(all="ignore"):
        sure = (v1 >= v2 * (1.0 + 2.0 ** -10)) & (v1 >= mm.FLOOR) & np.isfinite(mm.row_sums(rows))
    assert sure.sum() > 20000 and (out[sure, 3] != 0).all()


@pytest.mark.parametrize("K", [2, 3, 4, 5, 7, 8, 16, 32])
def test_near_ties_at_every_scale(lib, K):
    rng = np.random.Generator(np.random.PCG64(1200 + K))
    rows = mm.near_tie_rows(rng, K)
    out = hold(lib, rows)
    # both kinds of row are there: gaps above the margin fire, gaps below it do not; and float ties do occur
    assert (out[:, 3] != 0).sum() > 300 and (out[:, 3] == 0).sum() > 300
    assert (out[:, 1] > 0).any()
    # ... and the second quotient lies on both sides of 1 / K, the top one (never below it) next to it
    cum = mm.row_sums(rows)
    v1, v2 = mm.top_two(rows)
    ok = np.isfinite(cum) & (v1 >= mm.FLOOR)
    with np.errstate(all="ignore"):
        q1, q2 = (v1 / cum)[ok], (v2 / cum)[ok]
    assert (q1 < (1.0 + 2.0 ** -9) / K).any() and (q2 < 1.0 / K).any()
    if K > 2:
        assert (q2 > 1.0 / K).any()


@pytest.mark.parametrize("K", [2, 3, 5, 7])
def test_sums_next_to_epsilon(lib, K):
    rng = np.random.Generator(np.random.PCG64(1300 + K))
    rows = mm.epsilon_rows(rng, K, 20000)
    cum = mm.row_sums(rows)
    assert (cum > mm.EPSILON).sum() > 1000 and (cum <= mm.EPSILON).sum() > 1000
    assert np.abs(cum / mm.EPSILON - 1.0).max() < 1e-14
    out = hold(lib, rows)
    assert (out[:, 3] != 0).sum() > 1000 and (out[:, 3] == 0).sum() > 100


@pytest.mark.parametrize("K", [2, 3, 4, 7])
def test_special_rows(lib, K):
    rows = mm.special_rows(K)
    out = hold(lib, rows)
    cum = mm.row_sums(rows)
    # a row with a NaN or inf entry or sum, a zero sum, or an exact tie at the top never takes the shortcut
    v1, v2 = mm.top_two(rows)
    never = ~np.isfinite(cum) | ~(cum > 0) | (v1 == v2) | np.isnan(rows).any(axis=1)
    assert never.sum() > 50 and not (out[never, 3] != 0).any()
    assert (out[:, 3] != 0).sum() > 20


def test_single_class_rows(lib):
    rows = np.array([[1.0], [0.0], [5e-324], [1e-20], [np.inf], [np.nan], [2.0 ** -1000], [1e308]])
    out = hold(lib, rows)
    assert np.array_equal(out[:, 0], np.zeros(8)) and np.array_equal(out[:, 3] != 0, [True, False, False, True, False, False, True, True])
