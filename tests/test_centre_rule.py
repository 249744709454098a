"""The centres of a non-empty NCEM class in integers (density_fused_body's centre_of, nem_kernels.hip) against the float
rule it stands in for -- ComputeMedian's three-way comparison of the zero count with N_k / 2 in float32, the inertia that
goes with it, twice the inertia truncated to an integer and the two mismatch mask bits abs((int)(x - mu)), x = 0, 1.
No GPU: both rules are stated here in numpy, the float one in float32 operation by operation as the kernel's other path
(and k_finish) compute it.  Exhaustive for N_k <= 300, random pairs below 2^24, every S1 at N_k = 2^24 - 1; N_k = 2^24
and 2^24 + 1 must take the float path (at 2^24 + 1 the two rules do differ)."""
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gate():
    """kCentreIntMax as the kernel source states it"""
    src = open(os.path.join(ROOT, "pangenomenem_amd", "csrc", "nem_kernels.hip")).read()
    m = re.search(r"constexpr int kCentreIntMax = 1 << (\d+);", src)
    assert m, "kCentreIntMax not found in nem_kernels.hip"
    return 1 << int(m.group(1))


def takes_integer_path(nk):
    return 0 < nk < gate()


def float_rule(nk, s1):
    """centre, inertia, (long long)(2.0f * inertia), a0, a1 -- float32 throughout (nk: int, s1: int64 array)"""
    nkf = F(nk)
    half = nkf / F(2)
    s0f = (nk - s1).astype(F)
    gt, eq = s0f > half, s0f == half
    mu = np.where(gt, F(0), np.where(eq, F(0.5), F(1))).astype(F)
    inertia = np.where(gt, s1.astype(F), np.where(eq, F(0.5) * nkf, s0f)).astype(F)
    twice = (F(2) * inertia).astype(np.int64)
    a0 = np.abs((F(0) - mu).astype(np.int32)) != 0       # (astype truncates toward zero, as the C cast does)
    a1 = np.abs((F(1) - mu).astype(np.int32)) != 0
    return mu, inertia, twice, a0, a1


def integer_rule(nk, s1):
    s0 = nk - s1
    inertia = np.minimum(s0, s1)
    a0, a1 = s0 < s1, s0 > s1
    mu = np.where(a1, F(0), np.where(a0, F(1), F(0.5))).astype(F)
    return mu, inertia.astype(F), 2 * inertia, a0, a1


def assert_same(nk, s1):
    s1 = np.asarray(s1, np.int64)
    want, got = float_rule(nk, s1), integer_rule(nk, s1)
    for name, u, v in zip(("centre", "inertia", "twice the inertia", "a0", "a1"), want, got):
        assert u.dtype == v.dtype, (name, u.dtype, v.dtype)
        bad = np.nonzero(u != v)[0]
        assert bad.size == 0, (name, nk, int(s1[bad[0]]), u[bad[0]], v[bad[0]])


def test_gate_is_two_to_the_24():
    assert gate() == 1 << 24
    assert takes_integer_path((1 << 24) - 1)
    assert not takes_integer_path(1 << 24) and not takes_integer_path((1 << 24) + 1)
    assert not takes_integer_path(0)                     # the empty class keeps its centres


def test_exhaustive_small_classes():
    for nk in range(1, 301):
        assert_same(nk, np.arange(nk + 1))


def test_ties_and_near_ties():
    """even N_k with S0 = N_k / 2 (centre 1/2, no mask bit) and the counts one to either side of it"""
    for nk in (2, 4, 300, 20000, (1 << 24) - 2):
        s1 = np.array([nk // 2 - 1, nk // 2, nk // 2 + 1], np.int64)
        mu, _, twice, a0, a1 = integer_rule(nk, s1)
        assert mu.tolist() == [0.0, 0.5, 1.0]
        assert a0.tolist() == [False, False, True] and a1.tolist() == [True, False, False]
        assert twice.tolist() == [nk - 2, nk, nk - 2]
        assert_same(nk, s1)
    for nk in (3, 301, 19999, (1 << 24) - 1):            # odd: no tie
        s1 = np.array([nk // 2, nk // 2 + 1], np.int64)
        assert integer_rule(nk, s1)[0].tolist() == [0.0, 1.0]
        assert_same(nk, s1)


def test_random_pairs_below_the_gate():
    rng = np.random.default_rng(24)
    nks = np.concatenate([rng.integers(1, 1 << 24, 3000), (1 << rng.integers(1, 25, 200)) - rng.integers(0, 2, 200)])
    for nk in nks.tolist():
        nk = min(max(int(nk), 1), (1 << 24) - 1)
        s1 = np.concatenate([rng.integers(0, nk + 1, 64), [0, nk, nk // 2, (nk + 1) // 2, max(nk // 2 - 1, 0), min(nk // 2 + 1, nk)]])
        assert_same(nk, s1)


def test_largest_class_on_the_integer_path():
    nk = (1 << 24) - 1
    assert takes_integer_path(nk)
    assert_same(nk, np.arange(nk + 1, dtype=np.int64))
    # a thread's rows and a wave's lanes add the inertia in 32 bits: four rows, 64 lanes, at most N_k / 2 each
    assert 4 * 64 * (nk // 2) < 1 << 31


def test_sizes_that_keep_the_float_path():
    """2^24 is still exact in float32 (the rules agree; the gate is the kernel's usual `< 2^24`); at 2^24 + 1 the class
    size rounds and the rules part: S1 = 2^23 + 1 ties in float32, not in integers"""
    nk = 1 << 24
    assert not takes_integer_path(nk)
    assert_same(nk, np.array([0, 1, nk // 2 - 1, nk // 2, nk // 2 + 1, nk - 1, nk], np.int64))
    nk = (1 << 24) + 1
    assert not takes_integer_path(nk)
    s1 = np.array([(1 << 23) + 1], np.int64)
    assert float_rule(nk, s1)[0][0] == F(0.5) and integer_rule(nk, s1)[0][0] == F(1)
