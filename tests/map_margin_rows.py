"""Rows of unnormalised class probabilities (cinum of ComputeLocalProba, non-negative doubles, inf, NaN) for the tests of
the NCEM label shortcut (pangenomenem_amd/csrc/nem_map.hpp), a plain numpy restatement of what the reference makes of a
row (ComputeLocalProba's normalisation, nem_alg.c:2589-2607, then ComputeMAP's first maximum and count of later equal
entries, nem_alg.c:603-640) and of the decision "clear", and the ctypes signatures of the two test hooks."""
import ctypes as C

import numpy as np

EPSILON = 1e-20
MARGIN = 2.0 ** -16
FLOOR = 2.0 ** -1000
# binary exponents of the rows' common scale: the subnormal range, both sides of the floor 2^-1000, both sides of
# cum = 1e-20 (2^-67 = 6.8e-21, 2^-66 = 1.36e-20, times K), around 1, and up to where the sum overflows
SCALES = (-1070, -1040, -1023, -1022, -1001, -1000, -999, -960, -70, -69, -68, -67, -66, -65, -1, 0, 1, 511, 1000, 1018, 1021, 1022)


def declare(lib):
    lib.nemgpu_map_margin_host.restype = C.c_int
    lib.nemgpu_map_margin_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.nemgpu_map_margin_device.restype = C.c_int
    lib.nemgpu_map_margin_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p]
    return lib


def host_rows(lib, rows):
    """out[i] = (full path's label, full path's nequal, unnormalised row's first maximum, clear)"""
    rows = np.ascontiguousarray(rows, np.float64)
    out = np.zeros((rows.shape[0], 4), np.int32)
    assert lib.nemgpu_map_margin_host(rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data) == 0
    return out


def device_rows(lib, pkf, ctx=None, beta=0.0):
    pkf = np.ascontiguousarray(pkf, np.float64)
    use_nei = ctx is not None
    ctx = np.ascontiguousarray(ctx if use_nei else np.zeros(pkf.shape), np.float32)
    out = np.zeros((pkf.shape[0], 4), np.int32)
    assert lib.nemgpu_map_margin_device(pkf.ctypes.data, ctx.ctypes.data, pkf.shape[0], pkf.shape[1], beta, int(use_nei), 0, out.ctypes.data) == 0
    return out


def row_sums(rows):
    with np.errstate(all="ignore"):
        cum = np.zeros(rows.shape[0])
        for k in range(rows.shape[1]):
            cum = cum + rows[:, k]
    return cum


def numpy_full(rows):
    """(label, nequal) of the reference's arithmetic, IEEE double and float operations one by one"""
    n, K = rows.shape
    cum = row_sums(rows)
    with np.errstate(all="ignore"):
        a = ((1 / cum)[:, None] * rows).astype(np.float32)
        b = ((1 / (cum / EPSILON))[:, None] * (rows / EPSILON)).astype(np.float32)
    cf = np.where((cum > EPSILON)[:, None], a, b)
    cf[~(cum > 0)] = np.float32(1.0 / K)
    ukmax = cf[:, 0].copy()
    kmax = np.zeros(n, np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(1, K):
            g = cf[:, k] > ukmax
            ukmax[g] = cf[g, k]
            kmax[g] = k
        nequal = np.zeros(n, np.int64)
        for k in range(1, K):
            nequal += (k > kmax) & (cf[:, k] == ukmax)
    return kmax, nequal


def top_two(rows):
    """largest entry and the largest of the others (a second copy of the largest counts); NaN rows: whatever"""
    s = np.sort(np.where(np.isnan(rows), -1.0, rows), axis=1)
    v1 = s[:, -1]
    v2 = s[:, -2] if rows.shape[1] > 1 else np.zeros(rows.shape[0])
    return v1, v2


def numpy_clear(rows):
    cum = row_sums(rows)
    v1, v2 = top_two(rows)
    with np.errstate(all="ignore"):
        return (cum > 0) & np.isfinite(cum) & (v1 >= FLOOR) & (v2 <= v1 * (1.0 - MARGIN))


def whole_range_rows(rng, K, n):
    """every entry's exponent uniform over the doubles' whole range, a few zeros"""
    x = np.ldexp(1.0 + rng.random((n, K)), rng.integers(-1074, 1024, size=(n, K)))
    x[rng.random((n, K)) < 0.03] = 0.0
    return x


def narrow_rows(rng, K, n):
    """entries within a few binades of each other (rows the normalisation does not trivialise), at every scale"""
    e0 = rng.integers(-1074, 1021, size=(n, 1))
    return np.ldexp(1.0 + rng.random((n, K)), np.minimum(e0 + rng.integers(-3, 4, size=(n, K)), 1023))


def near_tie_rows(rng, K):
    """the two largest entries a factor 1 + 2^-t apart (and an ulp either side of it), t = 10 .. 30, the others at or
    just below the second: the top quotient v1 / cum lies just above 1 / K -- for K = 2, 4, 8, 16, 32 a power of two,
    where the spacing of the float row changes -- and the second one on either side of it; at every scale of SCALES;
    positions shuffled"""
    mant = (1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), 1.5)
    rows = []
    for t in range(10, 31):
        for e in SCALES:
            for rep in range(8):
                m = mant[rep % 4] if rep < 4 else 1.0 + rng.random()
                v = np.ldexp(m, e)
                top = v * (1.0 + 2.0 ** -t)
                if rep % 3 == 1:
                    top = np.nextafter(top, np.inf)
                elif rep % 3 == 2:
                    top = np.nextafter(top, 0.0)
                d = rng.choice([0.0, 2.0 ** -t, 2.0 ** -(t + 1), 2.0 ** -12, 2.0 ** -30], size=K - 2) * rng.random(K - 2)
                if rep % 4 == 3:
                    d[:] = 0.0                           # (all others equal to the second: its quotient is below 1 / K)
                row = np.concatenate([[top, v], v * (1.0 - d)])
                rng.shuffle(row)
                rows.append(row)
    with np.errstate(over="ignore"):
        return np.array(rows)


def epsilon_rows(rng, K, n):
    """rows whose sum lands within a few ulps of EPSILON, on both sides (the sum decides the normalisation branch)"""
    r = rng.random((n, K)) * np.ldexp(1.0, rng.integers(-6, 1, size=(n, K)))
    r[:, 0] = r[:, 1] * (1.0 + np.ldexp(1.0, -rng.integers(8, 31, size=n)))   # some near ties
    r = r[np.arange(n)[:, None], rng.permuted(np.tile(np.arange(K), (n, 1)), axis=1)]
    return r * (EPSILON / row_sums(r))[:, None]


def special_rows(K):
    """exact ties, zeros, subnormal entries and sums, the floor, inf and NaN, sums that overflow"""
    tiny = 5e-324
    big = np.finfo(np.float64).max
    heads = [
        [1.0, 1.0], [0.3, 0.3], [2.0, 1.0], [1.0, 2.0], [0.0, 0.0], [0.0, 1.0], [1.0, 0.0],
        [tiny, 0.0], [tiny, tiny], [2 * tiny, tiny], [1e-310, 2e-310], [3e-310, 2e-310], [1e-310, 1e-310],
        [FLOOR, FLOOR / 2], [np.nextafter(FLOOR, 0.0), FLOOR / 4], [FLOOR, FLOOR], [FLOOR * 2, tiny],
        [1e-21, 3e-21], [1e-20, 0.0], [np.nextafter(1e-20, 1.0), 0.0], [np.nextafter(1e-20, 0.0), 0.0], [5e-21, 5e-21],
        [np.inf, 1.0], [1.0, np.inf], [np.inf, np.inf], [np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [np.inf, np.nan],
        [np.inf, 0.0], [0.0, np.nan],
        [big, big / 2], [big, big], [big / 4, big / 16], [1e308, 1e300], [1e308, 1e308 * (1 + 2.0 ** -12)], [big / 2, big / 2],
    ]
    rows = []
    for h in heads:
        for fill in (0.0, min(h), max(h)):           # (min / max of a NaN pair: NaN)
            for rot in range(K):
                rows.append(np.roll(np.array(h + [fill] * (K - 2)), rot))
    return np.array(rows)
