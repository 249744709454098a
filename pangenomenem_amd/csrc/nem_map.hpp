// nem_map.hpp -- an NCEM site's label from the UNNORMALISED row, where the row's maximum is clear.
//
// ComputeLocalProba (reference nem_alg.c:2576-2613) turns the row  cinum[k] = pkf[k] * exp(beta ctx[k])  (doubles,
// non-negative, or NaN / inf where the factor overflowed), cum = their sum in index order, into the float row
//     cum > EPSILON :   cf[k] = (float)(invz * cinum[k]),              invz = 1 / cum
//     0 < cum <= EPSILON: cf[k] = (float)(invz * (cinum[k] / EPSILON)),  invz = 1 / (cum / EPSILON)        (EPSILON = 1e-20)
// and ComputeMAP (nem_alg.c:603-640) takes of it only the first position of the maximum and how many later entries
// EQUAL it as floats.  The fuzzy algorithm stores cf; NCEM does not, and the divisions (five in the second branch) are
// most of a site evaluation's double-rate instructions.
//
// A row is CLEAR (map_clear) when, with v1 = its largest entry (first position k1) and v2 = the largest of the others,
//     0 < cum < inf,    v1 >= kMapFloor,    v2 <= RN(v1 (1 - m)),  m = kMapMargin = 2^-16
// (every comparison false on a NaN; it implies v1 >= v2 (1 + m): v2 <= v1 (1 - m)(1 + 2^-53) and 1 / (1 - m) > 1 + m + m^2).
// One product per row, of the maximum, which is a normal double; K comparisons.   LEMMA: a clear row of non-negative entries has cf[k1] > cf[k] for every k != k1,
// in either branch, so ComputeMAP returns k1 with nequal = 0 and no draw is taken.
//   1. Ranges.  All entries are >= 0 and none is a NaN (one NaN makes cum a NaN, and `cum > 0` is false), so
//      v1 <= cum <= K v1 (1 + 2^-53)^(K-1), K <= 32, and cum is finite and at least 2^-1000.  First branch:
//      invz = RN(1 / cum) is positive -- a subnormal one above 2^-1025 when cum > 2^1022, which costs it precision but
//      it is one constant for the whole row -- and x1 = RN(invz v1) lies in [1/K (1 - 2^-50), 1 + 2^-50].  Second
//      branch: v1 / EPSILON and cum / EPSILON are normal (>= 2^-1000 / 1e-20 > 2^-934; even the smallest double at
//      all, 2^-1074, over 1e-20 is about 2^-1008, still normal, and its reciprocal is finite), invz =
//      RN(1 / RN(cum / EPSILON)) is normal, and x1 is in the same interval up to two more roundings.  So
//      cf[k1] = RN24(x1) is a normal float of at least about 1/K, at most 1.
//   2. Monotone.  Each step from cinum[k] to cf[k] -- RN(. / EPSILON), RN(invz .) with the same positive invz for
//      the whole row, RN24(.) -- is a non-decreasing map, so cf[k] <= cf[k2] for every k != k1, k2 = v2's position:
//      it is enough to separate cf[k1] from cf[k2].
//   3. Gap.  While the intermediate values of v2 stay normal, each double step keeps the ratio of the two up to a factor
//      (1 - 2^-53) / (1 + 2^-53): x1 / x2 >= (1 + m)(1 - 2^-51) after at most two steps each.  RN24 moves either by at
//      most a relative 2^-24, so cf[k1] / cf[k2] >= (1 + m)(1 - 2^-51)(1 - 2^-24) / (1 + 2^-24) > 1 as soon as
//      m >= 2^-22.  Where an intermediate value of v2 is subnormal or its float is subnormal or zero, that value is
//      below every normal one, thus below v1's, which is normal at every step: the order is kept strictly as well.
//   kMapMargin = 2^-16 is 64 times what step 3 needs; kMapFloor = 2^-1000 keeps step 1, and the test's own product
//   v1 (1 - m), in normal doubles.
// Rows that are not clear -- near ties, exact ties, zero density, inf or NaN entries or sum, a maximum below the floor --
// take the reference's arithmetic unchanged.  tests/test_map_margin.py holds the decision against that arithmetic.
#pragma once
#include "nem_ff.hpp"

namespace nemk {

constexpr double kMapMargin = 0x1p-16, kMapShrink = 1.0 - kMapMargin;   // (1 - 2^-16: exact)
constexpr double kMapFloor = 0x1p-1000, kMapCumMax = 0x1.fffffffffffffp1023;   // (the largest finite double)
constexpr double kMapEpsilon = 1e-20;                      // the reference's EPSILON (nem_typ.h)

// v1 = the row's largest entry, v2 = the largest of the others (0 for a row of one), cum = the row's sum
NEMFF_HD inline bool map_clear(double v1, double v2, double cum)
{
    return cum > 0.0 && cum <= kMapCumMax && v1 >= kMapFloor && v2 <= v1 * kMapShrink;
}

// The decision on a row: k1 = the first position of its maximum; returns map_clear(v1, v2, cum) -- written as "EVERY
// other entry is below the threshold", the same thing as "the largest of them is", which keeps one double alive across
// the row instead of two.  A NaN entry is below nothing: its row is not clear (nor is its sum).
template <int KA>
NEMFF_HD inline bool map_clear_row(const double* cinum, int K, double cum, int& k1)
{
    k1 = 0;
    double v1 = cinum[0];
#pragma unroll
    for (int k = 1; k < KA; k++) if (k < K && cinum[k] > v1) { v1 = cinum[k]; k1 = k; }
    // (& and |, not && and ||: a handful of comparisons, cheaper done than branched around lane by lane)
    bool clear = (cum > 0.0) & (cum <= kMapCumMax) & (v1 >= kMapFloor);
    const double thr = v1 * kMapShrink;
#pragma unroll
    for (int k = 0; k < KA; k++) if (k < K) clear &= (k == k1) | (cinum[k] <= thr);
    return clear;
}

// the reference's arithmetic: the normalised float row (ComputeLocalProba; returns true for "density = 0") ...
template <int KA>
NEMFF_HD inline bool map_normalise(const double* cinum, int K, double cum, float* cf)
{
    if (cum > 0) {                                       // nem_alg.c:2589-2601
        if (cum > kMapEpsilon) {
            const double invz = 1 / cum;
#pragma unroll
            for (int k = 0; k < KA; k++) if (k < K) cf[k] = (float)(invz * cinum[k]);
        } else {
            const double invz = 1 / (cum / kMapEpsilon);
#pragma unroll
            for (int k = 0; k < KA; k++) if (k < K) cf[k] = (float)(invz * (cinum[k] / kMapEpsilon));
        }
        return false;
    }
    const float u = (float)(1.0 / K);                    // nem_alg.c:2603-2607
#pragma unroll
    for (int k = 0; k < KA; k++) if (k < K) cf[k] = u;
    return true;
}
// ... and ComputeMAP's reading of it (nem_alg.c:603-640): first maximum, number of later entries equal to it
template <int KA>
NEMFF_HD inline int map_full(const float* cf, int K, int& nequal)
{
    int kmax = 0; float ukmax = cf[0];
#pragma unroll
    for (int k = 1; k < KA; k++) if (k < K && cf[k] > ukmax) { ukmax = cf[k]; kmax = k; }
    nequal = 0;
#pragma unroll
    for (int k = 1; k < KA; k++) if (k < K && k > kmax && cf[k] == ukmax) nequal++;
    return kmax;
}

// one row, both ways, on the CPU (test hook): the full path's label and nequal; returns whether the row is clear and
// then the shortcut's label in *k_clear
inline bool map_row_host(const double* cinum, int K, int* k_full, int* nequal_full, int* k_clear)
{
    constexpr int KA = 32;                               // kMaxKernelK
    double cum = 0.0;
    for (int k = 0; k < K; k++) cum = cum + cinum[k];
    float cf[KA];
    map_normalise<KA>(cinum, K, cum, cf);
    *k_full = map_full<KA>(cf, K, *nequal_full);
    return map_clear_row<KA>(cinum, K, cum, *k_clear);
}

}  // namespace nemk
