// nem_scan.hpp -- the block scans and the wave segment reduction that the units working on sorted records share
// (nem_orders.hip: the master's build and append; nem_project.hip: a partition's projection; nem_matrix.hip: the family
// table; nem_edges.hip: the edge table).  256-thread blocks of 4 waves; a scan is three launches (tile totals, their
// prefixes, the tiles), in place allowed.  With them what they do around rocPRIM's radix sort: the key widths, a call's
// scratch buffers, the sort itself, the search of a CSR's rows.  Then what the readers of the master share beyond that:
// the segments of sorted (segment, length) keys -- run heads, segment starts, the scans of the distinct lengths and a
// segment's statistics from them -- and the copy of a run of text out of LDS in aligned 8-byte words.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <vector>

// in a function that returns a hipError_t
#define HIPTRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

namespace nemk {
namespace seg {

constexpr int kThreads = 256;
constexpr int kScanItems = 8, kScanTile = kThreads * kScanItems;

struct OpMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct OpOr { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; } };
template <class T> struct OpSum { __device__ T operator()(T a, T b) const { return a + b; } };

__device__ inline int lane_id() { return threadIdx.x & 63; }

// the last j in [0, count) with a[j] <= x (a non-decreasing, a[0] <= x): the row of entry x in a CSR's pointers
__device__ inline int last_le(const int* a, int count, int x)
{
    int lo = 0, hi = count;
    while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (a[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// the first j in [lo, hi) with a[j] >= x (hi: none)
template <class T> __device__ inline int lower_bound(const T* a, int lo, int hi, T x)
{
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

__device__ inline int digits_of(int v)            // decimal digits of v >= 0
{
    return 1 + (v >= 10) + (v >= 100) + (v >= 1000) + (v >= 10000) + (v >= 100000) + (v >= 1000000) + (v >= 10000000) + (v >= 100000000) +
           (v >= 1000000000);
}

// the value of an inclusive scan before position p
template <class T> __device__ inline T before(const T* inclusive, int p) { return p > 0 ? inclusive[p - 1] : (T)0; }

constexpr uint32_t kLenBias = 0x80000000u;        // a length as an unsigned key field: negatives sort first

// the bits of a key field that holds 0 .. count - 1 (at least 1)
static inline int bits_for(int count) { int b = 1; while (b < 31 && (1ll << b) < count) b++; return b; }
static inline int blocks(long long n) { return (int)((n + kThreads - 1) / kThreads); }

// device buffers that live as long as their owner (hidden: each unit's own, as everything here is)
struct __attribute__((visibility("hidden"))) Scratch {
    std::vector<void*> mem;
    ~Scratch() { for (void* p : mem) (void)hipFree(p); }
    template <class T> hipError_t alloc(T** p, size_t count)
    {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) mem.push_back(v);
        *p = (T*)v;
        return e;
    }
};

// a device array of a result that outlives the call (at least one item)
template <class T> static hipError_t dev_alloc(T** p, size_t count)
{
    return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
}

// (k0, v0) sorted by the keys' bits [0, end_bit) with (k1, v1) as the other halves of rocPRIM's double buffers; *k_out,
// *v_out: the halves that hold the result; the sort's temporary storage is mem's
template <class K> static hipError_t sort_pairs(Scratch& mem, K* k0, K* k1, uint32_t* v0, uint32_t* v1, int count, int end_bit, const K** k_out,
                                                const uint32_t** v_out, hipStream_t s)
{
    rocprim::double_buffer<K> keys(k0, k1);
    rocprim::double_buffer<uint32_t> vals(v0, v1);
    size_t bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, keys, vals, (unsigned)count, 0u, (unsigned)end_bit, s);
    if (e != hipSuccess) return e;
    char* tmp = nullptr;
    if ((e = mem.alloc(&tmp, bytes)) != hipSuccess) return e;
    if ((e = rocprim::radix_sort_pairs(tmp, bytes, keys, vals, (unsigned)count, 0u, (unsigned)end_bit, s)) != hipSuccess) return e;
    *k_out = keys.current();
    *v_out = vals.current();
    return hipSuccess;
}

// keys alone, the same way: k0 sorted by its bits [0, end_bit), k1 the other half; *k_out: the half that holds the result
template <class K> static hipError_t sort_keys(Scratch& mem, K* k0, K* k1, int count, int end_bit, const K** k_out, hipStream_t s)
{
    rocprim::double_buffer<K> keys(k0, k1);
    size_t bytes = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, bytes, keys, (unsigned)count, 0u, (unsigned)end_bit, s);
    if (e != hipSuccess) return e;
    char* tmp = nullptr;
    if ((e = mem.alloc(&tmp, bytes)) != hipSuccess) return e;
    if ((e = rocprim::radix_sort_keys(tmp, bytes, keys, (unsigned)count, 0u, (unsigned)end_bit, s)) != hipSuccess) return e;
    *k_out = keys.current();
    return hipSuccess;
}

// ---- scans ----------------------------------------------------------------------------------------------------
// exclusive prefix of v over the block's 256 threads (4 waves); *total (may be null): the block's total
template <class T, class Op> __device__ inline T block_exclusive(T v, Op op, T ident, T* s_tot, T* total)
{
    const int lane = lane_id(), w = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const T o = __shfl_up(inc, off); if (lane >= off) inc = op(o, inc); }
    if (lane == 63) s_tot[w] = inc;
    T ex = __shfl_up(inc, 1);
    if (lane == 0) ex = ident;
    __syncthreads();
    T pre = ident, all = ident;
    for (int j = 0; j < kThreads / 64; j++) { if (j < w) pre = op(pre, s_tot[j]); all = op(all, s_tot[j]); }
    if (total) *total = all;
    __syncthreads();
    return op(pre, ex);
}

template <class T, class Op> __global__ __launch_bounds__(kThreads) void k_scan_reduce(const T* __restrict__ in, int n, Op op, T ident,
                                                                                     T* __restrict__ partial)
{
    __shared__ T s_tot[kThreads / 64];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    T v = ident;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) if (base + j < n) v = op(v, in[base + j]);
    T all;
    (void)block_exclusive(v, op, ident, s_tot, &all);
    if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

// the tiles' totals -> their exclusive prefixes, in place (one block); *total_out (may be null) = the grand total
template <class T, class Op> __global__ __launch_bounds__(kThreads) void k_scan_partials(T* __restrict__ partial, int nb, Op op, T ident,
                                                                                       T* __restrict__ total_out)
{
    __shared__ T s_tot[kThreads / 64];
    T carry = ident;
    for (int base = 0; base < nb; base += kThreads) {
        const int i = base + threadIdx.x;
        const T v = i < nb ? partial[i] : ident;
        T all;
        const T ex = block_exclusive(v, op, ident, s_tot, &all);
        if (i < nb) partial[i] = op(carry, ex);
        carry = op(carry, all);
    }
    if (total_out && threadIdx.x == 0) *total_out = carry;
}

template <class T, class Op, bool kInclusive>
__global__ __launch_bounds__(kThreads) void k_scan_apply(const T* in, int n, Op op, T ident, const T* __restrict__ partial, T* out)
{
    __shared__ T s_tot[kThreads / 64];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    T item[kScanItems];
    T v = ident;
#pragma unroll
    for (int j = 0; j < kScanItems; j++) { item[j] = base + j < n ? in[base + j] : ident; v = op(v, item[j]); }
    T run = op(partial[blockIdx.x], block_exclusive(v, op, ident, s_tot, (T*)nullptr));
#pragma unroll
    for (int j = 0; j < kScanItems; j++) {
        const T next = op(run, item[j]);
        if (base + j < n) out[base + j] = kInclusive ? next : run;
        run = next;
    }
}

// out = scan of in over n items (in place allowed); partial: room for ceil(n / kScanTile) items
template <class T, class Op, bool kInclusive> void scan(const T* in, T* out, int n, Op op, T ident, T* partial, T* total_out, hipStream_t s)
{
    const int nb = (n + kScanTile - 1) / kScanTile;
    if (nb == 0) { if (total_out) (void)hipMemsetAsync(total_out, 0, sizeof(T), s); return; }   // (only the sums are called with n = 0)
    hipLaunchKernelGGL((k_scan_reduce<T, Op>), dim3(nb), dim3(kThreads), 0, s, in, n, op, ident, partial);
    hipLaunchKernelGGL((k_scan_partials<T, Op>), dim3(1), dim3(kThreads), 0, s, partial, nb, op, ident, total_out);
    hipLaunchKernelGGL((k_scan_apply<T, Op, kInclusive>), dim3(nb), dim3(kThreads), 0, s, in, n, op, ident, (const T*)partial, out);
}

// inclusive scan of val over the wave's lanes of equal key (equal keys are adjacent); tail: the segment's last lane
template <class K, class V, class Op> __device__ inline V wave_segment(K key, V val, Op op, bool& tail)
{
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const K k2 = __shfl_up(key, off);
        const V v2 = __shfl_up(val, off);
        if (lane >= off && k2 == key) val = op(v2, val);
    }
    const K kn = __shfl_down(key, 1);
    tail = lane == 63 || kn != key;
    return val;
}

// ---- segments of sorted keys ------------------------------------------------------------------------------------
// a run of equal keys starts at p; the keys from `none` up belong to no run and sort behind all
template <class K> __device__ inline bool is_head(const K* keys, int p, K none)
{
    const K k = keys[p];
    return k < none && (p == 0 || keys[p - 1] != k);
}

// sstart[i] = the first sorted position of segment i (i = count: the end of the keys that belong to one), the segment in
// the key's bits from `shift` up
template <class K> __global__ __launch_bounds__(kThreads) void k_seg_starts(const K* __restrict__ keys, int g, int shift, int count, int* __restrict__ sstart)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i <= count) sstart[i] = lower_bound(keys, 0, g, (K)(uint32_t)i << shift);
}

// per sorted (segment, length) key, the length (biased) in its low 32 bits: 1 and the length where a distinct length starts
template <class K> __global__ __launch_bounds__(kThreads) void k_seg_lengths(const K* __restrict__ keys, int g, K none, int* __restrict__ dflag,
                                                                           long long* __restrict__ dval)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const bool h = is_head(keys, p, none);
    dflag[p] = h ? 1 : 0;
    dval[p] = h ? (long long)(int)((uint32_t)keys[p] ^ kLenBias) : 0ll;
}

// the inclusive scans of k_seg_lengths' flags and values over g sorted keys, with the buffers they are made in
struct SegLengths {
    int *didx = nullptr, *partial = nullptr;
    long long *dsum = nullptr, *lpartial = nullptr;

    hipError_t alloc(Scratch& mem, int g)
    {
        HIPTRY(mem.alloc(&didx, g)); HIPTRY(mem.alloc(&dsum, g));
        HIPTRY(mem.alloc(&partial, (size_t)g / kScanTile + 2)); HIPTRY(mem.alloc(&lpartial, (size_t)g / kScanTile + 2));
        return hipSuccess;
    }
    // sums false: didx alone (dsum then holds the values unscanned)
    template <class K> void run(const K* keys, int g, K none, bool sums, hipStream_t s) const
    {
        hipLaunchKernelGGL(k_seg_lengths<K>, dim3(blocks(g)), dim3(kThreads), 0, s, keys, g, none, didx, dsum);
        scan<int, OpSum<int>, true>(didx, didx, g, OpSum<int>(), 0, partial, (int*)nullptr, s);
        if (sums) scan<long long, OpSum<long long>, true>(dsum, dsum, g, OpSum<long long>(), 0ll, lpartial, (long long*)nullptr, s);
    }
};

// what the distinct lengths of the segment at sorted positions [a, b) give, from the scans at its ends and its first and
// last key (an empty segment: zeros)
__device__ inline void length_stats(const uint64_t* key_len, const int* didx, const long long* dsum, int a, int b, int* distinct, long long* sum,
                                    int* min, int* max)
{
    *distinct = before(didx, b) - before(didx, a);
    *sum = before(dsum, b) - before(dsum, a);
    *min = b > a ? (int)((uint32_t)key_len[a] ^ kLenBias) : 0;
    *max = b > a ? (int)((uint32_t)key_len[b - 1] ^ kLenBias) : 0;
}

// ---- text ---------------------------------------------------------------------------------------------------------
__device__ inline char* put_digits(char* at, int v)      // v >= 0 in decimal at `at`; returns the end
{
    const int nd = digits_of(v);
    for (int q = nd - 1; q >= 0; q--) { at[q] = (char)('0' + v % 10); v /= 10; }
    return at + nd;
}

// the wave writes the run of `len` bytes at text + start: word_at(k, r0) gives the k-th 8-byte word of the run laid out at
// the global address's misalignment (start & 7), r0 its first byte relative to the run; whole words go out as words, the
// run's first and last partial words by their own bytes only.  staged (uniform over the wave): the lanes have just laid
// the run out in LDS and word_at reads other lanes' bytes -- they wait for each other before the words are read, and
// again before the caller's next run overwrites the stage
template <class WordAt> __device__ inline void store_run(char* __restrict__ text, long long start, int len, bool staged, WordAt word_at)
{
    if (staged) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int mis = (int)(start & 7);
    char* base = text + (start - mis);                        // 8-byte aligned: its words are the text's words
    const int nwords = (mis + len + 7) >> 3;
    for (int k = lane_id(); k < nwords; k += 64) {
        const int r0 = 8 * k - mis;
        const uint64_t word = word_at(k, r0);
        if (r0 >= 0 && r0 + 8 <= len) {
            *(uint64_t*)(base + 8 * (size_t)k) = word;
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++)
                if (r0 + b >= 0 && r0 + b < len) base[8 * (size_t)k + b] = (char)(word >> (8 * b));
        }
    }
    if (staged) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace seg
}  // namespace nemk
