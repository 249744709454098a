// nem_merge.hip -- see nem_merge.hpp.
#include "nem_merge.hpp"
#include "nem_scan.hpp"

#include <algorithm>

namespace nemk {

namespace {

using namespace seg;

// ---- the numbering ------------------------------------------------------------------------------------------------
// table[order[i]] = i: A's numbering by caller id (order null: the identity)
__global__ __launch_bounds__(kThreads) void k_merge_seed(const int* __restrict__ order, int n_a, int* __restrict__ table)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_a) table[order ? order[i] : i] = i;
}

// 1 for a family of B whose id A lacks
__global__ __launch_bounds__(kThreads) void k_merge_isnew(const int* __restrict__ ids, int n_b, const int* __restrict__ table, int* __restrict__ flag)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_b) flag[j] = table[ids[j]] < 0 ? 1 : 0;
}

// B's map (family j of B -> its number in the merged master), its inverse and the ids of the new families in B's order
__global__ __launch_bounds__(kThreads) void k_merge_map(const int* __restrict__ ids, int n_b, const int* __restrict__ table,
                                                        const int* __restrict__ rank, int n_a, int* __restrict__ mapb, int* __restrict__ bsrc,
                                                        int* __restrict__ new_ids)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n_b) return;
    const int id = ids[j];
    int m = table[id];
    if (m < 0) { m = n_a + rank[j]; new_ids[rank[j]] = id; }
    mapb[j] = m;
    bsrc[m] = j;                                              // (the ids are distinct: one writer per family)
}

// ---- the plan -----------------------------------------------------------------------------------------------------
// every entry of B: its place in A's row (a walk of the row), or -1; flag = 1 for an entry A lacks
__global__ __launch_bounds__(kThreads) void k_merge_lookup(int nnz_b, int n_b, const int* __restrict__ b_ptr, const int* __restrict__ b_idx,
                                                           const int* __restrict__ mapb, int n_a, const int* __restrict__ a_ptr,
                                                           const int* __restrict__ a_idx, int* __restrict__ apos, int* __restrict__ flag)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz_b) return;
    const int row = mapb[last_le(b_ptr, n_b, t)], nbr = mapb[b_idx[t]];
    int pos = -1;
    if (row < n_a && nbr < n_a)
        for (int u = a_ptr[row], u1 = a_ptr[row + 1]; u < u1; u++) if (a_idx[u] == nbr) { pos = u; break; }
    apos[t] = pos;
    flag[t] = pos < 0 ? 1 : 0;
}

// ---- the fill -----------------------------------------------------------------------------------------------------
// a merged row's degree: its A entries + the entries of its B row that A lacks (rank: the scanned flags, a segment's
// count = the difference at its row's ends)
__global__ __launch_bounds__(kThreads) void k_merge_degree(int n, int n_a, const int* __restrict__ a_ptr, const int* __restrict__ bsrc,
                                                           const int* __restrict__ b_ptr, const int* __restrict__ rank, int* __restrict__ deg)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const int j = bsrc[r];
    deg[r] = (r < n_a ? a_ptr[r + 1] - a_ptr[r] : 0) + (j >= 0 ? rank[b_ptr[j + 1]] - rank[b_ptr[j]] : 0);
}

// entry t of A keeps its place in its row: fwd[t] = where; there its neighbour and its A source
__global__ __launch_bounds__(kThreads) void k_merge_a_entries(int nnz_a, int n_a, const int* __restrict__ a_ptr, const int* __restrict__ a_idx,
                                                              const int* __restrict__ ptr, int* __restrict__ idx, int* __restrict__ src_a,
                                                              int* __restrict__ fwd)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz_a) return;
    const int r = last_le(a_ptr, n_a, t);
    const int e = ptr[r] + (t - a_ptr[r]);
    idx[e] = a_idx[t];
    src_a[e] = t;
    fwd[t] = e;
}

// entry t of B: A's entry where A has it, else behind its row's A entries by its rank among its B row's new ones, with
// its mapped neighbour; there its B source
__global__ __launch_bounds__(kThreads) void k_merge_b_entries(int nnz_b, int n_b, const int* __restrict__ b_ptr, const int* __restrict__ b_idx,
                                                              const int* __restrict__ mapb, const int* __restrict__ apos,
                                                              const int* __restrict__ rank, int n_a, const int* __restrict__ a_ptr,
                                                              const int* __restrict__ ptr, int* __restrict__ idx, int* __restrict__ src_b,
                                                              int* __restrict__ fwd)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz_b) return;
    const int rb = last_le(b_ptr, n_b, t);
    const int r = mapb[rb], op = apos[t];
    int e;
    if (op >= 0) e = ptr[r] + (op - a_ptr[r]);
    else {
        e = ptr[r] + (r < n_a ? a_ptr[r + 1] - a_ptr[r] : 0) + (rank[t] - rank[b_ptr[rb]]);
        idx[e] = mapb[b_idx[t]];
    }
    src_b[e] = t;
    fwd[t] = e;
}

// what the fill reads of one side: its edge_bits with their stride and the mask of the last word's data bits, its extras
// (xptr null: none)
struct Side {
    const uint32_t* bits;
    int wf;
    uint32_t last_mask;
    const int *xptr, *xorg, *xadd;
};

__device__ inline uint32_t side_word(const Side& m, int entry, int w)      // word w of the entry's organisms, 0 outside
{
    if (w < 0 || w >= m.wf) return 0u;
    const uint32_t v = m.bits[(size_t)entry * m.wf + w];
    return w == m.wf - 1 ? v & m.last_mask : v;
}

__device__ inline long long side_extra(const Side& m, int entry)          // the entry's copies beyond the first of each organism
{
    long long total = 0;
    if (m.xptr) for (int j = m.xptr[entry], j1 = m.xptr[entry + 1]; j < j1; j++) total += m.xadd[j];
    return total;
}

__device__ inline int side_bits(const Side& m, int entry)                 // the entry's organisms
{
    int total = 0;
    for (int w = 0; w < m.wf; w++) total += __popc(side_word(m, entry, w));
    return total;
}

// per merged entry (run when either master has extras): its number of extras (A's + B's), and the 2^24 bound where both
// masters have the entry (alone, each master holds it already).  An entry's count is its organisms + its extra
// copies: the bit rows are read only where the extra copies + all d organisms would pass the bound
__global__ __launch_bounds__(kThreads) void k_merge_xdeg(int nnz, const int* __restrict__ src_a, const int* __restrict__ src_b, Side a, Side b,
                                                         int d, int* __restrict__ xdeg, int* over)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nnz) return;
    const int sa = src_a[e], sb = src_b[e];
    const int x = (sa >= 0 && a.xptr ? a.xptr[sa + 1] - a.xptr[sa] : 0) + (sb >= 0 && b.xptr ? b.xptr[sb + 1] - b.xptr[sb] : 0);
    xdeg[e] = x;
    if (sa < 0 || sb < 0 || x == 0) return;
    const long long extra = side_extra(a, sa) + side_extra(b, sb);
    if (extra + d > (1 << 24) && extra + side_bits(a, sa) + side_bits(b, sb) > (1 << 24)) *over = 1;
}

// the merged edge_bits, one output word per thread: A's word, OR B's bits d_a bits further up -- the funnel shift of two
// of B's words (sh = d_a % 32 != 0) or B's word itself (q = d_a / 32 words further)
__global__ __launch_bounds__(kThreads) void k_merge_bits(long long words, int wf, const int* __restrict__ src_a, const int* __restrict__ src_b,
                                                         Side a, Side b, int q, int sh, uint32_t* __restrict__ bits)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= words) return;
    const long long e = i / wf;
    const int w = (int)(i - e * wf), sa = src_a[e], sb = src_b[e];
    uint32_t v = sa >= 0 ? side_word(a, sa, w) : 0u;
    if (sb >= 0) {
        const int k = w - q;
        v |= sh ? (side_word(b, sb, k) << sh) | (side_word(b, sb, k - 1) >> (32 - sh)) : side_word(b, sb, k);
    }
    bits[i] = v;
}

// extra j of a side's entry t goes to entry fwd[t]'s extras: A's at their head, B's behind the entry's A extras (skip: A's
// extras; every column of B lies behind every column of A), its organism shifted by `shift`
__global__ __launch_bounds__(kThreads) void k_merge_extras(int nx, int nnz_side, Side m, const int* __restrict__ fwd, const int* __restrict__ src_a,
                                                           const int* __restrict__ skip, int shift, const int* __restrict__ xptr,
                                                           int* __restrict__ xorg, int* __restrict__ xadd)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= nx) return;
    const int t = last_le(m.xptr, nnz_side, j);               // the extra's entry
    const int e = fwd[t];
    int dst = xptr[e] + (j - m.xptr[t]);
    if (skip) { const int sa = src_a[e]; if (sa >= 0) dst += skip[sa + 1] - skip[sa]; }
    xorg[dst] = m.xorg[j] + shift;
    xadd[dst] = m.xadd[j];
}

// A's organism rows at the merged stride, zero for the new families
__global__ __launch_bounds__(kThreads) void k_merge_xt_a(long long words, int nw64, int nw64_a, const uint64_t* __restrict__ a_xt,
                                                         uint64_t* __restrict__ xt)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= words) return;
    const long long o = i / nw64;
    const int w = (int)(i - o * nw64);
    xt[i] = w < nw64_a ? a_xt[(size_t)o * nw64_a + w] : 0ull;
}

// B's organism rows: one wave makes one 64-family word of one organism -- every lane tests the bit of its family's B
// source, the wave's ballot is the word
__global__ __launch_bounds__(kThreads) void k_merge_xt_b(long long waves, int nw64, int n, const int* __restrict__ bsrc,
                                                         const uint64_t* __restrict__ b_xt, int nw64_b, int d_a, uint64_t* __restrict__ xt)
{
    const long long wave = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (wave >= waves) return;                                // (uniform over the wave)
    const long long o = wave / nw64;
    const int w = (int)(wave - o * nw64), i = w * 64 + lane_id();
    const int j = i < n ? bsrc[i] : -1;
    const bool has = j >= 0 && ((b_xt[(size_t)o * nw64_b + (j >> 6)] >> (j & 63)) & 1ull);
    const uint64_t word = __ballot(has);
    if (lane_id() == 0) xt[((size_t)d_a + o) * nw64 + w] = word;
}

}  // namespace

struct MergeBuild : Scratch {
    MasterDev a{}, b{};
    int n = 0;
    int *mapb = nullptr, *bsrc = nullptr;                     // B's family -> merged family; merged family -> B's, or -1
    int *apos = nullptr, *rank = nullptr;                     // per entry of B: its place in A or -1; the scanned "A lacks it" flags
    int *partial = nullptr, *over = nullptr;
};

void merge_free(MergeBuild* m) { delete m; }

#define MRG(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { delete m; return e_; } } while (0)

hipError_t merge_number(const MasterDev& a, const int32_t* order_a, const MasterDev& b, const int32_t* ids_b, int f, hipStream_t s,
                        MergeBuild** out, int* n, int32_t* new_ids)
{
    *out = nullptr; *n = 0;
    MergeBuild* m = new MergeBuild();
    m->a = a; m->b = b;
    int *table, *ids, *ord = nullptr, *rank, *fresh;
    const size_t most = (size_t)a.n + (size_t)b.n + (size_t)b.nnz;   // (above the items of the scans over B's families, B's entries, the merged rows)
    MRG(m->alloc(&table, f)); MRG(m->alloc(&ids, b.n)); MRG(m->alloc(&rank, (size_t)b.n + 1)); MRG(m->alloc(&fresh, b.n));
    MRG(m->alloc(&m->mapb, b.n)); MRG(m->alloc(&m->bsrc, (size_t)a.n + b.n));
    MRG(m->alloc(&m->partial, most / kScanTile + 2)); MRG(m->alloc(&m->over, 1));
    MRG(hipMemsetAsync(table, 0xff, (size_t)f * 4, s));
    MRG(hipMemsetAsync(m->bsrc, 0xff, ((size_t)a.n + b.n) * 4, s));
    MRG(hipMemsetAsync(m->over, 0, sizeof(int), s));
    MRG(hipMemcpyAsync(ids, ids_b, (size_t)b.n * 4, hipMemcpyHostToDevice, s));
    if (order_a) { MRG(m->alloc(&ord, a.n)); MRG(hipMemcpyAsync(ord, order_a, (size_t)a.n * 4, hipMemcpyHostToDevice, s)); }
    hipLaunchKernelGGL(k_merge_seed, dim3(blocks(a.n)), dim3(kThreads), 0, s, ord, a.n, table);
    hipLaunchKernelGGL(k_merge_isnew, dim3(blocks(b.n)), dim3(kThreads), 0, s, ids, b.n, table, rank);
    scan<int, OpSum<int>, false>(rank, rank, b.n, OpSum<int>(), 0, m->partial, rank + b.n, s);
    hipLaunchKernelGGL(k_merge_map, dim3(blocks(b.n)), dim3(kThreads), 0, s, ids, b.n, table, rank, a.n, m->mapb, m->bsrc, fresh);
    MRG(hipGetLastError());
    int added = 0;
    MRG(hipMemcpyAsync(&added, rank + b.n, sizeof(int), hipMemcpyDeviceToHost, s));
    MRG(hipStreamSynchronize(s));
    if (added > 0) { MRG(hipMemcpyAsync(new_ids, fresh, (size_t)added * 4, hipMemcpyDeviceToHost, s)); MRG(hipStreamSynchronize(s)); }
    m->n = *n = a.n + added;                                  // (n_a + n_b families at most: both below 2^31 / 2 by their own keys)
    *out = m;
    return hipSuccess;
}

#undef MRG
#define MRG(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

hipError_t merge_plan(MergeBuild* m, hipStream_t s, long long* nnz)
{
    const MasterDev &a = m->a, &b = m->b;
    MRG(m->alloc(&m->apos, b.nnz)); MRG(m->alloc(&m->rank, (size_t)b.nnz + 1));
    if (b.nnz > 0)
        hipLaunchKernelGGL(k_merge_lookup, dim3(blocks(b.nnz)), dim3(kThreads), 0, s, b.nnz, b.n, b.nei_ptr, b.nei_idx, m->mapb, a.n, a.nei_ptr,
                           a.nei_idx, m->apos, m->rank);
    scan<int, OpSum<int>, false>(m->rank, m->rank, b.nnz, OpSum<int>(), 0, m->partial, m->rank + b.nnz, s);
    MRG(hipGetLastError());
    int added = 0;
    MRG(hipMemcpyAsync(&added, m->rank + b.nnz, sizeof(int), hipMemcpyDeviceToHost, s));
    MRG(hipStreamSynchronize(s));
    *nnz = (long long)a.nnz + added;
    return hipSuccess;
}

hipError_t merge_fill(MergeBuild* m, int nx_a, int nx_b, int nnz, uint64_t* xt, int nw64, int* ptr, int* idx, uint32_t* edge_bits, int wf,
                      int* extra_ptr, int* extra_org, int* extra_add, int* over, hipStream_t s)
{
    const MasterDev &a = m->a, &b = m->b;
    const int n = m->n;
    auto side = [](const MasterDev& v, int nx) {
        return Side{v.edge_bits, v.wf, (v.d & 31) ? (1u << (v.d & 31)) - 1u : ~0u, nx > 0 ? v.extra_ptr : nullptr, v.extra_org, v.extra_add};
    };
    const Side sa = side(a, nx_a), sb = side(b, nx_b);
    *over = 0;
    // the presence rows
    const long long words_a = (long long)a.d * nw64, waves_b = (long long)b.d * nw64;
    if (waves_b / (kThreads / 64) >= 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_merge_xt_a, dim3(blocks(words_a)), dim3(kThreads), 0, s, words_a, nw64, a.nw64, a.xt, xt);
    hipLaunchKernelGGL(k_merge_xt_b, dim3((unsigned)((waves_b + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, waves_b, nw64, n,
                       m->bsrc, b.xt, b.nw64, a.d, xt);
    // the rows
    hipLaunchKernelGGL(k_merge_degree, dim3(blocks(n)), dim3(kThreads), 0, s, n, a.n, a.nei_ptr, m->bsrc, b.nei_ptr, m->rank, ptr);
    scan<int, OpSum<int>, false>(ptr, ptr, n, OpSum<int>(), 0, m->partial, ptr + n, s);
    if (nnz > 0) {
        int *src_a, *src_b, *fwd_a, *fwd_b, *partial;         // (partial: merge_number's is sized by the inputs alone)
        MRG(m->alloc(&src_a, nnz)); MRG(m->alloc(&src_b, nnz)); MRG(m->alloc(&fwd_a, a.nnz)); MRG(m->alloc(&fwd_b, b.nnz));
        MRG(m->alloc(&partial, (size_t)nnz / kScanTile + 2));
        MRG(hipMemsetAsync(src_a, 0xff, (size_t)nnz * 4, s));
        MRG(hipMemsetAsync(src_b, 0xff, (size_t)nnz * 4, s));
        if (a.nnz > 0)
            hipLaunchKernelGGL(k_merge_a_entries, dim3(blocks(a.nnz)), dim3(kThreads), 0, s, a.nnz, a.n, a.nei_ptr, a.nei_idx, ptr, idx, src_a, fwd_a);
        if (b.nnz > 0)
            hipLaunchKernelGGL(k_merge_b_entries, dim3(blocks(b.nnz)), dim3(kThreads), 0, s, b.nnz, b.n, b.nei_ptr, b.nei_idx, m->mapb, m->apos,
                               m->rank, a.n, a.nei_ptr, ptr, idx, src_b, fwd_b);
        if (extra_ptr) {                                      // (no extras at all: no count above the organisms)
            hipLaunchKernelGGL(k_merge_xdeg, dim3(blocks(nnz)), dim3(kThreads), 0, s, nnz, src_a, src_b, sa, sb, a.d + b.d, extra_ptr, m->over);
            scan<int, OpSum<int>, false>(extra_ptr, extra_ptr, nnz, OpSum<int>(), 0, partial, extra_ptr + nnz, s);
        }
        const long long words = (long long)nnz * wf;
        hipLaunchKernelGGL(k_merge_bits, dim3(blocks(words)), dim3(kThreads), 0, s, words, wf, src_a, src_b, sa, sb, a.d >> 5, a.d & 31, edge_bits);
        if (nx_a > 0)
            hipLaunchKernelGGL(k_merge_extras, dim3(blocks(nx_a)), dim3(kThreads), 0, s, nx_a, a.nnz, sa, fwd_a, src_a, (const int*)nullptr, 0,
                               extra_ptr, extra_org, extra_add);
        if (nx_b > 0)
            hipLaunchKernelGGL(k_merge_extras, dim3(blocks(nx_b)), dim3(kThreads), 0, s, nx_b, b.nnz, sb, fwd_b, src_a, sa.xptr, a.d, extra_ptr,
                               extra_org, extra_add);
    }
    MRG(hipGetLastError());
    MRG(hipMemcpyAsync(over, m->over, sizeof(int), hipMemcpyDeviceToHost, s));
    MRG(hipStreamSynchronize(s));
    return hipSuccess;
}

#undef MRG

}  // namespace nemk
