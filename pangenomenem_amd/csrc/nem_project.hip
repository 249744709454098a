// nem_project.hip -- see nem_project.hpp.
#include "nem_project.hpp"

namespace nemk {

namespace {

using namespace seg;
constexpr int kNoFamily = -2;                     // a caller id that no master family has
constexpr int kRepeated = -1;                     // a gene of a repeated family
constexpr uint8_t kCoreBit = 4;                   // a family's byte: its class (0 .. 3) | kCoreBit when it is in every organism
constexpr int kNeiShift = 10;                     // a wave's neighbour counts packed: three fields of 10 bits (each <= 64)

// ---- the families ----------------------------------------------------------------------------------------------
// cls[i] |= kCoreBit for a family present in all d organisms: a column count over the organism-major rows, one block per
// word of 64 families, its four waves sharing the organisms
__global__ __launch_bounds__(kThreads) void k_project_family(const uint64_t* __restrict__ xt, int n, int d, int nw64, uint8_t* __restrict__ cls)
{
    __shared__ int s_cnt[kThreads / 64][64];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    int cnt = 0;
    for (int o = w; o < d; o += kThreads / 64) cnt += (int)((xt[(size_t)o * nw64 + blockIdx.x] >> lane) & 1ull);
    s_cnt[w][lane] = cnt;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 64 + lane;
    if (w == 0 && i < n) {
        int total = 0;
        for (int j = 0; j < kThreads / 64; j++) total += s_cnt[j][lane];
        cls[i] = (uint8_t)((cls[i] & 3) | (total == d ? kCoreBit : 0));
    }
}

// nei[row][k] = the entries of the row whose neighbour is of class k < 3: one lane per CSR entry, the lanes of one row
// reduced inside the wave, one atomic per (row, class) and wave
__global__ __launch_bounds__(kThreads) void k_project_neighbours(const int* __restrict__ ptr, const int* __restrict__ idx, int nnz, int n,
                                                                const uint8_t* __restrict__ cls, int* nei)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const bool valid = t < nnz;
    int row = -1;
    uint32_t v = 0;
    if (valid) {
        row = last_le(ptr, n, (int)t);                        // ptr[row] <= t < ptr[row + 1]
        const int k = cls[idx[t]] & 3;
        if (k < 3) v = 1u << (kNeiShift * k);
    }
    bool tail;
    v = wave_segment(row, v, OpSum<uint32_t>(), tail);
    if (valid && tail && v) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int cnt = (int)((v >> (kNeiShift * k)) & ((1u << kNeiShift) - 1));
            if (cnt) atomicAdd(&nei[(size_t)row * 3 + k], cnt);
        }
    }
}

// ---- the numbering's inverse -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_project_fill(int* __restrict__ v, int count, int value)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < count) v[i] = value;
}

// inv[order[i]] = i (order null: the identity); an id outside [0, f) has no gene here
__global__ __launch_bounds__(kThreads) void k_project_inverse(const int* __restrict__ order, int n, int f, int* __restrict__ inv)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int id = order ? order[i] : i;
    if (id >= 0 && id < f) inv[id] = i;
}

// ---- the genes --------------------------------------------------------------------------------------------------
// one lane per gene: its organism (its contig's), its master family (kRepeated, kNoFamily: not counted); the counters
// of its organism (one byte each per wave: persistent, shell, cloud, undefined, core_exact, accessory) summed over
// the wave's lanes of equal organism, one atomic per run and non-zero counter; its key (organism, family) for the copies
__global__ __launch_bounds__(kThreads) void k_project_genes(const int* __restrict__ genes, int g, const int* __restrict__ cptr, int c,
                                                           const int* __restrict__ corg, const uint8_t* __restrict__ repeated,
                                                           const int* __restrict__ inv, const uint8_t* __restrict__ cls, int bn,
                                                           int* __restrict__ gene_family, int* org_counts, uint64_t* __restrict__ keys,
                                                           uint32_t* __restrict__ vals, uint64_t none)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const bool valid = p < g;
    int org = -1;
    unsigned long long v = 0;
    if (valid) {
        org = corg[last_le(cptr, c, p)];                      // its contig's: cptr[j] <= p < cptr[j + 1]
        const int id = genes[p];
        const int fam = (repeated && repeated[id]) ? kRepeated : inv[id];
        if (gene_family) gene_family[p] = fam;
        if (fam >= 0) {
            const int k = cls[fam];
            v = (1ull << (8 * (k & 3))) + (1ull << (8 * (4 + ((k & kCoreBit) ? 0 : 1))));
        }
        if (keys) {
            keys[p] = fam >= 0 ? (((uint64_t)(uint32_t)org << bn) | (uint64_t)(uint32_t)fam) : none;
            vals[p] = (uint32_t)p;
        }
    }
    if (org_counts) {                                         // (uniform: every lane takes the shuffles)
        // the wave's runs of one organism, numbered: an organism may come back later in the wave (its contigs need not
        // be adjacent), and wave_segment wants equal keys to be contiguous
        const int lane = lane_id();
        const int before = __shfl_up(org, 1);
        const unsigned long long heads = __ballot(lane == 0 || before != org);
        const int run = __popcll(heads & ((2ull << lane) - 1ull));
        bool tail;
        v = wave_segment(run, v, OpSum<unsigned long long>(), tail);
        if (valid && tail && v) {
            int* row = org_counts + (size_t)org * kProjectCounters;
            int kept = 0;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const int cnt = (int)((v >> (8 * k)) & 0xffull);
                if (cnt) atomicAdd(&row[k], cnt);
                if (k >= 4) kept += cnt;
            }
            atomicAdd(&row[6], kept);
        }
    }
}

// ---- the copies -------------------------------------------------------------------------------------------------
// per sorted key: 1 where a run of equal (organism, family) starts; the keys of the genes not counted sort behind all
__global__ __launch_bounds__(kThreads) void k_project_heads(const uint64_t* __restrict__ keys, int g, uint64_t none, int* __restrict__ flags)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g) return;
    flags[i] = is_head(keys, i, none) ? 1 : 0;
}

// run r (rid - 1: the inclusive scan of the heads) starts at starts[r]; the last kept key closes the last run
__global__ __launch_bounds__(kThreads) void k_project_runs(const uint64_t* __restrict__ keys, int g, uint64_t none, const int* __restrict__ rid,
                                                          int* __restrict__ starts)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g) return;
    if (keys[i] >= none) return;
    const int r = rid[i] - 1;
    if (is_head(keys, i, none)) starts[r] = i;
    if (i + 1 == g || keys[i + 1] >= none) starts[r + 1] = i + 1;
}

__global__ __launch_bounds__(kThreads) void k_project_copies(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int g, uint64_t none,
                                                            const int* __restrict__ rid, const int* __restrict__ starts, int* __restrict__ copies)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g) return;
    if (keys[i] >= none) return;
    const int r = rid[i] - 1;
    copies[vals[i]] = starts[r + 1] - starts[r];
}

}  // namespace

hipError_t upload_orders(Scratch& mem, const GeneOrdersIn& in, int n, hipStream_t s, GeneOrdersDev* out)
{
    const int f = in.f, g = in.g, c = in.c;
    int* order = nullptr;
    out->rep = nullptr;
    HIPTRY(mem.alloc(&out->inv, f)); HIPTRY(mem.alloc(&out->genes, g)); HIPTRY(mem.alloc(&out->cptr, (size_t)c + 1)); HIPTRY(mem.alloc(&out->corg, c));
    if (in.order) { HIPTRY(mem.alloc(&order, n)); HIPTRY(hipMemcpyAsync(order, in.order, (size_t)n * 4, hipMemcpyHostToDevice, s)); }
    if (in.repeated) { HIPTRY(mem.alloc(&out->rep, f)); HIPTRY(hipMemcpyAsync(out->rep, in.repeated, (size_t)f, hipMemcpyHostToDevice, s)); }
    HIPTRY(hipMemcpyAsync(out->genes, in.genes, (size_t)g * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(out->cptr, in.contig_ptr, ((size_t)c + 1) * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(out->corg, in.contig_org, (size_t)c * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_project_fill, dim3(blocks(f)), dim3(kThreads), 0, s, out->inv, f, kNoFamily);
    hipLaunchKernelGGL(k_project_inverse, dim3(blocks(n)), dim3(kThreads), 0, s, (const int*)order, n, f, out->inv);
    return hipSuccess;
}

hipError_t project(const MasterDev& m, const ProjectIn& in, int32_t* org_counts, int32_t* nei_counts, int32_t* gene_family,
                   int32_t* gene_copies, hipStream_t s)
{
    const int n = m.n, d = m.d, g = in.o.g, c = in.o.c;
    Scratch mem;
    // the families: class | core bit
    uint8_t* cls;
    HIPTRY(mem.alloc(&cls, n));
    HIPTRY(hipMemcpyAsync(cls, in.part, (size_t)n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_project_family, dim3(m.nw64), dim3(kThreads), 0, s, m.xt, n, d, m.nw64, cls);
    // the neighbours' classes
    int* nei = nullptr;
    if (nei_counts) {
        HIPTRY(mem.alloc(&nei, (size_t)n * 3));
        HIPTRY(hipMemsetAsync(nei, 0, (size_t)n * 3 * 4, s));
        if (m.nnz > 0)
            hipLaunchKernelGGL(k_project_neighbours, dim3(blocks(m.nnz)), dim3(kThreads), 0, s, m.nei_ptr, m.nei_idx, m.nnz, n, cls, nei);
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(nei_counts, nei, (size_t)n * 3 * 4, hipMemcpyDeviceToHost, s));
    }
    // the genes
    int* oc = nullptr;
    if (org_counts) {
        HIPTRY(mem.alloc(&oc, (size_t)d * kProjectCounters));
        HIPTRY(hipMemsetAsync(oc, 0, (size_t)d * kProjectCounters * 4, s));
    }
    if (g > 0 && (org_counts || gene_family || gene_copies)) {
        GeneOrdersDev o;
        int* gfam = nullptr;
        if (gene_family) HIPTRY(mem.alloc(&gfam, g));
        HIPTRY(upload_orders(mem, in.o, n, s, &o));
        const int bn = bits_for(n), bd = bits_for(d);
        const uint64_t none = (uint64_t)1 << (bn + bd);       // (bn + bd <= 53)
        uint64_t *k0 = nullptr, *k1 = nullptr;
        uint32_t *v0 = nullptr, *v1 = nullptr;
        if (gene_copies) { HIPTRY(mem.alloc(&k0, g)); HIPTRY(mem.alloc(&k1, g)); HIPTRY(mem.alloc(&v0, g)); HIPTRY(mem.alloc(&v1, g)); }
        hipLaunchKernelGGL(k_project_genes, dim3(blocks(g)), dim3(kThreads), 0, s, o.genes, g, o.cptr, c, o.corg, o.rep, o.inv, cls, bn, gfam, oc, k0, v0, none);
        HIPTRY(hipGetLastError());
        if (gene_family) HIPTRY(hipMemcpyAsync(gene_family, gfam, (size_t)g * 4, hipMemcpyDeviceToHost, s));
        if (gene_copies) {
            int *rid, *starts, *partial, *copies;
            HIPTRY(mem.alloc(&rid, g)); HIPTRY(mem.alloc(&starts, (size_t)g + 1)); HIPTRY(mem.alloc(&partial, (size_t)g / kScanTile + 2));
            HIPTRY(mem.alloc(&copies, g));
            const uint64_t* ks;
            const uint32_t* vs;
            HIPTRY(sort_pairs<uint64_t>(mem, k0, k1, v0, v1, g, bn + bd + 1, &ks, &vs, s));
            HIPTRY(hipMemsetAsync(copies, 0, (size_t)g * 4, s));
            hipLaunchKernelGGL(k_project_heads, dim3(blocks(g)), dim3(kThreads), 0, s, ks, g, none, rid);
            scan<int, OpSum<int>, true>(rid, rid, g, OpSum<int>(), 0, partial, (int*)nullptr, s);
            hipLaunchKernelGGL(k_project_runs, dim3(blocks(g)), dim3(kThreads), 0, s, ks, g, none, (const int*)rid, starts);
            hipLaunchKernelGGL(k_project_copies, dim3(blocks(g)), dim3(kThreads), 0, s, ks, vs, g, none, (const int*)rid, (const int*)starts, copies);
            HIPTRY(hipGetLastError());
            HIPTRY(hipMemcpyAsync(gene_copies, copies, (size_t)g * 4, hipMemcpyDeviceToHost, s));
        }
    }
    HIPTRY(hipGetLastError());
    if (org_counts) HIPTRY(hipMemcpyAsync(org_counts, oc, (size_t)d * kProjectCounters * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    return hipSuccess;
}

}  // namespace nemk
