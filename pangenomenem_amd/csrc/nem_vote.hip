// nem_vote.hip -- kernels of the chunk vote (nem_vote.hpp; validate_family and the loop around it,
// ppanggolin.py:1015-1105).  Integer work and one float64 sum per class; gfx950, wave64.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_vote.hpp"

namespace nemk {

// Families of the pangenome (at least one selected organism, ppanggolin.py:982-993) and the core exact ones (all of them),
// from OR / AND over the selected organisms' 64-family words.  One block per word, the organisms spread over its threads.
__global__ __launch_bounds__(256) void k_vote_init(VoteState v, const uint64_t* __restrict__ xt, int nw64, const int* __restrict__ sel, int d_sel)
{
    __shared__ uint64_t s_or[256], s_and[256];
    const int g = blockIdx.x;
    uint64_t any = 0, all = ~0ull;
    for (int t = threadIdx.x; t < d_sel; t += 256) {
        const uint64_t w = xt[(size_t)sel[t] * nw64 + g];
        any |= w; all &= w;
    }
    s_or[threadIdx.x] = any; s_and[threadIdx.x] = all;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { s_or[threadIdx.x] |= s_or[threadIdx.x + h]; s_and[threadIdx.x] &= s_and[threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x < 64) {
        const int f = g * 64 + threadIdx.x;
        if (f < v.n) {
            const bool in = (s_or[0] >> threadIdx.x) & 1ull, core = (s_and[0] >> threadIdx.x) & 1ull;
            v.st[f] = (uint8_t)((in ? VOTE_IN_PAN : 0) | (in && core ? VOTE_CORE : 0));
            for (int c = 0; c < 4; c++) v.cnt[(size_t)f * 4 + c] = 0;
            v.first[f] = -1;
        }
    }
}

// A run's votes (run_partitioning, ppanggolin.py:1907-1957): thread h of a sample's block sums class h -- sum_mu = the
// centres that are not zero (a NaN is not zero: bool(nan) is True), sum_eps = the dispersions added in float64 left to
// right (Python 3.10's sum) -- then thread 0 takes the first maximum of each (max() keeps the first unless a later one is
// strictly greater) and maps the labels: P/S/C if persistent_k == 0 and shell_k == 1, else everything U (the ValueError
// branch, caught at :1977).  A run that ended with an emptied class has no .uf: everything U.
__global__ __launch_bounds__(64) void k_vote_classmap(const VoteDesc* __restrict__ desc, int k, uint8_t* __restrict__ maps)
{
    __shared__ int s_mu[8];
    __shared__ double s_eps[8];
    const VoteDesc d = desc[blockIdx.x];
    const int h = threadIdx.x;
    if (h < k && d.status == 0) {
        int mu = 0;
        double eps = 0.0;
        for (int o = 0; o < d.dc; o++) {
            mu += d.center[(size_t)h * d.dc + o] != 0.0f ? 1 : 0;
            eps += (double)d.disp[(size_t)h * d.dc + o];
        }
        s_mu[h] = mu; s_eps[h] = eps;
    }
    __syncthreads();
    if (h == 0) {
        bool ok = d.status == 0 && k == 3;
        if (ok) {
            int pk = 0, sk = 0;
            for (int c = 1; c < k; c++) {
                if (s_mu[c] > s_mu[pk]) pk = c;
                if (s_eps[c] > s_eps[sk]) sk = c;
            }
            ok = pk == 0 && sk == 1;
        }
        uint8_t* m = maps + (size_t)blockIdx.x * kVoteMapStride;
        for (int c = 0; c < kVoteMapStride; c++) m[c] = (uint8_t)(ok && c < 3 ? c : 3);
    }
}

// every kept family's code into its column of the sample's row of V
__global__ __launch_bounds__(256) void k_vote_scatter(const VoteDesc* __restrict__ desc, const uint8_t* __restrict__ maps,
                                                      uint8_t* __restrict__ V, int n)
{
    const VoteDesc d = desc[blockIdx.y];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.n) return;
    const int lab = d.lab[j] & 0x7F;
    V[(size_t)d.slot * n + d.list[j]] = maps[(size_t)blockIdx.y * kVoteMapStride + (lab < 3 ? lab : 3)];
}

// validate_family for one family over the rows 0 .. last of V, from its committed state (ppanggolin.py:1023-1031):
// every vote counts, validated or not; an unvalidated family is validated by the vote that makes its total exceed
// len(organisms) / chunk_size with an absolute majority, or exceed len(organisms); U is forced if it then has none.
struct FamilyVote { int c[4]; uint8_t st; int32_t first; int vslot; };
__device__ __forceinline__ void vote_rows(FamilyVote& fv, const uint8_t* __restrict__ V, int n, int f, int last, double quotient,
                                          int d_sel, int64_t base)
{
    for (int s = 0; s <= last; s++) {
        const int code = V[(size_t)s * n + f];
        if (code == kVoteNone) continue;
        fv.c[code & 3]++;
        if (fv.st & VOTE_VALIDATED) continue;
        const int sum = fv.c[0] + fv.c[1] + fv.c[2] + fv.c[3];
        const int mx = max(max(fv.c[0], fv.c[1]), max(fv.c[2], fv.c[3]));
        if (((double)sum > quotient && 2 * mx >= sum) || sum > d_sel) {
            fv.st |= VOTE_VALIDATED;
            if (2 * mx < sum) fv.st |= VOTE_FORCED_U;
            fv.first = (int32_t)(base + s);
            fv.vslot = s;
        }
    }
}

__device__ __forceinline__ FamilyVote vote_load(const VoteState& v, int f)
{
    FamilyVote fv;
    for (int c = 0; c < 4; c++) fv.c[c] = v.cnt[(size_t)f * 4 + c];
    fv.st = v.st[f]; fv.first = v.first[f]; fv.vslot = -1;
    return fv;
}

// pass 1: where the batch validates what; nothing is written back.  words[0] += families still unvalidated,
// words[1] = max(1 + row at which a family validated)
__global__ __launch_bounds__(256) void k_vote_scan(VoteState v, const uint8_t* __restrict__ V, int count, double quotient, int d_sel,
                                                   int* __restrict__ words)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    int unval = 0, top = 0;
    if (f < v.n && (v.st[f] & VOTE_IN_PAN)) {
        FamilyVote fv = vote_load(v, f);
        vote_rows(fv, V, v.n, f, count - 1, quotient, d_sel, 0);
        unval = (fv.st & VOTE_VALIDATED) ? 0 : 1;
        top = fv.vslot + 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unval += __shfl_xor(unval, o, 64);
        top = max(top, __shfl_xor(top, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (unval) atomicAdd(&words[0], unval);
        if (top) atomicMax(&words[1], top);
    }
}

// pass 2: the rows up to the stop (the last row if something is still unvalidated) into the committed state
__global__ __launch_bounds__(256) void k_vote_commit(VoteState v, const uint8_t* __restrict__ V, int count, double quotient, int d_sel,
                                                     int64_t base, const int* __restrict__ words)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= v.n || !(v.st[f] & VOTE_IN_PAN)) return;
    const int last = words[0] == 0 ? words[1] - 1 : count - 1;
    FamilyVote fv = vote_load(v, f);
    vote_rows(fv, V, v.n, f, last, quotient, d_sel, base);
    for (int c = 0; c < 4; c++) v.cnt[(size_t)f * 4 + c] = fv.c[c];
    v.st[f] = fv.st;
    v.first[f] = fv.first;
}

void launch_vote_init(const VoteState& v, const uint64_t* xt, int nw64, const int* sel, int d_sel, hipStream_t s)
{
    hipLaunchKernelGGL(k_vote_init, dim3(nw64), dim3(256), 0, s, v, xt, nw64, sel, d_sel);
}

void launch_vote_classmap(const VoteDesc* desc, int count, int k, uint8_t* maps, hipStream_t s)
{
    hipLaunchKernelGGL(k_vote_classmap, dim3(count), dim3(64), 0, s, desc, k, maps);
}

void launch_vote_scatter(const VoteDesc* desc, int count, int max_n, const uint8_t* maps, uint8_t* V, int n, hipStream_t s)
{
    if (max_n <= 0) return;
    hipLaunchKernelGGL(k_vote_scatter, dim3((max_n + 255) / 256, count), dim3(256), 0, s, desc, maps, V, n);
}

void launch_vote_scan(const VoteState& v, const uint8_t* V, int count, double quotient, int d_sel, int64_t base, int* words, hipStream_t s)
{
    const int blocks = (v.n + 255) / 256;
    hipLaunchKernelGGL(k_vote_scan, dim3(blocks), dim3(256), 0, s, v, V, count, quotient, d_sel, words);
    hipLaunchKernelGGL(k_vote_commit, dim3(blocks), dim3(256), 0, s, v, V, count, quotient, d_sel, base, words);
}

}  // namespace nemk
