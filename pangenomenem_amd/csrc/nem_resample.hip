// nem_resample.hip -- kernels of the evolution curve's stats (nem_resample.hpp; partition(just_stats=True),
// ppanggolin.py:982-993 and 1166-1170).  Integer work only; gfx950, wave64.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_resample.hpp"

namespace nemk {

// The families of a sample (at least one of its organisms, ppanggolin.py:982-993) split into core_exact (all of them)
// and accessory (the rest), as k_vote_init splits one selection.  Block (s, y) is sample s; its thread g = 64 y + lane
// holds 64-family word g of the master and ORs / ANDs it over the sample's organisms, so the lanes of a wave read
// consecutive words of one organism row.  The words' popcounts are summed over the wave, and its first lane adds them
// into the sample's two counters.
__global__ __launch_bounds__(kResampleCoreWave) void k_resample_core(const uint64_t* __restrict__ xt, int n, int nw64,
                                                                    const int* __restrict__ org, const int* __restrict__ off,
                                                                    int32_t* __restrict__ stats)
{
    const int s = blockIdx.x;
    const int g = blockIdx.y * kResampleCoreWave + threadIdx.x;
    int core = 0, acc = 0;
    if (g < nw64) {
        const int t0 = off[s], t1 = off[s + 1];
        uint64_t any = 0, all = ~0ull;
#pragma unroll 4
        for (int t = t0; t < t1; t++) {
            const uint64_t w = xt[(size_t)org[t] * nw64 + g];
            any |= w; all &= w;
        }
        const int tail = n - g * 64;                          // (families beyond n in the last word are not counted)
        const uint64_t valid = tail >= 64 ? ~0ull : (1ull << tail) - 1ull;
        core = __popcll(any & all & valid);
        acc = __popcll(any & ~all & valid);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        core += __shfl_xor(core, o, 64);
        acc += __shfl_xor(acc, o, 64);
    }
    if (threadIdx.x == 0) {
        if (core) atomicAdd(&stats[(size_t)s * kResampleStats + 4], core);
        if (acc) atomicAdd(&stats[(size_t)s * kResampleStats + 5], acc);
    }
}

// One sample per block: every kept family's label (bit 7 masked, as k_vote_scatter reads it) through the sample's
// code map, counted per code in each thread's registers, summed over the wave, then over the block's waves in LDS.
// A run that emptied a class maps every label to U (k_vote_classmap), so all its families are undefined.
constexpr int kTallyThreads = 256;
__global__ __launch_bounds__(kTallyThreads) void k_resample_tally(const VoteDesc* __restrict__ desc, const uint8_t* __restrict__ maps,
                                                                  int32_t* __restrict__ stats)
{
    __shared__ int s_cnt[kTallyThreads / 64][4];
    const VoteDesc d = desc[blockIdx.x];
    const uint8_t* m = maps + (size_t)blockIdx.x * kVoteMapStride;
    const int m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int j = threadIdx.x; j < d.n; j += kTallyThreads) {
        const int lab = d.lab[j] & 0x7F;
        const int code = lab == 0 ? m0 : lab == 1 ? m1 : lab == 2 ? m2 : m3;
        c0 += code == 0; c1 += code == 1; c2 += code == 2; c3 += code == 3;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o, 64);
        c1 += __shfl_xor(c1, o, 64);
        c2 += __shfl_xor(c2, o, 64);
        c3 += __shfl_xor(c3, o, 64);
    }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) { s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; s_cnt[wave][2] = c2; s_cnt[wave][3] = c3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        int sum = 0;
        for (int w = 0; w < kTallyThreads / 64; w++) sum += s_cnt[w][threadIdx.x];
        stats[(size_t)d.slot * kResampleStats + threadIdx.x] = sum;
    }
}

void launch_resample_core(const uint64_t* xt, int n, int nw64, const int* org, const int* off, int count, int32_t* stats,
                          hipStream_t s)
{
    if (count <= 0 || nw64 <= 0) return;
    hipLaunchKernelGGL(k_resample_core, dim3(count, (nw64 + kResampleCoreWave - 1) / kResampleCoreWave), dim3(kResampleCoreWave), 0, s,
                       xt, n, nw64, org, off, stats);
}

void launch_resample_tally(const VoteDesc* desc, int count, const uint8_t* maps, int32_t* stats, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_resample_tally, dim3(count), dim3(kTallyThreads), 0, s, desc, maps, stats);
}

}  // namespace nemk
