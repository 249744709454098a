// nem_sweep.hip -- every instance of the E2 relaxation round (k_sweep, its batched twin) and their launch wrapper.
// The round itself is sweep_body in nem_sweep_dev.hpp (ComputePartitionNEM / ComputeLocalProba / ComputeMAP,
// nem_alg.c:2330-2405, 2546-2616, 590-645).  A translation unit of its own: the instances are a third of the library's
// compile time, and build.py compiles the units side by side.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "nem_kernels.hpp"
#include "nem_sweep_dev.hpp"

namespace nemk {

template <int KT, bool NCEM, int BS, bool LIBC = false, bool COUNT = false>
__global__ __launch_bounds__(BS) void k_sweep(SweepArgs a) { sweep_body<KT, NCEM, BS, LIBC, COUNT>(a, blockIdx.x, gridDim.x); }
// round 0 of a start's beta sweep with the blind sweep inside it (sweep_body's BLIND; a name of its own in a trace)
template <int KT, bool COUNT>
__global__ __launch_bounds__(256) void k_sweep_blind(SweepArgs a) { sweep_body<KT, true, 256, false, COUNT, true>(a, blockIdx.x, gridDim.x); }
template <int KT, bool NCEM, int BS, bool LIBC = false>
__global__ __launch_bounds__(BS) void k_sweep_b(const void* arr, int stride, const int* gx) { NEM_B_HEAD(SweepArgs) sweep_body<KT, NCEM, BS, LIBC>(a, blockIdx.x, nblk); }

static int sweep_variant(int K, bool ncem, bool big, bool libc) { return (K >= 1 && K <= 10 ? K : 0) | (ncem ? 16 : 0) | (big ? 32 : 0) | (libc && ncem ? 64 : 0); }

template <bool BATCHED>
static void sweep_dispatch(int variant, dim3 grid, unsigned bdim, hipStream_t s, const SweepArgs* a, const void* arr, int stride, const int* gx)
{
    const int kt = variant & 15; const bool ncem = (variant & 16) != 0, big = (variant & 32) != 0, libc = (variant & 64) != 0;
    dim3 block(bdim);                                    // (256; the large-shard instances: SweepArgs::spb rounded up to whole waves, at most 1024)
    // the instance <KT, NCEM, BS, LIBC>, each a std::integral_constant
    auto launch = [&](auto KT, auto NC, auto BS, auto LC) {
        if (BATCHED) hipLaunchKernelGGL((k_sweep_b<decltype(KT)::value, decltype(NC)::value, decltype(BS)::value, decltype(LC)::value>), grid, block, 0, s, arr, stride, gx);
        else hipLaunchKernelGGL((k_sweep<decltype(KT)::value, decltype(NC)::value, decltype(BS)::value, decltype(LC)::value>), grid, block, 0, s, *a);
    };
    // fuzzy NEM, NCEM, NCEM with the reference's tie stream
    auto modes = [&](auto KT, auto BS) {
        if (!ncem) launch(KT, std::false_type{}, BS, std::false_type{});
        else if (libc) launch(KT, std::true_type{}, BS, std::true_type{});
        else launch(KT, std::true_type{}, BS, std::false_type{});
    };
    const std::integral_constant<int, 256> bs256; const std::integral_constant<int, 1024> bs1024;
    // (the generic K: a 256-site instance only, see sweep_block_sites)
    if (!dispatch_k<1, 10>(kt, [&](auto KT) { if (big) modes(KT, bs1024); else modes(KT, bs256); })) modes(std::integral_constant<int, 0>{}, bs256);
}

// the launch geometry of a round: block size (= sites per block) for n_local sites
static int sweep_block_sites(int n_local, int K, bool* big_out)
{
    const bool generic = !(K >= 1 && K <= 10);
    const bool big = n_local >= 65536 && !generic;
    int bs = 256;
    if (big) {
        const int waves_of_blocks = (n_local + 256 * 1024 - 1) / (256 * 1024);
        const int per_block = (n_local + 256 * waves_of_blocks - 1) / (256 * waves_of_blocks);
        bs = std::min(1024, std::max(256, (per_block + 63) / 64 * 64));
    }
    if (big_out) *big_out = big;
    return bs;
}

void launch_sweep(const SweepArgs& a0, bool ncem, hipStream_t s)
{
    // Large shards run up to 1024 sites per block (the per-block flag atomics -- one address -- were what a round cost
    // when every site reports something, e.g. all densities underflow at D = 5000; the tally now rides on the
    // last-block ticket, but a round is still bound by each block's instruction stream): as many sites per block as
    // fill the chip's 256 CUs evenly -- 200 000 sites: 241 blocks of 832 instead of 196 of 1024 on 256 CUs.
    bool big = false;
    SweepArgs a = a0;
    const int bs = sweep_block_sites(a.n_local, a.K, &big);
    a.spb = big ? bs : 0;
    dim3 grid((a.n_local + bs - 1) / bs);
    const int variant = sweep_variant(a.K, ncem, big, a.tie_rule == NEMGPU_TIE_LIBC);
    if (a.blind_off != 0) {
        // a start's first beta round with the blind sweep inside it (SweepArgs::blind_off): instances of its own, plain
        // and counting (not recordable: the batched twins have none); the engine asks for it where there is one only
        const bool count = a.post_stats != nullptr;
        if (!(current_recorder() == nullptr && ncem && !big && a.K >= 2 && a.K <= 7 && a.tie_rule != NEMGPU_TIE_LIBC && a.use_nei &&
              a.lo == 0 && a.slot_stride == 0 && a.flags_in == nullptr && a.prev_changed == nullptr &&
              a.lab_guess != nullptr && a.lab_guess == a.lab_old && a.lab_out != a.lab_guess &&
              (!count || (a.post_on && !a.post_no_masks && a.post_D >= 1 && a.post_D <= kFusedMaxD)))) {
            fprintf(stderr, "launch_sweep: no blind round for this shape\n");
            abort();
        }
        dispatch_k<2, 7>(a.K, [&](auto KT) {
            if (count) hipLaunchKernelGGL((k_sweep_blind<decltype(KT)::value, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_sweep_blind<decltype(KT)::value, false>), grid, dim3(256), 0, s, a);
        });
        return;
    }
    if (a.post_stats != nullptr) {
        // the counting round (SweepArgs::post_stats): an instance of its own, so that no other round carries its registers
        // (not recordable: the batched twins have no such instance)
        if (!(current_recorder() == nullptr && ncem && !big && a.K >= 1 && a.K <= 10 && a.tie_rule != NEMGPU_TIE_LIBC &&
              a.post_on && !a.post_no_masks && a.post_D >= 1 && a.post_D <= kFusedMaxD)) {
            fprintf(stderr, "launch_sweep: no counting round for this shape\n");
            abort();
        }
        dispatch_k<1, 10>(a.K, [&](auto KT) {
            hipLaunchKernelGGL((k_sweep<decltype(KT)::value, true, 256, false, true>), grid, dim3(256), 0, s, a);
        });
        return;
    }
    if (record_op(OP_SWEEP, variant, grid, (unsigned)bs, a)) return;
    sweep_dispatch<false>(variant, grid, (unsigned)bs, s, &a, nullptr, 0, nullptr);
}


// test hook: n given rows (pkf[n][K] densities, ctx[n][K] class contexts) through the two ways an NCEM round has to a
// label -- out[i] = {the normalised row's first maximum, the later entries equal to it, the unnormalised row's first
// maximum, whether the row is clear (nem_map.hpp)} -- with the device's own exp, divisions and conversions
constexpr int kMapDebugK = 8;
__global__ __launch_bounds__(256) void k_map_margin_debug(SweepArgs a, const float* ctx_rows, int4* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_local) return;
    const int K = a.K;
    double pkf[kMapDebugK], cinum[kMapDebugK];
    float ctx[kMapDebugK], cf[kMapDebugK];
#pragma unroll
    for (int k = 0; k < kMapDebugK; k++) {
        pkf[k] = k < K ? a.pkfki[(size_t)i * K + k] : 0.0;
        ctx[k] = k < K ? ctx_rows[(size_t)i * K + k] : 0.0f;
    }
    const double cum = local_cinum<kMapDebugK>(a, K, pkf, ctx, cinum);
    int k_clear;
    const bool clear = map_clear_row<kMapDebugK>(cinum, K, cum, k_clear);
    map_normalise<kMapDebugK>(cinum, K, cum, cf);
    int nequal = 0;
    const int k_full = map_full<kMapDebugK>(cf, K, nequal);
    out[i] = make_int4(k_full, nequal, k_clear, clear ? 1 : 0);
}
bool launch_map_margin_debug(const double* pkf, const float* ctx, int n, int K, float beta, int use_nei, int* out, hipStream_t s)
{
    if (n <= 0 || K < 1 || K > kMapDebugK) return false;
    SweepArgs a{};
    a.n_local = n; a.K = K; a.pkfki = pkf; a.beta = beta; a.use_nei = use_nei ? 1 : 0;
    hipLaunchKernelGGL(k_map_margin_debug, dim3((n + 255) / 256), dim3(256), 0, s, a, ctx, reinterpret_cast<int4*>(out));
    return true;
}

#ifdef NEM_PHASE_PROF
extern "C" int nemgpu_debug_sweep_phases(unsigned long long* out8)
{
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_sweep_phase), sizeof(unsigned long long) * 8);
}
// (the counting instance's stamps: the same eight phases)
extern "C" int nemgpu_debug_sweep_phases_count(unsigned long long* out8)
{
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_sweep_phase), sizeof(unsigned long long) * 8, sizeof(unsigned long long) * 8);
}
#endif

void sweep_dispatch_batched(int variant, dim3 grid, unsigned bdim, hipStream_t s, const void* arr, int stride, const int* gx)
{
    sweep_dispatch<true>(variant, grid, bdim, s, nullptr, arr, stride, gx);
}

}  // namespace nemk
