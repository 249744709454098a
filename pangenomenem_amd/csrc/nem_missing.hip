// nem_missing.hip -- NCEM on a matrix with missing cells: the three kernels an engine with an observed mask runs
// instead of k_density, k_mstep_counts and k_finish's parameter update (nem_kernels.hip).
//
// The reference's NEM treats a `nan` cell as not observed, and for the Bernoulli family that is a complete rule:
// DensBernoulli skips the cell (nem_mod.c:654), EstimSizes counts the observations per (class, variable) (:1310),
// ComputeMedian and EstimLaplaceIner walk the observed cells only (:1455, :1682), and InerToDisp* divide by the
// observed counts -- MISSING_IGNORE is forced for Bernoulli (:446-448).
//
// The mask has the matrix's layouts (launch_layout made them): ow[W][npad] beside xw, ot[d][nw64] beside xt, a set bit
// = observed, padding bits 0.  Every matrix word is read through the mask, so the matrix bit of an unobserved cell is
// don't-care.  E1 takes the two logs per (k, d) itself, as k_finish's table_entry takes them: k_finish writes tabT / tabL0
// for the classes on its general chain only (a class of one dispersion keeps two constants and bit masks instead), so
// the tables do not hold every class; it reads the unsorted matrix copy, so its result needs no hand-back in lane order.
// None of this is the hot path of a complete matrix: one lane per (family, class) without fast-forward,
// one block for the whole parameter update.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

#include "nem_kernels.hpp"

namespace nemk {

namespace {

constexpr int MD_CH = 512;          // organisms per chunk of the per-(k,d) step constants (LDS: 12 KB per block)

struct DensityMaskedArgs {
    const uint32_t* xw; const uint32_t* ow; int n, npad, dpad, D, K;
    const float* center; const float* disp; const uint32_t* nz0; const uint32_t* nz1;
    const double* pk; const float* logpk; double* pkfki; float* logpkfki; int* zero_flags; int n_zero_flags;
};

// E1.  grid = (npad / 256, K); lane tid of block (tile, k) walks family tile*256 + tid in class k.  The step constants
// are DensBernoulli's two logs per (k, d), taken as k_finish's table_entry takes them; nz0 / nz1 (null dispersion and a
// mismatch) are k_finish's.  A family without an observed cell keeps dk = 0: LogFk = 0, fk = 1 (nem_mod.c:676-681).
__global__ __launch_bounds__(256) void k_density_masked(DensityMaskedArgs a)
{
    __shared__ double2 sT[MD_CH];
    __shared__ double sL[MD_CH];
    const int tid = threadIdx.x, tile = blockIdx.x, k = blockIdx.y;
    const int i = tile * 256 + tid;                      // i < npad by construction
    const int npad = a.npad, dpad = a.dpad, D = a.D;
    const int W = dpad >> 5;
    // the sweep that follows this launch starts from clean flags (MOVED + the relaxation-round window), as behind k_density
    if (tile == 0 && k == 0)
        for (int t = tid; t < a.n_zero_flags; t += 256) a.zero_flags[t] = 0;
    float dk = 0.0f;
    uint32_t nul = 0;
    for (int d0 = 0; d0 < dpad; d0 += MD_CH) {
        const int dn = min(MD_CH, dpad - d0);
        __syncthreads();
        for (int t = tid; t < dn; t += 256) {
            const int dd = d0 + t;
            double t0 = 0.0, t1 = 0.0, l0 = 0.0;
            if (dd < D) {
                const float eps = a.disp[k * D + dd];
                const float mu = a.center[k * D + dd];
                const int ad0 = abs((int)(0.0f - mu)), ad1 = abs((int)(1.0f - mu));
                if ((double)eps > kEpsilonD) {
                    const double l1 = log((double)((1.0f - eps) / eps));
                    l0 = log((double)(1.0f - eps));
                    t0 = (double)ad0 * l1;
                    t1 = (double)ad1 * l1;
                }
            }
            sT[t] = make_double2(t0, t1);
            sL[t] = l0;
        }
        __syncthreads();
        const int w0 = d0 >> 5, wn = dn >> 5;            // (dpad is a multiple of 64: whole words)
        uint32_t xn = a.xw[(size_t)w0 * npad + i], on = a.ow[(size_t)w0 * npad + i];
        for (int w = 0; w < wn; w++) {
            const uint32_t x = xn, o = on;
            if (w + 1 < wn) { xn = a.xw[(size_t)(w0 + w + 1) * npad + i]; on = a.ow[(size_t)(w0 + w + 1) * npad + i]; }
            nul |= o & ((x & a.nz1[k * W + w0 + w]) | (~x & a.nz0[k * W + w0 + w]));
            if (o == 0u) continue;
            for (int b = 0; b < 32; b++) {
                if (!((o >> b) & 1u)) continue;          // not observed: no step (padding organisms are never observed)
                const double2 tt = sT[w * 32 + b];
                const double l0 = sL[w * 32 + b];
                const double add = ((x >> b) & 1u) ? tt.y : tt.x;
                dk = (float)(((double)dk + add) - l0);   // nem_mod.c:661
            }
        }
    }
    float logfk; double fk;
    if (!nul) { logfk = -dk; fk = exp((double)logfk); }  // nem_mod.c:679-680
    else { logfk = -FLT_MAX; fk = 0.0; }                 // nem_mod.c:685-686
    if (i < a.n) {
        a.pkfki[(size_t)k * npad + i] = a.pk[k] * fk;            // nem_alg.c:2282
        a.logpkfki[(size_t)k * npad + i] = a.logpk[k] + logfk;   // nem_alg.c:2283
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;                                            // (lane 0 holds the sum)
}

// NCEM statistics.  grid = D + 1 blocks: block d < D counts organism d's observed ones and observed cells per class
// from the organism-major rows, block D the class sizes (every member counts there, observed or not: EstimSizes' N_K).
__global__ __launch_bounds__(256) void k_mstep_counts_masked(CountsMaskedArgs a)
{
    __shared__ int s_ones[kMaxKernelK], s_obs[kMaxKernelK];
    const int tid = threadIdx.x, d = blockIdx.x;
    const int K = a.K, D = a.D, nw64 = a.nw64;
    if (tid < kMaxKernelK) { s_ones[tid] = 0; s_obs[tid] = 0; }
    __syncthreads();
    const bool sizes = d >= D;
    const uint64_t* xr = a.xt + (size_t)(sizes ? 0 : d) * nw64;
    const uint64_t* orow = a.ot + (size_t)(sizes ? 0 : d) * nw64;
    for (int k = 0; k < K; k++) {
        int ones = 0, obs = 0;
        for (int j = tid; j < nw64; j += 256) {
            const uint64_t m = a.mask[(size_t)k * nw64 + j];
            if (sizes) ones += __popcll(m);
            else {
                const uint64_t o = orow[j] & m;
                ones += __popcll(xr[j] & o);
                obs += __popcll(o);
            }
        }
        ones = wave_sum(ones); obs = wave_sum(obs);
        if ((tid & 63) == 0) { atomicAdd(&s_ones[k], ones); atomicAdd(&s_obs[k], obs); }
    }
    __syncthreads();
    if (tid < K) {
        if (sizes) a.stats[tid] = s_ones[tid];
        else { a.stats[K + tid * D + d] = s_ones[tid]; a.obs[tid * D + d] = s_obs[tid]; }
    }
}

// The parameter update from the counts, one block of 1024 threads.
//   N_K = class size, NbObs_KD = obs (EstimSizes).  With zeros = obs - ones, ComputeMedian (nem_mod.c:1439-1477) with
//   totwei = obs walks the observed zeros, then the observed ones: the centre is 0, 0.5 or 1 for 2 zeros >, =, < obs;
//   EstimLaplaceIner (:1669-1686) then gives ones, obs / 2 or zeros (all exact).  A (class, organism) without an
//   observed member keeps its centre (:1399-1401) and has inertia 0; so does every organism of an empty class.
//   InerToDisp* in their MISSING_IGNORE branches (:988-1170): the float sums of NbObs_KD and Iner_KD in the
//   reference's order, on one lane each (they pass 2^24 at real sizes and then round).
//   An engine holds at most 2^24 families (nemgpu_create): every count is exact as a float and 2 * zeros fits an int.
__global__ __launch_bounds__(1024) void k_finish_masked(FinishMaskedArgs a)
{
    __shared__ float s_disp[kMaxKernelK];
    __shared__ int s_valid[kMaxKernelK];
    __shared__ float s_vol;
    const int tid = threadIdx.x;
    const int K = a.K, D = a.D;
    for (int t = tid; t < K * D; t += 1024) {
        const int k = t / D;
        const int nk = a.stats[k], obs = a.obs[t], ones = a.stats[K + t];
        const float nkf = (float)nk;
        if (t - k * D == 0) a.nbobs_k[k] = nkf;
        float in = 0.0f;
        if ((double)nkf > kEpsilonD && obs > 0) {
            const int zeros = obs - ones;
            float mu;
            if (2 * zeros > obs) { mu = 0.0f; in = (float)ones; }
            else if (2 * zeros == obs) { mu = 0.5f; in = 0.5f * (float)obs; }
            else { mu = 1.0f; in = (float)zeros; }
            a.center[t] = mu;
        }
        a.iner[t] = in;
        a.nbobs_kd[t] = (float)obs;
    }
    __syncthreads();
    if (a.disper == NEMGPU_DISP_K_) {                    // InerToDispK_, :1043-1073
        if (tid < K) {
            const int k = tid;
            s_valid[k] = a.nbobs_k[k] > 0;
            if (s_valid[k]) {
                float sn = 0.0f, si = 0.0f;
                for (int d = 0; d < D; d++) { sn += a.nbobs_kd[k * D + d]; si += a.iner[k * D + d]; }
                s_disp[k] = si / sn;
            }
        }
        __syncthreads();
        for (int t = tid; t < K * D; t += 1024) {
            const int k = t / D;
            if (s_valid[k]) a.disp[t] = s_disp[k];
        }
    } else if (a.disper == NEMGPU_DISP___) {             // InerToDisp__, :988-1015
        if (tid == 0) {
            float vol = 0.0f, nobs = 0.0f;
            for (int k = 0; k < K; k++) {
                if (!(a.nbobs_k[k] > 0)) continue;
                for (int d = 0; d < D; d++) { vol += a.iner[k * D + d]; nobs += a.nbobs_kd[k * D + d]; }
            }
            s_vol = vol / nobs;
        }
        __syncthreads();
        for (int t = tid; t < K * D; t += 1024) a.disp[t] = s_vol;
    } else if (a.disper == NEMGPU_DISP__D) {             // InerToDisp_D, :1104-1126
        for (int d = tid; d < D; d += 1024) {
            float sn = 0.0f, si = 0.0f;
            for (int k = 0; k < K; k++) { sn += a.nbobs_kd[k * D + d]; si += a.iner[k * D + d]; }
            const float dd = si / sn;
            for (int k = 0; k < K; k++) a.disp[k * D + d] = dd;
        }
    } else {                                             // InerToDispKD, :1152-1170
        for (int t = tid; t < K * D; t += 1024)
            if ((double)a.nbobs_kd[t] > kEpsilonD) a.disp[t] = a.iner[t] / a.nbobs_kd[t];
    }
    if (tid < K) {                                       // EstimPara, :456-465
        if (a.propor == NEMGPU_PROP_K) a.prop[tid] = a.nbobs_k[tid] / (float)a.n_total;
        else a.prop[tid] = (float)(1.0 / K);
    }
    if (tid == 0) {                                      // EstimLaplaceCenters :1404-1408
        int ek = 0;
        for (int k = 0; k < K; k++) if (!((double)a.nbobs_k[k] > kEpsilonD)) ek = k + 1;
        a.flags[FLAG_EMPTYK] = ek;
    }
}

}  // namespace

void launch_density_masked(const FinishArgs& t, const DensityIO& io, const uint32_t* xw, const uint32_t* ow, hipStream_t s)
{
    DensityMaskedArgs a;
    a.xw = xw; a.ow = ow; a.n = io.n; a.npad = io.npad; a.dpad = t.dpad; a.D = t.D; a.K = t.K;
    a.center = t.center; a.disp = t.disp; a.nz0 = t.nz0; a.nz1 = t.nz1; a.pk = t.pk; a.logpk = t.logpk;
    a.pkfki = io.pkfki; a.logpkfki = io.logpkfki; a.zero_flags = io.zero_flags; a.n_zero_flags = io.n_zero_flags;
    hipLaunchKernelGGL(k_density_masked, dim3((unsigned)(io.npad / 256), (unsigned)t.K), dim3(256), 0, s, a);
}

void launch_mstep_counts_masked(const CountsMaskedArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_mstep_counts_masked, dim3((unsigned)(a.D + 1)), dim3(256), 0, s, a);
}

void launch_finish_masked(const FinishMaskedArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_finish_masked, dim3(1), dim3(1024), 0, s, a);
}

}  // namespace nemk
