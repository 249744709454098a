// nem_sweep_dev.hpp -- device code shared by the translation units that hold sweep kernels (nem_kernels.hip: the
// sweep + counts launch of the sharded path, the loop-control and bookkeeping kernels; nem_sweep.hip: every k_sweep
// instance): the tie-break hash, the device-side loop control, the last-block ticket, one site's row
// (ComputeLocalProba, nem_alg.c:2546-2616) and the relaxation round itself (ComputePartitionNEM's sweep,
// nem_alg.c:2330-2405, with ComputeMAP, nem_alg.c:590-645).  Compiled without relocatable device code: every
// translation unit instantiates what it launches.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_kernels.hpp"
#include "nem_map.hpp"

namespace nemk {

// development probe (-DNEM_PHASE_PROF, see nem_kernels.hip): the first block's first thread stamps the 100 MHz wall clock
// at the round's phase boundaries -- one copy per translation unit; nem_sweep.hip's is the one read back.  Slots 0-7: the
// head (0-4) and the tail (5: behind the tail barrier, 6: flags published, 7: the last count add issued); slots 8-15: the
// same eight of the counting instance, which a cycle's last plain round would otherwise overwrite
#ifdef NEM_PHASE_PROF
static __device__ unsigned long long g_sweep_phase[16];
#define NEM_SWEEP_PHASE(i) do { if (bx == 0 && threadIdx.x == 0) g_sweep_phase[(COUNT ? 8 : 0) + (i)] = wall_clock64(); } while (0)
// (the entry stamp is taken ahead of the stop test and stored by a block that is past it)
#define NEM_SWEEP_PHASE_TAKE(t) const unsigned long long t = wall_clock64()
#define NEM_SWEEP_PHASE_PUT(i, t) do { if (bx == 0 && threadIdx.x == 0) g_sweep_phase[(COUNT ? 8 : 0) + (i)] = t; } while (0)
#else
#define NEM_SWEEP_PHASE(i) do { } while (0)
#define NEM_SWEEP_PHASE_TAKE(t) do { } while (0)
#define NEM_SWEEP_PHASE_PUT(i, t) do { } while (0)
#endif

__host__ __device__ inline uint32_t mix32(uint32_t seed, uint32_t sweep, uint32_t site)
{
    // counter-based stand-in for the reference's time-seeded random() (nem_rnd.c:40-63);
    // identical to orc_mix32() in oracle/nem_oracle.c
    uint32_t h = seed * 0x9E3779B1u + sweep * 0x85EBCA77u + site * 0xC2B2AE3Du + 0x27D4EB2Fu;
    h ^= h >> 16; h *= 0x7FEB352Du;
    h ^= h >> 15; h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------------------------------
// Device-side loop control (one thread, once per EM iteration).  The host enqueues several
// iterations ahead; every loop kernel returns at once when ctrl[C_STOP] is set, so the host only
// has to look at `ctrl` once per batch instead of once per iteration (NemAlgo's loop test,
// nem_alg.c:1789-1840: convergence, empty class; plus "the sweep needs more relaxation rounds").
// Runs in the last block to finish of the iteration's bookkeeping kernel (k_labels_post /
// k_conv_fuzzy), or as its own tiny launch when there is no such kernel.
// ------------------------------------------------------------------------------------------
// (measured, round 3: out of line -- __noinline__, the block passed by value -- the kernels that call it need a private
//  segment, 176 bytes per lane, and every launch of theirs got 3-4 us longer; it stays inline)
__device__ inline void ctrl_logic(const CtrlArgs& a)
{
    int* c = a.ctrl;
    // One thread runs this at the tail of a launch (or as a launch of its own): a string of dependent read-modify-writes
    // of device memory would BE that tail (each ~0.1-0.4 us).  So everything the decision reads is requested up front
    // -- independent loads, one memory latency -- the tests run on registers, and what changed is stored at the end.
    constexpr int kMaxRounds = 8;                                 // (kRoundsMax in nem_engine.hip: the fuzzy loop's learned counts go up to 7)
    const int nr = a.n_rounds > 0 ? (a.n_rounds < kMaxRounds ? a.n_rounds : kMaxRounds) : 2;
    const int stop = c[C_STOP];
    int iters = c[C_ITERS], commits = c[C_COMMITS], sweep_rounds = c[C_SWEEP_ROUNDS], nzero = c[C_NZERO], firstzero = c[C_FIRSTZERO];
    int draws = c[C_DRAWS];
    const int sweep_next = *a.sweep_next;
    const int emptyk = a.iter_flags[FLAG_EMPTYK];
    int moved = __hip_atomic_load(&a.iter_flags[FLAG_MOVED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    static_assert(FLAG_ROUND_STRIDE == 4 && FLAG_CHANGED == 0 && FLAG_NZERO == 1 && FLAG_FIRSTZERO == 2 && FLAG_NTIES == 3, "a round's slot is one int4");
    int4 rf[kMaxRounds];
#pragma unroll
    for (int r = 0; r < kMaxRounds; r++) rf[r] = r < nr ? reinterpret_cast<const int4*>(a.round0)[r] : make_int4(1, 0, 0, 0);
    int4 bf = make_int4(0, 0, 0, 0);
    bool blind_ok = true;
    int blind_needed = 1;
    if (a.is_init && a.blind != nullptr) {
        if (a.blind_rounds > 1) {
            // TIE_LIBC: the blind sweep's sites are coupled through the draw counter, it ran verified rounds like any
            // sweep: its result is the first round that changed nothing (the rounds behind it did not run)
            blind_ok = false;
            for (int q = 0; q < a.blind_rounds && !blind_ok; q++) {
                const int4 f = reinterpret_cast<const int4*>(a.blind)[q];
                if (f.x == 0) { bf = f; blind_ok = true; blind_needed = q + 1; }
            }
        } else bf = *reinterpret_cast<const int4*>(a.blind);
    }
    int draw0 = 0, rank_draws = 0;
    if (a.draw_ctl != nullptr) {
        draw0 = a.draw_ctl[0];
        if (a.q_tot != nullptr)                                   // sharded: every rank's draws of the sweep's final round
            for (int r = 0; r < a.n_ranks; r++) rank_draws += *reinterpret_cast<const int*>(a.q_tot + (size_t)r * a.flag_stride);
    }
    int ch0 = 0, ch1 = 0, mv = 0;
    if (a.q_flags != nullptr) {                                   // sharded: every rank's flag bytes (all-gathered)
        for (int r = 0; r < a.n_ranks; r++) {
            const size_t o = (size_t)r * a.flag_stride;
            ch0 |= a.q_flags[o];
            ch1 |= a.r_flags[o];
            // every rank's 'one of MY labels moved' byte, next to its flag byte of the sweep's last round (1: round 1's,
            // 2: round 0's): every rank takes the same decision without another collective, and without a pass over
            // the other ranks' labels
            if (a.moved_bytes) mv |= (a.moved_bytes == 2 ? a.q_flags : a.r_flags)[o + 1];
        }
        if (a.moved_bytes) moved = mv;
    }
    if (stop) return;

    // which of the enqueued relaxation rounds changed nothing (= the sweep's fixed point)?  -1: none of them
    int last = -1;
    if (!a.use_nei) last = 0;                                     // one round, nothing to verify
    else if (a.q_flags != nullptr) last = !ch0 ? 0 : (!ch1 ? 1 : -1);   // sharded: two rounds
    else {
#pragma unroll
        for (int r = kMaxRounds - 1; r >= 0; r--) if (r < nr && rf[r].x == 0) last = r;
    }
    int4 f = rf[0];
#pragma unroll
    for (int r = 1; r < kMaxRounds; r++) if (last == r) f = rf[r];
    // the tie-break hash is keyed by the sweep number; sweeps 0 and 1 are the two initial ones
    if (a.is_init) *a.sweep_next = 2;
    else { iters += 1; c[C_ITERS] = iters; *a.sweep_next = sweep_next + 1; }
    if (a.is_init) {                                              // ComputePartitionFromPara(Needinit=1): no iteration counted
        if (!blind_ok) { c[C_NEED_ROUNDS] = 3; c[C_STOP] = 1; return; }   // (what ran behind the blind sweep is void: the host starts over)
        if (bf.y > 0) {                                           // the blind sweep's zero-density sites come first
            nzero += bf.y;
            if (firstzero == 0) firstzero = bf.z;
        }
        if (last >= 0) {
            sweep_rounds += last + 2;                             // blind sweep + this one
            if (f.y > 0) { nzero += f.y; if (firstzero == 0) firstzero = f.z; }
            c[C_FOLD] = f.y > 0;                                  // how the next sweeps tally such sites, see k_sweep
            c[C_SWEEP_ROUNDS] = sweep_rounds;
            c[C_INIT_ROUNDS] = (blind_needed << 8) | (last + 1);     // (what the two sweeps needed: the host enqueues accordingly)
            if (a.draw_ctl != nullptr && a.blind_rounds > 1) {    // TIE_LIBC: both sweeps' draws move the stream on
                const int nt = (bf.w & ((1 << 30) - 1)) + (f.w & ((1 << 30) - 1));
                a.draw_ctl[0] = draw0 + nt;
                c[C_DRAWS] = draws + nt;
                c[C_DRAWS_INIT] = nt;
            }
        }
        c[C_NZERO] = nzero; c[C_FIRSTZERO] = firstzero;
        if (last < 0) { c[C_NEED_ROUNDS] = 2; c[C_STOP] = 1; }
        return;
    }
    if (!a.param_fix && emptyk != 0) {                            // nem_alg.c:1831-1838: E-step "not run"
        c[C_STATUS] = NEMGPU_W_EMPTYCLASS;
        c[C_EMPTYK] = emptyk;
        c[C_STOP] = 1;
        return;
    }
    if (last < 0) { c[C_NEED_ROUNDS] = 1; c[C_STOP] = 1; return; }
    c[C_SWEEP_ROUNDS] = sweep_rounds + last + 1;
    if (last >= 2) c[C_DEEP] = iters;
    if (f.y > 0) {
        c[C_NZERO] = nzero + f.y;
        if (firstzero == 0) c[C_FIRSTZERO] = f.z;
    }
    c[C_FOLD] = f.y > 0;
    if (a.draw_ctl != nullptr) {                                  // TIE_LIBC: the sweep's draws move the stream on
        const int nt = a.q_tot != nullptr ? rank_draws : (f.w & ((1 << 30) - 1));
        a.draw_ctl[0] = draw0 + nt;
        c[C_DRAWS] = draws + nt;
    }
    c[C_COMMITS] = commits + 1;
    if (a.cvtest == NEMGPU_CV_CLAS) {                             // HasConverged, nem_alg.c:2075-2089
        const int conv = a.ncem ? (moved ? (1.0f < a.cvthres) : (0.0f < a.cvthres)) : !moved;
        if (conv) { c[C_CONVERGED] = 1; c[C_STOP] = 1; }
    }
}

// last-block-done ticket: returns true in exactly one thread of the grid, after every block's global
// writes (made before its call) are visible to it
// `bx`: the block's index among the `nblocks` that take part (default blockIdx.x; a launch whose ticket covers a
// trailing range of its blocks passes the index within that range).
// Two levels (groups of blocks, then the groups) once the grid is larger than 32 blocks: same-address atomics
// are served one after the other (~45 ns each on MI355X), so a flat counter costs 9 us at 200 blocks; with at most
// 32 groups on counters 128 bytes apart it is ~sqrt of that.  `ticket` points at kTicketWords zeroed ints.
// The counters are 64-bit: arrivals in the low word, and in the high word an optional grid-wide sum (`tally`, this
// block's share; the last block stores the total to *tally_out) that rides on the same atomics -- a sum that would
// otherwise cost one same-address atomic per block.
__device__ inline bool last_block_ticket(int* ticket, int nblocks, int tally = 0, int* tally_out = nullptr, int bx = -1)
{
    const int b = bx >= 0 ? bx : (int)blockIdx.x;
    __shared__ int s_last;
    // What the last block reads of the others are FLAGS, all of them updated by device-scope atomics: every wave waits
    // until its own are performed (vmcnt(0)), the block meets, one thread adds the arrival.  (A device-scope release
    // fence here -- `buffer_wbl2`, the whole L2 written back -- cost microseconds per launch once every block did one;
    // the last block's acquire fence below stays: it reads the flags with plain loads.)
    __builtin_amdgcn_s_waitcnt(0x0F70);                            // vmcnt(0)
    __syncthreads();
    if (threadIdx.x == 0 && tally_out == nullptr) {                // plain ticket: 32-bit counters
        int last = 0;
        if (nblocks <= 32) {
            const int t = atomicAdd(ticket, 1);
            last = (t == nblocks - 1);
            if (last) *ticket = 0;
        } else {
            const int gsz = (nblocks + 31) / 32;
            const int g = b / gsz;
            const int ng = (nblocks + gsz - 1) / gsz;
            const int members = min(gsz, nblocks - g * gsz);
            int* gc = ticket + 32 * (1 + g);
            if (atomicAdd(gc, 1) == members - 1) {                 // (the top arrival is issued once this one has returned)
                *gc = 0;
                if (atomicAdd(ticket, 1) == ng - 1) { *ticket = 0; last = 1; }
            }
        }
        if (last) __threadfence();
        s_last = last;
    } else if (threadIdx.x == 0) {
        using u64 = unsigned long long;
        const u64 mine = 1ull | ((u64)(unsigned)tally << 32);
        int last = 0;
        u64 total = 0;
        if (nblocks <= 32) {
            u64* tc = reinterpret_cast<u64*>(ticket);
            const u64 t = atomicAdd(tc, mine);
            last = ((int)(t & 0xffffffffull) == nblocks - 1);
            if (last) { *tc = 0; total = (t >> 32) + (u64)(unsigned)tally; }
        } else {
            const int gsz = (nblocks + 31) / 32;                   // blocks per group; at most 32 groups
            const int g = b / gsz;
            const int ng = (nblocks + gsz - 1) / gsz;
            const int members = min(gsz, nblocks - g * gsz);
            u64* gc = reinterpret_cast<u64*>(ticket + 32 * (1 + g));
            const u64 t = atomicAdd(gc, mine);
            if ((int)(t & 0xffffffffull) == members - 1) {
                *gc = 0;
                const u64 gsum = (t >> 32) + (u64)(unsigned)tally;
                u64* tc = reinterpret_cast<u64*>(ticket);
                const u64 tt = atomicAdd(tc, 1ull | (gsum << 32));
                if ((int)(tt & 0xffffffffull) == ng - 1) { *tc = 0; last = 1; total = (tt >> 32) + gsum; }
            }
        }
        if (last) {
            if (tally_out != nullptr) *tally_out = (int)total;
            __threadfence();
        }
        s_last = last;
    }
    __syncthreads();
    return s_last && threadIdx.x == 0;
}

// ------------------------------------------------------------------------------------------
// E2: one relaxation round of the Gauss-Seidel site sweep.
//
// The reference updates sites in index order, in place (UPDATE_SEQ): site i sees the NEW rows
// of neighbours j < i and the OLD rows of neighbours j >= i.  That is a lower-triangular
// system  c = F(c_{<i}, old_{>=i})  with a unique solution.  Each round evaluates every site
// in parallel against a guess of the new rows; when a round changes nothing the guess IS that
// solution, bit for bit.  Round r reads guess_r and writes out_r; rounds after the first
// unchanged one exit immediately (prev_changed == 0).
// ------------------------------------------------------------------------------------------
// One site's row: ComputeLocalProba (nem_alg.c:2576-2613) from the class contexts.  local_cinum: the unnormalised row
// and its sum; local_proba: cf = the normalised row, returns true when the site hit the "density = 0" branch.
template <int KA>
__device__ __forceinline__ double local_cinum(const SweepArgs& a, int K, const double* pkf, const float* ctx, double* cinum,
                                              const double* exp_tab = nullptr, int exp_tab_len = 0)
{
    double cum = 0.0;
    // (exp_tab[m] = exp((double)beta * (double)(float)m) from the same device exp: a context that is such an integer
    //  takes its factor from the table, every other one runs exp -- decided for the whole row, so that a row costs
    //  either K table reads or K calls)
    bool tab = exp_tab != nullptr;
    int mi[KA];
    if (tab) {
#pragma unroll
        for (int k = 0; k < KA; k++) {
            if (k < K) {
                const float c = ctx[k];
                mi[k] = (int)c;
                tab = tab && c >= 0.0f && c < (float)exp_tab_len && (float)mi[k] == c;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KA; k++) {
        if (k < K) {                                     // nem_alg.c:2581-2584
            double v = pkf[k];
            if (a.use_nei) v = v * (tab ? exp_tab[mi[k]] : exp((double)a.beta * (double)ctx[k]));
            cinum[k] = v;
            cum = cum + v;
        }
    }
    return cum;
}
template <int KA>
__device__ __forceinline__ bool local_proba(const SweepArgs& a, int K, const double* pkf, const float* ctx, float* cf,
                                            const double* exp_tab = nullptr, int exp_tab_len = 0)
{
    // (local_cinum's loops in its own text, as it was before there was a local_cinum: the fuzzy instances and the NCEM
    //  ones that do not take the label shortcut then compile to what they were, register for register)
    double cinum[KA];
    double cum = 0.0;
    bool tab = exp_tab != nullptr;
    int mi[KA];
    if (tab) {
#pragma unroll
        for (int k = 0; k < KA; k++) {
            if (k < K) {
                const float c = ctx[k];
                mi[k] = (int)c;
                tab = tab && c >= 0.0f && c < (float)exp_tab_len && (float)mi[k] == c;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KA; k++) {
        if (k < K) {                                     // nem_alg.c:2581-2584
            double v = pkf[k];
            if (a.use_nei) v = v * (tab ? exp_tab[mi[k]] : exp((double)a.beta * (double)ctx[k]));
            cinum[k] = v;
            cum = cum + v;
        }
    }
    if (cum > 0) {                                       // nem_alg.c:2589-2601
        if (cum > kEpsilonD) {
            const double invz = 1 / cum;
#pragma unroll
            for (int k = 0; k < KA; k++) if (k < K) cf[k] = (float)(invz * cinum[k]);
        } else {
            const double invz = 1 / (cum / kEpsilonD);
#pragma unroll
            for (int k = 0; k < KA; k++) if (k < K) cf[k] = (float)(invz * (cinum[k] / kEpsilonD));
        }
        return false;
    }
    const float u = (float)(1.0 / K);                    // nem_alg.c:2603-2607
#pragma unroll
    for (int k = 0; k < KA; k++) if (k < K) cf[k] = u;
    return true;                                         // counted by the caller, once per block
}

// Labels are bytes: class in the low 7 bits; bit 7 = "this site's C-step drew a random number" (TIE_LIBC only), so
// that a guess of the new partition carries the guess of who draws with it.
constexpr int kLabMask = 0x7F, kLabDrew = 0x80;
constexpr int kTabShort = 1 << 30;                       // in a round's FLAG_NTIES word: the draw table was too short
constexpr int kInnerCap = 64;                            // block-local iterations per round (any cap is exact)

// sum over the 64 lanes, in every lane (data-parallel-primitive adds, no LDS)
__device__ __forceinline__ int wave_sum_i32(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);   // row_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

// A site's label in the blind sweep (beta = 0, no neighbour term) from its K densities alone -- what a round with
// use_nei = 0 computes: local_cinum's row v = pkf[k], the clear row's maximum (nem_map.hpp) or else the normalised row
// and ComputeMAP, the tie pick keyed by (seed, the BLIND sweep's number, the true family index `site`) under `hash`
// and the first maximum under `first`.  One function for a block's own sites and for every neighbour it gathers from
// another block: equal densities give equal labels in every block.  *zero: the site hit the "density = 0" branch.
template <int KA>
__device__ __forceinline__ int blind_label(const SweepArgs& a, int K, const double* pkf, uint32_t site, bool* zero)
{
    double cinum[KA];
    double cum = 0.0;
#pragma unroll
    for (int k = 0; k < KA; k++) {
        if (k < K) {
            const double v = pkf[k];
            cinum[k] = v;
            cum = cum + v;
        }
    }
    *zero = !(cum > 0);
    int kmax = 0;
    if (!a.map_full && map_clear_row<KA>(cinum, K, cum, kmax)) return kmax;
    float cf[KA];
    map_normalise<KA>(cinum, K, cum, cf);
    kmax = 0; float ukmax = cf[0];                       // ComputeMAP, nem_alg.c:603-640
#pragma unroll
    for (int k = 1; k < KA; k++) if (k < K && cf[k] > ukmax) { ukmax = cf[k]; kmax = k; }
    if (a.tie_rule != NEMGPU_TIE_FIRST) {
        int nequal = 0;
#pragma unroll
        for (int k = 1; k < KA; k++) if (k < K && k > kmax && cf[k] == ukmax) nequal++;
        if (nequal > 0) {
            const int pick = (int)(mix32(a.tie_seed, a.blind_sweep_id, site) % (uint32_t)(nequal + 1));
            int seen_eq = 0, chosen = kmax;
#pragma unroll
            for (int k = 1; k < KA; k++)
                if (k < K && k > kmax && cf[k] == ukmax) { seen_eq++; if (seen_eq == pick) chosen = k; }
            kmax = chosen;
        }
    }
    return kmax;
}

// LIBC: the reference's tie stream (TIE_LIBC) -- its bookkeeping (who drew, per wave and block, at every block-local
// step) is compiled into the instances that need it only
// COUNT: the round also adds its block's M-step counts into SweepArgs::post_stats (the round that makes the class masks
// of a held sweep, see the shadow-verify schedule in nem_engine.hip); NCEM, 256 sites per block, D <= kFusedMaxD only
// BLIND: round 0 of a start's beta sweep with the blind sweep inside it (SweepArgs::blind_off): its guess and its old
// partition are both the blind labels, and it reads neither from memory -- a site's own label, and that of a neighbour
// in another block, come from blind_label() on the densities; the block's own labels go to lab_guess and into two LDS
// arrays (the running labels and the old ones).  No block reads what another block of the launch wrote.  With and
// without COUNT; NCEM, 256 sites per block, K = 2 .. 7 (the label shortcut's instances), unsharded (lo = 0)
template <int KT, bool NCEM, int BS, bool LIBC = false, bool COUNT = false, bool BLIND = false>
__device__ __forceinline__ void sweep_body(const SweepArgs& a, const int bx, const int nblk)
{
    static_assert(!COUNT || (NCEM && BS == 256 && !LIBC && KT > 0), "the counting round: NCEM, 256 sites per block");
    static_assert(!BLIND || (NCEM && BS == 256 && !LIBC && KT >= 2 && KT <= 7), "the blind round: NCEM, 256 sites per block, K = 2 .. 7");
    static_assert(C_STOP == 0 && C_FOLD == 1, "one 8-byte load");
    NEM_SWEEP_PHASE_TAKE(t_entry);
    const int spb = (BS > 256 && a.spb > 0) ? a.spb : BS;   // sites of this block (large shards: fewer than the launch bound)
    const int i = bx * spb + threadIdx.x;
    const bool active = (int)threadIdx.x < spb && i < a.n_local;
    const int gi = a.lo + (active ? i : 0);
    const int K = KT > 0 ? KT : a.K;
    constexpr int KA = KT > 0 ? KT : kMaxKernelK;
    // this site's own labels, requested with everything else at the head of the block: asked for where they are
    // used -- behind the label store, which they might alias -- they would be one more memory latency at the tail
    int my_guess = 0, my_old = 0, my_new = 255;           // my_guess: the whole byte; my_old: the class
    // (TIE_LIBC: the block's draw count in the guess, compared at the round's end -- asked for here, not there: a load at
    //  the tail is a memory latency added to the block's run time)
    int blk_cnt_guess = 0;
    // COUNT: the block's four words of organism rows d = threadIdx.x + 256 q, requested here for the same reason: they
    // do not depend on the labels, and the tail only ANDs them with the class masks
    constexpr int kCntRows = COUNT ? kFusedMaxD / BS : 1;
    uint64_t xs[kCntRows][4];
    double pkf[NCEM ? KA : 1];                           // NCEM: the site's densities
    int nb = 0, ne = 0;                                  // NCEM: the site's row of the graph
    int fold_hint = 0;
    bool skip;
    if constexpr (NCEM) {
        // A launch starts with cold caches, so everything whose address the block knows from its index alone is asked
        // for HERE, together, ahead of the stop word's and the previous round's tests and of the head barrier: the
        // labels, the counting round's rows, the densities and the row's bounds used to wait for the two tests one
        // after the other, and the last two for the barrier as well.  Each load keeps the condition that makes its
        // address valid; a block that then leaves at the stop word or skips its sites has read a few words for nothing.
        if (LIBC && threadIdx.x == 0 && a.tie_cnt_guess != nullptr) blk_cnt_guess = a.tie_cnt_guess[bx];
        if (COUNT) {
            const int w0 = 4 * bx;
#pragma unroll
            for (int q = 0; q < kCntRows; q++) {
                const int d = (int)threadIdx.x + q * BS;
#pragma unroll
                for (int w = 0; w < 4; w++)
                    xs[q][w] = (d < a.post_D && w0 + w < a.post_nw64) ? a.post_xt[(size_t)d * a.post_nw64 + w0 + w] : 0ull;
            }
        }
#pragma unroll
        for (int k = 0; k < KA; k++) if (k < K) pkf[k] = active ? a.pkfki[(size_t)k * a.npad + i] : 0.0;
        if (active && a.use_nei) { nb = a.nei_ptr[i]; ne = a.nei_ptr[i + 1]; }
        // the two control words, without a branch around either load (where two paths meet the loaded value would be
        // copied, and waited for): a null pointer reads a word of the densities instead, and the value is dropped
        const int* some = reinterpret_cast<const int*>(a.pkfki);
        int2 sf = *reinterpret_cast<const int2*>(a.stop != nullptr ? a.stop : some);
        int pc = *(a.prev_changed != nullptr ? a.prev_changed : some);
        // (the two bytes last: the compiler masks my_old where it is loaded, and waits for it there -- behind the other
        //  requests that wait is for all of them at once)
        if constexpr (!BLIND) { if (active) { my_guess = a.lab_guess[gi]; my_old = a.lab_old[gi] & kLabMask; } }
        if (a.stop == nullptr) sf = make_int2(0, 0);
        if (a.prev_changed == nullptr) pc = 1;
        // (a compiler-only fence, no instruction: without it the loads above are sunk below the tests, to their uses)
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        // (... and the previous round's word, which the leaving path does not use, would be asked for behind the stop
        //  test: the wave waits for all of its scalar loads at once, so needing it here adds no wait of its own)
        asm volatile("" :: "s"(pc));
        if (sf.x) return;
        fold_hint = sf.y;
        skip = (pc == 0);                                // the previous round was already the fixed point
    } else {
        if (a.stop != nullptr) {
            const int2 sf = *reinterpret_cast<const int2*>(a.stop);
            if (sf.x) return;
            fold_hint = sf.y;
        }
        skip = (a.prev_changed != nullptr && *a.prev_changed == 0);   // the previous round was already the fixed point
    }
    NEM_SWEEP_PHASE_PUT(0, t_entry);
    NEM_SWEEP_PHASE(1);
    if (a.flags_in != nullptr) {                         // sharded: did ANY rank change a label last round?
        int any = 0;
        for (int r = 0; r < a.n_ranks; r++) any |= a.flags_in[(size_t)r * a.slot_stride];
        if (!any) skip = true;
    }
    if (skip && !(NCEM && a.post_on)) {
        if (a.publish_byte != nullptr && bx == 0 && threadIdx.x == 0) *a.publish_byte = 0;
        // TIE_LIBC: the sweep's draw count rides on through the rounds that have nothing left to do, so that whoever was
        // enqueued behind the LAST of them finds it there (SweepArgs::draw_extra of the sweep that follows)
        if (LIBC && a.prev_changed != nullptr && bx == 0 && threadIdx.x == 0) a.flags[FLAG_NTIES] = a.prev_changed[FLAG_NTIES - FLAG_CHANGED];
        return;
    }
    __shared__ int s_nzero, s_first;
    // "a label changed" / "a label moved": per block, then ONE device-scope atomic -- behind a device-scope look at the
    // flag -- instead of one per wave behind a plain load (which another XCD's L2 answers with a stale 0 long after the
    // flag was set: at 200 000 x 5 000, where every wave has something to report, a round's 3 136 same-address atomics
    // were 10-40 us of its 24-52).  A launch of at most kNoLookBlocks blocks skips the look, see the round's tail.
    __shared__ int s_chg, s_mov;
    // NCEM: the MRF factor exp(beta * context) takes few distinct arguments -- the context of a class is a sum of edge
    // weights, small integers in PPanGGOLiN's graphs (numbers of organisms sharing an adjacency): the block fills a table
    // exp((double)beta * (double)(float)m), m = 0 .. kExpTab - 1, with the SAME device exp on the same argument the site
    // would pass (bit-identical by construction), one entry per thread, and a site whose context is such an integer
    // reads it instead of running three double-precision exp (a third of the round's vector instructions).
    // (A larger per-beta table for the contexts of PPanGGOLiN's own edge weights, which reach the hundreds, measured
    // neutral: NOTES_negative_results.md section 10.)
    constexpr int kExpTab = 64;
    __shared__ double s_exp[NCEM ? kExpTab : 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_lab[NCEM ? BS : 1];   // the block's labels while it iterates
    __shared__ uint64_t s_drew[BS / 64];                 // TIE_LIBC: per wave, which of its sites drew
    bool zero_density = false;
    bool changed = false;
    __shared__ int s_anydrew;                            // TIE_LIBC: a site of the block drew at some local step of this launch
    if (threadIdx.x == 0) { s_nzero = 0; s_first = 0; s_chg = 0; s_mov = 0; s_anydrew = 0; }
    // BLIND: the block's old labels (the blind partition; s_lab moves on with the block-local steps), and the blind
    // sweep's own zero-density tally.  The site's blind label: from its densities, which were asked for at entry
    __shared__ __attribute__((aligned(16))) uint8_t s_old[BLIND ? BS : 1];
    __shared__ int s_bnzero, s_bfirst;
    bool blind_zero = false;
    if constexpr (BLIND) {
        if (threadIdx.x == 0) { s_bnzero = 0; s_bfirst = 0; }
        bool z;
        my_guess = blind_label<KA>(a, K, pkf, (uint32_t)gi, &z);
        my_old = my_guess;
        blind_zero = active && z;
        s_old[threadIdx.x] = (uint8_t)my_guess;
        if (active) const_cast<uint8_t*>(a.lab_guess)[gi] = (uint8_t)my_guess;   // (stored, never read in this launch)
    }
    if (NCEM) s_lab[threadIdx.x] = (uint8_t)my_guess;
    if (NCEM && a.use_nei && !skip && threadIdx.x < kExpTab) s_exp[threadIdx.x] = exp((double)a.beta * (double)(float)threadIdx.x);
    // TIE_LIBC: draws of the blocks below this one, as the guess has them -- summed once by the block's first wave (a
    // lane that ties used to add the counts up itself: up to 78 loads in a row per tying lane, 2-3 us of a round on
    // data that tie in every sweep, the initial sweeps of a random start)
    __shared__ int s_lower;
    if (LIBC && !skip && threadIdx.x < 64 && a.tie_cnt_guess != nullptr) {
        int part = 0;
        for (int b = threadIdx.x; b < bx; b += 64) part += a.tie_cnt_guess[b];
        part = wave_sum_i32(part);
        if (threadIdx.x == 0) {
            if (a.rank_tot_in != nullptr)                // sharded: the ranks below, as the guess has them
                for (int r = 0; r < a.rank_index; r++) part += *reinterpret_cast<const int*>(a.rank_tot_in + (size_t)r * a.slot_stride);
            s_lower = part;
        }
    }
    // TIE_LIBC: does any site of the block carry "drew" in the guess?  Blocks without ties (most blocks, most rounds) skip
    // the per-step tally of who drew -- a ballot and a barrier per local step, and another pair at the round's end
    bool blk_drew = false;
    if (LIBC) blk_drew = __syncthreads_or((my_guess & kLabDrew) != 0) != 0;
    else __syncthreads();
    NEM_SWEEP_PHASE(2);

    if (NCEM) {
    // ------------------------------------------------------------------------------------------
    // NCEM.  A plain round would evaluate every site once against the guess.  Most Gauss-Seidel dependencies are
    // index-adjacent (the contiguity path), i.e. inside the block: so the block goes on evaluating its sites against
    // ITS OWN latest labels for the lower-indexed neighbours it holds (the guess for all others) until nothing in
    // the block changes -- Jacobi steps on a lower-triangular system, final for the block's first t sites after t
    // steps.  Exactness is untouched: the first step is the plain round, so the block reproduces its guess iff
    // the plain round would, and the sweep still ends with a round that changes nothing anywhere.  What it buys is
    // rounds: label changes run down the path inside one launch instead of one launch per hop.
    // ------------------------------------------------------------------------------------------
    constexpr bool libc = LIBC;
    // (the label shortcut of nem_map.hpp: in the instances for K <= 7 -- from K = 8 on, and in the instance for any K,
    //  the decision's registers on top of the row's cost a wave per SIMD or spill)
    constexpr bool kMapShort = KT >= 1 && KT <= 7;
    const int blk_lo = a.lo + bx * spb;          // first label slot of this block
    // (pkf, nb, ne: asked for at the head of the block)
    // the first four neighbours live in registers: index, weight, and the label when it cannot change in here
    int dyn[4]; float wn[4]; int fl[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { dyn[u] = -1; wn[u] = 0.0f; fl[u] = 255; }
    if (active && !skip && a.use_nei) {
        int jn[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool ok = nb + u < ne;
            jn[u] = ok ? a.nei_idx[nb + u] : gi;
            wn[u] = ok ? a.nei_w[nb + u] : 0.0f;
        }
        if constexpr (BLIND) {
            // a neighbour at or above the site in the block: the block's old labels; in another block: its K densities,
            // gathered for all four at once -- they depend on nei_idx exactly as the label gather did -- and
            // blind_label(), which the lanes of a wave that have such a neighbour branch into together
            // (one neighbour's densities at a time instead: the same register counts, K = 2 .. 7 -- the instance's peak is
            //  not here)
            bool far[4];
            double pn[4][KA];
#pragma unroll
            for (int u = 0; u < 4; u++) far[u] = nb + u < ne && (jn[u] < blk_lo || jn[u] >= blk_lo + BS);
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int k = 0; k < KA; k++) pn[u][k] = far[u] ? a.pkfki[(size_t)k * a.npad + (jn[u] - a.lo)] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (nb + u < ne) {
                    if (jn[u] < gi && jn[u] >= blk_lo) dyn[u] = jn[u] - blk_lo;
                    else if (!far[u]) fl[u] = s_old[jn[u] - blk_lo];
                    else { bool z; fl[u] = blind_label<KA>(a, K, pn[u], (uint32_t)jn[u], &z); }
                }
            }
        } else {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (nb + u < ne) {
                if (jn[u] < gi && jn[u] >= blk_lo) dyn[u] = jn[u] - blk_lo;
                else fl[u] = ((jn[u] < gi) ? a.lab_guess[jn[u]] : a.lab_old[jn[u]]) & kLabMask;
            }
        }
        }
    }
    const bool long_row = ne - nb > 4;
    NEM_SWEEP_PHASE(3);
    int lower_draws = -1;                                // (read from s_lower, written ahead of the barrier at the block's head)
    bool tab_short = false;                              // TIE_LIBC: a draw fell outside the table: the round is void
    int cur = my_guess;                                  // this site's byte in s_lab
    int seen[4] = {-1, -1, -1, -1};                      // labels the last evaluation used for the dyn neighbours
    uint64_t seen_drew = ~0ull; int seen_wave_draws = -1;
    for (int it = 0; it < kInnerCap; it++) {
        int below_in_block = 0;
        uint64_t drew_lt = 0;
        if (libc && blk_drew) {                          // who drew, per wave (block-uniform branch)
            const uint64_t bal = __ballot((s_lab[threadIdx.x] & kLabDrew) != 0);
            if ((threadIdx.x & 63) == 0) s_drew[threadIdx.x >> 6] = bal;
            __syncthreads();
            for (int w = 0; w < (int)(threadIdx.x >> 6); w++) below_in_block += (int)__popcll(s_drew[w]);
            drew_lt = s_drew[threadIdx.x >> 6] & ((1ull << (threadIdx.x & 63)) - 1ull);
        }
        int nxt = cur;
        if (active && !skip) {
            int lab[4];
            bool same = it != 0 && !long_row;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                lab[u] = dyn[u] >= 0 ? (s_lab[dyn[u]] & kLabMask) : fl[u];
                same = same && (dyn[u] < 0 || lab[u] == seen[u]);
            }
            if (libc) same = same && drew_lt == seen_drew && below_in_block == seen_wave_draws;
            if (!same) {
                float ctx[KA];
#pragma unroll
                for (int k = 0; k < KA; k++) ctx[k] = 0.0f;
                // (the adds keep the .nei order, SumNeighsOfClass nem_alg.c:2865-2875; w*1 = w, w*0: additive identity)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    seen[u] = lab[u];
                    if (nb + u < ne) {
#pragma unroll
                        for (int k = 0; k < KA; k++)
                            if (k < K) ctx[k] = ctx[k] + ((lab[u] == k) ? wn[u] : -0.0f);
                    }
                }
                for (int t = nb + 4; t < ne; t++) {      // rows longer than four neighbours: from memory
                    const int j = a.nei_idx[t];
                    const float wt = a.nei_w[t];
                    int l;
                    if (j < gi && j >= blk_lo) l = s_lab[j - blk_lo] & kLabMask;
                    else if constexpr (BLIND) {          // (the same three cases as the first four)
                        if (j >= blk_lo && j < blk_lo + BS) l = s_old[j - blk_lo];
                        else {
                            double pj[KA];
#pragma unroll
                            for (int k = 0; k < KA; k++) pj[k] = a.pkfki[(size_t)k * a.npad + (j - a.lo)];
                            bool z;
                            l = blind_label<KA>(a, K, pj, (uint32_t)j, &z);
                        }
                    }
                    else l = ((j < gi) ? a.lab_guess[j] : a.lab_old[j]) & kLabMask;
#pragma unroll
                    for (int k = 0; k < KA; k++)
                        if (k < K) ctx[k] = ctx[k] + ((l == k) ? wt : -0.0f);
                }
                // a row whose maximum is clear has its label without the normalised row (nem_map.hpp); the lanes of
                // a wave that are not sure branch together, around all the divisions
                float cf[KA];
                int kmax = 0;
                bool clear = false;
                if constexpr (kMapShort) {
                    double cinum[KA];
                    const double cum = local_cinum<KA>(a, K, pkf, ctx, cinum, s_exp, kExpTab);
                    zero_density = !(cum > 0);
                    clear = !a.map_full && map_clear_row<KA>(cinum, K, cum, kmax);
                    if (!clear) map_normalise<KA>(cinum, K, cum, cf);
                } else zero_density = local_proba<KA>(a, K, pkf, ctx, cf, s_exp, kExpTab);
                int drew = 0;
                if (!clear) {                            // every other row: the reference's arithmetic, as it was
                // ComputeMAP, nem_alg.c:603-640
                kmax = 0; float ukmax = cf[0];
#pragma unroll
                for (int k = 1; k < KA; k++) if (k < K && cf[k] > ukmax) { ukmax = cf[k]; kmax = k; }
                if (a.tie_rule != NEMGPU_TIE_FIRST) {
                    int nequal = 0;
#pragma unroll
                    for (int k = 1; k < KA; k++) if (k < K && k > kmax && cf[k] == ukmax) nequal++;
                    if (nequal > 0) {
                        uint32_t r;
                        if (libc) {
                            // the reference's stream (nem_rnd.c:53-61): this site's draw is number
                            //   draws before the sweep + sites below it that drew in this sweep
                            if (lower_draws < 0) lower_draws = s_lower;
                            int base = a.draw_base, tab0 = a.draw_tab0;
                            if (a.draw_ctl != nullptr) { base = a.draw_ctl[0]; tab0 = a.draw_ctl[1]; }
                            if (a.draw_extra != nullptr) base += *a.draw_extra & (kTabShort - 1);
                            const int at = base + lower_draws + below_in_block + (int)__popcll(drew_lt) - tab0;
                            if (at >= 0 && at < a.draw_tab_len) r = a.draw_tab[at];
                            else { r = 0; tab_short = true; }
                            drew = kLabDrew;
                        } else {
                            const uint32_t sid = a.sweep_id_ptr != nullptr ? (uint32_t)*a.sweep_id_ptr : a.sweep_id;
                            // the hash is keyed by the TRUE family index (label slots of a sharded run carry a flag tail per rank)
                            const uint32_t site = a.slot_stride > 0 ? (uint32_t)(gi - (gi / a.slot_stride) * a.slot_pad) : (uint32_t)gi;
                            r = mix32(a.tie_seed, sid, site);
                        }
                        const int pick = (int)(r % (uint32_t)(nequal + 1));
                        int seen_eq = 0, chosen = kmax;
#pragma unroll
                        for (int k = 1; k < KA; k++)
                            if (k < K && k > kmax && cf[k] == ukmax) { seen_eq++; if (seen_eq == pick) chosen = k; }
                        kmax = chosen;
                    }
                }
                }                                        // (!clear)
                nxt = kmax | drew;
                seen_drew = drew_lt; seen_wave_draws = below_in_block;
            }
        }
        __syncthreads();                                 // every read of s_lab / s_drew of this step is done
        const bool moved_now = nxt != cur;
        cur = nxt;
        s_lab[threadIdx.x] = (uint8_t)cur;
        // (__syncthreads_or hands back a truth value, not the OR of the arguments: "somebody drew" travels through LDS,
        //  written ahead of the barrier, and sticks -- a block that has met a tie keeps the tally for the rest of the launch)
        if (libc && !blk_drew && (cur & kLabDrew) != 0) s_anydrew = 1;
        const int any_moved = __syncthreads_or(moved_now);
        if (libc && !blk_drew) blk_drew = s_anydrew != 0;
        if (!any_moved) break;
    }
    if (active && !skip) {
        changed = (cur != my_guess) || tab_short;         // (a void round never passes for the fixed point)
        my_new = cur & kLabMask;
        a.lab_out[gi] = (uint8_t)cur;
        if (tab_short) atomicOr(&a.flags[FLAG_NTIES], kTabShort);
    }
    if (libc && !skip) {
        // the block's draws of this round, next to the labels they belong to: a guess is (labels, counts)
        if (blk_drew) {
            const uint64_t bal = __ballot(active && (cur & kLabDrew) != 0);
            if ((threadIdx.x & 63) == 0) s_drew[threadIdx.x >> 6] = bal;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            int cnt = 0;
            if (blk_drew) for (int w = 0; w < (int)(blockDim.x >> 6); w++) cnt += (int)__popcll(s_drew[w]);
            if (cnt != blk_cnt_guess) changed = true;
            a.tie_cnt_out[bx] = cnt;
            if (cnt > 0) atomicAdd(&a.flags[FLAG_NTIES], cnt);
        }
    }
    } else if (active && !skip) {
    // ------------------------------------------------------------------------------------------
    // fuzzy NEM: one evaluation of every site against the guess
    // ------------------------------------------------------------------------------------------
    float ctx[KA];
    double pkf[KA];
#pragma unroll
    for (int k = 0; k < KA; k++) ctx[k] = 0.0f;
    // the densities do not depend on the graph: requested first, so that they travel while the neighbour lists do
#pragma unroll
    for (int k = 0; k < KA; k++) if (k < K) pkf[k] = a.pkfki[(size_t)k * a.npad + i];
    if (a.use_nei) {
        const int b = a.nei_ptr[i], e = a.nei_ptr[i + 1];
        for (int t = b; t < e; t++) {
            const int j = a.nei_idx[t];
            const float wt = a.nei_w[t];
            const float* row = ((j < gi) ? a.c_guess : a.c_old) + (size_t)j * K;
#pragma unroll
            for (int k = 0; k < KA; k++)
                if (k < K) ctx[k] = ctx[k] + (wt * row[k]);
        }
    }
    float cf[KA];
    zero_density = local_proba<KA>(a, K, pkf, ctx, cf);
    const float* g = a.c_guess + (size_t)gi * K;
    float* o = a.c_out + (size_t)gi * K;
#pragma unroll
    for (int k = 0; k < KA; k++) {
        if (k < K) {
            changed |= (__float_as_uint(cf[k]) != __float_as_uint(g[k]));
            o[k] = cf[k];
        }
    }
    }
    NEM_SWEEP_PHASE(4);
    if (__any(changed) && (threadIdx.x & 63) == 0) s_chg = 1;
    // the iteration's bookkeeping, when it rides in this round (see SweepArgs): the site's label, "moved"
    int post_lab = 255;
    if (NCEM && a.post_on) {
        int moved = 0;
        if (active) {
            // (a round that skipped its sites and posts its own output reads that output back: not a case the
            //  engine enqueues, the verification round posts its guess)
            // (a round that skipped its sites -- a round before it changed nothing -- has no output of its own: the
            //  partition is in the sweep's first buffer, the guess of odd rounds and the output of even ones)
            if (skip) post_lab = (a.post_skip_guess ? my_guess : (int)a.lab_out[gi]) & kLabMask;
            else post_lab = a.post_from_guess ? (my_guess & kLabMask) : (my_new != 255 ? my_new : ((int)a.lab_out[gi] & kLabMask));
            if (a.post_moved) moved = (post_lab != my_old);
        }
        if (__any(moved) && (threadIdx.x & 63) == 0) s_mov = 1;
    }
    // zero-density sites (nem_alg.c:2603-2613): count and first index, one pair of atomics per block
    const uint64_t zmask = __ballot(zero_density);
    if (zmask != 0ull && (threadIdx.x & 63) == 0) {
        atomicAdd(&s_nzero, (int)__popcll(zmask));
        atomicMax(&s_first, a.n_total - (gi + (int)__ffsll((long long)zmask) - 1));   // lanes are consecutive sites
    }
    if constexpr (BLIND) {                               // the blind sweep's tally: the block's OWN sites' blind evaluations
        const uint64_t bmask = __ballot(blind_zero);
        if (bmask != 0ull && (threadIdx.x & 63) == 0) {
            atomicAdd(&s_bnzero, (int)__popcll(bmask));
            atomicMax(&s_bfirst, a.n_total - (gi + (int)__ffsll((long long)bmask) - 1));
        }
    }
    __syncthreads();
    NEM_SWEEP_PHASE(5);
    // BLIND: into the blind sweep's flag slot, as a blind round's blocks would (its FLAG_CHANGED stays 0: nobody reads it)
    if (BLIND && threadIdx.x == 0 && s_bnzero > 0) {
        int* bf = a.flags + a.blind_off;
        atomicAdd(&bf[FLAG_NZERO], s_bnzero);
        if (bf[FLAG_FIRSTZERO] < s_bfirst) atomicMax(&bf[FLAG_FIRSTZERO], s_bfirst);
    }
    // One same-address atomic per block is what a round costs when every site reports (all densities underflow at
    // D = 5000: 196 blocks x ~45 ns, 12 of a round's 26 us at 200 000 x 5 000).  Once the loop control has seen
    // such a sweep (ctrl[C_FOLD], set by ctrl_logic, read with the stop word) the tally rides on the last-block
    // counters instead.
    const bool fold = fold_hint != 0 && a.fold_ticket != nullptr && nblk > 32;
    if (threadIdx.x == 0 && s_nzero > 0) {
        if (!fold) atomicAdd(&a.flags[FLAG_NZERO], s_nzero);
        if (a.flags[FLAG_FIRSTZERO] < s_first) atomicMax(&a.flags[FLAG_FIRSTZERO], s_first);   // first site = n_total - max
    }
    // "changed" and "moved": the look that thins same-address atomics out on grids of thousands of waves (see s_chg) is a
    // device-scope round trip per flag on thread 0, and in the counting round the whole block's adds wait for both at the
    // barrier below.  The blocks of a small grid reach the look within its own latency of each other, most see 0 and send
    // the atomic anyway: up to kNoLookBlocks blocks (`nblk`, the round's own) the no-return atomic goes straight out, and
    // thread 0 waits for nothing.  Larger grids keep the look.
    constexpr int kNoLookBlocks = 128;
    if (threadIdx.x == 0) {
        const bool look = nblk > kNoLookBlocks;
        if (s_chg && !(look && __hip_atomic_load(&a.flags[FLAG_CHANGED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0))
            atomicOr(&a.flags[FLAG_CHANGED], 1);
        if (NCEM && a.post_on && s_mov && !(look && __hip_atomic_load(&a.post_flags[FLAG_MOVED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0))
            atomicOr(&a.post_flags[FLAG_MOVED], 1);
    }
    NEM_SWEEP_PHASE(6);
    __shared__ uint64_t s_cmask[COUNT ? KA : 1][4];      // COUNT: the block's class masks, [class][wave]
    if (NCEM && a.post_on) {                             // k_labels_post's work, see SweepArgs
        const int wave = i >> 6;
        if (COUNT) {                                     // (every wave: one past the labels has empty masks)
            for (int k = 0; k < K; k++) {
                const uint64_t m = __ballot(post_lab == k);
                if ((threadIdx.x & 63) == 0) {
                    if (wave < a.post_nw64) a.post_mask[(size_t)k * a.post_nw64 + wave] = m;
                    s_cmask[k][threadIdx.x >> 6] = m;
                }
            }
        } else if (wave < a.post_nw64 && !a.post_no_masks) {
            for (int k = 0; k < K; k++) {
                const uint64_t m = __ballot(post_lab == k);
                if ((threadIdx.x & 63) == 0) a.post_mask[(size_t)k * a.post_nw64 + wave] = m;
            }
        }
    }
    if (COUNT) {
        // k_mstep_counts' work for this block's 256 families: S1[k][d] and N_k are integer counts, so the blocks' partial
        // counts add up to the same statistics in any order -- one no-return device-scope atomic per nonzero partial, into
        // words an earlier launch of the batch zeroed; the launch boundary behind this round publishes the sums
        __syncthreads();
        const int D = a.post_D;
        int* st = a.post_stats;
#pragma unroll
        for (int q = 0; q < kCntRows; q++) {
            const int d = (int)threadIdx.x + q * BS;
            if (d < D) {
#pragma unroll
                for (int k = 0; k < KA; k++) {
                    const int v = __popcll(xs[q][0] & s_cmask[k][0]) + __popcll(xs[q][1] & s_cmask[k][1]) +
                                  __popcll(xs[q][2] & s_cmask[k][2]) + __popcll(xs[q][3] & s_cmask[k][3]);
                    if (v != 0) atomicAdd(&st[K + k * D + d], v);
                }
            }
        }
        if ((int)threadIdx.x < K) {
            const int k = threadIdx.x;
            const int v = __popcll(s_cmask[k][0]) + __popcll(s_cmask[k][1]) + __popcll(s_cmask[k][2]) + __popcll(s_cmask[k][3]);
            if (v != 0) atomicAdd(&st[k], v);
        }
    }
    NEM_SWEEP_PHASE(7);
    const bool post_ctrl = NCEM && a.post_on && a.post_ctrl.ctrl != nullptr;
    if (a.publish_byte != nullptr || post_ctrl || fold) {
        int* ticket = a.publish_byte != nullptr ? a.publish_ticket : (post_ctrl ? a.post_ctrl.ticket : a.fold_ticket);
        if (last_block_ticket(ticket, nblk, fold ? s_nzero : 0, fold ? &a.flags[FLAG_NZERO] : nullptr, bx)) {
            if (a.publish_byte != nullptr) {
                *a.publish_byte = (uint8_t)(__hip_atomic_load(&a.flags[FLAG_CHANGED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
                if (NCEM && a.post_on && a.post_moved)          // (sharded: this rank's 'a label moved' byte rides next to it)
                    a.publish_byte[1] = (uint8_t)(__hip_atomic_load(&a.post_flags[FLAG_MOVED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
                if (LIBC && a.rank_tot_out != nullptr)           // (... and its draws of this round)
                    *reinterpret_cast<int*>(a.rank_tot_out) =
                        __hip_atomic_load(&a.flags[FLAG_NTIES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (kTabShort - 1);
            }
            if (post_ctrl) ctrl_logic(a.post_ctrl);
        }
    }
}

}  // namespace nemk
