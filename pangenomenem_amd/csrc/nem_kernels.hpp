// nem_kernels.hpp -- kernel launch interface (device pointers only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/nem_mi355x.h"

namespace nemk {

constexpr int kMaxKernelK = 32;
constexpr int kTicketWords = 32 * 33;   // last-block ticket: top counter + 32 group counters, 128 bytes apart
constexpr double kEpsilonD = 1e-20;   // EPSILON, reference nem_typ.h:63

// per-round flag slot of an E2 sweep
// FLAG_NTIES (TIE_LIBC): random draws the round's sites made; bit 30: a draw fell outside the draw table
enum { FLAG_CHANGED = 0, FLAG_NZERO = 1, FLAG_FIRSTZERO = 2, FLAG_NTIES = 3, FLAG_ROUND_STRIDE = 4 };
// per-iteration flag block.  FLAG_EMPTYK is overwritten by every k_mstep_disp; FLAG_MOVED and the
// relaxation-round window that follows this block are zeroed by k_density, which precedes every
// sweep of the EM loop (so no memset launches are needed).  Under the shadow-verify schedule (nem_engine.hip) an engine
// keeps three such blocks, each with its round window, and a density launch clears only the one of its own iteration.
// FLAG_FAULT: a kernel could not finish its work (bit 0: a hand-over of k_mstep_fuzzy_pc never completed).  Sticky: only
// a reset clears it; the host turns it into NEMGPU_E_INTERNAL wherever it reads the flags back.
enum { FLAG_EMPTYK = 0, FLAG_EMPTY_PROP = 1, FLAG_FAULT = 2, FLAG_MOVED = 3, FLAG_ITER_STRIDE = 4 };

// device-side loop control block (ints), see k_ctrl
// C_FOLD sits next to C_STOP so that a sweep block reads both with one 8-byte scalar load: "the last sweep met
// zero-density sites" (how the next sweeps tally them, see k_sweep); it survives a restart.
enum { C_STOP = 0, C_FOLD = 1, C_ITERS = 10, C_COMMITS = 2, C_STATUS = 3, C_EMPTYK = 4, C_CONVERGED = 5, C_NEED_ROUNDS = 6,
       C_SWEEP_ROUNDS = 7, C_NZERO = 8, C_FIRSTZERO = 9, C_DRAWS = 11, C_DEEP = 12, C_DRAWS_INIT = 13, C_INIT_ROUNDS = 14, C_WORDS = 16 };
// C_DRAWS_INIT (TIE_LIBC): of C_DRAWS, what the run's two initial sweeps drew; C_INIT_ROUNDS: the rounds they needed (blind << 8 | beta)
// C_DEEP: the last iteration of the batch (1-based) whose sweep used more than two of its relaxation rounds

struct CtrlArgs {
    int* ctrl; const int* iter_flags; const int* round0;   // round0: flag slot of relaxation round 0 (round r: r slots on)
    int n_rounds;                  // relaxation rounds enqueued per sweep (0: two)
    int param_fix, use_nei, cvtest, ncem; float cvthres;
    int* sweep_next;               // device word: number of the next sweep (tie-break hash key)
    int* ticket;                   // last-block-done counter (self-resetting)
    // sharded runs: every rank's "some label changed" byte for round 0 / round 1, as all-gathered at the tail
    // of each rank's block of the label arrays (nullptr on a single GPU: the int flags above are used)
    const uint8_t* q_flags; const uint8_t* r_flags; int n_ranks, flag_stride;
    int moved_bytes;               // sharded: the byte behind a rank's flag byte says 'one of its labels moved' (1: in r_flags, 2: in q_flags)
    int is_init;                   // the two initial sweeps: no iteration is counted, the sweep number becomes 2
    const int* blind;              // is_init: flag slot of the blind beta = 0 sweep (its zero-density tally), or nullptr
    int blind_rounds;              // is_init, TIE_LIBC: the blind sweep ran this many verified rounds, their slots from `blind` on (0: one slot, nothing to verify)
    int* draw_ctl;                 // TIE_LIBC: {draws made so far, first draw of the table} (device), else nullptr
    const uint8_t* q_tot;          // TIE_LIBC, sharded: rank 0's draw total in the tail of the sweep's first buffer (flag_stride apart)
};
void launch_ctrl(const CtrlArgs& a, hipStream_t s);

struct SweepArgs {
    int n_local, lo, n_total, K, npad, use_nei;
    const int* nei_ptr; const int* nei_idx; const float* nei_w;
    float beta;
    const double* pkfki;                       // [K][npad], local families
    // NCEM state: labels, GLOBAL family indexing
    const uint8_t* lab_old; const uint8_t* lab_guess; uint8_t* lab_out;
    // fuzzy state: float rows [n_total][K], GLOBAL family indexing
    const float* c_old; const float* c_guess; float* c_out;
    int tie_rule; uint32_t tie_seed; uint32_t sweep_id;
    uint32_t blind_sweep_id;                   // a BLIND round (blind_off below): the blind sweep's number, which keys ITS ties
    const int* sweep_id_ptr;                  // when set, the sweep number is read from the device instead
    int* flags;                                // this round's slot
    const int* prev_changed;                   // previous round's FLAG_CHANGED (nullptr for round 0)
    const int* stop;                           // loop-control stop word (nullptr outside the pipelined loop)
    // sharded runs: label arrays are laid out in per-rank blocks of `slot_stride` bytes (labels + flag tail);
    // flags_in = previous round's all-gathered flag bytes (round exits when none is set)
    const uint8_t* flags_in; int n_ranks, slot_stride, slot_pad;
    // NCEM, pipelined loop: the iteration's bookkeeping (k_labels_post: class masks, "moved" flag, loop control in
    // the last block) folded into the last enqueued round.  post_from_guess: the final labels are this round's
    // guess (a verification round: if it changes anything the loop control stops the pipeline and the host redoes
    // the bookkeeping), else this round's output.
    // post_skip_guess: where the partition is when this round skips its sites (a round before it changed nothing):
    // the sweep's first buffer -- this round's guess if it is an odd round, its output buffer if it is an even one
    int post_on, post_from_guess, post_moved, post_nw64, post_skip_guess;
    int post_no_masks;             // the bookkeeping without the class masks (a verifying round whose guess has them already)
    uint64_t* post_mask; int* post_flags;
    CtrlArgs post_ctrl;
    // sharded runs: the last block to finish stores this rank's "some label changed in this round" byte behind
    // its label block (the label all-gather then carries it to every rank)
    uint8_t* publish_byte; int* publish_ticket;
    // zero-density tally of a large grid (see k_sweep): last-block counters to fold it through, or nullptr
    int* fold_ticket;
    // TIE_LIBC (the reference's own tie stream, nem_alg.c:617-637 -> nem_rnd.c:53-61): the site that ties draws
    // random() number  draws before the sweep + sites below it that drew in this sweep.  draw_tab holds draws
    // draw_tab0 .. draw_tab0 + draw_tab_len - 1 of the stream; draws-before-the-sweep and draw_tab0 come from
    // draw_ctl[0..1] (device, pipelined loop) or by value; draw_extra: a count to add (a preceding sweep's draws
    // that no loop control has booked yet).  tie_cnt_*: draws per block of the guess / of this round's output.
    const uint32_t* draw_tab; int draw_tab_len, draw_base, draw_tab0;
    const int* draw_ctl; const int* draw_extra;
    const int* tie_cnt_guess; int* tie_cnt_out;
    // ... sharded: the sites of the ranks below come first in the draw order.  Every rank's draws of the round that
    // produced a label buffer ride in its block's tail (an int32), all-gathered with the labels: rank_tot_in = rank 0's
    // in the GUESS buffer (the others slot_stride bytes apart), rank_index = this rank, rank_tot_out = this rank's slot
    // in the output buffer (written by the last block of the round)
    const uint8_t* rank_tot_in; int rank_index; uint8_t* rank_tot_out;
    // sites per block of the large-shard kernel instances (set by launch_sweep; 0: the kernel's block size)
    int spb;
    // A start's first beta round with the blind sweep inside it (sweep_body's BLIND instances; 0: an ordinary round).
    // Such a round computes every blind label it needs from the densities and reads no labels buffer: its blocks STORE
    // their own sites' blind labels to lab_guess (= lab_old: the buffer the blind sweep would have written) and tally
    // the blind sweep's zero-density sites into that sweep's flag slot, flags + blind_off.  (This word and
    // blind_sweep_id sit where the struct had padding: no other argument moved.)
    int blind_off;
    // shadow-verify schedule, the round that makes the class masks of a held sweep: the M-step counts of those masks
    // (k_mstep_counts' {N_k, S1[k][d]}) added into post_stats, zeroed by an earlier launch -- every block its 256
    // families' share, from the organism-major bit rows post_xt ([post_D][post_nw64]).  nullptr: no counting.
    int* post_stats; const uint64_t* post_xt; int post_D;
    // NCEM: a site's label comes from the unnormalised row where its maximum is clear (nem_map.hpp); nonzero: every row
    // is normalised, as the reference does (NEM_MI355X_MAP_MARGIN=0)
    int map_full;
};
// argument blocks of the smaller kernels; the engine makes each in one place (nem_engine.hip, next to finish_args) and
// the launch wrappers below take them whole
struct LabelsPostArgs { int n_local, lo, K, nw64; const uint8_t* lab_new; const uint8_t* lab_old; uint64_t* mask; int* flags;
                        const int* stop; CtrlArgs ca; };
struct CountsArgs { int K, D, nw64; const uint64_t* xt; const uint64_t* mask; int* stats; const int* stop; CtrlArgs prev_ctrl; };
struct FuzzyArgs { int n, npad, K, D; const uint32_t* xw; const uint64_t* xt; int nw64; const float* c; float* nbobs_k;
                   float* in0; float* in1; float* inh_k; int* lastz; int* any1; float* center; float* iner; const int* stop;
                   float* ct; int ctpad;      // ct: class-major copy of c, [K][ctpad]
                   float* chk;                // the zeros' chains every 64 families, [K][nwin + 1][64 DB]
                   int* fault;                // the iteration flags' FLAG_FAULT word (nullptr: faults go unreported)
                   int inject; };             // test hook (NEM_MI355X_FAULT_INJECT=fuzzy_pc): one producer skips a hand-over
struct ConvFuzzyArgs { size_t m; const float* c; const float* cold; float thres; int* flags; const int* stop; CtrlArgs ca; };
struct OnehotArgs { int n, K; const uint8_t* lab; float* c; };
struct CritArgs { int n, K, npad; const int* nei_ptr; const int* nei_idx; const float* nei_w; int use_nei; float beta;
                  const float* c; const double* pkfki; const float* logpkfki; float* dik; float* gik; double* lfi; double* lzi;
                  float* crit6; int hard; };
struct FillArgs { int* ptr; int words; int value; };
struct CopyArgs { const int* src; int* dst; int words; };
// up to eight device-to-device copies in one launch (the logged run's set-aside behind an iteration; not recordable)
struct CopySegsArgs { const int* src[8]; int* dst[8]; int words[8]; int n; };
void launch_copy_segments(const CopySegsArgs& a, hipStream_t s);
struct LayoutArgs { const uint32_t* xf; const int* perm; int n, wf, W, npad, d, nw64; uint32_t* xw; uint32_t* xws; uint64_t* xt; };

// ---- batched launches: B independent problems per launch ---------------------------------------------------------
// A host thread that sets a Recorder gets the launches of the code it then runs RECORDED instead of issued (same
// argument blocks, same grids); the batch driver (nem_engine.hip) records one sequence per problem, checks that the
// sequences agree launch for launch (same_launch), and issues each position once for all problems with launch_zipped:
// through the kernel's batched twin k_X_b, which takes an ARRAY of argument blocks in device memory and runs problem
// blockIdx.z of it.  What is recordable is ONE list, NEM_OPS in nem_kernels.hip: an entry there makes the kernel, its
// twin, the op's kind and its case in launch_zipped; the launch wrapper hands the kind and the kernel to issue().
// The two template kernels (the sweep round, nem_sweep.hip; the M-step counts) have hand-written pairs and the first two
// kinds; the list's kinds follow them.
enum OpKind { OP_SWEEP = 1, OP_COUNTS, OP_LISTED };
constexpr int kOpArgBytes = 512;
struct OpRecord {
    int kind, variant;             // variant: template instance / block size, part of what must agree across problems
    unsigned gx, gy, block;
    int nbytes;
    alignas(16) unsigned char args[kOpArgBytes];
};
// may the two launches go out as one?  (Everything but the argument blocks and the grid widths, which are per problem.)
inline bool same_launch(const OpRecord& a, const OpRecord& b)
{
    return a.kind == b.kind && a.variant == b.variant && a.block == b.block && a.gy == b.gy && a.nbytes == b.nbytes;
}
struct Recorder { std::vector<OpRecord> ops; };
void set_recorder(Recorder* r);    // thread-local; nullptr: launches are issued
Recorder* current_recorder();
// position `kind`/`variant` for B problems: dev_args = B argument blocks `stride` bytes apart, dev_gx[B] = each
// problem's own grid width (blocks beyond it return at once)
void launch_zipped(int kind, int variant, int B, const void* dev_args, int stride, const int* dev_gx, unsigned max_gx,
                   unsigned gy, unsigned block, hipStream_t s);
void launch_fill(int* ptr, int words, int value, hipStream_t s);   // recordable memset of 32-bit words
void launch_copy_words(const int* src, int* dst, int words, hipStream_t s);   // recordable device-to-device copy


void launch_layout(const LayoutArgs& a, hipStream_t s);
// parameter update + density tables (k_finish); also carries the table pointers k_density reads
struct FinishArgs {
    int mode;                      // 0: tables only; 1: NCEM centres from counts + dispersion + tables; 2: dispersion + tables
    int K, D, dpad, n_total, disper, propor;
    const int* stats;              // NCEM counts {N_k, S1[k][d]}: stats_ranks partial arrays, stats_rank_stride ints apart
    int stats_ranks, stats_rank_stride;   // (1, 0 on a single GPU; sharded: every rank's partial counts, summed on read)
    float* prop; float* center; float* disp; float* nbobs_k; float* iner;
    double2* tabT; double* tabL0; uint32_t* nz0; uint32_t* nz1;
    uint32_t* am0; uint32_t* am1; double2* uni; int* nonuni;
    double* pk; float* logpk; int* flags;
    const int* stop;
    // head of a restart batch (mode 0, reset_prop != nullptr): reload the initial parameters and clear the loop
    // control words in this launch instead of five copy / fill operations
    const float* reset_prop; const float* reset_center; const float* reset_disp;
    int* reset_ctrl; int reset_ctrl_words; int* reset_sweep_next;
    const int* perm;               // density kernels: lane i of the (sorted) matrix copy is family perm[i]
    int use_ff;                    // density kernels: fast-forward the uniform chain inside float binades (nem_ff.hpp), an FFMode
    uint2* ffq;                    // [K][256] (q0, q1 - q0): the fast-forward increments per class, built next to the tables
    // fused density (mode 1): where an empty class keeps its centre and dispersions from (nullptr: center / disp)
    const float* prev_center; const float* prev_disp;
    // statistics words to clear for a counting round that follows (fused density and the restart head; nullptr: none)
    int* zero_stats; int n_zero_stats;
};
void launch_finish(const FinishArgs& a, hipStream_t s);
// what a density launch takes besides the FinishArgs (host side only: the launchers copy it into the kernels' blocks)
struct DensityIO { const uint32_t* xw; int n, npad; double* pkfki; float* logpkfki; int* zero_flags; int n_zero_flags; };
void launch_density(const FinishArgs& t, const DensityIO& io, hipStream_t s);
// NCEM, sk_/skd, D <= kFusedMaxD: parameter update from t.stats folded into the density kernel (no k_finish); not recordable
constexpr int kFusedMaxD = 1024;   // beyond this the per-block parameter derivation costs more than a k_finish launch
// FinishArgs::use_ff.  FF_BATCHED: the fused density kernels (33 .. kFusedMaxD organisms, a grid the device holds at
// once) let every lane walk its own row and cross binades in batches (chain_ff_batched); every other kernel and shape
// reads it as FF_WORD.
enum FFMode { FF_OFF = 0, FF_WORD = 1, FF_BATCHED = 2 };
void launch_density_fused(const FinishArgs& t, const DensityIO& io, hipStream_t s);
// the start of a run in ONE launch (k_density_start): the restart head (t.reset_*: initial parameters into t.prop / center /
// disp, class sizes zeroed, loop control and sweep counter cleared, t.zero_stats cleared) and the density of the given
// parameters, every block deriving its class constants from them.  The table buffers are not rebuilt.  Same shapes as
// launch_density_fused; not recordable.
void launch_density_start(const FinishArgs& t, const DensityIO& io, hipStream_t s);
// ... and the same density beside the last relaxation round of the previous iteration's sweep, in ONE launch
// (k_density_verify); the round's arguments are complete, its last-block ticket included.  Not recordable.
bool density_verify_supported(int n_local, int K, int tie_rule);
void launch_density_verify(const FinishArgs& t, const DensityIO& io, const SweepArgs& sw, hipStream_t s);
void launch_sweep(const SweepArgs& a, bool ncem, hipStream_t s);
// one NCEM relaxation round and the M-step counts (of the partition whose class masks exist already) in ONE launch;
// returns false when the shape has no such kernel (2 <= K <= 5, fewer than 65 536 families, not recordable)
bool launch_sweep_counts(const SweepArgs& sw, const CountsArgs& c, hipStream_t s);   // (c.prev_ctrl is not read)
void launch_labels_post(const LabelsPostArgs& a, hipStream_t s);
void launch_mstep_counts(const CountsArgs& a, hipStream_t s);
void launch_mstep_fuzzy(const FuzzyArgs& a, hipStream_t s);   // (sets ctpad itself)
void launch_conv_fuzzy(const ConvFuzzyArgs& a, hipStream_t s);
void launch_chain_debug(const double* x, long long n, float init, float* out, hipStream_t s);
bool launch_map_margin_debug(const double* pkf, const float* ctx, int n, int K, float beta, int use_nei, int* out, hipStream_t s);   // K <= 8; out[n][4]
bool launch_halfsum_debug(const float* x, int n, int waves, float* out, hipStream_t s, long long* stamps = nullptr);   // n <= 8192, waves 1 | 16; out[2], stamps[6] when timing
void launch_calib_read(const uint32_t* buf, size_t words, uint32_t* sink, hipStream_t s);
void launch_onehot(const OnehotArgs& a, hipStream_t s);
void launch_criteria(const CritArgs& a, hipStream_t s);   // a.hard: one-hot rows (NCEM)

// ---- matrices with missing cells (nem_missing.hip): the three kernels of a masked NCEM iteration --------------------
// ow / ot: the observed mask in xw's and xt's layouts (launch_layout made them), read word for word beside the matrix.
// E1, the general chain of k_density with the step taken only where the cell was observed (DensBernoulli,
// nem_mod.c:654); t: k_finish's pk / logpk / nz0 / nz1 and the parameters; io.xw is not read (xw: the unsorted copy)
void launch_density_masked(const FinishArgs& t, const DensityIO& io, const uint32_t* xw, const uint32_t* ow, hipStream_t s);
// per (class, organism): stats[K + k*D + d] = observed ones, obs[k*D + d] = observed cells; stats[k] = class size
struct CountsMaskedArgs { int K, D, nw64; const uint64_t* xt; const uint64_t* ot; const uint64_t* mask; int* stats; int* obs; };
void launch_mstep_counts_masked(const CountsMaskedArgs& a, hipStream_t s);
// EstimLaplaceCenters + EstimLaplaceIner + InerToDisp* (MISSING_IGNORE) + proportions with NbObs_KD = obs; one block
struct FinishMaskedArgs { int K, D, n_total, disper, propor; const int* stats; const int* obs;
                          float* prop; float* center; float* disp; float* nbobs_k; float* iner; float* nbobs_kd; int* flags; };
void launch_finish_masked(const FinishMaskedArgs& a, hipStream_t s);

// the head of every batched kernel twin: problem = blockIdx.z, its own grid width, its argument block
#define NEM_B_HEAD(Args)                                                   \
    const int p__ = blockIdx.z;                                            \
    const int nblk = gx[p__];                                              \
    if ((int)blockIdx.x >= nblk) return;                                   \
    const Args a = *reinterpret_cast<const Args*>(reinterpret_cast<const char*>(arr) + (size_t)p__ * stride);

// a launch wrapper's first step: with a recorder set on this thread the launch is stored, not issued
template <typename Args>
inline bool record_op(int kind, int variant, dim3 grid, unsigned block, const Args& a)
{
    static_assert(sizeof(Args) <= kOpArgBytes, "argument block too large for an OpRecord");
    static_assert(std::is_trivially_copyable<Args>::value, "argument blocks are copied byte for byte");
    Recorder* r = current_recorder();
    if (r == nullptr) return false;
    r->ops.emplace_back();
    OpRecord& o = r->ops.back();
    o.kind = kind; o.variant = variant; o.gx = grid.x; o.gy = grid.y; o.block = block; o.nbytes = (int)sizeof(Args);
    memcpy(o.args, &a, sizeof(Args));
    return true;
}
// ... and the whole of most: the launch of a recordable op, stored or issued (no dynamic shared memory: a record has none)
template <typename Args>
inline void issue(int kind, int variant, void (*kernel)(Args), dim3 grid, unsigned block, const Args& a, hipStream_t s)
{
    if (record_op(kind, variant, grid, block, a)) return;
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, a);
}
// the batched twin of a recorded k_sweep position (nem_sweep.hip)
void sweep_dispatch_batched(int variant, dim3 grid, unsigned bdim, hipStream_t s, const void* arr, int stride, const int* gx);

// A run-time K as a compile-time constant: f(std::integral_constant<int, K>{}) for LO <= K <= HI; false: no instance
template <int LO, int HI, typename F>
inline bool dispatch_k(int K, F&& f)
{
    if constexpr (LO > HI) return false;
    else {
        if (K == LO) { f(std::integral_constant<int, LO>{}); return true; }
        return dispatch_k<LO + 1, HI>(K, f);
    }
}

}  // namespace nemk
