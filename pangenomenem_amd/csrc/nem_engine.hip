// nem_engine.hip -- the in-memory NEM engine: device buffers, the EM driver and the nemgpu_* C ABI.
//
// Mirrors the reference's in-memory path ClassifyByNem -> ClassifyByNemOneBeta(INIT_PARAM_FILE)
// -> NemAlgo (/root/reference/ppanggolin/NEM/nem_alg.c:546-584, 1151-1169, 1746-1879) with all
// numeric work in the kernels of nem_kernels.hip.  There is no CPU compute path here: every
// entry point returns NEMGPU_E_DEVICE when HIP is unusable.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <pthread.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "nem_internal.hpp"
#include "nem_ff.hpp"
#include "nem_chain.hpp"
#include "nem_halfsum.hpp"
#include "nem_map.hpp"
#include "nem_rng.hpp"
#include "nem_kernels.hpp"
#include "nem_chunks.hpp"
#include "nem_master.hpp"
#include "nem_vote.hpp"
#include "nem_resample.hpp"

using namespace nemk;

namespace nemk {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
}  // namespace nemk

namespace {
constexpr int kRoundCap = 64;     // relaxation rounds per flag window
// what is zeroed ahead of every sweep (by the density launch, or a fill): FLAG_MOVED and the round window
constexpr int kSweepFlagWords = 1 + kRoundCap * FLAG_ROUND_STRIDE;
constexpr int kFlagSetWords = FLAG_ITER_STRIDE + kRoundCap * FLAG_ROUND_STRIDE;   // one iteration flag block + its round window
constexpr int kRoundBatchMax = 4;
constexpr int kRoundsMax = 7;       // most rounds a sweep of the pipelined loop is given ahead (ctrl_logic reads 8 slots)
constexpr int kFzPositions = 16;    // fuzzy NEM: leading iterations of a run whose round counts are learned

// an engine's freshness flags (tables_fresh, density_fresh, flags_clean, masks_valid)
struct HostFlags { bool tables_fresh = false, density_fresh = false, flags_clean = false, masks_valid = false; };

// Launch sequences captured into hipGraphs (run_graphed), one slot per shape.  desc: everything the captured launches
// depend on, compared on a key hit -- a 64-bit hash alone would replay the wrong graph on a collision.  A full cache
// starts over.  host_flags: a replay sets the owner's freshness flags as the captured enqueue left them (post).
// sticky: clear() keeps the slots and their sightings, so a shape seen before the graphs were dropped is captured
// the next time it comes.
struct GraphCache {
    struct Slot { uint64_t key; std::vector<uint64_t> desc; int asked; hipGraphExec_t exec; HostFlags post; };
    size_t capacity; bool host_flags, sticky;
    std::vector<Slot> slots;
    GraphCache(size_t cap, bool flags, bool keep_sightings) : capacity(cap), host_flags(flags), sticky(keep_sightings) {}
    Slot& find_or_add(const std::vector<uint64_t>& desc)
    {
        uint64_t key = 1469598103934665603ull;                    // FNV-1a
        for (uint64_t v : desc) key = (key ^ v) * 1099511628211ull;
        for (Slot& s : slots) if (s.key == key && s.desc == desc) return s;
        if (slots.size() >= capacity) { clear(); slots.clear(); }
        slots.push_back({key, desc, 0, nullptr, {}});
        return slots.back();
    }
    void clear()                                                  // destroys the captured graphs
    {
        for (Slot& s : slots) if (s.exec) { (void)hipGraphExecDestroy(s.exec); s.exec = nullptr; }
        if (!sticky) slots.clear();
    }
};
}  // namespace

struct nemgpu_engine {
    int n_total = 0, d = 0, k = 0, lo = 0, hi = 0, n = 0;
    int n_true = 0;               // families of the whole problem (= n_total unless label slots carry padding)
    void* rccl_comm = nullptr;           // native RCCL communicator of a sharded engine (nemgpu_rccl_attach)
    int sh_world = 1, sh_rank = 0, sh_blk = 0, sh_stride = 0;   // sharded label-slot layout (stride 0 = plain)
    const uint8_t* shard_lab[3] = {nullptr, nullptr, nullptr};   // the driver's three all-gathered label arrays (TIE_LIBC: tie_cnt[b] goes with shard_lab[b])
    int sh_tot_off() const { return ((sh_blk + 3) & ~3) + 4; }   // a rank's int32 draw total inside its block (behind the flag bytes)
    int npad = 0, dpad = 0, W = 0, wf = 0, nw64 = 0, device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    nemgpu_config cfg{};
    bool have_matrix = false, have_params = false, has_graph = false;
    bool reset_pending = false;          // set_params / configure: the device half of the reset is still to do
                                         // (a run that starts with the restart launch does it there)

    uint32_t* xw = nullptr;
    // E1's own copy of the matrix: uint4[ceil(W/4)][npad], lane i holds family perm[i].  Inside every 256-family
    // tile (one block of the density kernels) the families are ordered by their number of present organisms, so
    // the lanes of a wave run similar chains and cross float binades in the same words (what keeps the
    // fast-forward of nem_ff.hpp coherent across a wave; a global sort gains almost nothing over the tile-local
    // one).  The block puts its 256 results back in family order through LDS, so its stores are contiguous and
    // nothing outside the density kernels sees the order.
    uint32_t* xws = nullptr;
    int* perm = nullptr;
    // the family-major bit rows as uploaded (random starts pick centres from them): pinned when they fit the pool's
    // staging limit -- then the upload is a true asynchronous copy out of them -- else host_bits_own's
    uint32_t* host_bits = nullptr; size_t host_bits_words = 0, host_bits_pin = 0;
    std::vector<uint32_t> host_bits_own;
    // pinned sources of uploads that may still be in flight on the stream (matrix order, graph, parameters): they go
    // back to the pool when the engine is destroyed or an input is replaced (after a wait)
    struct Staged { char* p; size_t size; };
    std::vector<Staged> staging;
    bool use_sort = true;
    uint64_t* xt = nullptr;
    int *nei_ptr = nullptr, *nei_idx = nullptr;
    float* nei_w = nullptr;
    int nnz = 0;

    float *prop = nullptr, *center = nullptr, *disp = nullptr;
    float *prop0 = nullptr, *center0 = nullptr, *disp0 = nullptr;
    // prop | center | disp | nbobs_k live in ONE block (sections 256-byte aligned), and so do the initial values
    // (with a zero tail where nbobs_k is): a reset, an upload and a download are one copy each
    size_t par_o_center = 0, par_o_disp = 0, par_o_nb = 0, par_words = 0;
    float *nbobs_k = nullptr, *iner = nullptr;
    int *fz_lastz = nullptr, *fz_any1 = nullptr;
    float *fz_in0 = nullptr, *fz_in1 = nullptr, *fz_inh = nullptr;
    float* fz_ct = nullptr;       // class-major copy of the memberships, [k][npad] (the fuzzy M-step)
    float* fz_chk = nullptr;      // the zeros' chains every 64 families, [k][ceil(n/64) + 1][64 ceil(d/64)] (the fuzzy M-step)
    double2* tabT = nullptr;
    double* tabL0 = nullptr;
    uint32_t *nz0 = nullptr, *nz1 = nullptr, *am0 = nullptr, *am1 = nullptr;
    double2* uni = nullptr;
    int* nonuni = nullptr;
    uint2* ffq = nullptr;         // [k][256] fast-forward increments of the classes on the uniform chain (k_finish)
    int* sweep_next = nullptr;    // device word: number of the next E-step sweep (tie-break hash key)
    bool tables_fresh = false;    // density tables match prop/center/disp
    bool density_fresh = false;   // pkfki / logpkfki match the tables
    double* pk = nullptr;
    float* logpk = nullptr;
    double* pkfki = nullptr;
    float* logpkfki = nullptr;

    uint8_t* lab[3] = {nullptr, nullptr, nullptr};   // NCEM partitions (labels), n_total each
    // TIE_LIBC (the reference's tie stream): draws per sweep block of each label buffer; the stream's table on the
    // device (draws draw_tab0 .. +draw_cap-1 of glibc random() after srandom(tie_seed)); {draws made, draw_tab0} for
    // the pipelined loop (device words); draws made so far (host)
    int* tie_cnt[3] = {nullptr, nullptr, nullptr};
    uint32_t* draw_tab = nullptr; int draw_cap = 0; long draw_tab0 = 0; bool draw_valid = false;
    std::vector<uint32_t> draw_host; nemk::GlibcRandom draw_gen{1}; long draw_gen_pos = 0;
    int* draw_ctl = nullptr;
    float crit_ref = 0.0f;               // CVTEST_CRIT: the criterion the next iteration's is compared with
    int draws = 0; bool tie_heavy = false;
    bool draw_borrowed = false;          // the table is the parent's (lock-step random starts): never written through this engine
    int draws_after_init = 0;                  // TIE_LIBC: the stream's position behind a run's two initial sweeps
    char* rs_par_host = nullptr; size_t rs_par_host_size = 0;   // random starts under TIE_LIBC: the starts' parameters, pinned
    // NCEM, stateless tie rules: rounds enqueued for a start's beta sweep.  round_batch (three) until three starts in a row
    // were through in two -- the third launch then only finds out that it has nothing to do, 4.4 us of every restart;
    // a start that needs the third round after that is finished from the host and the count goes back up for good.
    int init_rounds_ncem = 0; int init_two_streak = 0; bool init_rounds_locked = false;
    int libc_ra = 3, libc_rb = 3;              // TIE_LIBC, pipelined start: rounds enqueued for the blind / the beta initial sweep (batch_plan sets them; part of a first batch's graph)
    const int* draw_extra_once = nullptr;      // TIE_LIBC: the next sweep set up adds this device word to the draws before it (a sweep enqueued behind one whose count the host has not seen)
    int libc_init_hist[2][17] = {};            // TIE_LIBC random starts: how many relaxation rounds the blind / the beta initial sweep of the starts so far needed (16: more)
    int rs_two_waits = 0;                      // ... starts of phase A whose blind sweep was not through in the rounds enqueued (done again, sweep by sweep)
    int rs_rounds = 0, rs_lockstep = 0, rs_alone = 0, rs_redone = 0;   // the last nemgpu_run_random: lock-step rounds, starts that stood in them, starts run alone, starts thrown away
    bool libc() const { return cfg.algo == NEMGPU_ALGO_NCEM && cfg.tie_rule == NEMGPU_TIE_LIBC; }
    float* cbuf[3] = {nullptr, nullptr, nullptr};    // fuzzy partitions, n_total*k each
    int cur = 0;
    uint64_t* mask = nullptr;
    int* stats = nullptr;
    int* flags_dev = nullptr;     // [C_WORDS loop control] then flag_sets x ([FLAG_ITER_STRIDE] [kRoundCap * FLAG_ROUND_STRIDE])
    int* flags_host = nullptr;    // pinned mirror
    const int* stop_ptr = nullptr;   // &ctrl[C_STOP] while the pipelined loop is being enqueued, else nullptr

    float* c_onehot = nullptr;                        // lazily allocated (criteria / NCEM)
    float *crit_dik = nullptr, *crit_gik = nullptr, *crit6_dev = nullptr;
    double *crit_lfi = nullptr, *crit_lzi = nullptr;
    // a second set: the logged run evaluates the criteria of two partitions in the same launches (criteria_pair_enqueue)
    float *crit2_dik = nullptr, *crit2_gik = nullptr, *crit2_6 = nullptr, *c_onehot2 = nullptr;
    double *crit2_lfi = nullptr, *crit2_lzi = nullptr;
    char* crit_pair_dev = nullptr;                   // the two argument blocks of each of those launches

    // run state
    uint32_t sweep_counter = 0;
    int iters = 0, converged = 0, emptyk = 0, status = NEMGPU_OK;
    int zero_density = 0, first_zero = -1, sweep_rounds = 0;
    bool masks_valid = false;
    bool flags_clean = false;     // MOVED + round window are zero (set by k_density, consumed by a sweep)

    // captured batches of the pipelined loop, keyed by (with initial sweeps, current buffer, iterations, leading
    // iterations with one round more): room for every such shape, so nothing is evicted
    GraphCache batch_graphs{2 * 3 * 8 * 8, true, true};
    bool use_graphs = true;
    // Shadow-verify schedule (NEM_MI355X_SHADOW_VERIFY, default on; see shadow_batch_enqueue): a sweep's verifying round
    // runs in the next iteration's density launch, so an iteration's parameters, densities and flag block are written
    // before the loop control has accepted the one before.  Three copies of each, one per label buffer; prop, center,
    // disp, nbobs_k, pkfki, logpkfki and the flag accessors show copy `fset`, which outside a batch's enqueue is the
    // copy of the last accepted iteration.  (flag_sets: 3 when the copies exist, else 1.)
    bool shadow_verify = true;
    int flag_sets = 1, fset = 0;
    // ... and under it (NEM_MI355X_ROUND_COUNTS, default on; see shadow_batch_enqueue) the round that makes a held sweep's
    // class masks also adds up the next iteration's M-step counts, so that iteration has no k_mstep_counts launch.  They
    // go to one of two statistics slots (stats_slot[0] is `stats`); stats_last is the slot with the counts a batch left
    // last, which is what a reader of the statistics outside a batch gets.
    bool round_counts = true;
    // ... and (NEM_MI355X_START_FUSED, default on; see enqueue_init) a start's restart head runs inside its density launch
    // (k_density_start) instead of as a k_finish launch ahead of k_density.
    bool start_fused = true;
    // ... and (NEM_MI355X_BLIND_FOLD, default on; see blind_fold_on) the start has no blind launch: round 0 of its beta
    // sweep computes the blind labels it needs (sweep_body's BLIND instances).  n_blind_folds: starts that went out so.
    bool blind_fold = true;
    int n_blind_folds = 0;
    int blind_slot_once = -1; uint32_t blind_id_once = 0;   // the next sweep_enqueue's round 0 is such a round: the blind sweep's flag slot and number

    int* stats_slot[2] = {};
    int* stats_last = nullptr;
    float* par_copy[3] = {}; double* pkfki_copy[3] = {}; float* logpkfki_copy[3] = {};
    // relaxation rounds enqueued per sweep before anybody looks (round 0, its verification, and one more that costs
    // an early-exit launch when it is not needed and a host round trip when it is missing); NEM_MI355X_ROUNDS=2..4
    int round_batch = 3;
    // ... per sweep of an ITERATION: two (the round and its verification) until a sweep of this engine needed more --
    // then every later one gets round_batch.  (Labels are sticky: on the bench's pre-convergence data only the sweep
    // that starts from the blind partition needs a third round; an early-exit launch per iteration costs 2.5 us.)
    int rounds_iter = 2;
    // ... but not all iterations are alike: the first ones after a start move many labels and tend to need the
    // extra round, the later ones almost never do.  The first deep_iters iterations of a run get round_batch rounds;
    // an iteration further on whose sweep the host had to finish moves the mark (it is kept across restarts: the
    // bench and PPanGGOLiN's repeated solves of similar problems find the same pattern every time).
    int deep_iters = 2;
    // Fuzzy NEM: the sweeps of a run's FIRST iterations need more rounds than the later ones (memberships move
    // everywhere after a start), and a sweep that runs out of enqueued rounds stops the pipeline for a host round trip
    // (round 3: 162 of them in 2 700 timed steps).  fz_need[p]: rounds to enqueue for iteration p of a run (0: the
    // default rule), raised to what the host had to add when it finished that iteration's sweep; fz_init_need: the
    // same for the start's beta sweep.  Kept across restarts, like deep_iters.
    uint8_t fz_need[kFzPositions] = {}; uint8_t fz_init_need = 0;
    int run_deep_used = 0; bool run_tracked = false;   // this run: the last iteration that used the extra round
    bool capture_first = false;          // capture a batch shape the first time it is enqueued (nemgpu_set_graph_policy)
    int n_plain = 0, n_captured = 0, n_replayed = 0, n_host_rounds = 0;   // nemgpu_graph_counters
    int ff_mode = -1;                    // density: binade fast-forward of the uniform chain (nem_ff.hpp): 0 off, 1 on, -1 auto
    // auto: on from 256 organisms (below that the chain is mostly the small-binade prefix that is stepped anyway
    // and the table build is pure overhead).  Measured on MI355X: 20k x 500 on par with plain stepping
    // (latency-bound, one wave per SIMD), 50k x 1000 1.7x, 200k x 5000 9x faster.
    // parameter update folded into the density launch: per-organism dispersions (skd) and one dispersion per class
    // (sk_).  Where InerToDispK_'s d-ordered sums can round (N*D > 2^24) every block redoes the two D-step chains
    // -- at most 1024 steps, 4.4 us, in parallel in all blocks -- which is still cheaper than k_finish's launch.
    bool fused_update() const
    {
        return d <= kFusedMaxD && (cfg.disper == NEMGPU_DISP_KD || cfg.disper == NEMGPU_DISP_K_);
    }
    bool use_ff() const { return ff_mode < 0 ? d >= 256 : ff_mode != 0; }
    // the fused density kernels walk the fast-forwarded chain lane by lane and cross binades in batches (chain_ff_batched);
    // NEM_MI355X_FF_BATCH=0: word by word, as every other density kernel does
    bool ff_batch = true;
    // an NCEM round takes a site's label from the unnormalised row where the maximum is clear (nem_map.hpp);
    // NEM_MI355X_MAP_MARGIN=0: every row is normalised
    bool map_margin = true;
    // a kernel's FLAG_FAULT seen on the host (cleared, device word included, by the next reset / restart);
    // fault_inject: NEM_MI355X_FAULT_INJECT=fuzzy_pc makes one producer of k_mstep_fuzzy_pc skip a hand-over (tests)
    bool fault_seen = false; int fault_inject = 0;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // nemgpu_profile_density
    hipEvent_t ev_flags = nullptr;             // libc_init_one_wait: the flag block has reached the host
    bool defer_layout = false, layout_pending = false;   // nemgpu_solve_many: the device layouts are made by the group's run (zipped)
    hipEvent_t ready_ev = nullptr;             // nemgpu_solve_many: recorded behind the engine's uploads on its builder's stream,
    bool ready_pending = false;                // which carries other engines' uploads too -- a run waits for the event, not the stream

    // Device memory comes from a few large zeroed chunks (one hipMalloc + one fill each) that buffers are carved
    // from and that live as long as the engine: a nem() call creates and destroys an engine, and ~50 hipMalloc /
    // fill / hipFree triples were a fifth of its time at configs[1].
    struct Chunk { char* base; size_t size, used; bool owned = true; };
    std::vector<Chunk> chunks;
    int shared_chunk = -1;                     // the chunk small buffers are carved from
    uint8_t* best_lab = nullptr; float* best_c = nullptr;   // nemgpu_run_random: the best start's partition
    uint32_t* xf_stage = nullptr;                            // nemgpu_set_matrix_bits: upload staging (small matrices)
    bool ctrl_pending = false; CtrlArgs ctrl_deferred{};     // loop control left to the next iteration's counts launch
    // lock-step batches (iterate_many): a state-only twin of another engine -- matrix, graph and draw table are the
    // parent's, everything it allocates is carved from a slab the parent owns
    nemgpu_engine* parent = nullptr;
    bool carve_all = false;
    bool dry_run = false; size_t dry_bytes = 0;               // dev_alloc only adds up what it would carve
    std::vector<nemgpu_engine*> clones;                      // random starts in lock step: state-only twins of this engine
    char* clone_slab = nullptr; int* clone_flags_host = nullptr; float* clone_par0 = nullptr; size_t clone_bytes = 0;
    bool flags_host_borrowed = false;
    size_t clone_slab_size = 0, clone_flags_size = 0, flags_host_size = 0;   // real sizes of the pooled blocks
    // What the lead engine of a lock-step batch works with: the slab the members' argument blocks go through, the
    // area their flag blocks are gathered in, and the launch sequences captured so far (they hold the slabs'
    // addresses).  It belongs to the device, not to the engine: a lead takes one from the device's pool and hands it
    // back when it is destroyed, so the next group of problems of the same shape REPLAYS the graphs this one captured.
    // (the graphs' desc: kernel, variant, members, strides, grids, slab offsets; the lead's host state is not theirs)
    struct ZipContext {
        char* zip_host = nullptr; char* zip_dev = nullptr; size_t zip_cap = 0;
        int* zip_flags_host = nullptr; int* zip_flags_dev = nullptr; size_t zip_flags_cap = 0;
        size_t zip_host_size = 0, zip_dev_size = 0, zip_flags_host_size = 0, zip_flags_dev_size = 0;
        GraphCache zip_graphs{64, false, false};
    };
    ZipContext* zc = nullptr;
    // a rank alone in the sharded EM (no collective inside a batch): its batches as hipGraphs of the library's own,
    // captured the second time a shape is enqueued (nemgpu_shard_enqueue_batch)
    GraphCache shard_graphs{64, true, false};

    // Missing cells (nemgpu_set_observed_bits): the observed mask in the matrix's three layouts, the observed counts per
    // (class, organism) as the masked M-step takes them (ints) and as the reference keeps them (NbObs_KD, floats), and the
    // upload staging.  has_obs sends do_density / do_mstep to the kernels of nem_missing.hip and iterate() to
    // iterate_stepwise; without it nothing below is touched.
    bool has_obs = false;
    uint32_t *ow = nullptr, *ows = nullptr, *obs_stage = nullptr;
    uint64_t* ot = nullptr;
    int* obs_stats = nullptr;
    float* nbobs_kd = nullptr;

    bool ncem() const { return cfg.algo == NEMGPU_ALGO_NCEM; }
    int* ctrl() const { return flags_dev; }
    int* iter_flags() const { return flags_dev + C_WORDS + (size_t)fset * kFlagSetWords; }
    int* round_flags(int r) const { return iter_flags() + FLAG_ITER_STRIDE + (r % kRoundCap) * FLAG_ROUND_STRIDE; }
    size_t flag_words() const { return C_WORDS + (size_t)flag_sets * kFlagSetWords; }   // what the host mirrors
    const int* h_ctrl() const { return flags_host; }
    const int* h_iter() const { return flags_host + C_WORDS + (size_t)fset * kFlagSetWords; }
    const int* h_round(int r) const { return h_iter() + FLAG_ITER_STRIDE + (r % kRoundCap) * FLAG_ROUND_STRIDE; }
};

// nemgpu_resamples_solve: where every lock-step group's runs are reduced to their P/S/C/U counts (nem_resample.hpp)
struct ResampleTally {
    int device = 0;
    hipStream_t stream = nullptr;
    nemk::VoteDesc* desc = nullptr;                   // [kTallyGroupCap]
    uint8_t* maps = nullptr;                          // [kTallyGroupCap][kVoteMapStride]
    int32_t* stats = nullptr;                         // [count][kResampleStats], row = the sample's index in the call
};
constexpr int kTallyGroupCap = 256;                   // (solve_many_one's largest lock-step group)
// what nemgpu_solve_chunks hands to the builders of nemgpu_solve_many's pipeline instead of host matrices and graphs
struct ChunkSource {
    const nemgpu_master* master = nullptr;
    const nemk::ChunkPlan* plans = nullptr;           // host copies (device pointers inside), one per problem
    const int* nnz = nullptr;                         // directed edges of each chunk's graph
    uint8_t* const* labels = nullptr;                 // per problem: where the NCEM labels go (or null)
    nemgpu_votes* votes = nullptr;                    // (nemgpu_votes_solve) every group's runs voted on the device ...
    const int* slot = nullptr;                        // ... problem i into row slot[i] of the vote matrix
    ResampleTally* tally = nullptr;                   // (nemgpu_resamples_solve) every group's runs counted into stats[slot[i]]
};
// The vote over the samples of partition()'s loop for one master and one organism selection (nem_vote.hpp): the
// counts stay on the device, a batch of samples goes through a vote matrix of `batch` rows.
struct nemgpu_votes {
    const nemgpu_master* master = nullptr;
    int device = 0, n = 0, d_sel = 0, chunk_size = 0, batch = 0;
    double quotient = 0.0;                            // len(organisms) / chunk_size, as Python divides
    int64_t samples_voted = 0;
    bool done = false;                                // every family of the pangenome validated
    hipStream_t stream = nullptr;
    char* block = nullptr;                            // cnt | st | first | V | maps | desc | words
    nemk::VoteState state{};
    uint8_t* V = nullptr;
    uint8_t* maps = nullptr;
    nemk::VoteDesc* desc = nullptr;
    int* words = nullptr;
    int* words_host = nullptr;                        // (pinned)
};

namespace {

// Every memory operation of an engine is ordered on ITS stream (a non-blocking one) and never touches the legacy
// default stream: several engines may run on different host threads at once (pangenomenem_amd/batch.py), and a
// legacy-stream operation of one thread would collide with a graph capture in progress on another.
thread_local hipStream_t g_alloc_stream = nullptr;      // stream of the engine whose buffers are being allocated
thread_local nemgpu_engine* g_alloc_engine = nullptr;   // ... and the engine itself (owner of the chunks)
void alloc_for(nemgpu_engine* e) { g_alloc_engine = e; g_alloc_stream = e->stream; }

// What an engine needs before it can do anything -- a stream, device memory, the pinned block the loop control is
// copied to -- costs ~2 ms to create and up to 2 ms to release (hipFree waits for the whole device, other engines'
// work included): what a destroyed engine held is kept in a per-device pool and handed to the next engines on that
// device (PPanGGOLiN calls nem() once per chunk of organisms, each call creating and destroying an engine; a
// lock-step batch has tens of engines alive at once).  The pool keeps up to NEM_MI355X_POOL_MB (default 8192) of
// device memory per device; nemgpu_release_cached() frees everything it holds.
struct ResourcePool {
    std::mutex m;
    std::vector<hipStream_t> streams;
    std::vector<hipStream_t> run_streams;                   // highest priority (nemgpu_solve_many's lock-step runs)
    std::multimap<size_t, char*> dev, pinned;
    size_t dev_bytes = 0, pinned_bytes = 0;
    std::vector<nemgpu_engine::ZipContext*> zips;           // lock-step contexts (slabs + captured graphs), most recent last
};
constexpr int kPoolDevices = 64;
constexpr size_t kPoolStreams = 256, kPoolPinnedBytes = (size_t)512 << 20;
ResourcePool* g_pools = new ResourcePool[kPoolDevices];     // (never destroyed: engines may outlive static destructors)
size_t pool_dev_cap()
{
    static const size_t cap = [] {
        const char* g = getenv("NEM_MI355X_POOL_MB");
        return (size_t)(g ? std::max(0ll, atoll(g)) : 8192ll) << 20;
    }();
    return cap;
}
size_t pool_round(size_t bytes)
{
    const size_t g = bytes >= ((size_t)1 << 20) ? ((size_t)1 << 20) : ((size_t)64 << 10);
    return (std::max<size_t>(bytes, 1) + g - 1) / g * g;
}
static std::atomic<long long> g_pool_miss[2], g_pool_spill[2];   // NEM_MI355X_BATCH_PROF: blocks allocated / freed for real (device, pinned)
// a block of at least `bytes` (at most a quarter more) from the pool, else a new one; *got = its real size
hipError_t pool_get(int device, bool pinned, size_t bytes, char** out, size_t* got)
{
    const size_t want = pool_round(bytes);
    if (device >= 0 && device < kPoolDevices) {
        ResourcePool& P = g_pools[device];
        std::lock_guard<std::mutex> lock(P.m);
        auto& M = pinned ? P.pinned : P.dev;
        auto it = M.lower_bound(want);
        if (it != M.end() && it->first <= want + want / 4) {
            *out = it->second; *got = it->first;
            (pinned ? P.pinned_bytes : P.dev_bytes) -= it->first;
            M.erase(it);
            return hipSuccess;
        }
    }
    *got = want;
    g_pool_miss[pinned ? 1 : 0]++;
    hipError_t err = pinned ? hipHostMalloc((void**)out, want) : hipMalloc((void**)out, want);
    if (err != hipSuccess) {                             // out of memory with blocks idle in the pool: give them back
        (void)hipGetLastError();
        nemgpu_release_cached();
        err = pinned ? hipHostMalloc((void**)out, want) : hipMalloc((void**)out, want);
    }
    if (err != hipSuccess) *out = nullptr;
    return err;
}
void pool_put(int device, bool pinned, char* ptr, size_t size)
{
    if (!ptr) return;
    if (device >= 0 && device < kPoolDevices && size > 0) {
        ResourcePool& P = g_pools[device];
        std::lock_guard<std::mutex> lock(P.m);
        size_t& held = pinned ? P.pinned_bytes : P.dev_bytes;
        if (held + size <= (pinned ? kPoolPinnedBytes : pool_dev_cap())) {
            (pinned ? P.pinned : P.dev).emplace(size, ptr);
            held += size;
            return;
        }
    }
    g_pool_spill[pinned ? 1 : 0]++;
    if (pinned) (void)hipHostFree(ptr); else (void)hipFree(ptr);
}
// an engine's blocks in one visit to the pool (a destroyed engine gives back about ten: with 8-16 threads destroying
// the members of a finished group at once, a lock per block was 0.1-0.25 ms per engine in lock hand-overs)
struct PoolBlock { bool pinned; char* ptr; size_t size; };
void pool_put_many(int device, std::vector<PoolBlock>& blocks)
{
    std::vector<PoolBlock> spill;
    if (device >= 0 && device < kPoolDevices) {
        ResourcePool& P = g_pools[device];
        std::lock_guard<std::mutex> lock(P.m);
        for (const PoolBlock& b : blocks) {
            if (!b.ptr) continue;
            size_t& held = b.pinned ? P.pinned_bytes : P.dev_bytes;
            if (b.size > 0 && held + b.size <= (b.pinned ? kPoolPinnedBytes : pool_dev_cap())) {
                (b.pinned ? P.pinned : P.dev).emplace(b.size, b.ptr);
                held += b.size;
            } else spill.push_back(b);
        }
    } else spill = blocks;
    for (const PoolBlock& b : spill) if (b.ptr) { g_pool_spill[b.pinned ? 1 : 0]++; if (b.pinned) (void)hipHostFree(b.ptr); else (void)hipFree(b.ptr); }
    blocks.clear();
}
void release_staging(nemgpu_engine* e);
void zip_context_release(nemgpu_engine* lead);
// a non-blocking stream from the device's pool (creating one costs ~6 ms on this stack, destroying one ~2 ms)
hipError_t pool_stream_get(int device, hipStream_t* out)
{
    *out = nullptr;
    if (device >= 0 && device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[device].m);
        if (!g_pools[device].streams.empty()) { *out = g_pools[device].streams.back(); g_pools[device].streams.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
void pool_stream_put(int device, hipStream_t s)             // (idle)
{
    if (!s) return;
    if (device >= 0 && device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[device].m);
        if (g_pools[device].streams.size() < kPoolStreams) { g_pools[device].streams.push_back(s); return; }
    }
    (void)hipStreamDestroy(s);
}
// The stream of nemgpu_solve_many's lock-step runs: of the highest priority the device offers.  A run is a chain of ~45
// dependent launches; on a plain stream every one of them queued behind whatever the builders' streams had in flight
// (16 MB fills, layout kernels, uploads) and a group took 2-2.4 ms next to the builders against 0.9 ms alone.
hipError_t pool_run_stream_get(int device, hipStream_t* out)
{
    *out = nullptr;
    if (device >= 0 && device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[device].m);
        auto& v = g_pools[device].run_streams;
        if (!v.empty()) { *out = v.back(); v.pop_back(); return hipSuccess; }
    }
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
    return hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
}
void pool_run_stream_put(int device, hipStream_t s)         // (idle)
{
    if (!s) return;
    if (device >= 0 && device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[device].m);
        if (g_pools[device].run_streams.size() < 16) { g_pools[device].run_streams.push_back(s); return; }
    }
    (void)hipStreamDestroy(s);
}
constexpr size_t kStageMax = (size_t)64 << 20;          // larger uploads take the blocking path from the caller's memory
// a pinned block the engine owns until its next release_staging() -- the source of an asynchronous upload
char* stage(nemgpu_engine* e, size_t bytes)
{
    if (bytes > kStageMax) return nullptr;
    if (e->staging.size() >= 32) {                       // (an engine whose inputs are replaced over and over)
        if (hipStreamSynchronize(e->stream) != hipSuccess) return nullptr;
        release_staging(e);
    }
    char* p = nullptr; size_t got = 0;
    if (pool_get(e->device, true, bytes, &p, &got) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    e->staging.push_back({p, got});
    return p;
}
nemgpu_engine::ZipContext* zip_context(nemgpu_engine* lead)
{
    if (lead->zc) return lead->zc;
    if (lead->device >= 0 && lead->device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[lead->device].m);
        auto& Z = g_pools[lead->device].zips;
        if (!Z.empty()) { lead->zc = Z.back(); Z.pop_back(); }
    }
    if (!lead->zc) lead->zc = new nemgpu_engine::ZipContext();
    return lead->zc;
}
void zip_context_free(int device, nemgpu_engine::ZipContext* z)
{
    z->zip_graphs.clear();
    pool_put(device, true, z->zip_host, z->zip_host_size);
    pool_put(device, false, z->zip_dev, z->zip_dev_size);
    pool_put(device, true, (char*)z->zip_flags_host, z->zip_flags_host_size);
    pool_put(device, false, (char*)z->zip_flags_dev, z->zip_flags_dev_size);
    delete z;
}
void zip_context_release(nemgpu_engine* lead)           // (the lead's stream is idle)
{
    nemgpu_engine::ZipContext* z = lead->zc;
    if (!z) return;
    lead->zc = nullptr;
    if (lead->device >= 0 && lead->device < kPoolDevices) {
        std::lock_guard<std::mutex> lock(g_pools[lead->device].m);
        if (g_pools[lead->device].zips.size() < 8) { g_pools[lead->device].zips.push_back(z); return; }
    }
    zip_context_free(lead->device, z);
}
void release_staging(nemgpu_engine* e)                  // (the caller has waited for the stream)
{
    for (const nemgpu_engine::Staged& st : e->staging) pool_put(e->device, true, st.p, st.size);
    e->staging.clear();
}

// A forked child inherits a HIP runtime it cannot use (and handles parked by its parent that mean nothing to it).
// PPanGGOLiN's multiprocessing.Pool forks (ppanggolin.py:1039): if the parent has already run nem(), the workers must
// be started with the spawn / forkserver method -- a child of a GPU-using parent fails fast here instead of hanging.
std::atomic<bool> g_hip_used{false}, g_forked_after_hip{false};
std::once_flag g_atfork_once;
void atfork_child()
{
    if (g_hip_used.load()) g_forked_after_hip.store(true);
    g_pools = new ResourcePool[kPoolDevices];               // the parent's handles: leaked on purpose, never touched
}

constexpr size_t kChunkShared = (size_t)16 << 20;       // small buffers share 16 MB chunks
constexpr size_t kChunkOwn = (size_t)4 << 20;           // from 4 MB on a buffer gets a chunk of its own

int chunk_new(nemgpu_engine* e, size_t bytes)
{
    char* base = nullptr;
    size_t got = 0;
    HIPCHK(pool_get(e->device, false, bytes, &base, &got));
    e->chunks.push_back({base, got, 0});
    HIPCHK(hipMemsetAsync(base, 0, got, g_alloc_stream));     // (every later use is on the same stream)
    return NEMGPU_OK;
}

// zeroed device memory that lives until the engine is destroyed
template <typename T>
int dev_alloc(T** p, size_t count)
{
    *p = nullptr;
    nemgpu_engine* e = g_alloc_engine;
    if (e == nullptr) { set_error("dev_alloc outside an engine"); return NEMGPU_E_FUNCARG; }
    if (count == 0) count = 1;
    const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    if (e->dry_run) { e->dry_bytes += bytes; *p = reinterpret_cast<T*>((uintptr_t)256); return NEMGPU_OK; }
    int r;
    if (e->carve_all && e->shared_chunk >= 0 && e->chunks[e->shared_chunk].size - e->chunks[e->shared_chunk].used >= bytes) {
        nemgpu_engine::Chunk& c = e->chunks[e->shared_chunk];
        *p = reinterpret_cast<T*>(c.base + c.used);
        c.used += bytes;
        return NEMGPU_OK;
    }
    if (bytes >= kChunkOwn) {
        if ((r = chunk_new(e, bytes))) return r;
        e->chunks.back().used = bytes;
        *p = reinterpret_cast<T*>(e->chunks.back().base);
        return NEMGPU_OK;
    }
    if (e->shared_chunk < 0 || e->chunks[e->shared_chunk].size - e->chunks[e->shared_chunk].used < bytes) {
        if ((r = chunk_new(e, kChunkShared))) return r;
        e->shared_chunk = (int)e->chunks.size() - 1;
    }
    nemgpu_engine::Chunk& c = e->chunks[e->shared_chunk];
    *p = reinterpret_cast<T*>(c.base + c.used);
    c.used += bytes;
    return NEMGPU_OK;
}

// blocking copy on the engine's stream
hipError_t copy_sync(nemgpu_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
void drop_graphs(nemgpu_engine* e);

// everything an engine owns besides the matrix layouts and the graph: parameters, tables, densities, masks, flags
int alloc_model_buffers(nemgpu_engine* e)
{
    const int k = e->k;
    const size_t kd = (size_t)k * e->d, kdp = (size_t)k * e->dpad;
    int r = NEMGPU_OK;
    auto A = [&](int rr) { if (r == NEMGPU_OK) r = rr; };
    {
        auto a64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
        e->par_o_center = a64((size_t)k); e->par_o_disp = e->par_o_center + a64(kd); e->par_o_nb = e->par_o_disp + a64(kd);
        e->par_words = e->par_o_nb + a64((size_t)k);
        float* pb = nullptr;
        A(dev_alloc(&pb, e->par_words));
        e->prop = pb; e->center = pb + e->par_o_center; e->disp = pb + e->par_o_disp; e->nbobs_k = pb + e->par_o_nb;
        if (e->parent == nullptr) {
            float* p0 = nullptr;
            A(dev_alloc(&p0, e->par_words));
            e->prop0 = p0; e->center0 = p0 + e->par_o_center; e->disp0 = p0 + e->par_o_disp;
        }
    }
    A(dev_alloc(&e->iner, kd));
    A(dev_alloc(&e->tabT, kdp)); A(dev_alloc(&e->tabL0, kdp));
    A(dev_alloc(&e->nz0, (size_t)k * e->W)); A(dev_alloc(&e->nz1, (size_t)k * e->W));
    A(dev_alloc(&e->am0, (size_t)k * e->W)); A(dev_alloc(&e->am1, (size_t)k * e->W));
    A(dev_alloc(&e->ffq, (size_t)k * 256));
    A(dev_alloc(&e->uni, (size_t)k)); A(dev_alloc(&e->nonuni, (size_t)k)); A(dev_alloc(&e->sweep_next, (size_t)32 + kTicketWords));   // [0] sweep number, [32..] last-block ticket counters
    A(dev_alloc(&e->pk, (size_t)k)); A(dev_alloc(&e->logpk, (size_t)k));
    A(dev_alloc(&e->pkfki, (size_t)k * e->npad)); A(dev_alloc(&e->logpkfki, (size_t)k * e->npad));
    e->par_copy[0] = e->prop; e->pkfki_copy[0] = e->pkfki; e->logpkfki_copy[0] = e->logpkfki;
    for (int c = 1; c < e->flag_sets; c++) {
        A(dev_alloc(&e->par_copy[c], e->par_words));
        A(dev_alloc(&e->pkfki_copy[c], (size_t)k * e->npad)); A(dev_alloc(&e->logpkfki_copy[c], (size_t)k * e->npad));
    }
    A(dev_alloc(&e->mask, (size_t)k * e->nw64));
    A(dev_alloc(&e->stats, (size_t)k + kd));
    e->stats_slot[0] = e->stats; e->stats_last = e->stats;
    if (e->flag_sets == 3 && e->round_counts) A(dev_alloc(&e->stats_slot[1], (size_t)k + kd));
    A(dev_alloc(&e->flags_dev, e->flag_words()));
    return r;
}

int ensure_state_buffers(nemgpu_engine* e)
{
    alloc_for(e);
    if (e->ncem()) {
        for (int b = 0; b < 3; b++)
            if (!e->lab[b]) { int r = dev_alloc(&e->lab[b], (size_t)e->n_total); if (r) return r; }
        for (int b = 0; b < 3; b++)
            if (!e->tie_cnt[b]) { int r = dev_alloc(&e->tie_cnt[b], (size_t)e->n / 256 + 2); if (r) return r; }
    } else {
        for (int b = 0; b < 3; b++)
            if (!e->cbuf[b]) { int r = dev_alloc(&e->cbuf[b], (size_t)e->n_total * e->k); if (r) return r; }
        if (!e->fz_in0) {
            size_t kd = (size_t)e->k * e->d;
            int r;
            if ((r = dev_alloc(&e->fz_in0, kd))) return r;
            if ((r = dev_alloc(&e->fz_in1, kd))) return r;
            if ((r = dev_alloc(&e->fz_inh, (size_t)e->k))) return r;
            if ((r = dev_alloc(&e->fz_lastz, kd))) return r;
            if ((r = dev_alloc(&e->fz_any1, kd))) return r;
            if ((r = dev_alloc(&e->fz_ct, (size_t)e->k * ((size_t)(e->n + 1023) / 1024 * 1024)))) return r;   // [k][n up to whole 1024-family windows]
            if ((r = dev_alloc(&e->fz_chk, (size_t)e->k * ((size_t)(e->n + 63) / 64 + 1) * ((size_t)(e->d + 63) / 64 * 64)))) return r;
        }
    }
    return NEMGPU_OK;
}

hipError_t copy_sync(nemgpu_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    hipError_t err = hipMemcpyAsync(dst, src, bytes, kind, e->stream);
    if (err != hipSuccess) return err;
    return hipStreamSynchronize(e->stream);
}

// the iteration flags are on the host: did a kernel report that it could not finish its work?
int check_fault(nemgpu_engine* e)
{
    if (e->h_iter()[FLAG_FAULT] == 0) return NEMGPU_OK;
    e->fault_seen = true;
    set_error("internal: a kernel reported a fault (a producer/consumer hand-over of the fuzzy M-step never completed); "
              "the results of this call are not to be used");
    return NEMGPU_E_INTERNAL;
}
int clear_fault(nemgpu_engine* e)
{
    if (!e->fault_seen) return NEMGPU_OK;
    e->fault_seen = false;
    e->flags_host[C_WORDS + FLAG_FAULT] = 0;
    HIPCHK(hipMemsetAsync(e->iter_flags() + FLAG_FAULT, 0, sizeof(int), e->stream));
    return NEMGPU_OK;
}

// ---- the kernels' argument blocks: each is made HERE, once, from the engine, and a caller adds only what is its own.
// FinishArgs: finish_args, restart_head, shard_stats.  SweepArgs: sweep_args (buffers, flag slot, post / hold / blind,
// shard and draw fields are the callers').  CtrlArgs: ctrl_args.  The density launchers: density_io; density_launch and
// finish_launch also set the host flags that go with their launch.
// The smaller kernels: counts_args, fuzzy_args, labels_post_args, conv_fuzzy_args, crit_args, layout_args.
FinishArgs finish_args(nemgpu_engine* e, int mode, const int* stats)
{
    FinishArgs t;
    t.mode = mode; t.K = e->k; t.D = e->d; t.dpad = e->dpad; t.n_total = e->n_true; t.disper = e->cfg.disper; t.propor = e->cfg.propor;
    t.stats = stats; t.stats_ranks = 1; t.stats_rank_stride = 0;
    t.prop = e->prop; t.center = e->center; t.disp = e->disp; t.nbobs_k = e->nbobs_k; t.iner = e->iner;
    t.tabT = e->tabT; t.tabL0 = e->tabL0; t.nz0 = e->nz0; t.nz1 = e->nz1;
    t.am0 = e->am0; t.am1 = e->am1; t.uni = e->uni; t.nonuni = e->nonuni;
    t.pk = e->pk; t.logpk = e->logpk; t.flags = e->iter_flags(); t.stop = e->stop_ptr;
    t.reset_prop = nullptr; t.reset_center = nullptr; t.reset_disp = nullptr; t.reset_ctrl = nullptr; t.reset_ctrl_words = 0; t.reset_sweep_next = nullptr;
    t.prev_center = nullptr; t.prev_disp = nullptr; t.zero_stats = nullptr; t.n_zero_stats = 0;
    t.use_ff = !e->use_ff() ? FF_OFF : e->ff_batch ? FF_BATCHED : FF_WORD; t.perm = e->perm; t.ffq = e->ffq;
    return t;
}
// the head of a restart: the initial parameters back in place, loop control and sweep counter cleared
void restart_head(nemgpu_engine* e, FinishArgs& t)
{
    t.reset_prop = e->prop0; t.reset_center = e->center0; t.reset_disp = e->disp0;
    t.reset_ctrl = e->ctrl(); t.reset_ctrl_words = C_WORDS; t.reset_sweep_next = e->sweep_next;
}
// sharded: the statistics are every rank's partial counts, in the tails of the gathered label blocks
void shard_stats(const nemgpu_engine* e, FinishArgs& t) { t.stats_ranks = e->sh_world; t.stats_rank_stride = e->sh_stride / 4; }
// what every round of a sweep shares, made in place (a recorder's member makes one per sweep: no copy of the block).
// on_device: the sweep's number is read from e->sweep_next (pipelined loop), not `id`
void sweep_args(const nemgpu_engine* e, SweepArgs& a, float beta, uint32_t id, bool on_device = false)
{
    a = SweepArgs{};
    a.n_local = e->n; a.lo = e->lo; a.n_total = e->n_total; a.K = e->k; a.npad = e->npad;
    a.use_nei = (e->has_graph && beta != 0.0f) ? 1 : 0; a.nei_ptr = e->nei_ptr; a.nei_idx = e->nei_idx; a.nei_w = e->nei_w;
    a.beta = beta; a.pkfki = e->pkfki;
    a.tie_rule = e->cfg.tie_rule; a.tie_seed = e->cfg.tie_seed; a.map_full = e->map_margin ? 0 : 1;
    a.sweep_id = id; a.sweep_id_ptr = on_device ? e->sweep_next : nullptr;
}
// the loop control behind a sweep of n_rounds enqueued rounds.  A sweep is verified (use_nei) when its sites are coupled:
// through the graph, or through the reference's tie stream
CtrlArgs ctrl_args(nemgpu_engine* e, int n_rounds, float beta)
{
    CtrlArgs ca{};
    ca.ctrl = e->ctrl(); ca.iter_flags = e->iter_flags(); ca.round0 = e->round_flags(0); ca.n_rounds = n_rounds;
    ca.param_fix = e->cfg.param_fix; ca.use_nei = ((e->has_graph && beta != 0.0f) || e->libc()) ? 1 : 0; ca.cvtest = e->cfg.cvtest;
    ca.ncem = e->ncem() ? 1 : 0; ca.cvthres = e->cfg.cvthres; ca.sweep_next = e->sweep_next; ca.ticket = e->sweep_next + 32;
    ca.draw_ctl = e->libc() ? e->draw_ctl : nullptr;
    return ca;
}
CountsArgs counts_args(const nemgpu_engine* e, int* stats, const CtrlArgs* prev_ctrl)
{
    CountsArgs a{};
    a.K = e->k; a.D = e->d; a.nw64 = e->nw64; a.xt = e->xt; a.mask = e->mask; a.stats = stats; a.stop = e->stop_ptr;
    if (prev_ctrl != nullptr) a.prev_ctrl = *prev_ctrl;
    return a;
}
// c: memberships [n_total][K] (this engine's rows are read); ctpad is the launch wrapper's
FuzzyArgs fuzzy_args(nemgpu_engine* e, const float* c, const int* stop)
{
    FuzzyArgs a{};
    a.n = e->n; a.npad = e->npad; a.K = e->k; a.D = e->d; a.xw = e->xw; a.xt = e->xt; a.nw64 = e->nw64;
    a.c = c + (size_t)e->lo * e->k; a.nbobs_k = e->nbobs_k; a.center = e->center; a.iner = e->iner; a.stop = stop;
    a.in0 = e->fz_in0; a.in1 = e->fz_in1; a.inh_k = e->fz_inh; a.lastz = e->fz_lastz; a.any1 = e->fz_any1;
    a.ct = e->fz_ct; a.chk = e->fz_chk; a.fault = e->iter_flags() + FLAG_FAULT; a.inject = e->fault_inject;
    return a;
}
LabelsPostArgs labels_post_args(nemgpu_engine* e, const uint8_t* lab_new, const uint8_t* lab_old, const CtrlArgs* ctrl)
{
    LabelsPostArgs a{};
    a.lo = e->lo; a.n_local = e->n; a.K = e->k; a.nw64 = e->nw64; a.lab_new = lab_new; a.lab_old = lab_old;
    a.mask = e->mask; a.flags = e->iter_flags(); a.stop = e->stop_ptr;
    if (ctrl != nullptr) a.ca = *ctrl;
    return a;
}
// c_new, c_old: memberships [n_total][K] (this engine's rows are compared)
ConvFuzzyArgs conv_fuzzy_args(nemgpu_engine* e, const float* c_new, const float* c_old, const int* stop, const CtrlArgs* ctrl)
{
    ConvFuzzyArgs a{};
    a.m = (size_t)e->n * e->k; a.c = c_new + (size_t)e->lo * e->k; a.cold = c_old + (size_t)e->lo * e->k;
    a.thres = e->cfg.cvthres; a.flags = e->iter_flags(); a.stop = stop;
    if (ctrl != nullptr) a.ca = *ctrl;
    return a;
}
// c: memberships or one-hot rows [n][K]; second: the evaluation writes the crit2_* set of buffers
CritArgs crit_args(const nemgpu_engine* e, const float* c, bool second)
{
    CritArgs a{};
    a.n = e->n; a.K = e->k; a.npad = e->npad; a.nei_ptr = e->nei_ptr; a.nei_idx = e->nei_idx; a.nei_w = e->nei_w;
    a.use_nei = e->has_graph ? 1 : 0; a.beta = e->cfg.beta; a.c = c; a.pkfki = e->pkfki; a.logpkfki = e->logpkfki;
    a.dik = second ? e->crit2_dik : e->crit_dik; a.gik = second ? e->crit2_gik : e->crit_gik;
    a.lfi = second ? e->crit2_lfi : e->crit_lfi; a.lzi = second ? e->crit2_lzi : e->crit_lzi;
    a.crit6 = second ? e->crit2_6 : e->crit6_dev; a.hard = e->ncem() ? 1 : 0;
    return a;
}
// xf: the uploaded family-major bit matrix
LayoutArgs layout_args(const nemgpu_engine* e, const uint32_t* xf)
{
    return LayoutArgs{xf, e->perm, e->n, e->wf, e->W, e->npad, e->d, e->nw64, e->xw, e->xws, e->xt};
}
DensityIO density_io(nemgpu_engine* e)
{
    return DensityIO{e->xws, e->n, e->npad, e->pkfki, e->logpkfki, e->iter_flags() + FLAG_MOVED, kSweepFlagWords};
}
// k_finish and the host flags behind it: the tables are those of the parameters now in place, the densities are not
void finish_launch(nemgpu_engine* e, const FinishArgs& t) { launch_finish(t, e->stream); e->tables_fresh = true; e->density_fresh = false; }
// A density launch that derives the parameters itself: with a held sweep round beside it (held), as the start of a run (t
// carries the restart head), else fused.  None rebuilds the table buffers.  flags = false: the host flags stay (the probes)
void density_launch(nemgpu_engine* e, const FinishArgs& t, const SweepArgs* held = nullptr, bool flags = true)
{
    if (held != nullptr) launch_density_verify(t, density_io(e), *held, e->stream);
    else if (t.reset_prop != nullptr) launch_density_start(t, density_io(e), e->stream);
    else launch_density_fused(t, density_io(e), e->stream);
    if (flags) { e->flags_clean = true; e->tables_fresh = false; e->density_fresh = true; }
}

// density tables from the current parameters (k_finish mode 0); a no-op when they are up to date
int do_tables(nemgpu_engine* e)
{
    if (e->tables_fresh) return NEMGPU_OK;
    finish_launch(e, finish_args(e, 0, nullptr));
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// an engine with an observed mask: what cannot run on it says so before any launch
int masked_refuse(const nemgpu_engine* e, const char* who)
{
    if (!e->has_obs) return NEMGPU_OK;
    set_error(std::string(who) + ": the engine has an observed mask (missing cells); masked data runs NCEM through nemgpu_run, "
              "nemgpu_iterate, the logged runs and the single steps only");
    return NEMGPU_E_ARG;
}
int masked_algo_check(const nemgpu_engine* e)
{
    if (!e->has_obs || e->ncem()) return NEMGPU_OK;
    set_error("missing cells: only algo = ncem runs on an engine with an observed mask (the fuzzy M-step has no masked form)");
    return NEMGPU_E_ARG;
}

int do_density(nemgpu_engine* e)
{
    if (e->has_obs) launch_density_masked(finish_args(e, 0, nullptr), density_io(e), e->xw, e->ow, e->stream);
    else launch_density(finish_args(e, 0, nullptr), density_io(e), e->stream);
    HIPCHK(hipGetLastError());
    e->flags_clean = true;
    e->density_fresh = true;
    return NEMGPU_OK;
}

// One full Gauss-Seidel sweep == relaxation rounds until a round changes nothing.
// sweep_enqueue() launches the first batch of rounds without waiting; sweep_complete() reads the
// flags back (one D2H copy + sync), launches more rounds if the batch did not reach the fixed
// point, and reports whether it had to.  The new partition ends up in buffer (cur+1)%3 and `cur`
// is NOT advanced (the caller commits).
struct SweepCtx {
    SweepArgs a{};
    bool multi = false;  // the sweep needs verified relaxation rounds: it reads neighbours, or its ties share a draw stream
    int r = 0;           // rounds launched so far
    int checked = 0;     // rounds whose flags the host has examined
    int slot_base = 0;   // first flag slot of the round window (the blind initial sweep takes a slot of its own)
    // NCEM pipelined loop: fold the iteration's bookkeeping into the last round of the first batch
    bool post = false; bool post_moved = false; CtrlArgs post_ctrl{};
    // shadow-verify schedule: the last round of the first batch is not launched but left here, bookkeeping and loop
    // control included, for the next density launch; the round before it makes the class masks and "moved"
    SweepArgs* hold = nullptr;
    // ... and the round that makes the masks adds the M-step counts of its labels into this (zeroed) slot (nullptr: no)
    int* count_into = nullptr;
    // a start's beta sweep without a blind launch ahead of it (blind_fold_on): round 0 computes the blind labels it
    // needs, stores its own sites' into the sweep's old buffer and tallies into the blind sweep's flag slot (-1: no)
    int blind_slot = -1; uint32_t blind_id = 0;
};

int clear_sweep_flags(nemgpu_engine* e)
{
    if (current_recorder()) launch_fill(e->iter_flags() + FLAG_MOVED, kSweepFlagWords, 0, e->stream);
    else HIPCHK(hipMemsetAsync(e->iter_flags() + FLAG_MOVED, 0, kSweepFlagWords * sizeof(int), e->stream));
    e->flags_clean = true;
    return NEMGPU_OK;
}

// ---- TIE_LIBC: the reference's random() stream ------------------------------------------------
// The device reads draws from a table that covers a window of the stream; the host keeps the generator behind it.
// Makes draws [lo, lo + count) available (regenerating / sliding / growing the window as needed).
int ensure_draw_window(nemgpu_engine* e, long lo, long count)
{
    if (e->draw_valid && e->draw_tab0 <= lo && lo + count <= e->draw_tab0 + e->draw_cap) return NEMGPU_OK;
    if (e->draw_borrowed) {                                  // a twin that outgrew its parent's window gets a table of its own
        e->draw_borrowed = false; e->draw_valid = false; e->draw_tab = nullptr; e->draw_cap = 0;
    }
    long cap = std::max<long>(e->draw_cap, 1024);
    while (cap < 2 * count) cap *= 2;
    if (!e->draw_valid || lo < e->draw_tab0) {               // a new stream (seed / restart below the window)
        e->draw_gen.seed(e->cfg.tie_seed); e->draw_gen_pos = 0; e->draw_host.clear(); e->draw_tab0 = 0;
    }
    // slide the host window to start at lo
    const long have_end = e->draw_tab0 + (long)e->draw_host.size();
    if (lo >= have_end) {
        while (e->draw_gen_pos < lo) { (void)e->draw_gen.next(); e->draw_gen_pos++; }
        e->draw_host.clear();
    } else if (lo > e->draw_tab0) {
        e->draw_host.erase(e->draw_host.begin(), e->draw_host.begin() + (lo - e->draw_tab0));
    }
    e->draw_tab0 = lo;
    while ((long)e->draw_host.size() < cap) { e->draw_host.push_back((uint32_t)e->draw_gen.next()); e->draw_gen_pos++; }
    if (cap > e->draw_cap) {
        HIPCHK(hipStreamSynchronize(e->stream));
        alloc_for(e);
        int r = dev_alloc(&e->draw_tab, (size_t)cap);        // (a smaller table stays in its chunk until the engine goes)
        if (r) return r;
        e->draw_cap = (int)cap;
        drop_graphs(e);                                      // table pointer and length are kernel arguments
    }
    HIPCHK(hipMemcpyAsync(e->draw_tab, e->draw_host.data(), (size_t)e->draw_cap * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->draw_valid = true;
    return NEMGPU_OK;
}
long draw_need(const nemgpu_engine* e) { return e->tie_heavy ? 8l * e->n + 1024 : 1024; }

// one draw on the host (RandNemAlgo's MakeRandomPara shares the stream with the ties)
int host_draw(nemgpu_engine* e, uint32_t* out)
{
    int r = ensure_draw_window(e, e->draws, draw_need(e));
    if (r) return r;
    *out = e->draw_host[(size_t)(e->draws - e->draw_tab0)];
    e->draws++;
    return NEMGPU_OK;
}

// the draw-stream side of a sweep's arguments; by_value: the host knows how many draws were made (else the device does)
void sweep_draw_args(nemgpu_engine* e, SweepArgs& a, bool by_value)
{
    a.draw_tab = e->draw_tab; a.draw_tab_len = e->draw_cap;
    a.draw_base = e->draws; a.draw_tab0 = (int)e->draw_tab0;
    a.draw_ctl = by_value ? nullptr : e->draw_ctl;
    a.draw_extra = e->draw_extra_once; e->draw_extra_once = nullptr;
}
// the device words the pipelined loop reads the stream position from (outside any graph capture)
int publish_draw_ctl(nemgpu_engine* e)
{
    if (current_recorder()) {
        launch_fill(e->draw_ctl, 1, e->draws, e->stream);
        launch_fill(e->draw_ctl + 1, 1, (int)e->draw_tab0, e->stream);
        return NEMGPU_OK;
    }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->draw_ctl, e->draws, 1, e->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(e->draw_ctl + 1), (int)e->draw_tab0, 1, e->stream));
    return NEMGPU_OK;
}

int sweep_launch_rounds(nemgpu_engine* e, SweepCtx& c, int count)
{
    const bool ncem = e->ncem();
    const int P = e->cur, Q = (e->cur + 1) % 3, R = (e->cur + 2) % 3;
    const int r0 = c.r;
    for (int b = 0; b < count; b++, c.r++) {
        const int r = c.r;
        const int gb = (r == 0) ? P : ((r - 1) % 2 == 0 ? Q : R);
        const int ob = (r % 2 == 0) ? Q : R;
        if (ncem) {
            c.a.lab_old = e->lab[P]; c.a.lab_guess = e->lab[gb]; c.a.lab_out = e->lab[ob];
            c.a.tie_cnt_guess = e->tie_cnt[gb]; c.a.tie_cnt_out = e->tie_cnt[ob];
        } else { c.a.c_old = e->cbuf[P]; c.a.c_guess = e->cbuf[gb]; c.a.c_out = e->cbuf[ob]; }
        c.a.flags = e->round_flags(c.slot_base + r);
        c.a.fold_ticket = e->sweep_next + 32;
        c.a.prev_changed = (r == r0) ? nullptr : (e->round_flags(c.slot_base + r - 1) + FLAG_CHANGED);
        c.a.stop = e->stop_ptr;
        c.a.post_on = 0;
        c.a.post_stats = nullptr;
        const bool blind = ncem && c.blind_slot >= 0 && r == 0;    // (round 0 only: every later round reads the labels it wrote)
        c.a.blind_off = blind ? (int)(e->round_flags(c.blind_slot) - c.a.flags) : 0;   // (its guess and its old buffer are both P)
        c.a.blind_sweep_id = blind ? c.blind_id : 0u;
        if (c.hold != nullptr && c.post && ncem && r0 == 0 && count >= 2 && b >= count - 2) {
            c.a.post_on = 1; c.a.post_skip_guess = (r % 2 == 1) ? 1 : 0;
            c.a.post_nw64 = e->nw64; c.a.post_mask = e->mask; c.a.post_flags = e->iter_flags();
            if (b == count - 2) {
                // the masks and "moved" from this round's output: final whenever the next round changes nothing
                c.a.post_from_guess = 0; c.a.post_moved = c.post_moved ? 1 : 0; c.a.post_no_masks = 0; c.a.post_ctrl = CtrlArgs{};
                if (c.count_into != nullptr) { c.a.post_stats = c.count_into; c.a.post_xt = e->xt; c.a.post_D = e->d; }
            } else {
                // the verifying round: the loop control in its last-block ticket, nothing else
                c.a.post_from_guess = 1; c.a.post_moved = 0; c.a.post_no_masks = 1; c.a.post_ctrl = c.post_ctrl;
                *c.hold = c.a;
                continue;
            }
        } else if (c.post && ncem && r0 == 0 && b == count - 1) {
            // (the sweep's final labels are in buffer Q, the out buffer of even rounds)
            c.a.post_on = 1; c.a.post_from_guess = (r % 2 == 1) ? 1 : 0; c.a.post_moved = c.post_moved ? 1 : 0;
            c.a.post_skip_guess = c.a.post_from_guess;
            c.a.post_nw64 = e->nw64; c.a.post_mask = e->mask; c.a.post_flags = e->iter_flags(); c.a.post_ctrl = c.post_ctrl;
        }
        launch_sweep(c.a, ncem, e->stream);
    }
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// the arguments every round of one sweep shares (takes the sweep's number)
int sweep_setup(nemgpu_engine* e, float beta, SweepCtx& c, bool id_by_value)
{
    sweep_args(e, c.a, beta, e->sweep_counter++, e->stop_ptr != nullptr && !id_by_value);   // pipelined loop: the device keeps count
    c.multi = c.a.use_nei || e->libc();
    if (e->libc()) {
        if (e->stop_ptr == nullptr) { int r = ensure_draw_window(e, e->draws, draw_need(e)); if (r) return r; }
        sweep_draw_args(e, c.a, e->stop_ptr == nullptr);
    }
    return NEMGPU_OK;
}

// what a sweep_enqueue may ask for beyond the plain sweep (post_ctrl .. count_into: NCEM, as SweepCtx explains them)
struct SweepOpts {
    bool id_by_value = false;             // the sweep's number as an argument even inside the pipelined loop
    int slot_base = 0, rounds = 0;        // first flag slot of the round window; rounds to enqueue (0: round_batch)
    const CtrlArgs* post_ctrl = nullptr; bool post_moved = false; SweepArgs* hold = nullptr; int* count_into = nullptr;
};

int sweep_enqueue(nemgpu_engine* e, float beta, SweepCtx& c, const SweepOpts& o = SweepOpts())
{
    c = SweepCtx();
    c.slot_base = o.slot_base;
    c.blind_slot = e->blind_slot_once; c.blind_id = e->blind_id_once; e->blind_slot_once = -1;
    if (o.post_ctrl != nullptr && e->ncem()) {
        c.post = true; c.post_moved = o.post_moved; c.post_ctrl = *o.post_ctrl; c.hold = o.hold;
        c.count_into = o.hold != nullptr ? o.count_into : nullptr;
    }
    { int r = sweep_setup(e, beta, c, o.id_by_value); if (r) return r; }
    if (!e->flags_clean) { int r = clear_sweep_flags(e); if (r) return r; }
    e->flags_clean = false;
    return sweep_launch_rounds(e, c, c.multi ? (o.rounds > 0 ? o.rounds : e->round_batch) : 1);
}

// `extra` is set when rounds beyond the first batch were needed (work enqueued after the first
// batch read a partition that was not final yet and must be redone by the caller).
// `grow`: every further batch of rounds is as long as all the rounds before it (up to 16) instead of round_batch -- for
// sweeps whose need is long-tailed (the initial sweeps of a random start that ties at thousands of families).
int sweep_complete(nemgpu_engine* e, SweepCtx& c, int* rounds_out, bool* extra, bool flags_ready = false, bool grow = false)
{
    int done_at = -1;
    if (extra) *extra = false;
    for (;;) {
        if (!flags_ready) {                                  // (a lock-step batch has fetched every member's flags already)
            HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost,
                                  e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
        }
        flags_ready = false;
        { const int fr = check_fault(e); if (fr) return fr; }
        if (!c.multi) { done_at = 0; break; }
        bool tab_short = false;
        for (int q = c.checked; q < c.r; q++) {
            if (e->h_round(c.slot_base + q)[FLAG_CHANGED] == 0) { done_at = q; break; }
            if (e->h_round(c.slot_base + q)[FLAG_NTIES] & (1 << 30)) tab_short = true;
        }
        c.checked = c.r;
        if (done_at >= 0) break;
        if (extra) *extra = true;
        if (tab_short) {
            // a site needed a draw beyond the table: those rounds were void (they flagged a change).  From now on
            // the window covers whatever a batch of sweeps can draw.
            e->tie_heavy = true;
            int rr = ensure_draw_window(e, e->draws, draw_need(e));
            if (rr) return rr;
            sweep_draw_args(e, c.a, true);
        }
        const int more = grow ? std::min(16, std::max(e->round_batch, c.r % kRoundCap)) : e->round_batch;
        if (c.r % kRoundCap == 0 || c.r % kRoundCap + more > kRoundCap) {
            // the flag window is about to wrap: every earlier round has been examined, start a clean window
            // (keeps the parity of r, which selects the ping-pong buffers)
            HIPCHK(hipMemsetAsync(e->round_flags(0), 0, kRoundCap * FLAG_ROUND_STRIDE * sizeof(int), e->stream));
            while (c.r % kRoundCap != 0) c.r += 2;       // skip to the window start, same parity
            c.checked = c.r;
        }
        int rr = sweep_launch_rounds(e, c, more);
        if (rr) return rr;
    }
    // the round that changed nothing recomputed every site: its zero-density tally is the sweep's
    const int* f = e->h_round(c.slot_base + done_at);
    if (e->libc()) e->draws += f[FLAG_NTIES] & ((1 << 30) - 1);
    if (f[FLAG_NZERO] > 0) {
        e->zero_density += f[FLAG_NZERO];
        if (e->first_zero < 0) e->first_zero = e->n_total - f[FLAG_FIRSTZERO];
    }
    // result: the out buffer of round done_at; when that is R it equals Q bit for bit (see k_sweep)
    e->sweep_rounds += done_at + 1;
    if (rounds_out) *rounds_out = done_at + 1;
    return NEMGPU_OK;
}

int do_sweep(nemgpu_engine* e, float beta, int* rounds_out)
{
    SweepCtx c;
    int r = sweep_enqueue(e, beta, c);
    if (r) return r;
    return sweep_complete(e, c, rounds_out, nullptr);
}

int do_labels_post(nemgpu_engine* e, int newbuf, int oldbuf, const CtrlArgs* ctrl = nullptr)
{
    launch_labels_post(labels_post_args(e, e->lab[newbuf], oldbuf >= 0 ? e->lab[oldbuf] : nullptr, ctrl), e->stream);
    HIPCHK(hipGetLastError());
    e->masks_valid = true;
    return NEMGPU_OK;
}

// EstimPara (nem_mod.c:415-469) on the current partition; leaves FLAG_EMPTYK in the iteration flags.
int do_mstep(nemgpu_engine* e, const CtrlArgs* prev_ctrl = nullptr)
{
    if (e->has_obs) {
        // masked counts, the update with NbObs_KD = observed counts, then the tables of the new parameters (k_finish mode 0)
        { const int r = masked_algo_check(e); if (r) return r; }
        if (!e->masks_valid) { int r = do_labels_post(e, e->cur, -1); if (r) return r; }
        launch_mstep_counts_masked(CountsMaskedArgs{e->k, e->d, e->nw64, e->xt, e->ot, e->mask, e->stats, e->obs_stats}, e->stream);
        launch_finish_masked(FinishMaskedArgs{e->k, e->d, e->n_true, e->cfg.disper, e->cfg.propor, e->stats, e->obs_stats, e->prop,
                                              e->center, e->disp, e->nbobs_k, e->iner, e->nbobs_kd, e->iter_flags()}, e->stream);
        finish_launch(e, finish_args(e, 0, nullptr));
        e->stats_last = e->stats;
        HIPCHK(hipGetLastError());
        return NEMGPU_OK;
    }
    if (e->ncem()) {
        if (!e->masks_valid) { int r = do_labels_post(e, e->cur, -1); if (r) return r; }
        launch_mstep_counts(counts_args(e, e->stats, prev_ctrl), e->stream);
        finish_launch(e, finish_args(e, 1, e->stats));
        e->stats_last = e->stats;
    } else {
        launch_mstep_fuzzy(fuzzy_args(e, e->cbuf[e->cur], e->stop_ptr), e->stream);
        finish_launch(e, finish_args(e, 2, nullptr));
    }
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

int read_iter_flags(nemgpu_engine* e)
{
    HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, (C_WORDS + (size_t)e->fset * kFlagSetWords + FLAG_ITER_STRIDE) * sizeof(int),
                          hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return check_fault(e);
}

int reset_device(nemgpu_engine* e);
int reset_state(nemgpu_engine* e, bool lazy = false);
int flush_reset(nemgpu_engine* e);
int criteria_enqueue(nemgpu_engine* e, int buf, bool second = false);
void fill_result(nemgpu_engine* e, nemgpu_result* res);

// ComputePartitionFromPara(Needinit = 1), nem_alg.c:1967-1981
int init_partition(nemgpu_engine* e)
{
    int r;
    if (!e->have_matrix || !e->have_params) { set_error("matrix and parameters must be set first"); return NEMGPU_E_FUNCARG; }
    if ((r = masked_algo_check(e))) return r;
    if ((r = flush_reset(e))) return r;
    if ((r = ensure_state_buffers(e))) return r;
    if ((r = do_tables(e))) return r;
    if ((r = do_density(e))) return r;
    // ClassifM starts as zeros (calloc, nem_exe.c:524-526): the blind beta = 0 sweep never reads it
    if ((r = do_sweep(e, 0.0f, nullptr))) return r;                // blind sweep: one round, no neighbour reads
    e->cur = (e->cur + 1) % 3;
    if ((r = do_sweep(e, e->cfg.beta, nullptr))) return r;
    e->cur = (e->cur + 1) % 3;
    e->masks_valid = false;
    if (e->ncem()) { if ((r = do_labels_post(e, e->cur, -1))) return r; }
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->sweep_next, (int)e->sweep_counter, 1, e->stream));
    return NEMGPU_OK;
}

// NemAlgo's loop body (nem_alg.c:1789-1840), up to n_iters iterations, as a device-controlled
// pipeline: the host enqueues up to kPipeDepth whole iterations back to back; k_ctrl (one thread, at
// the end of each iteration) applies the loop tests on the device and raises ctrl[C_STOP]; every loop
// kernel returns at once when it is set.  The host synchronises once per batch.  The bookkeeping of
// an iteration (label masks + "moved" flag, or the fuzzy convergence test) is enqueued right behind
// the first two relaxation rounds; if a sweep needs more rounds than that, the pipeline stops and the
// host finishes that iteration round by round (rare: labels are sticky).
// `ctrl` (pipelined loop only): the loop tests run in the last block of the bookkeeping kernel
int post_sweep(nemgpu_engine* e, int newbuf, int oldbuf, const CtrlArgs* ctrl = nullptr)
{
    if (e->ncem()) return do_labels_post(e, newbuf, oldbuf, ctrl);
    if (e->cfg.cvtest == NEMGPU_CV_CLAS) {
        launch_conv_fuzzy(conv_fuzzy_args(e, e->cbuf[newbuf], e->cbuf[oldbuf], e->stop_ptr, ctrl), e->stream);
        HIPCHK(hipGetLastError());
    } else if (ctrl != nullptr) {
        launch_ctrl(*ctrl, e->stream);
        HIPCHK(hipGetLastError());
    }
    return NEMGPU_OK;
}

constexpr int kPipeDepth = 7;       // (the graph table holds batches of up to 7 iterations)

// A sweep of the pipelined loop whose two enqueued rounds did not reach the fixed point (or, TIE_LIBC, ran out of
// the draw table): the context from which the host goes on with rounds 2, 3, ... (current partition = e->cur)
int host_rounds_ctx(nemgpu_engine* e, SweepCtx& sc, uint32_t sweep_id, int launched)
{
    sc = SweepCtx();
    sc.multi = true;
    sweep_args(e, sc.a, e->cfg.beta, sweep_id);
    sc.r = launched; sc.checked = launched;               // (the enqueued rounds all changed something)
    if (e->libc()) {
        for (int q = 0; q < launched; q++) if (e->h_round(q)[FLAG_NTIES] & (1 << 30)) e->tie_heavy = true;
        int r = ensure_draw_window(e, e->draws, draw_need(e));
        if (r) return r;
        sweep_draw_args(e, sc.a, true);
    }
    return NEMGPU_OK;
}

// puts e->cur back when an enqueue step that set it for its own launches leaves, by whichever exit
struct CurGuard { nemgpu_engine* e; int saved; ~CurGuard() { e->cur = saved; } };

// enqueue one whole iteration whose current partition is buffer `cur`.  defer_ctrl: another iteration follows in
// the same batch -- an NCEM iteration's loop control then runs in that iteration's counts launch (k_mstep_counts)
// instead of in a last-block ticket at the tail of the last sweep round.
// rounds enqueued for the sweep of iteration `pos` of a run (pos < 0: not known)
int iteration_rounds(const nemgpu_engine* e, int pos, bool deep)
{
    // (fuzzy sweeps need their third round nearly always -- memberships keep moving in the last digits -- : round_batch
    //  everywhere, and what the host had to add for the leading iterations of a run)
    int want = (current_recorder() != nullptr || deep || !e->ncem()) ? e->round_batch : e->rounds_iter;
    if (!e->ncem() && current_recorder() == nullptr && pos >= 0 && pos < kFzPositions && e->fz_need[pos] > want) want = e->fz_need[pos];
    return want;
}

int enqueue_iteration(nemgpu_engine* e, int cur, uint32_t sweep_id, bool defer_ctrl, bool deep, int pos = -1)
{
    int r;
    const CurGuard restore{e, e->cur};
    e->cur = cur;
    // one engine alone: the parameter update rides in the density launch (a launch boundary costs more than the
    // redundant per-block derivation).  In a lock-step batch the launch is shared by all members and the kernels are
    // bound by instruction issue: there the update runs once per class (k_finish) and the density blocks only load it
    const bool fused = !e->cfg.param_fix && e->ncem() && e->fused_update() && current_recorder() == nullptr;
    const bool counts_first = !e->cfg.param_fix && e->ncem();      // the iteration starts with k_mstep_counts
    if (e->ctrl_pending && !counts_first) {                        // (not reached: the mode is fixed within a batch)
        launch_ctrl(e->ctrl_deferred, e->stream);
        e->ctrl_pending = false;
    }
    if (fused) {
        // M-step counts, then ONE kernel: parameter update (per block, from the counts) + density
        if (!e->masks_valid) { if ((r = do_labels_post(e, e->cur, -1))) return r; }
        launch_mstep_counts(counts_args(e, e->stats, e->ctrl_pending ? &e->ctrl_deferred : nullptr), e->stream);
        e->ctrl_pending = false;
        density_launch(e, finish_args(e, 1, e->stats));
        HIPCHK(hipGetLastError());
    } else {
        if (!e->cfg.param_fix) {                                   // nem_alg.c:1806
            if ((r = do_mstep(e, e->ctrl_pending ? &e->ctrl_deferred : nullptr))) return r;
            e->ctrl_pending = false;
            if ((r = do_tables(e))) return r;
        }
        if ((r = do_density(e))) return r;
    }
    SweepCtx c;
    e->sweep_counter = sweep_id;
    // (members of a lock-step batch all take the same number of rounds: a member with a sequence of its own would
    //  need launches of its own)
    const int it_rounds = iteration_rounds(e, pos, deep);
    const CtrlArgs ca = ctrl_args(e, it_rounds, e->cfg.beta);
    // NCEM: the bookkeeping (masks, "moved", loop tests) rides in the last relaxation round's launch -- the loop
    // tests in the next iteration's counts launch when there is one
    const bool defer = defer_ctrl && counts_first;
    const CtrlArgs none{};
    SweepOpts o; o.post_ctrl = e->ncem() ? (defer ? &none : &ca) : nullptr; o.post_moved = true; o.rounds = it_rounds;
    if ((r = sweep_enqueue(e, e->cfg.beta, c, o))) return r;
    if (defer) { e->ctrl_deferred = ca; e->ctrl_pending = true; }
    if (!e->ncem()) { if ((r = post_sweep(e, (cur + 1) % 3, cur, &ca))) return r; }
    else e->masks_valid = true;
    return NEMGPU_OK;
}

// the restart + the two initial sweeps as the head of a pipelined batch (buffers 0 -> 1 -> 2)
// defer_ctrl: an iteration follows in the same batch (see enqueue_iteration)
int libc_init_usual(const nemgpu_engine* e, int which, int percent);
// TIE_LIBC: is a run's start part of its first pipelined batch (verified on the device, see ctrl_logic), or completed
// from the host before it (NEM_MI355X_LIBC_INIT=host)?
static bool libc_init_pipelined()
{
    const char* v = getenv("NEM_MI355X_LIBC_INIT");          // (read every time: a switch for tests and A/B runs)
    return !(v && strcmp(v, "host") == 0);
}

// relaxation rounds a pipelined start enqueues for its beta sweep (enqueue_init; batch_finish continues from there)
static int init_beta_rounds(const nemgpu_engine* e)
{
    int n = std::max<int>(e->round_batch, (!e->ncem() && current_recorder() == nullptr) ? e->fz_init_need : 0);
    if (e->libc()) n = e->libc_rb;                       // (what 95 % of the starts so far needed: batch_plan)
    else if (e->ncem() && current_recorder() == nullptr && e->init_rounds_ncem >= 2) n = e->init_rounds_ncem;
    return n;
}

bool shadow_engine(const nemgpu_engine* e);

// Does a start of this engine go out without its blind launch (round 0 of the beta sweep labels the blind partition
// itself, sweep_body's BLIND instances)?  The fused start of a shadow-verify engine, K = 2 .. 7 (the instances there
// are), NEM_MI355X_BLIND_FOLD not 0 -- and a round of at most kBlindFoldMaxBlocks blocks of 256 sites.  128, not more:
// the sharded driver keeps its three launches, and tests/test_gpu_distributed.py holds it within 1.3 times the single
// engine at 50 000 x 1 000 (196 blocks), where the ratio stands at 1.25-1.29 -- no room for a gain on one side alone.
// Raising it belongs with a change that gives the sharded start as much.
constexpr int kBlindFoldMaxBlocks = 128;
static bool blind_fold_on(const nemgpu_engine* e)
{
    return e->blind_fold && e->start_fused && shadow_engine(e) && e->k >= 2 && e->k <= 7 &&
           (e->n + 255) / 256 <= kBlindFoldMaxBlocks;
}

// hold (shadow-verify schedule, NCEM): the beta sweep's last round and the loop control are left in *hold for the first
// iteration's density launch (defer_ctrl is then ignored); count_into (with hold): the round before it adds the first
// iteration's M-step counts into these statistics, which this launch's restart head zeroes
int enqueue_init(nemgpu_engine* e, bool defer_ctrl, SweepArgs* hold = nullptr, int* count_into = nullptr)
{
    int r;
    FinishArgs t = finish_args(e, 0, nullptr);
    restart_head(e, t);
    if (hold != nullptr && count_into != nullptr) { t.zero_stats = count_into; t.n_zero_stats = e->k + e->k * e->d; }
    e->cur = 0;
    if (e->start_fused && shadow_engine(e)) {
        // one launch: initial parameters back in place, loop control and sweep flag slots cleared, and the density, every
        // block deriving its class constants from the given parameters (k_density_start)
        density_launch(e, t);
        HIPCHK(hipGetLastError());
    } else {
        // one launch: initial parameters back in place, loop control cleared, density tables built
        finish_launch(e, t);
        HIPCHK(hipGetLastError());
        if ((r = do_density(e))) return r;                         // (also clears every sweep flag slot)
    }
    SweepCtx c0, c1;
    e->sweep_counter = 0;
    // blind sweep: one round, 0 -> 1, on a flag slot of its own so that no clear is needed before the next sweep.
    // TIE_LIBC: its sites are coupled through the draw counter -- `ra` verified rounds on the window's last slots; the
    // beta sweep behind it takes the blind sweep's draw count from the last of those slots on the device (the rounds
    // behind a fixed point carry it along), the loop control checks both sweeps and books their draws (ctrl_logic).
    const bool libc = e->libc();
    const int ra = libc ? e->libc_ra : 1;
    const bool fold = blind_fold_on(e);
    if (fold) {
        // no blind launch: round 0 of the beta sweep below computes the blind labels, stores them in buffer 1 and
        // tallies into the blind sweep's slot.  The host state as it would be behind the blind sweep (number 0).
        e->blind_slot_once = kRoundCap - ra; e->blind_id_once = e->sweep_counter++;
        e->n_blind_folds++;
    } else {
        SweepOpts o; o.id_by_value = true; o.slot_base = kRoundCap - ra; o.rounds = libc ? ra : 0;
        if ((r = sweep_enqueue(e, 0.0f, c0, o))) return r;
    }
    e->flags_clean = true;
    e->cur = 1;
    CtrlArgs ca = ctrl_args(e, init_beta_rounds(e), e->cfg.beta);
    ca.is_init = 1;
    ca.blind = e->round_flags(kRoundCap - ra);
    ca.blind_rounds = libc ? ra : 0;
    const bool defer = defer_ctrl && e->ncem() && !e->cfg.param_fix && hold == nullptr;
    const CtrlArgs none{};
    if (libc) e->draw_extra_once = e->round_flags(kRoundCap - 1) + FLAG_NTIES;
    SweepOpts o; o.id_by_value = true; o.post_ctrl = e->ncem() ? (defer ? &none : &ca) : nullptr; o.rounds = ca.n_rounds;
    o.hold = hold; o.count_into = count_into;
    if ((r = sweep_enqueue(e, e->cfg.beta, c1, o))) return r;   // 1 -> 2 (and 0 as the pong buffer)
    e->draw_extra_once = nullptr;
    if (defer) { e->ctrl_deferred = ca; e->ctrl_pending = true; }
    if (e->ncem()) e->masks_valid = true;
    else { launch_ctrl(ca, e->stream); HIPCHK(hipGetLastError()); }
    e->cur = 2;
    return NEMGPU_OK;
}

// ---- TIE_LIBC start: the two initial sweeps draw from ONE stream, the blind one first, so each is completed (its
// rounds verified from the host, its draws booked) before the next is enqueued.  Three enqueue steps with a host step
// after the first two; recordable like everything else.
int libc_init_a(nemgpu_engine* e, SweepCtx& c, int rounds = 0)
{
    int r;
    FinishArgs t = finish_args(e, 0, nullptr);                 // initial parameters back in place, loop control cleared, tables
    restart_head(e, t);
    finish_launch(e, t);
    e->cur = 0; e->sweep_counter = 0;
    if ((r = do_density(e))) return r;
    SweepOpts o; o.rounds = rounds;
    return sweep_enqueue(e, 0.0f, c, o);                       // blind sweep 0 -> 1
}
int libc_init_b(nemgpu_engine* e, SweepCtx& c, int rounds = 0)
{
    e->cur = 1;
    SweepOpts o; o.rounds = rounds;
    return sweep_enqueue(e, e->cfg.beta, c, o);                // 1 -> 2
}
int libc_init_c(nemgpu_engine* e)
{
    int r;
    e->cur = 2;
    e->masks_valid = false;
    if ((r = do_labels_post(e, 2, -1))) return r;
    launch_fill(e->sweep_next, 1, (int)e->sweep_counter, e->stream);
    return NEMGPU_OK;
}

// The same start with ONE wait: the beta sweep's rounds go out behind the blind sweep's, taking the blind sweep's draw
// count from the flag slot of its last round on the device (rounds behind a sweep's fixed point carry the count along),
// and the class masks behind them.  `ra` blind rounds on the last slots of the flag window, `rb` beta rounds from slot 0.
// Then the host looks once: blind sweep at its fixed point within ra rounds?  (else what ran behind it is void:
// *redo = true, nothing booked, the caller starts over with libc_init_a)  beta sweep within rb?  (else it is continued
// from the host as any sweep is, and the masks are made again).  rounds[0..1]: what the two sweeps needed.
int libc_init_one_wait(nemgpu_engine* e, int ra, int rb, bool* redo, int rounds[2])
{
    int r;
    *redo = false;
    ra = std::max(1, std::min(ra, kRoundCap / 4)); rb = std::max(1, std::min(rb, kRoundCap / 2));
    FinishArgs t = finish_args(e, 0, nullptr);
    restart_head(e, t);
    finish_launch(e, t);
    e->cur = 0; e->sweep_counter = 0;
    if ((r = do_density(e))) return r;                             // (also clears every sweep flag slot)
    SweepCtx ca, cb;
    const int base_a = kRoundCap - ra;
    SweepOpts oa, ob; oa.slot_base = base_a; oa.rounds = ra; ob.rounds = rb;
    if ((r = sweep_enqueue(e, 0.0f, ca, oa))) return r;            // blind sweep 0 -> 1
    e->flags_clean = true;                                         // (the beta sweep's slots have not been touched)
    e->cur = 1;
    e->draw_extra_once = e->round_flags(kRoundCap - 1) + FLAG_NTIES;
    if ((r = sweep_enqueue(e, e->cfg.beta, cb, ob))) return r;     // 1 -> 2
    e->draw_extra_once = nullptr;
    // the flags leave as soon as the rounds are through (an event marks the copy); the class masks and the sweep counter
    // run while the host wakes up and draws the next start's centres
    HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    nemgpu_engine* ev_owner = e->parent ? e->parent : e;     // (the twins of a random-start round share their parent's event: one start at a time)
    if (!ev_owner->ev_flags) HIPCHK(hipEventCreateWithFlags(&ev_owner->ev_flags, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_owner->ev_flags, e->stream));
    e->cur = 2;
    e->masks_valid = false;
    if ((r = do_labels_post(e, 2, -1))) return r;
    launch_fill(e->sweep_next, 1, (int)e->sweep_counter, e->stream);
    // (polled: the wait is tens of microseconds and its end is on the critical path of every start; a blocking wait's
    //  wake-up cost 5-10 us more)
    for (;;) {
        const hipError_t q = hipEventQuery(ev_owner->ev_flags);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { HIPCHK(q); }
        __builtin_ia32_pause();
    }
    if ((r = check_fault(e))) return r;
    auto book = [&](const int* f, int done_at) {
        e->draws += f[FLAG_NTIES] & ((1 << 30) - 1);
        if (f[FLAG_NZERO] > 0) { e->zero_density += f[FLAG_NZERO]; if (e->first_zero < 0) e->first_zero = e->n_total - f[FLAG_FIRSTZERO]; }
        e->sweep_rounds += done_at + 1;
    };
    int done_a = -1; bool tab_short = false;
    for (int q = 0; q < ra && done_a < 0; q++) {
        const int* f = e->h_round(base_a + q);
        if (f[FLAG_NTIES] & (1 << 30)) tab_short = true;
        if (f[FLAG_CHANGED] == 0) done_a = q;
    }
    if (done_a < 0 || tab_short) { *redo = true; e->cur = 0; e->sweep_counter = 0; e->masks_valid = false; e->flags_clean = false; return NEMGPU_OK; }
    const int blind_draws = e->h_round(base_a + done_a)[FLAG_NTIES] & ((1 << 30) - 1);
    book(e->h_round(base_a + done_a), done_a);
    rounds[0] = done_a + 1;
    int done_b = -1;
    for (int q = 0; q < rb && done_b < 0; q++) {
        const int* f = e->h_round(q);
        if (f[FLAG_NTIES] & (1 << 30)) tab_short = true;
        if (f[FLAG_CHANGED] == 0) done_b = q;
    }
    if (done_b >= 0 && !tab_short) { book(e->h_round(done_b), done_b); rounds[1] = done_b + 1; return NEMGPU_OK; }
    // the beta sweep goes on from the host: its draws-before by value now (the blind sweep's are booked)
    e->cur = 1;
    cb.a.draw_base += blind_draws; cb.a.draw_extra = nullptr;
    if ((r = sweep_complete(e, cb, &rounds[1], nullptr, true, true))) return r;
    e->cur = 2;
    e->masks_valid = false;
    if ((r = do_labels_post(e, 2, -1))) return r;
    return NEMGPU_OK;
}

// How many rounds of an initial sweep go out at once: what `percent` % of the runs so far got by with (which: 0 the blind
// sweep, 1 the beta sweep; the tally lives on the engine that owns the twins)
int libc_init_usual(const nemgpu_engine* e, int which, int percent)
{
    const nemgpu_engine* o = e->parent ? e->parent : e;
    const int* h = o->libc_init_hist[which];
    int total = 0; for (int q = 0; q <= 16; q++) total += h[q];
    int acc = 0, q = 0;
    for (; q < 16; q++) { acc += h[q]; if (total > 0 && 100 * acc >= percent * total) break; }
    return total > 0 ? std::max(2, q) : std::max(3, e->round_batch);      // (nothing seen yet: three)
}
void libc_init_tally(nemgpu_engine* e, const int rounds[2])
{
    nemgpu_engine* o = e->parent ? e->parent : e;
    o->libc_init_hist[0][std::max(0, std::min(16, rounds[0]))]++;
    o->libc_init_hist[1][std::max(0, std::min(16, rounds[1]))]++;
}
// a TIE_LIBC run's start: the one-wait form, or (asked for, or its blind sweep was not through) sweep by sweep
int libc_init(nemgpu_engine* e, int* rounds_beta = nullptr, bool* was_redone = nullptr)
{
    static const bool one_wait = !(getenv("NEM_MI355X_STARTS_ONE_WAIT") && getenv("NEM_MI355X_STARTS_ONE_WAIT")[0] == '0');
    int r;
    int rounds[2] = {0, 0};
    bool redo = false;
    const int ra = std::min(8, libc_init_usual(e, 0, 90)), rb = libc_init_usual(e, 1, 70);
    if (one_wait && current_recorder() == nullptr) { if ((r = libc_init_one_wait(e, ra, rb, &redo, rounds))) return r; }
    if (was_redone) *was_redone = redo;
    if (!one_wait || redo || current_recorder() != nullptr) {
        SweepCtx sc;
        if ((r = libc_init_a(e, sc, ra)) || (r = sweep_complete(e, sc, &rounds[0], nullptr, false, true))) return r;
        if ((r = libc_init_b(e, sc, rb)) || (r = sweep_complete(e, sc, &rounds[1], nullptr, false, true))) return r;
        if ((r = libc_init_c(e))) return r;
    }
    HIPCHK(hipGetLastError());
    libc_init_tally(e, rounds);
    if (rounds_beta) *rounds_beta = rounds[1];
    e->draws_after_init = e->draws;
    return NEMGPU_OK;
}

// ---- one batch of the pipelined loop, in three pieces so that the same code drives ONE engine (iterate) or SEVERAL
// in lock step (iterate_many: the pieces' launches are recorded per engine and issued once for all of them) ----------
struct LoopCursor {
    int remaining = 0;            // iterations still allowed
    bool first = false;           // the next batch starts with the restart + the two initial sweeps
    // the batch in flight
    int g = 0, base = 0; uint32_t sweep0 = 0; bool batch_first = false;
    int deep = 0;                 // leading iterations of the batch that get round_batch relaxation rounds
    int pos0 = 0;                 // run-relative number of the batch's first iteration (fuzzy: selects the learned round counts)
    bool shadow = false;          // the batch takes the shadow-verify schedule (shadow_batch_enqueue)
    bool active() const { return remaining > 0 || first; }
};

// host half of a restart (the device half is the head of the first batch)
int loop_begin(nemgpu_engine* e, LoopCursor& lc, int n_iters, bool with_init)
{
    int r;
    lc = LoopCursor();
    lc.remaining = n_iters; lc.first = with_init;
    if (!with_init) { if ((r = flush_reset(e))) return r; }
    if (with_init) {
        if (!e->have_matrix || !e->have_params) { set_error("matrix and parameters must be set first"); return NEMGPU_E_FUNCARG; }
        if ((r = ensure_state_buffers(e))) return r;
            if ((r = clear_fault(e))) return r;
        e->reset_pending = false;                          // (the head of the first batch is the device half of a reset)
        e->run_deep_used = 0; e->run_tracked = true;
        e->cur = 0; e->sweep_counter = 0;
        e->iters = 0; e->converged = 0; e->emptyk = 0; e->status = NEMGPU_OK;
        e->zero_density = 0; e->first_zero = -1; e->sweep_rounds = 0; e->masks_valid = false;
    }
    return NEMGPU_OK;
}
bool loop_wants_batch(const nemgpu_engine* e, const LoopCursor& lc)
{
    return lc.active() && !e->converged && e->status == NEMGPU_OK;
}

bool shadow_engine(const nemgpu_engine* e);

// what the next batch is; the state every batch may rely on (issued / recorded ahead of it)
int batch_plan(nemgpu_engine* e, LoopCursor& lc)
{
    int r;
    lc.g = std::min(lc.remaining, kPipeDepth);
    lc.batch_first = lc.first;
    lc.base = lc.first ? 2 : e->cur;
    lc.sweep0 = lc.first ? 2u : e->sweep_counter;
    lc.deep = current_recorder() != nullptr ? lc.g : std::max(0, std::min(lc.g, e->deep_iters - (lc.first ? 0 : e->iters)));
    lc.pos0 = lc.first ? 0 : e->iters;
    // (a batch with a sweep behind which an iteration follows; g and `first` are part of a captured batch's key)
    lc.shadow = shadow_engine(e) && (lc.g >= 2 || (lc.first && lc.g >= 1));
    // (fuzzy: the round counts of a batch's iterations depend on where in the run it starts; the graph table's last
    //  index tells the classes apart -- a stale class would only enqueue another number of rounds, never change a result)
    if (!e->ncem() && current_recorder() == nullptr) lc.deep = lc.pos0 >= kFzPositions ? 0 : std::min(7, 1 + lc.pos0 / kPipeDepth);
    // class masks of the current labels, fresh tables when the parameters are fixed (otherwise k_finish rebuilds them
    // inside the batch)
    if (!lc.first) {
        if (e->ncem() && !e->cfg.param_fix && !e->masks_valid) { if ((r = do_labels_post(e, e->cur, -1))) return r; }
        if (e->cfg.param_fix) { if ((r = do_tables(e))) return r; }
    }
    if (e->libc()) {
        if (lc.first) {
            // the rounds of the two initial sweeps: what most runs so far got by with (at most 8: the loop control's window)
            // (95 %: a start that needs more costs a whole batch and a second start from the host here, not one more wait)
            const int ra = std::max(2, std::min(8, libc_init_usual(e, 0, 95))), rb = std::max(2, std::min(8, libc_init_usual(e, 1, 95)));
            if (ra != e->libc_ra || rb != e->libc_rb) { e->libc_ra = ra; e->libc_rb = rb; drop_graphs(e); }
        }
        if ((r = ensure_draw_window(e, e->draws, draw_need(e)))) return r;      // (may drop the graphs)
        if ((r = publish_draw_ctl(e))) return r;
    }
    return NEMGPU_OK;
}

// ---- shadow-verify schedule (NCEM, fused parameter update, one engine alone) -------------------------------------------
// A sweep's last, verifying round changes nothing in steady state; what it decides is whether the iteration stands.  The
// next iteration's counts and density do not need that decision: they need the labels of the round before, final
// whenever the verifying round confirms them.  So that round (and the loop control in its last-block ticket) runs in the
// next iteration's density launch (k_density_verify), and the round before it makes the class masks and "moved":
//   today:  counts(t+1)[+ctrl(t)] -> density(t+1) -> R0(t+1) -> R1(t+1) -> counts(t+2)[+ctrl(t+1)] -> ...
//   here:   R0(t) -> counts(t+1) -> [density(t+1) | R1(t) + ctrl(t)] -> R0(t+1) -> ...
// If the verifying round changes something, the loop control stops the batch and batch_finish finishes the sweep from
// the host as before.  density(t+1) runs before t is accepted, so it writes a copy of its own of the parameters, the
// densities and the flag block: iteration j of a batch of g writes copy shadow_copy(j, g) -- the batch's last iteration
// copy 0, the copy everything outside a batch reads, the ones before it 1 and 2 in turn (j = -1: the restart head).  A
// batch that stops elsewhere has its accepted copy moved to 0 afterwards (accept_copy).  The copies depend on (first
// batch, g, j) only, so a captured batch replays with the same ones.
int shadow_copy(int j, int g) { return j == g - 1 ? 0 : 1 + (g - 2 - j) % 2; }
// ... and (NEM_MI355X_ROUND_COUNTS) its M-step counts slot shadow_stats(j, g): the last iteration's are in `stats`, the
// ones before alternate, so that the slot a mask round adds into is never the one the density beside it reads
int shadow_stats(int j, int g) { return (g - 1 - j) % 2; }
// Does the mask round count (NEM_MI355X_ROUND_COUNTS and the shape)?  Its tail grows with the partial counts it adds, one
// atomic per (block, class, organism), all blocks on the same K*D words; the launch it saves does not.  Measured on
// MI355X (NOTES_negative_results.md section 12): 79 blocks x 1 500 (configs[1]) made the round 1.7 us longer and the step
// 1 us shorter; 196 x 3 000 (50 000 x 1 000) made the step 5.4 us longer.
constexpr long kRoundCountsMaxAdds = 1l << 17;
bool round_counts_on(const nemgpu_engine* e)
{
    return e->round_counts && (long)((e->n + 255) / 256) * e->k * e->d <= kRoundCountsMaxAdds;
}

void use_copy(nemgpu_engine* e, int c)
{
    e->fset = c;
    e->prop = e->par_copy[c]; e->center = e->prop + e->par_o_center; e->disp = e->prop + e->par_o_disp; e->nbobs_k = e->prop + e->par_o_nb;
    e->pkfki = e->pkfki_copy[c]; e->logpkfki = e->logpkfki_copy[c];
}

// copy c (parameters, densities, flag block -- the host mirror's too) becomes copy 0
int accept_copy(nemgpu_engine* e, int c)
{
    const size_t kn = (size_t)e->k * e->npad;
    HIPCHK(hipMemcpyAsync(e->par_copy[0], e->par_copy[c], e->par_words * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->pkfki_copy[0], e->pkfki_copy[c], kn * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->logpkfki_copy[0], e->logpkfki_copy[c], kn * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->flags_dev + C_WORDS, e->flags_dev + C_WORDS + (size_t)c * kFlagSetWords, kFlagSetWords * sizeof(int),
                          hipMemcpyDeviceToDevice, e->stream));
    memcpy(e->flags_host + C_WORDS, e->flags_host + C_WORDS + (size_t)c * kFlagSetWords, kFlagSetWords * sizeof(int));
    return NEMGPU_OK;
}

// does this engine's pipelined loop take the shadow-verify schedule?  (Everything else keeps the one above: lock-step
// twins, TIE_LIBC, fuzzy NEM, fixed or k_finish-updated parameters, sharded runs, sweeps without neighbours.)
bool shadow_engine(const nemgpu_engine* e)
{
    return e->flag_sets == 3 && e->parent == nullptr && current_recorder() == nullptr && e->ncem() && !e->cfg.param_fix &&
           e->fused_update() && e->has_graph && e->cfg.beta != 0.0f && e->lo == 0 && e->hi == e->n_total &&
           density_verify_supported(e->n, e->k, e->cfg.tie_rule);
}

// iteration `cur` of a shadow-verify batch: counts into `stats` (unless the held sweep's mask round added them up
// there: *pending and *counted), then the density (with the previous sweep's verifying round when *pending), then the
// sweep's rounds -- its last one left in *held (*pending set) when `hold`.  count_into (with hold): the mask round adds
// the next iteration's counts into these statistics (*counted set), which the density launch zeroes first.
int enqueue_iteration_shadow(nemgpu_engine* e, int cur, uint32_t sweep_id, bool hold, bool deep, int pos, int prev, int copy,
                             SweepArgs* held, bool* pending, int* stats, int* count_into, bool* counted)
{
    int r;
    const CurGuard restore{e, e->cur};
    e->cur = cur;
    if (!(*pending && *counted)) {
        if (!e->masks_valid) { if ((r = do_labels_post(e, e->cur, -1))) return r; }
        launch_mstep_counts(counts_args(e, stats, nullptr), e->stream);
    }
    if (!hold) count_into = nullptr;
    use_copy(e, copy);
    FinishArgs t = finish_args(e, 1, stats);
    if (count_into != nullptr) { t.zero_stats = count_into; t.n_zero_stats = e->k + e->k * e->d; }
    t.prev_center = e->par_copy[prev] + e->par_o_center; t.prev_disp = e->par_copy[prev] + e->par_o_disp;
    density_launch(e, t, *pending ? held : nullptr);
    *pending = false;
    HIPCHK(hipGetLastError());
    SweepCtx c;
    e->sweep_counter = sweep_id;
    const int it_rounds = iteration_rounds(e, pos, deep);
    // (what the rule gives under shadow_engine(e): use_nei = 1, ncem = 1, param_fix = 0, and no draw words -- the schedule
    //  has no TIE_LIBC)
    const CtrlArgs ca = ctrl_args(e, it_rounds, e->cfg.beta);
    if (hold) *held = SweepArgs{};
    SweepOpts o; o.post_ctrl = &ca; o.post_moved = true; o.rounds = it_rounds; o.hold = hold ? held : nullptr; o.count_into = count_into;
    if ((r = sweep_enqueue(e, e->cfg.beta, c, o))) return r;
    *pending = hold && held->post_ctrl.ctrl != nullptr;    // (a sweep of one round has nothing to hold back)
    *counted = *pending && count_into != nullptr;
    e->masks_valid = true;
    return NEMGPU_OK;
}

int shadow_batch_enqueue(nemgpu_engine* e, const LoopCursor& lc)
{
    int r = NEMGPU_OK;
    SweepArgs held{};
    bool pending = false, counted = false;
    int prev = 0;                                          // the copy the next density keeps an empty class's parameters from
    // the statistics of iteration j: slot shadow_stats(j, g) -- added up by the mask round of the sweep before (zeroed by
    // the launch before that round: the restart head or the density of j - 1), or stored by a counts launch
    const bool rc = round_counts_on(e);
    auto stats = [&](int j) { return rc ? e->stats_slot[shadow_stats(j, lc.g)] : e->stats; };
    if (lc.batch_first) {
        prev = shadow_copy(-1, lc.g);
        use_copy(e, prev);
        r = enqueue_init(e, false, &held, rc ? stats(0) : nullptr);
        pending = r == NEMGPU_OK && held.post_ctrl.ctrl != nullptr;
        counted = pending && rc;
    }
    for (int j = 0; j < lc.g && r == NEMGPU_OK; j++) {
        const int copy = shadow_copy(j, lc.g);
        r = enqueue_iteration_shadow(e, (lc.base + j) % 3, lc.sweep0 + j, j + 1 < lc.g, j < lc.deep, lc.pos0 + j, prev, copy,
                                     &held, &pending, stats(j), rc && j + 1 < lc.g ? stats(j + 1) : nullptr, &counted);
        prev = copy;
    }
    use_copy(e, 0);
    return r;
}

// the batch's launches (issued, captured or recorded by the caller's choice), ending with the copy of the control block
// after_iter (optional): called behind the launches of every iteration of the batch (the logged run's snapshots)
int batch_enqueue(nemgpu_engine* e, LoopCursor& lc, bool with_copy, const std::function<int(int)>* after_iter = nullptr)
{
    int r = NEMGPU_OK;
    e->ctrl_pending = false;                               // (a batch never inherits a deferred loop control)
    hipError_t herr = hipSuccess;
    if (!lc.batch_first) {                                 // (the restart launch clears the loop control itself)
        if (current_recorder()) launch_fill(e->ctrl(), C_WORDS, 0, e->stream);
        else herr = hipMemsetAsync(e->ctrl(), 0, C_WORDS * sizeof(int), e->stream);
    }
    e->stop_ptr = e->ctrl() + C_STOP;
    lc.shadow = lc.shadow && after_iter == nullptr && current_recorder() == nullptr;
    if (lc.shadow && herr == hipSuccess) r = shadow_batch_enqueue(e, lc);
    else if (lc.batch_first && herr == hipSuccess) r = enqueue_init(e, lc.g > 0);
    for (int j = 0; j < lc.g && !lc.shadow && r == NEMGPU_OK && herr == hipSuccess; j++) {
        r = enqueue_iteration(e, (lc.base + j) % 3, lc.sweep0 + j, j + 1 < lc.g && after_iter == nullptr, e->ncem() ? j < lc.deep : false, lc.pos0 + j);
        if (r == NEMGPU_OK && after_iter != nullptr) r = (*after_iter)(j);
    }
    e->stop_ptr = nullptr;
    if (herr == hipSuccess && r == NEMGPU_OK && with_copy)
        herr = hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost, e->stream);
    if (r) return r;
    HIPCHK(herr);
    return NEMGPU_OK;
}

// after the batch has run (stream synchronised, control block on the host): account for it, finish from the host what
// the pipeline could not
int batch_finish(nemgpu_engine* e, LoopCursor& lc)
{
    int r;
    if ((r = check_fault(e))) return r;
    const int* c = e->h_ctrl();
    const int done = c[C_ITERS], commits = c[C_COMMITS];
    const bool first = lc.batch_first;
    const int base = lc.base;
    const uint32_t sweep0 = lc.sweep0;
    if (lc.shadow) {                                           // the copy of the last iteration the loop control saw
        const int acc = shadow_copy(done - 1, lc.g);
        if (acc != 0 && (r = accept_copy(e, acc))) return r;
    }
    // the statistics the batch counted last: those of the iteration behind the one whose loop control stopped it (its
    // counts were added up, or launched, before that control ran), else of the batch's last iteration
    e->stats_last = lc.shadow && round_counts_on(e) ? e->stats_slot[shadow_stats(std::min(done, lc.g - 1), lc.g)] : e->stats;
    if (first && e->libc()) {
        if (c[C_NEED_ROUNDS] >= 2) {
            // TIE_LIBC: one of the two initial sweeps was not through in the rounds enqueued (or a draw left the table):
            // nothing was booked, everything behind returned at the stop word -- the start is done again from the host
            e->n_host_rounds++;
            e->flags_clean = false;
            if ((r = libc_init(e))) return r;
            lc.first = false;
            return NEMGPU_OK;
        }
        const int got[2] = {c[C_INIT_ROUNDS] >> 8, c[C_INIT_ROUNDS] & 0xFF};
        libc_init_tally(e, got);                               // (what the two sweeps needed, as the loop control saw it)
        e->draws_after_init = e->draws + c[C_DRAWS_INIT];
    }
    e->iters += done;
    e->draws += c[C_DRAWS];
    e->sweep_rounds += c[C_SWEEP_ROUNDS];
    if (c[C_NZERO] > 0) {
        e->zero_density += c[C_NZERO];
        if (e->first_zero < 0) e->first_zero = e->n_total - c[C_FIRSTZERO];
    }
    e->flags_clean = false;
    e->tables_fresh = e->cfg.param_fix;                        // (the fused density kernel does not rebuild the table buffers)
    if (e->ncem()) e->masks_valid = true;
    const int init_launched = first ? init_beta_rounds(e) : 0;    // (before the count below is touched)
    if (first && !e->libc() && e->ncem() && current_recorder() == nullptr && e->has_graph && e->cfg.beta != 0.0f) {
        if (c[C_NEED_ROUNDS] == 2) {
            if (e->init_rounds_ncem != 0) { e->init_rounds_ncem = 0; drop_graphs(e); }       // (back to round_batch)
            e->init_rounds_locked = true; e->init_two_streak = 0;
        } else if (!e->init_rounds_locked && e->init_rounds_ncem == 0) {
            e->init_two_streak = (c[C_INIT_ROUNDS] & 0xFF) <= 2 ? e->init_two_streak + 1 : 0;
            if (e->init_two_streak >= 3 && e->round_batch > 2) { e->init_rounds_ncem = 2; drop_graphs(e); }
        }
    }
    if (first && c[C_NEED_ROUNDS] == 2) {
        // the initial beta sweep (buffers 1 -> 2/0) is not at its fixed point after the enqueued rounds; every
        // iteration behind it returned at the stop word.  Finish it from the host, then go on.
        e->cur = 1;
        e->n_host_rounds++;
        SweepCtx sc;
        const int launched = init_launched;
        if ((r = host_rounds_ctx(e, sc, 1u, launched))) return r;
        if ((r = sweep_launch_rounds(e, sc, e->round_batch))) return r;
        int init_rounds = 0;
        if ((r = sweep_complete(e, sc, &init_rounds, nullptr))) return r;
        if (!e->ncem() && current_recorder() == nullptr && std::min(kRoundsMax, init_rounds) > e->fz_init_need) {
            e->fz_init_need = (uint8_t)std::min(kRoundsMax, init_rounds);     // the next starts get them enqueued
            drop_graphs(e);
        }
        e->sweep_rounds += 1;                                  // + the blind sweep
        e->cur = 2; e->sweep_counter = 2;
        e->masks_valid = false;
        if (e->ncem()) { if ((r = do_labels_post(e, 2, -1))) return r; }
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->sweep_next, 2, 1, e->stream));
        lc.first = false;
        return NEMGPU_OK;
    }
    lc.first = false;
    e->cur = (base + commits) % 3;
    e->sweep_counter = sweep0 + (uint32_t)done;
    lc.remaining -= done;
    if (c[C_DEEP] > 0) e->run_deep_used = std::max(e->run_deep_used, e->iters - done + c[C_DEEP]);
    // a whole run in which the leading iterations did not use their extra round: one of them loses it next time
    auto run_ends = [&]() {
        if (e->run_tracked && current_recorder() == nullptr && (e->converged || e->iters >= e->deep_iters) &&
            e->run_deep_used < e->deep_iters) e->deep_iters--;
        e->run_tracked = false;
    };
    if (c[C_STATUS] == NEMGPU_W_EMPTYCLASS) {                  // nem_alg.c:1831-1838
        e->status = NEMGPU_W_EMPTYCLASS;
        e->emptyk = c[C_EMPTYK];
        e->masks_valid = false;                                // the speculative E-step rebuilt them for a discarded partition
        run_ends();
        return NEMGPU_OK;
    }
    if (c[C_CONVERGED]) { e->converged = 1; run_ends(); return NEMGPU_OK; }
    if (c[C_NEED_ROUNDS]) {
        // iteration #commits of this batch ran its M-step, density and the enqueued relaxation rounds and is
        // not at the fixed point yet: continue its rounds from the host, then redo the bookkeeping.
        const int oldbuf = e->cur, newbuf = (e->cur + 1) % 3;
        e->n_host_rounds++;
        SweepCtx sc;
        const int pos = lc.pos0 + done - 1;                          // the run-relative number of that iteration
        const int launched = iteration_rounds(e, pos, e->ncem() && done - 1 < lc.deep);
        if ((r = host_rounds_ctx(e, sc, sweep0 + (uint32_t)(done - 1), launched))) return r;
        e->deep_iters = std::max(e->deep_iters, e->iters);          // from now on: one round more up to this iteration of a run
        e->run_deep_used = std::max(e->run_deep_used, e->iters);
        if ((r = sweep_launch_rounds(e, sc, e->round_batch))) return r;
        int rounds = 0;
        if ((r = sweep_complete(e, sc, &rounds, nullptr))) return r;
        if (!e->ncem() && current_recorder() == nullptr && pos >= 0 && pos < kFzPositions && std::min(kRoundsMax, rounds) > e->fz_need[pos]) {
            e->fz_need[pos] = (uint8_t)std::min(kRoundsMax, rounds);       // this position gets them enqueued from now on
            drop_graphs(e);
        }
        HIPCHK(hipMemsetAsync(e->iter_flags() + FLAG_MOVED, 0, sizeof(int), e->stream));
        if ((r = post_sweep(e, newbuf, oldbuf))) return r;
        if ((r = read_iter_flags(e))) return r;
        e->cur = newbuf;
        if (e->cfg.cvtest == NEMGPU_CV_CLAS) {
            const int moved = e->h_iter()[FLAG_MOVED];
            if (e->ncem()) e->converged = moved ? (1.0f < e->cfg.cvthres) : (0.0f < e->cfg.cvthres);
            else e->converged = !moved;
        }
    }
    if (e->converged || lc.remaining <= 0) run_ends();
    return NEMGPU_OK;
}

void drop_graphs(nemgpu_engine* e)
{
    e->batch_graphs.clear();
    e->shard_graphs.clear();
}

// What run_graphed did with a batch (none: the capture failed with enqueue()'s error, which it returns).
enum class Graphed { none, plain, captured, replayed };

// One batch on stream s: the captured graph of desc's slot in `cache` is replayed if there is one; else the batch is
// enqueued (enqueue()) as plain launches, or -- once the shape has been asked for capture_after times, or at once
// under owner->capture_first -- captured, and the graph launched.  A failed capture turns owner->use_graphs off for
// good; nothing of it ran, so the owner's freshness flags go back to what they were, rewind() puts back the rest of
// the host state enqueue() changed, and the batch goes out as plain launches.  cache == nullptr: plain launches.
template <typename Enqueue, typename Rewind>
int run_graphed(nemgpu_engine* owner, GraphCache* cache, const std::vector<uint64_t>& desc, int capture_after, hipStream_t s,
                Enqueue&& enqueue, Rewind&& rewind, Graphed* how)
{
    auto get_flags = [owner]() { return HostFlags{owner->tables_fresh, owner->density_fresh, owner->flags_clean, owner->masks_valid}; };
    auto set_flags = [owner](const HostFlags& f) {
        owner->tables_fresh = f.tables_fresh; owner->density_fresh = f.density_fresh;
        owner->flags_clean = f.flags_clean; owner->masks_valid = f.masks_valid;
    };
    *how = Graphed::none;
    GraphCache::Slot* slot = cache != nullptr && owner->use_graphs ? &cache->find_or_add(desc) : nullptr;
    if (slot != nullptr && slot->exec != nullptr) {
        HIPCHK(hipGraphLaunch(slot->exec, s));
        if (cache->host_flags) set_flags(slot->post);
        *how = Graphed::replayed;
        return NEMGPU_OK;
    }
    if (slot != nullptr && (slot->asked++ >= capture_after - 1 || owner->capture_first)) {
        const HostFlags before = get_flags();
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int r = enqueue();
        hipGraph_t graph = nullptr;
        const hipError_t cerr = hipStreamEndCapture(s, &graph);
        hipGraphExec_t exec = nullptr;
        if (r == NEMGPU_OK && cerr == hipSuccess && graph != nullptr && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
            (void)hipGraphDestroy(graph);
            slot->exec = exec;
            slot->post = get_flags();
            *how = Graphed::captured;
            HIPCHK(hipGraphLaunch(exec, s));
            return NEMGPU_OK;
        }
        if (graph) (void)hipGraphDestroy(graph);
        if (getenv("NEM_MI355X_DEBUG"))
            fprintf(stderr, "[nem] batch capture failed: enqueue rc %d (%s), end-capture %s\n", r, g_last_error.c_str(), hipGetErrorString(cerr));
        (void)hipGetLastError();
        owner->use_graphs = false;                                 // plain launches from now on
        if (r != NEMGPU_OK) return r;
        set_flags(before);
        rewind();
    }
    *how = Graphed::plain;
    return enqueue();
}

int iterate_pipelined(nemgpu_engine* e, int n_iters, bool with_init)
{
    int r;
    LoopCursor lc;
    if ((r = loop_begin(e, lc, n_iters, with_init))) return r;
    if (lc.first && e->libc() && !libc_init_pipelined()) {
        // TIE_LIBC, NEM_MI355X_LIBC_INIT=host: the two initial sweeps are completed from the host (one wait:
        // libc_init_one_wait); the iterations behind them are pipelined
        if ((r = libc_init(e))) return r;
        lc.first = false;
    }
    while (loop_wants_batch(e, lc)) {
        if ((r = batch_plan(e, lc))) return r;
        // the first batch of a shape goes out as plain launches: capturing and instantiating a graph costs more than
        // it saves unless the batch is replayed, and a nem() call's engine enqueues most shapes once.  (A batch's
        // enqueue changes cur and sweep_counter besides the freshness flags; a capture counts as a replay too.)
        const int cur0 = e->cur; const uint32_t sweep_counter0 = e->sweep_counter;
        const int folds0 = e->n_blind_folds;
        Graphed how;
        r = run_graphed(e, lc.g < 8 ? &e->batch_graphs : nullptr, {(uint64_t)lc.batch_first, (uint64_t)lc.base, (uint64_t)lc.g, (uint64_t)lc.deep},
                        2, e->stream, [&]() { return batch_enqueue(e, lc, true); },
                        [&]() { e->cur = cur0; e->sweep_counter = sweep_counter0; e->n_blind_folds = folds0; }, &how);
        // (a replayed start was captured by this engine with the switch and the shape it has now)
        if (how == Graphed::replayed && lc.batch_first && blind_fold_on(e)) e->n_blind_folds++;
        e->n_plain += how == Graphed::plain;
        e->n_captured += how == Graphed::captured;
        e->n_replayed += how == Graphed::replayed || (how == Graphed::captured && r == NEMGPU_OK);
        if (r) return r;
        HIPCHK(hipStreamSynchronize(e->stream));
        if ((r = batch_finish(e, lc))) return r;
    }
    return NEMGPU_OK;
}

int criteria(nemgpu_engine* e, float crit6[6], int buf);

// An engine with an observed mask (missing cells): NemAlgo's loop body (nem_alg.c:1789-1840) one launch group at a time,
// from the steps init_partition uses -- M-step, tables, density, sweep, bookkeeping -- with do_mstep and do_density on the
// masked kernels.  No graph, no pipelining: the host reads the iteration's flags (empty class, "a label moved") once per
// iteration, besides the sweep's own round trip.
int iterate_stepwise(nemgpu_engine* e, int n_iters, bool with_init)
{
    int r;
    if ((r = masked_algo_check(e))) return r;
    if (with_init) {
        const int draws = e->draws;                                // (the caller's: one srandom per nem() call)
        if ((r = reset_state(e))) return r;
        e->draws = draws;
        if ((r = init_partition(e))) return r;
    } else if ((r = flush_reset(e))) return r;
    for (int it = 0; it < n_iters && !e->converged && e->status == NEMGPU_OK; it++) {
        if (!e->cfg.param_fix) { if ((r = do_mstep(e))) return r; }
        if ((r = do_tables(e))) return r;
        e->iters++;
        if (!e->cfg.param_fix) {
            if ((r = read_iter_flags(e))) return r;
            const int ek = e->h_iter()[FLAG_EMPTYK];
            if (ek != 0) {                                         // nem_alg.c:1831-1838: the E-step does not run
                e->status = NEMGPU_W_EMPTYCLASS; e->emptyk = ek;
                break;
            }
        }
        if ((r = do_density(e))) return r;
        const int oldbuf = e->cur, newbuf = (e->cur + 1) % 3;
        if ((r = do_sweep(e, e->cfg.beta, nullptr))) return r;
        if ((r = do_labels_post(e, newbuf, oldbuf))) return r;     // (FLAG_MOVED was cleared by the density launch)
        if ((r = read_iter_flags(e))) return r;
        e->cur = newbuf;
        if (e->cfg.cvtest == NEMGPU_CV_CLAS) {                     // HasConverged, nem_alg.c:2075-2089
            const int moved = e->h_iter()[FLAG_MOVED];
            e->converged = moved ? (1.0f < e->cfg.cvthres) : (0.0f < e->cfg.cvthres);
        }
    }
    return NEMGPU_OK;
}
// one or more iterations, no criterion test: pipelined, or step by step for an engine with an observed mask
int iterate_plain(nemgpu_engine* e, int n_iters, bool with_init)
{
    return e->has_obs ? iterate_stepwise(e, n_iters, with_init) : iterate_pipelined(e, n_iters, with_init);
}

// CVTEST_CRIT (HasConverged, nem_alg.c:2090-2105): iterate until the chosen criterion (M, DEFAULT_CRIT nem_typ.h:80)
// moves by less than the threshold, relatively.  The criterion is an i-ordered float sum over all families that the
// loop does not otherwise need, so this test runs one iteration per host round trip: iteration, criteria, decision.
// The value the first iteration is compared with: 0 (Criteria = {0}, nem_exe.c:264) or, for a run that logs, the
// criterion of the initial partition (WriteLogCrit at the end of the initial sweep, nem_alg.c:1980, 2398).
int iterate_crit(nemgpu_engine* e, int n_iters, bool with_init)
{
    int r;
    if (with_init) {
        if ((r = iterate_plain(e, 0, true))) return r;
        e->crit_ref = 0.0f;
        if (e->cfg.cvtest == NEMGPU_CV_CRIT_LOGGED) {
            float c6[6];
            if ((r = criteria(e, c6, -1))) return r;
            e->crit_ref = c6[3];
        }
    }
    for (int it = 0; it < n_iters && !e->converged && e->status == NEMGPU_OK; it++) {
        const float oldcrit = e->crit_ref;
        if ((r = iterate_plain(e, 1, false))) return r;
        if (e->status != NEMGPU_OK) break;
        float c6[6];
        if ((r = criteria(e, c6, -1))) return r;
        const float curcrit = c6[3];
        e->crit_ref = curcrit;
        float critdif;
        if (curcrit != 0) critdif = (float)fabs((curcrit - oldcrit) / curcrit);
        else critdif = FLT_MAX;                                    // MAXFLOAT
        if (critdif < e->cfg.cvthres) e->converged = 1;
    }
    return NEMGPU_OK;
}

bool crit_test(const nemgpu_engine* e) { return e->cfg.cvtest == NEMGPU_CV_CRIT || e->cfg.cvtest == NEMGPU_CV_CRIT_LOGGED; }

int iterate(nemgpu_engine* e, int n_iters, bool with_init = false)
{
    return crit_test(e) ? iterate_crit(e, n_iters, with_init) : iterate_plain(e, n_iters, with_init);
}

// ============================================================================================
// Lock-step batches: B independent problems, ONE launch per step for all of them.
// PPanGGOLiN solves many NEM problems of the same kind -- one per 500-organism chunk (ppanggolin.py:1045-1086),
// fifty random starts of one problem in RandNemAlgo (nem_alg.c:1574-1742) -- and one problem of that size leaves
// the chip >95 % empty.  Every engine of a batch runs the code it would run alone, with its launches RECORDED
// (nem_kernels.hpp); the records of all members agree position by position (same kernels, own arguments), so each
// position goes out once, problem = blockIdx.z, and the host synchronises once per batch for everybody.  Members
// whose sequences differ (another batch length, a missing bookkeeping step) form groups of their own.
// ============================================================================================
int zip_reserve(nemgpu_engine* lead, size_t bytes)
{
    nemgpu_engine::ZipContext* z = zip_context(lead);
    if (z->zip_cap >= bytes) return NEMGPU_OK;
    HIPCHK(hipStreamSynchronize(lead->stream));
    z->zip_graphs.clear();                                        // (they hold the old slab's addresses)
    pool_put(lead->device, true, z->zip_host, z->zip_host_size);
    pool_put(lead->device, false, z->zip_dev, z->zip_dev_size);
    z->zip_host = nullptr; z->zip_dev = nullptr; z->zip_cap = 0;
    size_t cap = (size_t)1 << 20, got = 0;
    while (cap < bytes) cap *= 2;
    HIPCHK(pool_get(lead->device, true, cap, &z->zip_host, &got)); z->zip_host_size = got;
    HIPCHK(pool_get(lead->device, false, cap, &z->zip_dev, &got)); z->zip_dev_size = got;
    z->zip_cap = cap;
    return NEMGPU_OK;
}

// may two members' recorded sequences go out as one?  (launch for launch the same kernel, variant, block, grid height)
bool same_sequence(const Recorder& a, const Recorder& b)
{
    bool same = a.ops.size() == b.ops.size();
    for (size_t t = 0; same && t < a.ops.size(); t++) same = same_launch(a.ops[t], b.ops[t]);
    return same;
}

// One position of a zipped sequence in an argument slab: from `args_off` on the B members' argument blocks, `stride`
// bytes apart (a block's size rounded up to 16), behind them (gx_off) their grid widths, rounded up to 16 bytes.
struct ZipPos { int kind, variant, B, stride; size_t args_off, gx_off; unsigned max_gx, gy, block; };

// Lays out the sequences of `groups` (each a list of members, indices into recs, whose sequences same_sequence holds
// alike) in `slab`, position after position and group after group; *out: the positions.  Returns the size.
// slab == nullptr: nothing is written and the same size and positions come out -- what a caller reserves by.
size_t zip_pack(char* slab, const Recorder* recs, const std::vector<std::vector<int>>& groups, std::vector<ZipPos>* out)
{
    size_t off = 0;
    if (out) out->clear();
    for (const std::vector<int>& g : groups) {
        const int B = (int)g.size();
        for (size_t t = 0; t < recs[g[0]].ops.size(); t++) {
            const OpRecord& o0 = recs[g[0]].ops[t];
            const int stride = (o0.nbytes + 15) & ~15;
            ZipPos L{o0.kind, o0.variant, B, stride, off, off + (size_t)B * stride, 0, o0.gy, o0.block};
            for (int b = 0; b < B; b++) {
                const OpRecord& o = recs[g[b]].ops[t];
                L.max_gx = std::max(L.max_gx, o.gx);
                if (slab == nullptr) continue;
                memcpy(slab + L.args_off + (size_t)b * stride, o.args, (size_t)o0.nbytes);
                reinterpret_cast<int*>(slab + L.gx_off)[b] = (int)o.gx;
            }
            if (out) out->push_back(L);
            off = L.gx_off + (((size_t)B * sizeof(int) + 15) & ~(size_t)15);
        }
    }
    return off;
}

// ... and its launch, the slab being at `dev` on the device
void zip_issue(const ZipPos& L, const char* dev, hipStream_t s)
{
    launch_zipped(L.kind, L.variant, L.B, dev + L.args_off, L.stride, reinterpret_cast<const int*>(dev + L.gx_off), L.max_gx, L.gy,
                  L.block, s);
}

// issue the recorded sequences of `members` (indices into recs / E) on the lead's stream; flags_words > 0: behind them,
// one copy of every member's flag block to the host (gathered on the device first)
int zip_and_launch(nemgpu_engine* lead, const std::vector<Recorder>& recs, const std::vector<int>& members, size_t flags_words)
{
    if (members.empty()) return NEMGPU_OK;
    nemgpu_engine::ZipContext* z = zip_context(lead);
    // groups of members with the same sequence of (kernel, variant, block, grid height)
    std::vector<std::vector<int>> groups;
    for (int m : members) {
        bool placed = false;
        for (auto& g : groups) {
            if (same_sequence(recs[g[0]], recs[m])) { g.push_back(m); placed = true; break; }
        }
        if (!placed) groups.push_back({m});
    }
    int r = zip_reserve(lead, zip_pack(nullptr, recs.data(), groups, nullptr));
    if (r) return r;
    std::vector<ZipPos> launches;
    const size_t off = zip_pack(z->zip_host, recs.data(), groups, &launches);
    std::vector<uint64_t> desc;                                   // everything a captured sequence depends on
    for (const ZipPos& L : launches)
        for (uint64_t v : {(uint64_t)L.kind, (uint64_t)L.variant, (uint64_t)L.B, (uint64_t)L.stride, (uint64_t)L.max_gx, (uint64_t)L.gy,
                           (uint64_t)L.block, (uint64_t)L.args_off, (uint64_t)L.gx_off}) desc.push_back(v);
    desc.push_back(flags_words);
    if (off == 0 && flags_words == 0) return NEMGPU_OK;
    if (off) HIPCHK(hipMemcpyAsync(z->zip_dev, z->zip_host, off, hipMemcpyHostToDevice, lead->stream));
    // The launches themselves depend only on the shape (kernels, grids, slab offsets), not on the argument blocks'
    // content: a shape seen before is replayed from its captured graph
    auto issue = [&]() -> int {
        for (const ZipPos& L : launches) zip_issue(L, z->zip_dev, lead->stream);
        if (flags_words)
            HIPCHK(hipMemcpyAsync(z->zip_flags_host, z->zip_flags_dev, flags_words * sizeof(int), hipMemcpyDeviceToHost, lead->stream));
        return NEMGPU_OK;
    };
    // Capturing and instantiating costs ~160 us per node (8 ms for a batch of 7 iterations) and a replay saves
    // 0.15-0.35 ms of issue time: a shape pays for its graph after some thirty replays.  The contexts live as long as
    // the process (a pangenome's chunks are hundreds of batches of one shape), so: from the fourth sighting on.
    Graphed how;
    if ((r = run_graphed(lead, &z->zip_graphs, desc, 4, lead->stream, issue, []() {}, &how))) return r;
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// record `fn(engine)` for every member, issue the records zipped, fetch every member's flag block, wait
template <typename F>
int lockstep(std::vector<nemgpu_engine*>& E, const std::vector<int>& members, std::vector<Recorder>& recs, F&& fn, bool fetch_flags)
{
    if (members.empty()) return NEMGPU_OK;
    nemgpu_engine* lead = E[0];
    HIPCHK(hipStreamSynchronize(lead->stream));                // (the argument slab of the previous step is free again)
    static const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    int r = NEMGPU_OK;
    for (int m : members) {
        recs[m].ops.clear();
        set_recorder(&recs[m]);
        r = fn(m);
        set_recorder(nullptr);
        if (r) return r;
    }
    const auto t1 = std::chrono::steady_clock::now();
    const size_t fw = C_WORDS + kFlagSetWords;             // (members of a lock-step batch use flag set 0 only)
    nemgpu_engine::ZipContext* z = zip_context(lead);
    if (fetch_flags) {
        // every member's flag block goes to one staging area on the device (a last zipped launch) and from there
        // to the host in ONE copy
        const size_t need = fw * E.size();
        if (z->zip_flags_cap < need) {
            pool_put(lead->device, true, (char*)z->zip_flags_host, z->zip_flags_host_size);
            pool_put(lead->device, false, (char*)z->zip_flags_dev, z->zip_flags_dev_size);
            z->zip_flags_host = nullptr; z->zip_flags_dev = nullptr; z->zip_flags_cap = 0;
            z->zip_graphs.clear();
            HIPCHK(pool_get(lead->device, true, need * sizeof(int), (char**)&z->zip_flags_host, &z->zip_flags_host_size));
            HIPCHK(pool_get(lead->device, false, need * sizeof(int), (char**)&z->zip_flags_dev, &z->zip_flags_dev_size));
            z->zip_flags_cap = need;
        }
        size_t slot = 0;
        for (int m : members) {
            set_recorder(&recs[m]);
            launch_copy_words(E[m]->flags_dev, z->zip_flags_dev + slot * fw, (int)fw, lead->stream);
            set_recorder(nullptr);
            slot++;
        }
    }
    if ((r = zip_and_launch(lead, recs, members, fetch_flags ? fw * members.size() : 0))) return r;
    const auto t2 = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(lead->stream));
    if (fetch_flags) {
        size_t slot = 0;
        for (int m : members) { memcpy(E[m]->flags_host, z->zip_flags_host + slot * fw, fw * sizeof(int)); slot++; }
    }
    if (prof) {
        const auto t3 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[lockstep] members %zu ops %zu: record %.0f us, zip+launch+copies %.0f us, wait %.0f us\n", members.size(),
                recs[members[0]].ops.size(), us(t0, t1), us(t1, t2), us(t2, t3));
    }
    return NEMGPU_OK;
}

// the EM loops of several engines in lock step (all on E[0]'s stream); L: their cursors after loop_begin
// a member whose matrix was uploaded by nemgpu_solve_many's builders: its device layouts ride at the head of the group's
// first step (recorded: one launch each for all members)
static void pending_layout(nemgpu_engine* e)
{
    if (!e->layout_pending) return;
    launch_layout(layout_args(e, e->xf_stage), e->stream);
    e->layout_pending = false;
}

int iterate_many(std::vector<nemgpu_engine*>& E, std::vector<LoopCursor>& L)
{
    int r;
    const int B = (int)E.size();
    std::vector<Recorder> recs((size_t)B);
    std::vector<int> members;
    // TIE_LIBC members: the two initial sweeps, completed one after the other (see libc_init_a)
    members.clear();
    for (int i = 0; i < B; i++) if (L[i].first && E[i]->libc() && !libc_init_pipelined()) members.push_back(i);
    if (!members.empty()) {
        std::vector<SweepCtx> ctx((size_t)B);
        if ((r = lockstep(E, members, recs, [&](int m) { pending_layout(E[m]); return libc_init_a(E[m], ctx[m]); }, true))) return r;
        for (int m : members) if ((r = sweep_complete(E[m], ctx[m], nullptr, nullptr, true))) return r;
        if ((r = lockstep(E, members, recs, [&](int m) { return libc_init_b(E[m], ctx[m]); }, true))) return r;
        for (int m : members) if ((r = sweep_complete(E[m], ctx[m], nullptr, nullptr, true))) return r;
        if ((r = lockstep(E, members, recs, [&](int m) { return libc_init_c(E[m]); }, false))) return r;
        for (int m : members) { L[m].first = false; E[m]->draws_after_init = E[m]->draws; }
    }
    for (;;) {
        members.clear();
        for (int i = 0; i < B; i++) if (loop_wants_batch(E[i], L[i])) members.push_back(i);
        if (members.empty()) break;
        r = lockstep(E, members, recs, [&](int m) {
            pending_layout(E[m]);
            int rr = batch_plan(E[m], L[m]);
            if (rr == NEMGPU_OK) rr = batch_enqueue(E[m], L[m], false);
            return rr;
        }, true);
        if (r) return r;
        for (int m : members) { E[m]->n_plain++; if ((r = batch_finish(E[m], L[m]))) return r; }
    }
    return NEMGPU_OK;
}

// ---- RandNemAlgo's per-iteration log with the starts in lock step ------------------------------------------------
// What one start writes to <Fname>.log (nem_alg.c:1662-1669, 2361, 2398): line 0 for its initial partition, then a line
// per iteration -- the six criteria of the partition the E-step started from and of the one it left, both on the new
// densities, and the iteration's parameters.  The criteria are i-ordered float sums (four lone blocks per partition,
// 75-100 us at configs[1] size): one start after the other they are most of a logged iteration; with the starts in lock
// step the blocks of all starts run side by side.  The lines are kept per start and handed to the caller's writer in the
// reference's order afterwards.
//
// What every logged path shares.  A line on its way to the writer is a LogLine: a view of numbers someone else holds -- a
// staging slot on the host, the caller's arrays, a StartLogLine -- that emit() turns into the caller's event.
struct LogLine {
    int kind = NEMGPU_LOG_LINE, iter = 0, emptyk = 0;
    const float *cb = nullptr, *ca = nullptr, *prop = nullptr, *center = nullptr, *disp = nullptr, *nb = nullptr;   // (nb: not in line 0; all an emptied class has)
    static LogLine empty(int iter, int emptyk, const float* sizes) { return {NEMGPU_LOG_EMPTY, iter, emptyk, nullptr, nullptr, nullptr, nullptr, nullptr, sizes}; }
};
static void emit(nemgpu_log_fn fn, void* user, int start, const LogLine& ln)
{
    const nemgpu_log_event ev{ln.kind, start, ln.iter, ln.emptyk, ln.cb, ln.ca, ln.prop, ln.center, ln.disp, ln.nb};   // (the header's order)
    fn(&ev, user);
}
// the owning copy of a line (the starts in lock step keep theirs until the round is through): a view into its own numbers
struct StartLogLine {
    LogLine v; std::vector<float> buf;
    StartLogLine(const LogLine& src, size_t k, size_t kd) : v(src)
    {
        buf.reserve(2 * (6 + k + kd));                             // (no growth below: the pointers stay good, also when the line is moved)
        auto own = [&](const float*& p, size_t count) { if (p) { buf.insert(buf.end(), p, p + count); p = buf.data() + buf.size() - count; } };
        own(v.cb, 6); own(v.ca, 6); own(v.prop, k); own(v.center, kd); own(v.disp, kd); own(v.nb, k);
    }
    StartLogLine(StartLogLine&&) = default;                        // (and no copies: theirs would point into the original)
};

// a device and a pinned block from the pool (either may be left out) for the length of a scope: whichever way the scope is
// left, the stream that may still be copying into them is waited for before they go back
struct PooledPair {
    int device; hipStream_t stream;
    char* dev = nullptr; char* host = nullptr; size_t dev_size = 0, host_size = 0;
    PooledPair(int device_, hipStream_t s) : device(device_), stream(s) {}
    PooledPair(const PooledPair&) = delete;
    hipError_t get(bool pinned, size_t bytes) { return pool_get(device, pinned, bytes, pinned ? &host : &dev, pinned ? &host_size : &dev_size); }
    int get_both(size_t bytes, const char* no_pinned)
    {
        HIPCHK(get(false, bytes));
        if (get(true, bytes) != hipSuccess) { set_error(no_pinned); return NEMGPU_E_DEVICE; }
        return NEMGPU_OK;
    }
    void put() { pool_put(device, false, dev, dev_size); pool_put(device, true, host, host_size); dev = host = nullptr; }   // (nothing queued targets them any more)
    ~PooledPair() { if (dev || host) { (void)hipStreamSynchronize(stream); put(); } }
};

// The lines' staging slots, each [6 criteria before | 6 criteria after | the engine's parameter block].  With a device block
// the words go there by recordable copy kernels and fetch() brings the slots to the pinned block; without, by copy commands.
struct LogSlot {
    enum Side : size_t { kBefore = 0, kAfter = 6, kPar = 12 };
    const nemgpu_engine* e;                                        // (its parameter block's shape, its stream: a group's lead)
    PooledPair st{e->device, e->stream};
    size_t bytes(int slots) const { return (size_t)slots * (kPar + e->par_words) * sizeof(float); }
    float* at(char* block, int m, size_t side) const { return reinterpret_cast<float*>(block) + (size_t)m * (kPar + e->par_words) + side; }
    float* par_dev(int m) const { return at(st.dev, m, kPar); }
    hipError_t put(int m, Side side, const float* src) const       // the six criteria at `src`, or the parameter block
    {
        const size_t count = side == kPar ? e->par_words : 6;
        if (!st.dev) return hipMemcpyAsync(at(st.host, m, side), src, count * sizeof(float), hipMemcpyDeviceToHost, st.stream);
        launch_copy_words(reinterpret_cast<const int*>(src), reinterpret_cast<int*>(at(st.dev, m, side)), (int)count, st.stream);
        return hipSuccess;
    }
    hipError_t fetch(int slots) const                              // the first `slots` to the host, and the wait for them
    {
        const hipError_t err = hipMemcpyAsync(st.host, st.dev, bytes(slots), hipMemcpyDeviceToHost, st.stream);
        return err != hipSuccess ? err : hipStreamSynchronize(st.stream);
    }
    LogLine line(int m, int iter) const                            // (host slot m, once the stream has been waited for)
    {
        const float *f = at(st.host, m, 0), *p = f + kPar;
        return {NEMGPU_LOG_LINE, iter, 0, f + kBefore, f + kAfter, p, p + e->par_o_center, p + e->par_o_disp, p + e->par_o_nb};
    }
};

// the line of an iteration whose sweep the host had to finish: the plain sequence of calls
static int plain_line(nemgpu_engine* e, float cb[6], float ca[6], float* prop, float* center, float* disp, float* nb)
{
    int r;
    if ((r = criteria(e, cb, (e->cur + 2) % 3)) || (r = criteria(e, ca, -1))) return r;
    return nemgpu_get_results(e, prop, center, disp, nb, nullptr);
}
// EstimSizes (nem_mod.c:1275-1317) ran before the empty class was found: i-ordered float sums per class
static int estim_sizes_host(nemgpu_engine* e, float* nb)
{
    std::vector<float> part((size_t)e->n * e->k);
    const int r = nemgpu_get_partition(e, part.data());
    for (int h = 0; h < e->k && r == NEMGPU_OK; h++) {
        nb[h] = 0.0f;
        for (int i = 0; i < e->n; i++) nb[h] += part[(size_t)i * e->k + h];
    }
    return r;
}

// E: the starts' engines behind their initial partitions (cur = 2; blind partition in buffer 1); L: their cursors with
// first = false; host_par: the starts' own parameters, `par` floats apart (prop | center | disp)
static int iterate_many_logged(std::vector<nemgpu_engine*>& E, std::vector<LoopCursor>& L, const float* host_par, size_t par,
                               std::vector<std::vector<StartLogLine>>& logs)
{
    int r;
    const int B = (int)E.size();
    nemgpu_engine* lead = E[0];
    const int k = lead->k, d = lead->d;
    const size_t kd = (size_t)k * d;
    std::vector<Recorder> recs((size_t)B);
    std::vector<int> members((size_t)B), left((size_t)B), it_no((size_t)B, 0);
    for (int i = 0; i < B; i++) { members[i] = i; left[i] = L[i].remaining; }
    LogSlot slot{lead};
    if ((r = slot.st.get_both(slot.bytes(B), "no pinned memory for the starts' log lines"))) return r;
    auto two_criteria = [&](int m, int before, int after) -> int {   // (recorded: zipped over the members)
        nemgpu_engine* c = E[m];
        int rr = criteria_enqueue(c, before);
        if (rr == NEMGPU_OK) HIPCHK(slot.put(m, LogSlot::kBefore, c->crit6_dev));
        if (rr == NEMGPU_OK) rr = criteria_enqueue(c, after);
        if (rr == NEMGPU_OK) HIPCHK(slot.put(m, LogSlot::kAfter, c->crit6_dev));
        return rr;
    };
    // ---- line 0: the initial partition (before: the blind sweep's, buffer 1; after: the beta sweep's, buffer 2)
    if ((r = lockstep(E, members, recs, [&](int m) { return two_criteria(m, 1, 2); }, false))) return r;
    HIPCHK(slot.fetch(B));
    for (int m = 0; m < B; m++) {
        LogLine ln = slot.line(m, 0);                              // (its criteria; the parameters are the start's own, no sizes yet)
        ln.prop = host_par + (size_t)m * par; ln.center = ln.prop + k; ln.disp = ln.center + kd; ln.nb = nullptr;
        logs[(size_t)m].emplace_back(ln, (size_t)k, kd);
    }
    // ---- one iteration per step for every start that still runs
    float cb[6], ca[6];
    std::vector<float> own((size_t)2 * k + 2 * kd);                // (a line the host puts together: prop | center | disp | sizes)
    float* const own_nb = own.data() + k + 2 * kd;
    for (;;) {
        members.clear();
        for (int i = 0; i < B; i++) if (left[i] > 0 && !E[i]->converged && E[i]->status == NEMGPU_OK) members.push_back(i);
        if (members.empty()) break;
        r = lockstep(E, members, recs, [&](int m) -> int {
            nemgpu_engine* c = E[m];
            L[m].remaining = 1;
            int rr = batch_plan(c, L[m]);
            const int oldbuf = L[m].base, newbuf = (L[m].base + 1) % 3;
            if (rr == NEMGPU_OK) rr = batch_enqueue(c, L[m], false);
            if (rr == NEMGPU_OK) rr = two_criteria(m, oldbuf, newbuf);           // (speculated: void if the sweep was not through)
            if (rr == NEMGPU_OK) HIPCHK(slot.put(m, LogSlot::kPar, c->prop));
            return rr;
        }, true);
        if (r) return r;
        HIPCHK(slot.fetch(B));
        for (int m : members) {
            nemgpu_engine* c = E[m];
            const bool clean = c->h_ctrl()[C_NEED_ROUNDS] == 0 && c->h_ctrl()[C_STATUS] != NEMGPU_W_EMPTYCLASS;
            c->n_plain++;
            if ((r = batch_finish(c, L[m]))) return r;
            left[m] -= 1; it_no[m] += 1;
            LogLine ln = slot.line(m, it_no[m]);
            if (c->status == NEMGPU_W_EMPTYCLASS) {
                if ((r = estim_sizes_host(c, own_nb))) return r;
                ln = LogLine::empty(it_no[m], c->emptyk, own_nb);
            } else if (!clean) {                                   // (the sweep was finished from the host, this start alone)
                ln.cb = cb; ln.ca = ca; ln.prop = own.data(); ln.center = ln.prop + k; ln.disp = ln.center + kd; ln.nb = own_nb;
                if ((r = plain_line(c, cb, ca, own.data(), own.data() + k, own.data() + k + kd, own_nb))) return r;
            }
            logs[(size_t)m].emplace_back(ln, (size_t)k, kd);
        }
    }
    for (int i = 0; i < B; i++) L[i].remaining = 0;
    return NEMGPU_OK;
}

// several whole runs (nemgpu_run) in lock step; every engine complete (matrix, graph, parameters, configuration), all on
// one device.  They are run on E[0]'s stream for the duration.
// A group's results in one block (nemgpu_solve_many): every member's partition and parameter block (the layout of
// nemgpu_get_results' staging block) are copied by zipped launches behind the criteria into `dev`, `stride` bytes apart,
// and reach `host` (pinned) in ONE copy before run_many returns.  Per-member copies from the workers' threads cost
// 0.2-0.7 ms each once 8-16 threads were inside the runtime together.
struct GroupFetch { char* dev = nullptr; char* host = nullptr; size_t stride = 0; bool filled = false; };
static size_t result_part_bytes(const nemgpu_engine* e) { return e->ncem() ? ((size_t)e->n + 3) & ~(size_t)3 : sizeof(float) * (size_t)e->n * e->k; }
static size_t result_block_bytes(const nemgpu_engine* e) { return result_part_bytes(e) + sizeof(float) * e->par_words; }

// a staging block [partition (b_part bytes) | prop | center | disp | nbobs_k] into the caller's arrays
static void result_unpack(const nemgpu_engine* e, const char* st, size_t b_part, float* prop, float* center, float* disp, float* nbobs_k, float* c_nk)
{
    const size_t kd = (size_t)e->k * e->d, n = (size_t)e->n, k = (size_t)e->k;
    const char* par = st + b_part;
    if (c_nk) {
        if (e->ncem()) {
            const uint8_t* lab = (const uint8_t*)st;
            for (size_t i = 0; i < n; i++)                          // LabelToClassVector, nem_alg.c:649-664
                for (size_t h = 0; h < k; h++) c_nk[i * k + h] = ((size_t)(lab[i] & 0x7F) == h) ? 1.0f : 0.0f;
        } else memcpy(c_nk, st, sizeof(float) * n * k);
    }
    if (prop) memcpy(prop, par, sizeof(float) * k);
    if (center) memcpy(center, par + sizeof(float) * e->par_o_center, sizeof(float) * kd);
    if (disp) memcpy(disp, par + sizeof(float) * e->par_o_disp, sizeof(float) * kd);
    if (nbobs_k) memcpy(nbobs_k, par + sizeof(float) * e->par_o_nb, sizeof(float) * k);
}

// What a run of zero iterations still owes before its criteria, nem_alg.c:1845-1851.  (nemgpu_run reads a fuzzy M-step's
// fault flag between these calls: another sequence, stated there.)
int finish_unstepped(nemgpu_engine* e)
{
    int r;
    if ((r = do_mstep(e)) || (r = do_tables(e))) return r;
    return do_density(e);
}

// The six criteria of every member of a lock-step group (all on E[0]'s stream) into crit[m]: the members' criteria
// launches zipped, behind each member's its six words to the group's staging area, ONE copy to the host, ONE wait -- a
// copy per member into pageable memory cost ~20 us each (16 problems: 0.3 ms of a 2 ms batch), and is what remains
// where the group has no staging area of that size.  with_member(m) is recorded behind member m's criteria in the same
// pass; behind_pass() enqueues, behind the pass, what the same wait is to cover.
int criteria_many(std::vector<nemgpu_engine*>& E, float (*crit)[6], const std::function<void(int)>& with_member = nullptr,
                  const std::function<int()>& behind_pass = nullptr)
{
    int r;
    const int B = (int)E.size();
    nemgpu_engine* lead = E[0];
    std::vector<Recorder> recs((size_t)B);
    std::vector<int> all((size_t)B);
    for (int m = 0; m < B; m++) all[m] = m;
    nemgpu_engine::ZipContext* z = zip_context(lead);
    const bool staged = z != nullptr && z->zip_flags_dev != nullptr && z->zip_flags_host != nullptr && z->zip_flags_cap >= (size_t)8 * B;
    if ((r = lockstep(E, all, recs, [&](int m) {
            const int rr = criteria_enqueue(E[m], -1);
            if (rr == NEMGPU_OK && staged) launch_copy_words(reinterpret_cast<const int*>(E[m]->crit6_dev), z->zip_flags_dev + (size_t)8 * m, 6, lead->stream);
            if (rr == NEMGPU_OK && with_member) with_member(m);
            return rr;
        }, false))) return r;
    if (behind_pass && (r = behind_pass())) return r;
    if (staged) HIPCHK(hipMemcpyAsync(z->zip_flags_host, z->zip_flags_dev, (size_t)8 * B * sizeof(int), hipMemcpyDeviceToHost, lead->stream));
    else for (int m = 0; m < B; m++) HIPCHK(hipMemcpyAsync(crit[m], E[m]->crit6_dev, 6 * sizeof(float), hipMemcpyDeviceToHost, lead->stream));
    HIPCHK(hipStreamSynchronize(lead->stream));
    if (staged) for (int m = 0; m < B; m++) memcpy(crit[m], z->zip_flags_host + (size_t)8 * m, 6 * sizeof(float));
    return NEMGPU_OK;
}

int run_many(std::vector<nemgpu_engine*>& E, nemgpu_result* results, GroupFetch* gf = nullptr)
{
    int r;
    const int B = (int)E.size();
    nemgpu_engine* lead = E[0];
    for (int i = 0; i < B; i++) {
        if (E[i]->device != lead->device) { set_error("a batch lives on one device"); return NEMGPU_E_ARG; }
        if (E[i]->lo != 0 || E[i]->hi != E[i]->n_total) { set_error("sharded engines cannot join a batch"); return NEMGPU_E_ARG; }
    }
    // The members run on the lead's stream for the duration.  Whatever way this function is left, the lead's stream is
    // waited for BEFORE the members get their own streams back: a later call on a member's stream must not race with
    // work still queued on the lead's.
    struct StreamLoan {
        std::vector<nemgpu_engine*>& E; nemgpu_engine* lead; std::vector<hipStream_t> own; int taken = 0;
        StreamLoan(std::vector<nemgpu_engine*>& E_, nemgpu_engine* l) : E(E_), lead(l), own(E_.size()) {}
        void give_back() {
            if (taken == 0) return;
            (void)hipStreamSynchronize(lead->stream);
            for (int i = 0; i < taken; i++) E[i]->stream = own[i];
            taken = 0;
        }
        ~StreamLoan() { give_back(); }
    } loan(E, lead);
    static const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    auto tp = std::chrono::steady_clock::now();
    double laps[6] = {0, 0, 0, 0, 0, 0};
    auto lap = [&](int j) { auto t1 = std::chrono::steady_clock::now(); laps[j] += std::chrono::duration<double>(t1 - tp).count() * 1e6; tp = t1; };
    for (int i = 0; i < B; i++) {
        if (E[i]->ready_pending) {                             // (built by nemgpu_solve_many: see ready_ev)
            HIPCHK(hipStreamWaitEvent(lead->stream, E[i]->ready_ev, 0));
            E[i]->ready_pending = false;
        } else HIPCHK(hipStreamSynchronize(E[i]->stream));     // (an early return gives back what was taken so far)
        loan.own[i] = E[i]->stream;
        E[i]->stream = lead->stream;
        loan.taken = i + 1;
    }
    auto restore = [&]() { loan.give_back(); };
    for (int i = 0; i < B; i++) {
        if (crit_test(E[i])) {                                     // (a host round trip per iteration: nothing to share)
            for (int j = 0; j < B; j++) pending_layout(E[j]);      // (still on the lead's stream, behind the waits for the uploads)
            restore();
            for (int j = 0; j < B; j++) { int rr = nemgpu_run(E[j], results ? &results[j] : nullptr); if (rr) return rr; }
            return NEMGPU_OK;
        }
    }
    lap(0);
    auto t0 = std::chrono::steady_clock::now();
    std::vector<LoopCursor> L((size_t)B);
    r = NEMGPU_OK;
    for (int i = 0; i < B && r == NEMGPU_OK; i++) { E[i]->draws = 0; r = loop_begin(E[i], L[i], E[i]->cfg.it_max, true); }
    lap(1);
    if (r == NEMGPU_OK) r = iterate_many(E, L);
    for (int i = 0; i < B; i++) pending_layout(E[i]);             // (it_max 0: no step has carried them)
    lap(2);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < B && r == NEMGPU_OK; i++)
        if (E[i]->iters == 0) r = finish_unstepped(E[i]);
    lap(3);
    if (r == NEMGPU_OK && results != nullptr) {
        // with the criteria, in the same pass and under the same wait: every member's results to the group's block
        std::vector<float> crits((size_t)B * 6);
        float (*crit)[6] = reinterpret_cast<float (*)[6]>(crits.data());
        r = criteria_many(E, crit, [&](int m) {
            if (gf == nullptr) return;
            nemgpu_engine* e = E[m];
            char* dst = gf->dev + gf->stride * (size_t)m;
            const size_t b_part = result_part_bytes(e);
            const void* part = e->ncem() ? (const void*)(e->lab[e->cur] + e->lo) : (const void*)(e->cbuf[e->cur] + (size_t)e->lo * e->k);
            launch_copy_words(reinterpret_cast<const int*>(part), reinterpret_cast<int*>(dst), (int)(b_part / 4), lead->stream);
            launch_copy_words(reinterpret_cast<const int*>(e->prop), reinterpret_cast<int*>(dst + b_part), (int)e->par_words, lead->stream);
        }, [&]() -> int {
            if (gf == nullptr) return NEMGPU_OK;
            HIPCHK(hipMemcpyAsync(gf->host, gf->dev, gf->stride * (size_t)B, hipMemcpyDeviceToHost, lead->stream));
            gf->filled = true;                                     // (once criteria_many's wait is over)
            return NEMGPU_OK;
        });
        for (int i = 0; i < B && r == NEMGPU_OK; i++) {
            fill_result(E[i], &results[i]);
            results[i].loop_seconds = secs;
            memcpy(results[i].crit, crit[i], sizeof crit[i]);
        }
    }
    lap(4);
    restore();
    lap(5);
    if (prof) fprintf(stderr, "[run_many] %d members: waits for the uploads %.0f us, loop_begin %.0f, iterations %.0f, it_max 0 %.0f, criteria + results %.0f, streams back %.0f\n",
                      B, laps[0], laps[1], laps[2], laps[3], laps[4], laps[5]);
    return r;
}

int ensure_crit_buffers(nemgpu_engine* e)
{
    alloc_for(e);
    int r;
    size_t nk = (size_t)e->n * e->k;
    if (!e->crit_dik) {
        if ((r = dev_alloc(&e->crit_dik, nk))) return r;
        if ((r = dev_alloc(&e->crit_gik, nk))) return r;
        if ((r = dev_alloc(&e->crit_lfi, (size_t)e->n))) return r;
        if ((r = dev_alloc(&e->crit_lzi, (size_t)e->n))) return r;
        if ((r = dev_alloc(&e->crit6_dev, 16))) return r;     // six criteria + the four chains' results
    }
    if (e->ncem() && !e->c_onehot) { if ((r = dev_alloc(&e->c_onehot, (size_t)e->n_total * e->k))) return r; }
    return NEMGPU_OK;
}

// ComputeCrit on the partition in buffer `buf` (default: the current one) with the current densities: the launches.
// second: the evaluation writes the crit2_* set of buffers (criteria_pair_enqueue has made them)
int criteria_enqueue(nemgpu_engine* e, int buf = -1, bool second)
{
    int r;
    if (e->lo != 0 || e->hi != e->n_total) { set_error("criteria need the whole partition on one engine"); return NEMGPU_E_FUNCARG; }
    if ((r = ensure_crit_buffers(e))) return r;
    if (buf < 0) buf = e->cur;
    const float* c = e->cbuf[buf];
    if (e->ncem()) {
        float* onehot = second ? e->c_onehot2 : e->c_onehot;
        launch_onehot(OnehotArgs{e->n_total, e->k, e->lab[buf], onehot}, e->stream);
        c = onehot;
    }
    launch_criteria(crit_args(e, c, second), e->stream);
    if (!current_recorder()) HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}
// The criteria of TWO partitions of the engine (label / membership buffers buf_a and buf_b) in the same launches --
// problem = blockIdx.z, through the kernels' batched twins: the i-ordered reductions are four lone blocks each and
// take as long for two partitions as for one.  Results: crit6_dev (buf_a), crit2_6 (buf_b).
constexpr size_t kCritPairBytes = 2048;                // crit_pair_dev: the two evaluations' records, packed (under 1 KB)
int criteria_pair_enqueue(nemgpu_engine* e, int buf_a, int buf_b)
{
    int r;
    if ((r = ensure_crit_buffers(e))) return r;
    const size_t nk = (size_t)e->n * e->k;
    if (!e->crit2_dik) {
        alloc_for(e);
        if ((r = dev_alloc(&e->crit2_dik, nk))) return r;
        if ((r = dev_alloc(&e->crit2_gik, nk))) return r;
        if ((r = dev_alloc(&e->crit2_lfi, (size_t)e->n))) return r;
        if ((r = dev_alloc(&e->crit2_lzi, (size_t)e->n))) return r;
        if ((r = dev_alloc(&e->crit2_6, 16))) return r;
        if (e->ncem()) { if ((r = dev_alloc(&e->c_onehot2, (size_t)e->n_total * e->k))) return r; }
        if ((r = dev_alloc(&e->crit_pair_dev, kCritPairBytes))) return r;
    }
    // the two evaluations as each would run alone, recorded; their launches are alike position by position
    Recorder recs[2];
    const int bufs[2] = {buf_a, buf_b};
    for (int p = 0; p < 2; p++) {
        recs[p].ops.reserve(4);                            // (one-hot, terms, reduce, final)
        set_recorder(&recs[p]);
        r = criteria_enqueue(e, bufs[p], p == 1);
        set_recorder(nullptr);
        if (r) return r;
    }
    if (!same_sequence(recs[0], recs[1])) { set_error("the paired criteria's launches differ"); return NEMGPU_E_INTERNAL; }
    const std::vector<std::vector<int>> both{{0, 1}};
    if (zip_pack(nullptr, recs, both, nullptr) > kCritPairBytes) { set_error("argument slab of the paired criteria"); return NEMGPU_E_INTERNAL; }
    char* st = stage(e, kCritPairBytes);
    if (!st) { set_error("no staging memory for the paired criteria"); return NEMGPU_E_DEVICE; }
    memset(st, 0, kCritPairBytes);
    std::vector<ZipPos> pos;
    zip_pack(st, recs, both, &pos);
    HIPCHK(hipMemcpyAsync(e->crit_pair_dev, st, kCritPairBytes, hipMemcpyHostToDevice, e->stream));
    for (const ZipPos& L : pos) zip_issue(L, e->crit_pair_dev, e->stream);
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

int criteria(nemgpu_engine* e, float crit6[6], int buf = -1)
{
    int r;
    if ((r = criteria_enqueue(e, buf))) return r;
    HIPCHK(hipMemcpyAsync(crit6, e->crit6_dev, 6 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NEMGPU_OK;
}

int reset_device(nemgpu_engine* e)
{
    if (e->have_params && e->parent == nullptr) {
        // (the initial block's tail, where nbobs_k is, stays zero)
        HIPCHK(hipMemcpyAsync(e->prop, e->prop0, sizeof(float) * e->par_words, hipMemcpyDeviceToDevice, e->stream));
    } else {
        if (e->have_params) {
            HIPCHK(hipMemcpyAsync(e->prop, e->prop0, sizeof(float) * e->k, hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(e->center, e->center0, sizeof(float) * e->k * e->d, hipMemcpyDeviceToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(e->disp, e->disp0, sizeof(float) * e->k * e->d, hipMemcpyDeviceToDevice, e->stream));
        }
        HIPCHK(hipMemsetAsync(e->nbobs_k, 0, sizeof(float) * e->k, e->stream));
    }
    HIPCHK(hipMemsetAsync(e->sweep_next, 0, sizeof(int), e->stream));
    return clear_fault(e);
}

int flush_reset(nemgpu_engine* e)
{
    if (!e->reset_pending) return NEMGPU_OK;
    e->reset_pending = false;
    return reset_device(e);
}

// host half now; the device half (initial parameters back in place, counters cleared) before the next thing that
// looks at the device state -- or never, when that is a run whose first launch does it anyway (enqueue_init)
int reset_state(nemgpu_engine* e, bool lazy)
{
    if (lazy) e->reset_pending = true;
    else { e->reset_pending = false; int r0 = reset_device(e); if (r0) return r0; }
    e->tables_fresh = false;
    e->density_fresh = false;
    e->cur = 0; e->sweep_counter = 0;
    e->iters = 0; e->converged = 0; e->emptyk = 0; e->status = NEMGPU_OK;
    e->zero_density = 0; e->first_zero = -1; e->sweep_rounds = 0; e->masks_valid = false;
    e->draws = 0;                                                  // srandom(seed): the stream starts over
    return NEMGPU_OK;
}

void fill_result(nemgpu_engine* e, nemgpu_result* res)
{
    if (!res) return;
    res->status = e->status; res->iters = e->iters; res->converged = e->converged; res->emptyk = e->emptyk;
    res->zero_density_sites = e->zero_density; res->first_zero_density_site = e->first_zero;
    res->sweep_rounds = e->sweep_rounds;
    res->tie_draws = e->draws;
}

}  // namespace

// nem_master.hip's HIP calls count for atfork_child as the engine's do
void nemk::note_hip_used() { g_hip_used.store(true); }

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

const char* nemgpu_last_error(void) { return g_last_error.c_str(); }

static const char kForkedMsg[] =
    "this process was forked from one that had already used the GPU: HIP is unusable in a forked child "
    "(start the workers with multiprocessing's 'spawn' or 'forkserver' method)";

int nemgpu_device_count(void)
{
    if (g_forked_after_hip.load()) return 0;                       // (no HIP call in such a child)
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int nemgpu_default_device(int* device)
{
    if (!device) return NEMGPU_E_FUNCARG;
    *device = 0;
    std::call_once(g_atfork_once, [] { pthread_atfork(nullptr, nullptr, atfork_child); });
    if (g_forked_after_hip.load()) { set_error(kForkedMsg); return NEMGPU_E_DEVICE; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no usable HIP device: this library has no CPU fallback");
        return NEMGPU_E_DEVICE;
    }
    g_hip_used.store(true);
    const char* s = getenv("NEM_MI355X_DEVICE");
    if (s == nullptr || s[0] == '\0') {
        // unset: a launcher's LOCAL_RANK when there is one (one process per GPU), else the calling thread's current HIP
        // device -- the embedding application's choice.  A pool of workers that selects nothing lands on device 0:
        // NEM_MI355X_DEVICE=auto spreads it (INTEGRATION.md says so first thing in its multi-GPU paragraph)
        if (const char* lr = getenv("LOCAL_RANK")) {
            char* end = nullptr;
            const long v = strtol(lr, &end, 10);
            if (end != lr && *end == '\0' && v >= 0) { *device = (int)((unsigned long)v % (unsigned long)ndev); return NEMGPU_OK; }
        }
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = 0; }
        *device = cur;
        return NEMGPU_OK;
    }
    if (!strcmp(s, "auto")) {
        unsigned long key = (unsigned long)getpid();
        if (const char* lr = getenv("LOCAL_RANK")) {
            char* end = nullptr;
            const long v = strtol(lr, &end, 10);
            if (end != lr && *end == '\0' && v >= 0) key = (unsigned long)v;
        }
        *device = (int)(key % (unsigned long)ndev);
        return NEMGPU_OK;
    }
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (end == s || *end != '\0' || v < 0 || v >= ndev) {
        set_error(std::string("NEM_MI355X_DEVICE=") + s + ": not a device index below " + std::to_string(ndev) + " (or \"auto\")");
        return NEMGPU_E_ARG;
    }
    *device = (int)v;
    return NEMGPU_OK;
}

int nemgpu_create(nemgpu_engine** out, int n_total, int d, int k, int site_lo, int site_hi, int device,
                  void* hip_stream)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (n_total <= 0 || d <= 0 || k <= 0 || k > kMaxKernelK || site_lo < 0 || site_hi > n_total || site_lo >= site_hi) {
        set_error("nemgpu_create: bad sizes (need n,d > 0, 1 <= k <= 32, 0 <= lo < hi <= n)");
        return NEMGPU_E_ARG;
    }
    if (n_total > (1 << 24)) {
        // class sizes are float sums of 0/1 memberships in the reference (EstimSizes, nem_mod.c:1293-1315): exact
        // integers only up to 2^24, which is what the popcount M-step reproduces
        set_error("nemgpu_create: more than 2^24 families (the reference's float class sizes stop being integers)");
        return NEMGPU_E_ARG;
    }
    std::call_once(g_atfork_once, [] { pthread_atfork(nullptr, nullptr, atfork_child); });
    if (g_forked_after_hip.load()) { set_error(kForkedMsg); return NEMGPU_E_DEVICE; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no usable HIP device: this library has no CPU fallback");
        return NEMGPU_E_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("nemgpu_create: bad device index"); return NEMGPU_E_ARG; }
    g_hip_used.store(true);
    HIPCHK(hipSetDevice(device));
    nemgpu_engine* e = new nemgpu_engine();
    e->n_total = n_total; e->n_true = n_total; e->d = d; e->k = k; e->lo = site_lo; e->hi = site_hi; e->n = site_hi - site_lo;
    e->device = device;
    e->npad = (e->n + 255) / 256 * 256;
    e->dpad = (d + 63) / 64 * 64;
    e->W = e->dpad / 32;
    e->wf = (d + 31) / 32;
    e->nw64 = (e->n + 63) / 64;
    e->cfg.algo = NEMGPU_ALGO_NCEM; e->cfg.beta = 0.5f; e->cfg.disper = NEMGPU_DISP_K_; e->cfg.propor = NEMGPU_PROP_K;
    e->cfg.cvtest = NEMGPU_CV_CLAS; e->cfg.cvthres = 1e-8f; e->cfg.it_max = 100; e->cfg.param_fix = 0;
    e->cfg.tie_rule = NEMGPU_TIE_HASH; e->cfg.tie_seed = 0;
    if (const char* g = getenv("NEM_MI355X_GRAPHS")) e->use_graphs = (g[0] != '0');   // 0: plain launches only
    if (const char* g = getenv("NEM_MI355X_SHADOW_VERIFY")) e->shadow_verify = (g[0] != '0');   // 0: every verifying round on its own
    e->flag_sets = e->shadow_verify ? 3 : 1;
    if (const char* g = getenv("NEM_MI355X_ROUND_COUNTS")) e->round_counts = (g[0] != '0');   // 0: a counts launch per iteration
    if (const char* g = getenv("NEM_MI355X_START_FUSED")) e->start_fused = (g[0] != '0');     // 0: k_finish + k_density start a run
    if (const char* g = getenv("NEM_MI355X_BLIND_FOLD")) e->blind_fold = (g[0] != '0');       // 0: the blind sweep as a launch of its own
    if (const char* g = getenv("NEM_MI355X_ROUNDS")) e->round_batch = std::max(2, std::min(kRoundBatchMax, atoi(g)));
    if (const char* g = getenv("NEM_MI355X_ROUNDS_ITER")) e->rounds_iter = std::max(2, std::min(e->round_batch, atoi(g)));
    e->rounds_iter = std::min(e->rounds_iter, e->round_batch);
    if (const char* g = getenv("NEM_MI355X_FAULT_INJECT")) e->fault_inject = !strcmp(g, "fuzzy_pc") ? 1 : 0;
    if (const char* g = getenv("NEM_MI355X_FF")) e->ff_mode = (g[0] == '0') ? 0 : (g[0] == '1') ? 1 : -1;   // 0 plain chain, 1 always
    if (const char* g = getenv("NEM_MI355X_FF_BATCH")) e->ff_batch = (g[0] != '0');   // 0: the word-synchronous chain everywhere
    if (const char* g = getenv("NEM_MI355X_MAP_MARGIN")) e->map_margin = (g[0] != '0');   // 0: every NCEM row normalised
    if (const char* g = getenv("NEM_MI355X_SORT")) e->use_sort = (g[0] != '0');       // 0: E1 lanes in family order
    if (hip_stream) { e->stream = (hipStream_t)hip_stream; e->own_stream = false; }
    else {
        if (pool_stream_get(device, &e->stream) != hipSuccess) { delete e; set_error("hipStreamCreate failed"); return NEMGPU_E_DEVICE; }
        e->own_stream = true;
    }
    int r = NEMGPU_OK;
    alloc_for(e);
    auto A = [&](int rr) { if (r == NEMGPU_OK) r = rr; };
    A(dev_alloc(&e->xw, (size_t)e->W * e->npad));
    A(dev_alloc(&e->xws, (size_t)((e->W + 3) / 4) * 4 * e->npad));   // uint4[ceil(W/4)][npad]
    A(dev_alloc(&e->perm, (size_t)e->npad));
    A(dev_alloc(&e->xt, (size_t)d * e->nw64));
    A(alloc_model_buffers(e));
    if (r == NEMGPU_OK && !e->flags_host &&
        pool_get(device, true, e->flag_words() * sizeof(int), (char**)&e->flags_host, &e->flags_host_size) != hipSuccess) {
        set_error("hipHostMalloc failed"); r = NEMGPU_E_DEVICE;
    }
    if (r != NEMGPU_OK) { nemgpu_destroy(e); return r; }
    e->draw_ctl = e->sweep_next + 8;                               // two of the spare words ahead of the ticket counters
    *out = e;
    return NEMGPU_OK;
}

void rccl_release(nemgpu_engine* e);

static std::atomic<long long> g_destroy_ns[5];               // NEM_MI355X_BATCH_PROF: where nemgpu_destroy's time goes
void nemgpu_destroy(nemgpu_engine* e)
{
    if (!e) return;
    for (nemgpu_engine* c : e->clones) nemgpu_destroy(c);
    e->clones.clear();
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](int j) { auto t1 = std::chrono::steady_clock::now(); g_destroy_ns[j] += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count(); t0 = t1; };
    (void)hipSetDevice(e->device);
    // (nemgpu_solve_many: an engine whose group never ran -- a failed job -- may still have uploads queued on its
    //  builder's stream, out of pinned blocks that go back to the pool below: wait for them)
    if (e->ready_pending && e->ready_ev) { (void)hipEventSynchronize(e->ready_ev); e->ready_pending = false; }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    lap(0);
    std::vector<PoolBlock> blocks;
    blocks.push_back({false, e->clone_slab, e->clone_slab_size});
    blocks.push_back({true, (char*)e->clone_flags_host, e->clone_flags_size});
    blocks.push_back({true, e->rs_par_host, e->rs_par_host_size});
    e->clone_slab = nullptr; e->clone_flags_host = nullptr; e->rs_par_host = nullptr; e->rs_par_host_size = 0;
    rccl_release(e);
    drop_graphs(e);
    if (g_alloc_engine == e) g_alloc_engine = nullptr;
    lap(1);
    // (the stream is idle: everything the engine held goes back to the device's pool for the next engines)
    for (const nemgpu_engine::Staged& st : e->staging) blocks.push_back({true, st.p, st.size});
    e->staging.clear();
    if (e->host_bits_pin) blocks.push_back({true, (char*)e->host_bits, e->host_bits_pin});
    for (const nemgpu_engine::Chunk& c : e->chunks) if (c.owned) blocks.push_back({false, c.base, c.size});
    if (e->flags_host && !e->flags_host_borrowed) blocks.push_back({true, (char*)e->flags_host, e->flags_host_size});
    pool_put_many(e->device, blocks);
    zip_context_release(e);
    if (e->own_stream && e->stream) pool_stream_put(e->device, e->stream);
    lap(2);
    if (e->ev_flags) (void)hipEventDestroy(e->ev_flags);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ready_ev) (void)hipEventDestroy(e->ready_ev);
    lap(3);
    delete e;
    lap(4);
}

void nemgpu_release_cached(void)
{
    for (int dev = 0; dev < kPoolDevices; dev++) {
        ResourcePool& P = g_pools[dev];
        std::vector<hipStream_t> streams;
        std::multimap<size_t, char*> devm, pin;
        std::vector<nemgpu_engine::ZipContext*> zips;
        { std::lock_guard<std::mutex> lock(P.m); zips.swap(P.zips); }
        if (!zips.empty()) (void)hipSetDevice(dev);
        for (nemgpu_engine::ZipContext* z : zips) zip_context_free(dev, z);      // (its blocks go through the pool ...)
        {
            std::lock_guard<std::mutex> lock(P.m);                                // (... which is emptied here)
            streams.swap(P.streams); devm.swap(P.dev); pin.swap(P.pinned);
            streams.insert(streams.end(), P.run_streams.begin(), P.run_streams.end()); P.run_streams.clear();
            P.dev_bytes = P.pinned_bytes = 0;
        }
        if (streams.empty() && devm.empty() && pin.empty()) continue;
        (void)hipSetDevice(dev);
        for (auto& kv : devm) (void)hipFree(kv.second);
        for (auto& kv : pin) (void)hipHostFree(kv.second);
        for (hipStream_t st : streams) (void)hipStreamDestroy(st);
    }
}

// room for the bit rows on the host: pinned (pooled) when they fit, else the engine's own vector
static uint32_t* host_bits_reserve(nemgpu_engine* e, size_t words)
{
    if (e->host_bits_pin) {
        (void)hipStreamSynchronize(e->stream);             // (a replaced matrix: its upload may still be reading them)
        pool_put(e->device, true, (char*)e->host_bits, e->host_bits_pin);
    }
    e->host_bits = nullptr; e->host_bits_pin = 0; e->host_bits_words = 0;
    // (behind the rows: room for the lanes' family order, npad ints -- upload_bits sends both in one copy)
    const size_t bytes = (std::max<size_t>(words, 1) + (size_t)e->npad) * sizeof(uint32_t);
    if (bytes <= kStageMax) {
        char* p = nullptr; size_t got = 0;
        if (pool_get(e->device, true, bytes, &p, &got) == hipSuccess) { e->host_bits = (uint32_t*)p; e->host_bits_pin = got; }
        else (void)hipGetLastError();
    }
    if (!e->host_bits) { e->host_bits_own.resize(words); e->host_bits = e->host_bits_own.data(); }
    else { std::vector<uint32_t>().swap(e->host_bits_own); }
    e->host_bits_words = words;
    return e->host_bits;
}

// bit rows (already in e->host_bits) -> device layouts.  pc: the rows' popcounts when the caller has them, else null.
// With pinned bit rows nothing here waits for the device: the copies and the layout kernels are ordered on the
// engine's stream ahead of everything that reads the layouts.
// Row popcounts of the family-major bit rows (the density kernels' lane order): with the CPU's popcnt instruction when
// it has one (20 000 x 500: 180 -> 45 us of a 0.36 ms engine build -- the builders are what bounds nemgpu_solve_many
// once the runs overlap them).  Host code only.
__attribute__((visibility("hidden"))) void nem_row_popcounts(const uint32_t* bits, int n, int wf, int* pc);
#if !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("popcnt"))) static void row_popcounts_hw(const uint32_t* bits, int n, int wf, int* pc)
{
    for (int i = 0; i < n; i++) {
        const uint32_t* row = bits + (size_t)i * wf;
        int c = 0, w = 0;
        for (; w + 2 <= wf; w += 2) { uint64_t v; memcpy(&v, row + w, 8); c += (int)__builtin_popcountll(v); }
        if (w < wf) c += __builtin_popcount(row[w]);
        pc[i] = c;
    }
}
static void row_popcounts_sw(const uint32_t* bits, int n, int wf, int* pc)
{
    for (int i = 0; i < n; i++) {
        const uint32_t* row = bits + (size_t)i * wf;
        int c = 0;
        for (int w = 0; w < wf; w++) c += __builtin_popcount(row[w]);
        pc[i] = c;
    }
}
void nem_row_popcounts(const uint32_t* bits, int n, int wf, int* pc)
{
    static const bool hw = __builtin_cpu_supports("popcnt") != 0;
    if (hw) row_popcounts_hw(bits, n, wf, pc); else row_popcounts_sw(bits, n, wf, pc);
}
#endif

static int upload_bits(nemgpu_engine* e, const int* pc_in)
{
    HIPCHK(hipSetDevice(e->device));
    const uint32_t* xbits_host = e->host_bits;
    uint32_t* xf = nullptr;
    size_t xf_size = 0;
    const size_t words = (size_t)e->n * e->wf;
    // lane order of the density kernels: inside each 256-family tile, families by popcount (stable)
    std::vector<int> perm_own;
    int* perm = e->host_bits_pin ? reinterpret_cast<int*>(e->host_bits + words) : nullptr;   // (the tail of the pinned block)
    const bool async = perm != nullptr;
    if (!perm) { perm_own.resize((size_t)e->npad); perm = perm_own.data(); }
    for (int i = 0; i < e->npad; i++) perm[i] = i;
    if (e->use_sort) {
        std::vector<int> pc_own;
        if (pc_in == nullptr) {
            pc_own.resize((size_t)e->n);
            nem_row_popcounts(xbits_host, e->n, e->wf, pc_own.data());
            pc_in = pc_own.data();
        }
        const int* pc = pc_in;
        // stable counting sort of every 256-family tile by popcount (0 .. d)
        std::vector<int> slot((size_t)e->d + 2);
        for (int t0 = 0; t0 < e->n; t0 += 256) {
            const int t1 = std::min(t0 + 256, e->n);
            int lo = e->d, hi = 0;
            for (int i = t0; i < t1; i++) { lo = std::min(lo, pc[i]); hi = std::max(hi, pc[i]); }
            std::fill(slot.begin() + lo, slot.begin() + hi + 2, 0);
            for (int i = t0; i < t1; i++) slot[pc[i] + 1]++;
            for (int c = lo + 1; c <= hi; c++) slot[c + 1] += slot[c];       // slot[c] = first position of popcount c
            for (int i = t0; i < t1; i++) perm[(size_t)t0 + slot[pc[i]]++] = i;
        }
    }
    // staging copy of the family-major bit rows: small ones live in the engine's chunk, large ones come and go
    const bool staged_in_chunk = words * sizeof(uint32_t) < kChunkOwn;
    if (staged_in_chunk) {
        if (!e->xf_stage) { alloc_for(e); int r = dev_alloc(&e->xf_stage, words + (size_t)e->npad); if (r) return r; }
        xf = e->xf_stage;
    } else {
        HIPCHK(pool_get(e->device, false, words * sizeof(uint32_t), (char**)&xf, &xf_size));
    }
    hipError_t err;
    if (async && staged_in_chunk) {
        // rows and lane order in ONE copy (host: the pinned block and its tail; device: the staging rows and theirs): a
        // copy's fixed cost on the copy engine -- 16 us median for the four copies of an engine in nemgpu_solve_many's
        // trace -- is what bounds that job
        int* dperm = reinterpret_cast<int*>(e->xf_stage + words);
        if (e->perm != dperm) { e->perm = dperm; drop_graphs(e); }      // (captured batches hold the old address)
        err = hipMemcpyAsync(xf, xbits_host, (words + (size_t)e->npad) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
    } else {
        err = hipMemcpyAsync(xf, xbits_host, words * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess)
            err = hipMemcpyAsync(e->perm, perm, (size_t)e->npad * sizeof(int), hipMemcpyHostToDevice, e->stream);
    }
    e->layout_pending = false;
    if (err == hipSuccess && e->defer_layout && async && staged_in_chunk) e->layout_pending = true;   // (run_many: pending_layout)
    else if (err == hipSuccess) {
        launch_layout(layout_args(e, xf), e->stream);
        err = hipGetLastError();
    }
    if (err == hipSuccess && !(async && staged_in_chunk)) err = hipStreamSynchronize(e->stream);
    if (!staged_in_chunk) pool_put(e->device, false, (char*)xf, xf_size);
    if (err != hipSuccess) { set_error(std::string("matrix upload failed: ") + hipGetErrorString(err)); return NEMGPU_E_DEVICE; }
    e->have_matrix = true;
    return NEMGPU_OK;
}

int nemgpu_set_matrix_bits(nemgpu_engine* e, const uint32_t* xbits_host)
{
    if (!e || !xbits_host) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    const size_t words = (size_t)e->n * e->wf;
    uint32_t* bits = host_bits_reserve(e, words);
    memcpy(bits, xbits_host, words * sizeof(uint32_t));
    // bits above organism d-1 in a row's last word are not data: cleared here, so that a caller's dirty padding can
    // neither count as organisms in the popcount M-step nor push a row's popcount past d in the lane ordering
    if (e->d & 31) {
        const uint32_t keep = (1u << (e->d & 31)) - 1u;
        for (size_t i = 0; i < (size_t)e->n; i++) bits[i * e->wf + (e->wf - 1)] &= keep;
    }
    return upload_bits(e, nullptr);
}

int nemgpu_set_observed_bits(nemgpu_engine* e, const uint32_t* obits_host)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    if (e->parent != nullptr || !(e->lo == 0 && e->hi == e->n_total)) {
        set_error("nemgpu_set_observed_bits: a whole single-GPU engine only (no shard, no lock-step twin)");
        return NEMGPU_E_ARG;
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    // the freshness flags are the unmasked kernels' or the masked ones': either way what they left is void now
    e->density_fresh = false; e->tables_fresh = false;
    if (obits_host == nullptr) { e->has_obs = false; return NEMGPU_OK; }
    const size_t words = (size_t)e->n * e->wf;
    if (!e->ow) {
        alloc_for(e);
        int r = NEMGPU_OK;
        auto A = [&](int rr) { if (r == NEMGPU_OK) r = rr; };
        A(dev_alloc(&e->obs_stage, words));
        A(dev_alloc(&e->ow, (size_t)e->W * e->npad));
        A(dev_alloc(&e->ows, (size_t)((e->W + 3) / 4) * 4 * e->npad));
        A(dev_alloc(&e->ot, (size_t)e->d * e->nw64));
        A(dev_alloc(&e->obs_stats, (size_t)e->k * e->d));
        A(dev_alloc(&e->nbobs_kd, (size_t)e->k * e->d));
        if (r) { e->obs_stage = e->ow = e->ows = nullptr; e->ot = nullptr; e->obs_stats = nullptr; e->nbobs_kd = nullptr; return r; }
    }
    // bits above organism d-1 are not cells: cleared in the library's copy, as the matrix's padding bits are
    std::vector<uint32_t> bits(obits_host, obits_host + words);
    if (e->d & 31) {
        const uint32_t keep = (1u << (e->d & 31)) - 1u;
        for (size_t i = 0; i < (size_t)e->n; i++) bits[i * e->wf + (e->wf - 1)] &= keep;
    }
    HIPCHK(copy_sync(e, e->obs_stage, bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
    // the matrix's layout kernels on the mask (the copy in E1's lane order, ows, is made with it and not read)
    LayoutArgs la = layout_args(e, e->obs_stage);
    la.xw = e->ow; la.xws = e->ows; la.xt = e->ot;
    launch_layout(la, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->has_obs = true;
    return NEMGPU_OK;
}

// engines packing a byte matrix right now, in all threads of the process: a lone caller takes helper threads, callers
// that already run side by side (pangenomenem_amd.batch) pack their own rows
static std::atomic<int> g_packers{0};

int nemgpu_set_matrix_bytes(nemgpu_engine* e, const uint8_t* x_host)
{
    if (!e || !x_host) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    const int d = e->d, wf = e->wf;
    uint32_t* bits = host_bits_reserve(e, (size_t)e->n * wf);
    std::vector<int> pc((size_t)e->n);
    // 8 values per load (bit 0 of each byte -> one byte), a whole 32-organism word at a time; then the rows' popcounts
    // (the density kernels' lane order)
    auto pack_rows = [&](int r0, int r1, uint64_t* bad_out) {
        uint64_t bad = 0;
        for (int i = r0; i < r1; i++) {
            const uint8_t* row = x_host + (size_t)i * d;
            uint32_t* out = bits + (size_t)i * wf;
            int j = 0;
            for (; j + 32 <= d; j += 32) {
                uint64_t w[4];
                memcpy(w, row + j, 32);
                bad |= (w[0] | w[1]) | (w[2] | w[3]);
                uint32_t v = 0;
                for (int q = 0; q < 4; q++)
                    v |= (uint32_t)(((w[q] & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << (8 * q);
                out[j >> 5] = v;
            }
            if (j < d) {
                uint32_t v = 0;
                int b = 0;
                for (; j + 8 <= d; j += 8, b += 8) {
                    uint64_t w8;
                    memcpy(&w8, row + j, 8);
                    bad |= w8;
                    v |= (uint32_t)(((w8 & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << b;
                }
                for (; j < d; j++, b++) { bad |= row[j]; v |= (uint32_t)(row[j] & 1u) << b; }
                out[wf - 1] = v;
            }
        }
        nem_row_popcounts(bits + (size_t)r0 * wf, r1 - r0, wf, pc.data() + r0);
        *bad_out = bad;
    };
    // rows are independent: matrices of 4 MB and more are packed by up to 4 threads
    const size_t bytes = (size_t)e->n * d;
    const unsigned hw = std::thread::hardware_concurrency();
    const int others = g_packers.fetch_add(1);
    int nt = (int)std::max(1u, std::min({4u, hw ? hw : 1u, (unsigned)(bytes >> 21)}));
    if (others > 0) nt = 1;
    uint64_t badv[4] = {0, 0, 0, 0};
    {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; t++)
            th.emplace_back(pack_rows, (int)((long long)e->n * t / nt), (int)((long long)e->n * (t + 1) / nt), &badv[t]);
        pack_rows(0, (int)((long long)e->n / nt), &badv[0]);
        for (std::thread& x : th) x.join();
    }
    g_packers.fetch_sub(1);
    const uint64_t bad = badv[0] | badv[1] | badv[2] | badv[3];
    if (bad & 0xFEFEFEFEFEFEFEFEull) { e->host_bits_words = 0; set_error("presence/absence matrix must hold 0/1 only"); return NEMGPU_E_ARG; }
    return upload_bits(e, pc.data());
}

int nemgpu_set_graph(nemgpu_engine* e, const int32_t* ptr, const int32_t* idx, const float* w)
{
    if (!e || !ptr) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    const int nnz = ptr[e->n] - ptr[0];
    if (ptr[0] != 0 || nnz < 0) { set_error("graph: ptr[0] must be 0 and ptr non-decreasing"); return NEMGPU_E_ARG; }
    for (int i = 0; i < e->n; i++) if (ptr[i + 1] < ptr[i]) { set_error("graph: ptr not monotone"); return NEMGPU_E_ARG; }
    for (int t = 0; t < nnz; t++)
        if (idx[t] < 0 || idx[t] >= e->n_total) { set_error("graph: neighbour index out of range"); return NEMGPU_E_ARG; }
    e->nei_ptr = nullptr; e->nei_idx = nullptr; e->nei_w = nullptr;   // (a replaced graph's arrays stay in their chunk)
    int r;
    alloc_for(e);
    // ptr | idx | w in one device block and one pinned block of the engine's: one copy, nothing waits (sources too
    // large for a pinned block: three copies from the caller's memory and one wait)
    const size_t b_ptr = sizeof(int) * ((size_t)e->n + 1), b_nz = sizeof(int) * (size_t)nnz;
    const size_t o_idx = (b_ptr + 255) & ~(size_t)255, o_w = (o_idx + b_nz + 255) & ~(size_t)255, total = o_w + b_nz;
    char* dev = nullptr;
    if ((r = dev_alloc(&dev, total))) return r;
    e->nei_ptr = (int*)dev; e->nei_idx = (int*)(dev + o_idx); e->nei_w = (float*)(dev + o_w);
    char* st = stage(e, total);
    if (st) {
        memcpy(st, ptr, b_ptr);
        if (nnz > 0) { memcpy(st + o_idx, idx, b_nz); memcpy(st + o_w, w, b_nz); }
        HIPCHK(hipMemcpyAsync(dev, st, total, hipMemcpyHostToDevice, e->stream));
    } else {
        HIPCHK(hipMemcpyAsync(e->nei_ptr, ptr, b_ptr, hipMemcpyHostToDevice, e->stream));
        if (nnz > 0) {
            HIPCHK(hipMemcpyAsync(e->nei_idx, idx, b_nz, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(e->nei_w, w, b_nz, hipMemcpyHostToDevice, e->stream));
        }
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    e->nnz = nnz;
    e->has_graph = nnz > 0;
    drop_graphs(e);
    return NEMGPU_OK;
}

int nemgpu_set_params(nemgpu_engine* e, const float* prop, const float* center, const float* disp)
{
    if (!e || !prop || !center || !disp) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    const size_t kd = (size_t)e->k * e->d;
    float* st = e->parent == nullptr ? (float*)stage(e, sizeof(float) * e->par_words) : nullptr;
    if (st) {
        // one copy of the whole block of initial values (its gaps and its tail are zeros)
        memset(st, 0, sizeof(float) * e->par_words);
        memcpy(st, prop, sizeof(float) * e->k); memcpy(st + e->par_o_center, center, sizeof(float) * kd);
        memcpy(st + e->par_o_disp, disp, sizeof(float) * kd);
        HIPCHK(hipMemcpyAsync(e->prop0, st, sizeof(float) * e->par_words, hipMemcpyHostToDevice, e->stream));
    } else {
        HIPCHK(copy_sync(e, e->prop0, prop, sizeof(float) * e->k, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(e, e->center0, center, sizeof(float) * kd, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(e, e->disp0, disp, sizeof(float) * kd, hipMemcpyHostToDevice));
    }
    e->have_params = true;
    return reset_state(e, true);
}

int nemgpu_configure(nemgpu_engine* e, const nemgpu_config* cfg)
{
    if (!e || !cfg) return NEMGPU_E_FUNCARG;
    if (cfg->algo != NEMGPU_ALGO_NEM && cfg->algo != NEMGPU_ALGO_NCEM) { set_error("algo must be nem or ncem"); return NEMGPU_E_ARG; }
    if (cfg->disper < 0 || cfg->disper > 3 || cfg->propor < 0 || cfg->propor > 1) { set_error("bad dispersion/proportion model"); return NEMGPU_E_ARG; }
    if (cfg->cvtest < NEMGPU_CV_NONE || cfg->cvtest > NEMGPU_CV_CRIT_LOGGED) { set_error("convergence must be none, clas or crit"); return NEMGPU_E_ARG; }
    if (cfg->cvtest != NEMGPU_CV_NONE && !(cfg->cvthres > 0)) { set_error("convergence threshold must be > 0"); return NEMGPU_E_ARG; }
    if (cfg->it_max < 0) { set_error("it_max must be >= 0"); return NEMGPU_E_ARG; }
    if (cfg->tie_rule != NEMGPU_TIE_FIRST && cfg->tie_rule != NEMGPU_TIE_HASH && cfg->tie_rule != NEMGPU_TIE_LIBC) { set_error("bad tie rule"); return NEMGPU_E_ARG; }
    if (cfg->tie_seed != e->cfg.tie_seed || cfg->tie_rule != e->cfg.tie_rule) e->draw_valid = false;
    e->cfg = *cfg;
    HIPCHK(hipSetDevice(e->device));
    drop_graphs(e);                                                // kernel arguments are baked into captured batches
    return reset_state(e, true);
}

int nemgpu_reset(nemgpu_engine* e)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    return reset_state(e);
}

int nemgpu_init_partition(nemgpu_engine* e)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    int r = init_partition(e);
    if (r) return r;
    e->crit_ref = 0.0f;
    if (e->cfg.cvtest == NEMGPU_CV_CRIT_LOGGED) {                  // (what the first iteration's criterion is compared with)
        float c6[6];
        if ((r = criteria(e, c6))) return r;
        e->crit_ref = c6[3];
    }
    return NEMGPU_OK;
}

int nemgpu_iterate(nemgpu_engine* e, int n_iters, nemgpu_result* res)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    auto t0 = std::chrono::steady_clock::now();
    int r = iterate(e, n_iters);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(e->stream));
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fill_result(e, res);
    if (res) res->loop_seconds = secs;
    return NEMGPU_OK;
}

// One EM iteration with everything a line of the reference's log needs -- the criteria of the partition the sweep
// started from and of the new one (WriteLogCrit, nem_alg.c:2361, 2398), the parameters (WriteLogClasses) -- in ONE
// stream submission and one wait: the two criteria passes and the copies are enqueued behind the iteration before
// anyone knows how it ended.  An iteration the host has to finish (more relaxation rounds) or a criterion-driven
// convergence test takes the plain sequence of calls instead.
// keep_draws: a start of RandNemAlgo -- the tie stream goes on where the start before left it (one srandom per nem() call)
static int iterate_logged_impl(nemgpu_engine* e, int with_init, bool keep_draws, nemgpu_result* res, float crit_before[6],
                               float crit_after[6], float* prop, float* center, float* disp, float* nbobs_k)
{
    if (!e || !crit_before || !crit_after) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const auto t0 = std::chrono::steady_clock::now();
    int r;
    bool speculated = false;
    LogSlot slot{e};                                               // (the pinned side alone: the line comes by copy commands)
    if (with_init && (crit_test(e) || e->libc() || e->has_obs || !(e->lo == 0 && e->hi == e->n_total))) {
        // (the start whose two sweeps the host completes one after the other: the plain sequence of calls)
        const int draws = e->draws;
        if ((r = reset_state(e))) return r;
        if (keep_draws) e->draws = draws;
        if ((r = init_partition(e))) return r;
        e->crit_ref = 0.0f;
        if (e->cfg.cvtest == NEMGPU_CV_CRIT_LOGGED) {              // (what the first iteration's criterion is compared with)
            float c6[6];
            if ((r = criteria(e, c6))) return r;
            e->crit_ref = c6[3];
        }
    } else if (!crit_test(e) && !e->has_obs && e->lo == 0 && e->hi == e->n_total) {
        LoopCursor lc;
        if (with_init && !keep_draws) e->draws = 0;
        if ((r = loop_begin(e, lc, with_init ? 0 : 1, with_init != 0))) return r;
        if (loop_wants_batch(e, lc)) {
            if ((r = batch_plan(e, lc))) return r;
            // (a start: the blind sweep's partition is in buffer 1, the beta sweep's in 2)
            const int oldbuf = with_init ? 1 : lc.base, newbuf = with_init ? 2 : (lc.base + 1) % 3;
            if (slot.st.get(true, slot.bytes(1)) != hipSuccess) (void)hipGetLastError();   // (without it: the plain sequence below)
            e->n_plain++;
            if ((r = batch_enqueue(e, lc, true))) return r;
            if (slot.st.host) {
                if ((r = criteria_pair_enqueue(e, newbuf, oldbuf))) return r;   // both partitions in the same launches
                HIPCHK(slot.put(0, LogSlot::kBefore, e->crit2_6));
                HIPCHK(slot.put(0, LogSlot::kAfter, e->crit6_dev));
                HIPCHK(slot.put(0, LogSlot::kPar, e->prop));
            }
            HIPCHK(hipStreamSynchronize(e->stream));
            const bool clean = e->h_ctrl()[C_NEED_ROUNDS] == 0 && e->h_ctrl()[C_STATUS] != NEMGPU_W_EMPTYCLASS;
            if ((r = batch_finish(e, lc))) return r;
            speculated = slot.st.host != nullptr && clean;
        }
    } else {
        if ((r = iterate(e, 1))) return r;
    }
    if (speculated) {
        const LogLine ln = slot.line(0, 0);
        const size_t kd = (size_t)e->k * e->d;
        memcpy(crit_before, ln.cb, 6 * sizeof(float)); memcpy(crit_after, ln.ca, 6 * sizeof(float));
        if (prop) memcpy(prop, ln.prop, sizeof(float) * e->k);
        if (center) memcpy(center, ln.center, sizeof(float) * kd);
        if (disp) memcpy(disp, ln.disp, sizeof(float) * kd);
        if (nbobs_k) memcpy(nbobs_k, ln.nb, sizeof(float) * e->k);
    }
    slot.st.put();
    if (!speculated && e->status != NEMGPU_W_EMPTYCLASS &&           // (an emptied class: the E-step did not run, nothing to log)
        (r = plain_line(e, crit_before, crit_after, prop, center, disp, nbobs_k))) return r;
    HIPCHK(hipStreamSynchronize(e->stream));
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fill_result(e, res);
    if (res) res->loop_seconds = secs;
    return NEMGPU_OK;
}

int nemgpu_iterate_logged(nemgpu_engine* e, int with_init, nemgpu_result* res, float crit_before[6], float crit_after[6],
                          float* prop, float* center, float* disp, float* nbobs_k)
{
    return iterate_logged_impl(e, with_init, false, res, crit_before, crit_after, prop, center, disp, nbobs_k);
}

// ---- one run with the reference's per-iteration log, the iterations pipelined ------------------------------------------
// nemgpu_iterate_logged is one EM iteration, two criteria evaluations and a wait per call: 0.3 ms per logged iteration at
// configs[1] size, of which the criteria's i-ordered sums (four lone blocks per partition) are 0.1-0.2 and the iteration
// itself 0.04.  Here a batch of up to seven iterations runs as the unlogged loop runs it (device-side loop control, one
// wait), and behind every iteration what its log line needs is set aside in a twin of the engine -- the partition the
// E-step started from, the one it left, the densities, the parameters (0.75 MB of device copies) -- so that the criteria
// of ALL the batch's iterations are one lock-step pass over the twins afterwards: their lone blocks side by side.
static int ensure_clones(nemgpu_engine* e, int count);

int nemgpu_run_logged(nemgpu_engine* e, nemgpu_result* res, nemgpu_log_fn fn, void* user)
{
    if (!e || !fn) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    int r;
    const int k = e->k, d = e->d;
    const size_t kd = (size_t)k * d;
    std::vector<float> prop((size_t)k), center(kd), disp(kd), nb((size_t)k);
    float cb[6], ca[6];
    nemgpu_result r1{};
    auto emit_own = [&](int iter, const float* sizes) { emit(fn, user, 0, LogLine{NEMGPU_LOG_LINE, iter, 0, cb, ca, prop.data(), center.data(), disp.data(), sizes}); };
    const auto t0 = std::chrono::steady_clock::now();
    static const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    auto lapt = t0;
    auto lap = [&](const char* what) { if (prof) { const auto now = std::chrono::steady_clock::now(); fprintf(stderr, "[logged run] %s: %.0f us\n", what, std::chrono::duration<double, std::micro>(now - lapt).count()); lapt = now; } };
    // ---- line 0: the start (reset, the two initial sweeps), both criteria, the parameters
    if ((r = iterate_logged_impl(e, 1, false, &r1, cb, ca, prop.data(), center.data(), disp.data(), nb.data()))) return r;
    emit_own(0, nullptr);                                          // (no EstimPara yet: no sizes, as the header says)
    lap("line 0 (start, two criteria)");
    static const bool batched_on = !(getenv("NEM_MI355X_LOG_BATCHED") && getenv("NEM_MI355X_LOG_BATCHED")[0] == '0');
    // (a masked engine: one logged iteration per call, each line emitted behind its iteration -- the drop-in's log callback
    //  reads that iteration's observed counts from the engine, nemgpu_get_observed_counts)
    const bool batched = batched_on && e->ncem() && !crit_test(e) && !e->has_obs && e->lo == 0 && e->hi == e->n_total && e->parent == nullptr;
    bool last_logged = false;
    if (!batched) {
        // (the fuzzy algorithm, the `crit` test, a sharded engine: one logged iteration per call, as nemgpu_iterate_logged)
        for (int iter = 1; iter <= e->cfg.it_max && !e->converged && e->status == NEMGPU_OK; iter++) {
            if ((r = iterate_logged_impl(e, 0, false, &r1, cb, ca, prop.data(), center.data(), disp.data(), nb.data()))) return r;
            if (e->status == NEMGPU_W_EMPTYCLASS) {
                emit(fn, user, 0, LogLine::empty(iter, e->emptyk, nullptr));   // (no sizes: only a random start hands them on)
                last_logged = false;
                break;
            }
            emit_own(iter, nb.data());
            last_logged = true;
        }
    } else {
        // two twins per iteration of a batch: the partition the E-step started from and the one it left, each with the
        // iteration's densities -- 14 criteria evaluations in one pass
        if ((r = ensure_clones(e, 2 * kPipeDepth))) return r;
        for (nemgpu_engine* c : e->clones) { c->cfg = e->cfg; c->stream = e->stream; }
        std::vector<nemgpu_engine*> T(e->clones.begin(), e->clones.begin() + 2 * kPipeDepth);
        LogSlot slot{e};
        if ((r = slot.st.get_both(slot.bytes(kPipeDepth), "no pinned memory for the log lines"))) return r;
        std::vector<Recorder> recs((size_t)2 * kPipeDepth);
        lap("twins and staging");
        int iter = 0;
        while (iter < e->cfg.it_max && !e->converged && e->status == NEMGPU_OK) {
            LoopCursor lc;
            // (a run that is through in one or two iterations -- chunks near their fixed point -- should not pay for seven
            //  enqueued ones: three first, then seven at a time)
            const int g = std::min(e->cfg.it_max - iter, iter == 0 ? 3 : kPipeDepth);
            if ((r = loop_begin(e, lc, g, false))) return r;
            if ((r = batch_plan(e, lc))) return r;
            const int base = lc.base;
            // behind iteration j: the partition it started from and the one it left, the densities, the parameters
            const std::function<int(int)> set_aside = [&](int j) -> int {
                const int P = (base + j) % 3, Q = (base + j + 1) % 3;
                CopySegsArgs cs{};
                int q = 0;
                auto seg = [&](const void* src, void* dst, size_t bytes) {
                    cs.src[q] = static_cast<const int*>(src); cs.dst[q] = static_cast<int*>(dst); cs.words[q] = (int)((bytes + 3) / 4); q++;
                };
                for (int side = 0; side < 2; side++) {
                    nemgpu_engine* c = T[(size_t)(2 * j + side)];
                    seg(e->lab[side ? Q : P], c->lab[0], (size_t)e->n_total);
                    seg(e->pkfki, c->pkfki, sizeof(double) * (size_t)k * e->npad);
                    seg(e->logpkfki, c->logpkfki, sizeof(float) * (size_t)k * e->npad);
                }
                seg(e->prop, slot.par_dev(j), sizeof(float) * e->par_words);
                cs.n = q;
                launch_copy_segments(cs, e->stream);                // (one launch: seven copy commands were 28 us of issue time per iteration)
                HIPCHK(hipGetLastError());
                return NEMGPU_OK;
            };
            e->n_plain++;
            if ((r = batch_enqueue(e, lc, true, &set_aside))) return r;
            HIPCHK(hipStreamSynchronize(e->stream));
            const int* hc = e->h_ctrl();
            const int done = hc[C_ITERS];
            const bool tail_open = hc[C_NEED_ROUNDS] != 0 || hc[C_STATUS] == NEMGPU_W_EMPTYCLASS;   // the last counted iteration did not end in the pipeline
            if ((r = batch_finish(e, lc))) return r;
            if (prof) fprintf(stderr, "[logged run]   g %d done %d need_rounds %d status %d converged %d deep %d\n", g, done, hc[C_NEED_ROUNDS], hc[C_STATUS], hc[C_CONVERGED], lc.deep);
            lap("a batch of iterations");
            const int whole = tail_open ? std::max(0, done - 1) : done;
            if (whole > 0) {
                // the criteria of the `whole` iterations in one lock-step pass over the twins
                std::vector<nemgpu_engine*> TT(T.begin(), T.begin() + 2 * whole);
                std::vector<int> all((size_t)2 * whole);
                for (int m = 0; m < 2 * whole; m++) all[(size_t)m] = m;
                if ((r = lockstep(TT, all, recs, [&](int m) -> int {   // (twin m: iteration m / 2, before or after)
                        nemgpu_engine* c = TT[(size_t)m];
                        const int rr = criteria_enqueue(c, 0);
                        if (rr == NEMGPU_OK) HIPCHK(slot.put(m / 2, m % 2 ? LogSlot::kAfter : LogSlot::kBefore, c->crit6_dev));
                        return rr;
                    }, false))) return r;
                HIPCHK(slot.fetch(whole));
                for (int m = 0; m < whole; m++) emit(fn, user, 0, slot.line(m, iter + m + 1));
                memcpy(ca, slot.line(whole - 1, 0).ca, sizeof ca);
                last_logged = true;
                lap("its criteria and lines");
            }
            iter += whole;
            if (tail_open && done > 0) {
                iter += 1;
                if (e->status == NEMGPU_W_EMPTYCLASS) {
                    emit(fn, user, 0, LogLine::empty(iter, e->emptyk, nullptr));
                    last_logged = false;
                    break;
                }
                if ((r = plain_line(e, cb, ca, prop.data(), center.data(), disp.data(), nb.data()))) return r;   // (its sweep was finished from the host)
                emit_own(iter, nb.data());
                last_logged = true;
            }
            if (done == 0) break;                                  // (nothing ran: the loop tests above end it)
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    fill_result(e, res);
    if (res) {
        res->loop_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        // (the last logged iteration's second criteria evaluation was of the final partition, on the final densities)
        if (last_logged && e->iters > 0) memcpy(res->crit, ca, sizeof ca);
        else res->crit[0] = NAN;                                   // the caller asks nemgpu_criteria (after its own iters == 0 steps)
    }
    return NEMGPU_OK;
}


int nemgpu_restart_iterate(nemgpu_engine* e, int n_iters, nemgpu_result* res)
{
    // reset + ComputePartitionFromPara(Needinit=1) + up to n_iters EM iterations as ONE pipelined batch sequence
    if (!e) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_restart_iterate"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    e->draws = 0;
    int r = iterate(e, n_iters, true);
    if (r) return r;
    fill_result(e, res);
    return NEMGPU_OK;
}

int nemgpu_run(nemgpu_engine* e, nemgpu_result* res)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    int r;
    HIPCHK(hipStreamSynchronize(e->stream));
    auto t0 = std::chrono::steady_clock::now();
    e->draws = 0;                                                  // one nem() call = one srandom(seed), nem_exe.c:621
    if ((r = iterate(e, e->cfg.it_max, true))) return r;           // restart + initial sweeps + EM loop, pipelined
    HIPCHK(hipStreamSynchronize(e->stream));
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (e->iters == 0) {                                           // nem_alg.c:1845-1851
        if ((r = do_mstep(e))) return r;
        if (!e->ncem() && (r = read_iter_flags(e))) return r;      // (a fuzzy M-step can report a fault)
        if ((r = do_tables(e))) return r;
        if ((r = do_density(e))) return r;
    }
    fill_result(e, res);
    if (res) {
        res->loop_seconds = secs;
        if ((r = criteria(e, res->crit))) return r;                // nem_alg.c:1852
    }
    return NEMGPU_OK;
}

// Several whole runs in lock step: one launch per step of the EM for ALL of them (see "Lock-step batches" above).
int nemgpu_run_many(nemgpu_engine** engines, int count, nemgpu_result* results)
{
    if (!engines || count <= 0) return NEMGPU_E_FUNCARG;
    std::vector<nemgpu_engine*> E((size_t)count);
    for (int i = 0; i < count; i++) {
        if (!engines[i]) return NEMGPU_E_FUNCARG;
        for (int j = 0; j < i; j++) if (engines[j] == engines[i]) { set_error("nemgpu_run_many: the same engine twice"); return NEMGPU_E_ARG; }
        E[i] = engines[i];
    }
    for (int i = 0; i < count; i++) { const int mr = masked_refuse(E[i], "nemgpu_run_many"); if (mr) return mr; }
    HIPCHK(hipSetDevice(E[0]->device));
    return run_many(E, results);
}

// Many whole problems, from host arrays to host arrays, in one call: `workers` threads of the library build the
// engines (bit packing, uploads out of pinned blocks -- nothing waits for the device), the calling thread runs every
// `group` of them in lock step as soon as it is complete (nemgpu_run_many), the workers fetch the results and recycle
// the engines while later groups are being built.  What PPanGGOLiN's chunk loop is when its chunks are arrays.
static int solve_many_one(nemgpu_problem* P, int count, const nemgpu_config* cfg, int device, int workers, int group, const ChunkSource* src = nullptr);
static int adopt_chunk(nemgpu_engine* e, const nemgpu_master* M, const nemk::ChunkPlan& plan, int nnz_c);
static int vote_group(nemgpu_votes* v, const std::vector<nemgpu_engine*>& E, const std::vector<int>& who,
                      const std::vector<nemgpu_result>& R, const ChunkSource* src);
static int tally_group(ResampleTally* t, const std::vector<nemgpu_engine*>& E, const std::vector<int>& who,
                       const std::vector<nemgpu_result>& R, const ChunkSource* src);
static thread_local bool tl_runner = false;                  // this thread is one of nemgpu_solve_many_devices' runners

// Four groups and more, six workers and more: two runners on the device (nemgpu_solve_many_devices with the device named
// twice), each with half of the workers.  Between the steps of a group its runner reads flags and records the next step
// -- 0.1-0.3 ms in which its stream is empty; the other runner's group fills them (256 problems of 20 000 x 500,
// 12 workers: 8 400 -> 9 900 problems/s).  NEM_MI355X_RUNNERS=n fixes the number (1: never split).
int nemgpu_solve_many(nemgpu_problem* P, int count, const nemgpu_config* cfg, int device, int workers, int group)
{
    if (!P || count <= 0 || !cfg) return NEMGPU_E_FUNCARG;
    static const int fixed = [] { const char* g = getenv("NEM_MI355X_RUNNERS"); return g ? std::max(0, std::min(atoi(g), 4)) : 0; }();
    const int g = std::max(1, std::min(group, 256));
    const int runners = tl_runner ? 1 : fixed > 0 ? fixed : (count >= 4 * g && workers >= 6 ? 2 : 1);
    if (runners <= 1 || count <= g) return solve_many_one(P, count, cfg, device, workers, group);
    const int devs[4] = {device, device, device, device};
    return nemgpu_solve_many_devices(P, count, cfg, devs, runners, workers, group);
}

static int solve_many_one(nemgpu_problem* P, int count, const nemgpu_config* cfg, int device, int workers, int group, const ChunkSource* src)
{
    if (!P || count <= 0 || !cfg) return NEMGPU_E_FUNCARG;
    workers = std::max(1, std::min(workers, 64));
    group = std::max(1, std::min(group, 256));
    for (int i = 0; i < count; i++) {
        nemgpu_problem& q = P[i];
        q.rc = NEMGPU_OK; q.result = nemgpu_result{};
        if (q.n <= 0 || q.d <= 0 || q.k <= 0 || (src == nullptr && (!q.x_bytes == !q.x_bits)) || !q.prop || !q.center || !q.disp ||
            (q.nei_ptr && q.nei_ptr[q.n] > 0 && (!q.nei_idx || !q.nei_w))) {
            set_error("nemgpu_solve_many: problem " + std::to_string(i) + " is incomplete (sizes, exactly one of x_bytes / x_bits, parameters)");
            return NEMGPU_E_FUNCARG;
        }
    }
    const int G = (count + group - 1) / group;
    std::vector<nemgpu_engine*> eng((size_t)count, nullptr);
    std::vector<std::string> errs((size_t)count);
    std::vector<int> built((size_t)G, 0);
    std::mutex m;
    std::condition_variable cv;
    std::deque<int> fetchq;
    struct GroupSlab { char* host = nullptr; size_t size = 0, stride = 0; int left = 0; };
    std::vector<GroupSlab> gslab((size_t)G);                     // a group's results on the host (GroupFetch), until its last fetch
    std::vector<int> gslot((size_t)count, -1);
    int build_next = 0, build_limit = std::min(count, 2 * group), fetched = 0;
    bool quit = false;

    // Streams are the expensive resource of this stack (6 ms to create one): the engines a worker builds share that
    // worker's stream, the lock-step runs have one of their own, so that a group's run and the next groups' uploads
    // are not ordered behind each other.
    std::vector<hipStream_t> wstream((size_t)workers, nullptr);
    hipStream_t rstream = nullptr, fstream = nullptr;
    (void)hipSetDevice(device);
    if (pool_run_stream_get(device, &rstream) != hipSuccess) { set_error("hipStreamCreate failed"); return NEMGPU_E_DEVICE; }
    if (pool_stream_get(device, &fstream) != hipSuccess) { (void)hipGetLastError(); fstream = nullptr; }
    const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); };
    double slow_build[6] = {0, 0, 0, 0, 0, 0}, slow_fetch[3] = {0, 0, 0};      // (profile: the slowest build / fetch, by stage)
    std::mutex pm;
    auto build = [&](int i, hipStream_t st) {
        nemgpu_problem& q = P[i];
        nemgpu_engine* e = nullptr;
        double t[6] = {0, 0, 0, 0, 0, 0};
        auto t0 = now();
        int r = nemgpu_create(&e, q.n, q.d, q.k, 0, q.n, device, st);
        if (r == NEMGPU_OK && st != nullptr) e->defer_layout = true;
        t[1] = since(t0);
        if (src != nullptr) {
            // a chunk of a master that lives on the device: matrix rows, lane order and graph are made THERE, into this
            // engine's own buffers (nem_chunks.hip) -- nothing of them crosses PCIe
            if (r == NEMGPU_OK) r = adopt_chunk(e, src->master, src->plans[i], src->nnz[i]);
            t[2] = t[3] = since(t0);
        } else {
        if (r == NEMGPU_OK) r = q.x_bits ? nemgpu_set_matrix_bits(e, q.x_bits) : nemgpu_set_matrix_bytes(e, q.x_bytes);
        t[2] = since(t0);
        if (r == NEMGPU_OK) {
            if (q.nei_ptr) r = nemgpu_set_graph(e, q.nei_ptr, q.nei_idx, q.nei_w);
            else { std::vector<int32_t> z((size_t)q.n + 1, 0); r = nemgpu_set_graph(e, z.data(), nullptr, nullptr); }
        }
        t[3] = since(t0);
        }
        if (r == NEMGPU_OK) r = nemgpu_set_params(e, q.prop, q.center, q.disp);
        if (r == NEMGPU_OK) r = nemgpu_configure(e, cfg);
        t[4] = since(t0);
        if (r == NEMGPU_OK && st != nullptr) {
            // the builder's stream goes on to other engines' uploads: the run waits for THIS engine's, by event
            if (hipEventCreateWithFlags(&e->ready_ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(e->ready_ev, st) == hipSuccess)
                e->ready_pending = true;
            else (void)hipGetLastError();                          // (no event: the run waits for the stream, as before)
        }
        t[5] = since(t0);
        if (prof) { std::lock_guard<std::mutex> lock(pm); if (t[5] > slow_build[5]) for (int j = 1; j < 6; j++) slow_build[j] = t[j]; slow_build[0] += t[5]; }
        if (r != NEMGPU_OK) { errs[(size_t)i] = g_last_error; if (e) nemgpu_destroy(e); e = nullptr; }
        q.rc = r;
        eng[(size_t)i] = e;
    };
    auto fetch = [&](int i) {
        nemgpu_problem& q = P[i];
        nemgpu_engine* e = eng[(size_t)i];
        if (!e) return;
        auto t0 = now();
        // (its run is over and was waited for: whatever it still copies goes to the fetch stream, not behind the uploads
        // its builder's stream has taken in the meantime)
        if (!e->own_stream && fstream != nullptr) e->stream = fstream;
        GroupSlab& gs = gslab[(size_t)(i / group)];
        uint8_t* lab_out = (src != nullptr && src->labels != nullptr) ? src->labels[i] : nullptr;
        if (q.rc == NEMGPU_OK && lab_out != nullptr && e->ncem()) {        // (chunks: the class of every kept family)
            if (gs.host != nullptr && gslot[(size_t)i] >= 0) {
                const uint8_t* lab = (const uint8_t*)(gs.host + gs.stride * (size_t)gslot[(size_t)i]);
                for (int f = 0; f < e->n; f++) lab_out[f] = lab[f] & 0x7F;
            } else {
                q.rc = nemgpu_get_labels(e, lab_out);
                if (q.rc != NEMGPU_OK) errs[(size_t)i] = g_last_error;
            }
        }
        if (q.rc == NEMGPU_OK && (q.out_prop || q.out_center || q.out_disp || q.out_nbobs_k || q.out_c)) {
            if (gs.host != nullptr && gslot[(size_t)i] >= 0)
                result_unpack(e, gs.host + gs.stride * (size_t)gslot[(size_t)i], result_part_bytes(e), q.out_prop, q.out_center, q.out_disp, q.out_nbobs_k, q.out_c);
            else {
                q.rc = nemgpu_get_results(e, q.out_prop, q.out_center, q.out_disp, q.out_nbobs_k, q.out_c);
                if (q.rc != NEMGPU_OK) errs[(size_t)i] = g_last_error;
            }
        }
        const double t1 = since(t0);
        nemgpu_destroy(e);
        const double t2 = since(t0);
        if (prof) { std::lock_guard<std::mutex> lock(pm); if (t2 > slow_fetch[2]) { slow_fetch[1] = t1; slow_fetch[2] = t2; } slow_fetch[0] += t2; }
        eng[(size_t)i] = nullptr;
    };
    auto worker = [&](int w) {
        (void)hipSetDevice(device);
        (void)pool_stream_get(device, &wstream[(size_t)w]);        // (nullptr: the engines take streams of their own)
        std::unique_lock<std::mutex> lock(m);
        for (;;) {
            cv.wait(lock, [&] { return quit || !fetchq.empty() || build_next < build_limit; });
            if (!fetchq.empty()) {                                 // results first: they free engines for the builders
                const int i = fetchq.front(); fetchq.pop_front();
                lock.unlock(); fetch(i); lock.lock();
                GroupSlab& gs = gslab[(size_t)(i / group)];
                if (gs.host != nullptr && --gs.left == 0) { pool_put(device, true, gs.host, gs.size); gs.host = nullptr; }
                fetched++;
                cv.notify_all();
            } else if (build_next < build_limit) {
                const int i = build_next++;
                lock.unlock(); build(i, wstream[(size_t)w]); lock.lock();
                built[(size_t)(i / group)]++;
                cv.notify_all();
            } else if (quit) return;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < workers; t++) pool.emplace_back(worker, t);
    int rc = NEMGPU_OK;
    std::string first_err;
    double t_wait = 0, t_run = 0, t_tail = 0;
    for (int g = 0; g < G; g++) {
        const int i0 = g * group, i1 = std::min(count, i0 + group);
        {
            const auto t0 = now();
            std::unique_lock<std::mutex> lock(m);
            cv.wait(lock, [&] { return built[(size_t)g] == i1 - i0; });
            t_wait += since(t0);
        }
        std::vector<nemgpu_engine*> E;
        std::vector<int> who;
        for (int i = i0; i < i1; i++) if (eng[(size_t)i]) { E.push_back(eng[(size_t)i]); who.push_back(i); }
        if (!E.empty()) {
            std::vector<nemgpu_result> R(E.size());
            (void)hipSetDevice(device);
            const auto t0 = now();
            // (the lead's own stream is a worker's: what it still has to upload is waited for, then the run moves)
            hipStream_t lead_own = E[0]->stream;
            int r = E[0]->ready_pending || hipStreamSynchronize(lead_own) == hipSuccess ? NEMGPU_OK : NEMGPU_E_DEVICE;
            if (r == NEMGPU_OK) {
                if (!E[0]->own_stream) E[0]->stream = rstream;
                // the group's partitions and parameters come back with the run, in one block
                GroupFetch gf;
                size_t dev_size = 0, host_size = 0;
                for (nemgpu_engine* e : E) gf.stride = std::max(gf.stride, (result_block_bytes(e) + 63) & ~(size_t)63);
                const size_t total = gf.stride * E.size();
                bool want = false;
                for (int i : who) want = want || P[i].out_prop || P[i].out_center || P[i].out_disp || P[i].out_nbobs_k || P[i].out_c ||
                                         (src != nullptr && src->labels != nullptr && src->labels[i] != nullptr);
                if (want && total <= kStageMax) {
                    if (pool_get(device, false, total, &gf.dev, &dev_size) != hipSuccess) { (void)hipGetLastError(); gf.dev = nullptr; }
                    if (gf.dev && pool_get(device, true, total, &gf.host, &host_size) != hipSuccess) { (void)hipGetLastError(); gf.host = nullptr; }
                }
                const bool grouped = gf.dev != nullptr && gf.host != nullptr;
                r = run_many(E, R.data(), grouped ? &gf : nullptr);
                if (!E[0]->own_stream) { (void)hipStreamSynchronize(rstream); E[0]->stream = lead_own; }
                if (gf.dev) pool_put(device, false, gf.dev, dev_size);
                if (grouped && r == NEMGPU_OK && gf.filled) {
                    std::lock_guard<std::mutex> lock(m);
                    GroupSlab& gs = gslab[(size_t)g];
                    gs.host = gf.host; gs.size = host_size; gs.stride = gf.stride; gs.left = (int)E.size();
                    for (size_t j = 0; j < E.size(); j++) gslot[(size_t)who[j]] = (int)j;
                } else if (gf.host) pool_put(device, true, gf.host, host_size);
            }
            // the group's votes, read from the engines' own label and parameter buffers before the fetches recycle them
            if (r == NEMGPU_OK && src != nullptr && src->votes != nullptr) r = vote_group(src->votes, E, who, R, src);
            if (r == NEMGPU_OK && src != nullptr && src->tally != nullptr) r = tally_group(src->tally, E, who, R, src);
            t_run += since(t0);
            for (size_t j = 0; j < E.size(); j++) { P[who[j]].result = R[j]; if (r != NEMGPU_OK) P[who[j]].rc = r; }
            if (r != NEMGPU_OK && rc == NEMGPU_OK) { rc = r; first_err = g_last_error; }
        }
        {
            std::lock_guard<std::mutex> lock(m);
            for (int i = i0; i < i1; i++) {
                if (eng[(size_t)i]) fetchq.push_back(i);
                else fetched++;
            }
            build_limit = std::min(count, (g + 3) * group);
        }
        cv.notify_all();
    }
    {
        const auto t0 = now();
        std::unique_lock<std::mutex> lock(m);
        cv.wait(lock, [&] { return fetched == count; });
        quit = true;
        t_tail = since(t0);
    }
    if (prof) {
        fprintf(stderr, "[destroy] stream wait %.2f ms, graphs %.2f, pool %.2f, events %.2f, delete %.2f (all engines so far)\n", g_destroy_ns[0] * 1e-6,
                g_destroy_ns[1] * 1e-6, g_destroy_ns[2] * 1e-6, g_destroy_ns[3] * 1e-6, g_destroy_ns[4] * 1e-6);
        for (auto& a : g_destroy_ns) a = 0;
        fprintf(stderr, "[pool] idle: device %.0f MB, pinned %.0f MB; since the last report: allocated %lld device / %lld pinned blocks, freed %lld / %lld\n",
                g_pools[device].dev_bytes / 1048576.0, g_pools[device].pinned_bytes / 1048576.0, (long long)g_pool_miss[0], (long long)g_pool_miss[1],
                (long long)g_pool_spill[0], (long long)g_pool_spill[1]);
        for (int j = 0; j < 2; j++) { g_pool_miss[j] = 0; g_pool_spill[j] = 0; }
    }
    if (prof)
        fprintf(stderr, "[solve_many] %d problems, %d workers, groups of %d: waited for builds %.2f ms, lock-step runs %.2f ms, "
                        "waited for the last results %.2f ms\n"
                        "             builds %.2f ms in all, the slowest: create %.0f us, matrix %.0f, graph %.0f, parameters %.0f, event %.0f; "
                        "fetches %.2f ms in all, the slowest: results %.0f us, destroy %.0f\n",
                count, workers, group, t_wait * 1e3, t_run * 1e3, t_tail * 1e3, slow_build[0] * 1e3, slow_build[1] * 1e6,
                (slow_build[2] - slow_build[1]) * 1e6, (slow_build[3] - slow_build[2]) * 1e6, (slow_build[4] - slow_build[3]) * 1e6,
                (slow_build[5] - slow_build[4]) * 1e6, slow_fetch[0] * 1e3, slow_fetch[1] * 1e6, (slow_fetch[2] - slow_fetch[1]) * 1e6);
    cv.notify_all();
    for (std::thread& t : pool) t.join();
    for (hipStream_t st : wstream) if (st) { (void)hipStreamSynchronize(st); pool_stream_put(device, st); }
    (void)hipStreamSynchronize(rstream);
    pool_run_stream_put(device, rstream);
    if (fstream) { (void)hipStreamSynchronize(fstream); pool_stream_put(device, fstream); }
    for (int i = 0; i < count; i++)
        if (P[i].rc != NEMGPU_OK && rc == NEMGPU_OK) { rc = P[i].rc; first_err = errs[(size_t)i]; }
    if (rc != NEMGPU_OK && !first_err.empty()) set_error(first_err);
    return rc;
}


// ============================================================================================
// Chunks of a master pangenome, formed on the device (nem_chunks.hpp / nem_chunks.hip): the samples of partition()'s
// voting loop (ppanggolin.py:1045-1086), each the input files of __write_nem_input_files (ppanggolin.py:821-930) for
// that sample -- without the files, and without a matrix or a graph crossing PCIe per sample.
// ============================================================================================
// the engine's matrix staging rows, lane order and graph block filled by the device from the master (the engine was
// created with n = the chunk's kept families, d = the sample's organisms)
static int adopt_chunk(nemgpu_engine* e, const nemgpu_master* M, const nemk::ChunkPlan& plan, int nnz_c)
{
    if (e->device != M->device) { set_error("a chunk's engine lives on its master's device"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(e->device));
    alloc_for(e);
    int r;
    const size_t words = (size_t)e->n * e->wf;
    if ((r = dev_alloc(&e->xf_stage, words + (size_t)e->npad))) return r;
    e->perm = reinterpret_cast<int*>(e->xf_stage + words);
    const int nnz = std::max(nnz_c, 0);
    const size_t b_ptr = sizeof(int) * ((size_t)e->n + 1), b_nz = sizeof(int) * (size_t)std::max(nnz, 1);
    const size_t o_idx = (b_ptr + 255) & ~(size_t)255, o_w = (o_idx + b_nz + 255) & ~(size_t)255, total = o_w + b_nz;
    char* dev = nullptr;
    if ((r = dev_alloc(&dev, total))) return r;
    e->nei_ptr = (int*)dev; e->nei_idx = (int*)(dev + o_idx); e->nei_w = (float*)(dev + o_w);
    nemk::ChunkFill f{e->n, e->d, e->wf, e->npad, e->xf_stage, e->perm, e->nei_ptr, e->nei_idx, e->nei_w};
    nemk::launch_chunk_fill(M->dev, plan, f, e->stream);
    HIPCHK(hipGetLastError());
    e->nnz = nnz; e->has_graph = nnz > 0;
    e->host_bits = nullptr; e->host_bits_words = 0;              // (no host copy of the rows: random starts are not for chunk engines)
    if (e->defer_layout) e->layout_pending = true;               // (the group's first step carries the layouts, zipped)
    else { launch_layout(layout_args(e, e->xf_stage), e->stream); HIPCHK(hipGetLastError()); }
    e->have_matrix = true;
    return NEMGPU_OK;
}

// nemgpu_solve_chunks; with `votes`, every run is also voted (vote_group), with `tally` counted into its stats row
// (tally_group), and then a sample that keeps no family is skipped (the reference writes empty files for it and gets no
// .uf) instead of refused
static int solve_chunks_impl(nemgpu_master* M, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                             const float* disp_k, const nemgpu_config* cfg, int workers, int group, nemgpu_votes* votes,
                             ResampleTally* tally = nullptr)
{
    if (!M || !chunks || count <= 0 || k <= 0 || k > kMaxKernelK || !prop || !center_k || !disp_k || !cfg) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(M->device));
    const int n = M->n, nw64 = M->nw64, wf = M->wf, nnz = M->nnz;
    size_t org_total = 0;
    int max_dc = 0;
    for (int c = 0; c < count; c++) {
        nemgpu_chunk& q = chunks[c];
        q.rc = NEMGPU_OK; q.n = 0; q.nnz = 0; q.result = nemgpu_result{};
        if (!q.organisms || q.dc <= 0 || q.dc > M->d) { set_error("nemgpu_solve_chunks: chunk " + std::to_string(c) + ": 1 .. d organisms are needed"); return NEMGPU_E_FUNCARG; }
        for (int t = 0; t < q.dc; t++)
            if (q.organisms[t] < 0 || q.organisms[t] >= M->d) { set_error("nemgpu_solve_chunks: chunk " + std::to_string(c) + ": organism index out of range"); return NEMGPU_E_ARG; }
        org_total += ((size_t)q.dc + 63) & ~(size_t)63;
        max_dc = std::max(max_dc, q.dc);
    }
    // ---- phase 1, all chunks: which families, which edges, how many of each
    const size_t b_mask = a256((size_t)wf * 4), b_keep = a256((size_t)nw64 * 8), b_list = a256((size_t)n * 4), b_cov = a256((size_t)std::max(nnz, 1) * 4),
                 b_ptr = a256(((size_t)n + 1) * 4), b_cnt = 256;
    (void)b_cnt;
    const size_t per = b_mask + 2 * b_list + b_cov + b_ptr;
    // (every chunk's two counters and kept-family bits sit together: two copies bring them all to the host)
    const size_t b_plans = a256((size_t)count * sizeof(nemk::ChunkPlan)), b_org = a256(org_total * 4), b_counts = a256((size_t)count * 8),
                 b_keeps = b_keep * (size_t)count;
    const size_t o_counts = b_plans + b_org, o_keeps = o_counts + b_counts, o_per = o_keeps + b_keeps;
    static const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    char* slab = nullptr;
    if (hipMalloc(&slab, o_per + per * (size_t)count) != hipSuccess) { (void)hipGetLastError(); set_error("nemgpu_solve_chunks: device memory for the chunk plans"); return NEMGPU_E_MEMORY; }
    struct SlabFree { char* p; ~SlabFree() { if (p) (void)hipFree(p); } } slab_free{slab};
    std::vector<nemk::ChunkPlan> plans((size_t)count);
    std::vector<int> org_host(org_total, 0);
    {
        size_t oo = 0;
        for (int c = 0; c < count; c++) {
            char* b = slab + o_per + per * (size_t)c;
            nemk::ChunkPlan& p = plans[(size_t)c];
            p.organisms = reinterpret_cast<const int*>(slab + b_plans) + oo; p.dc = chunks[c].dc;
            memcpy(org_host.data() + oo, chunks[c].organisms, (size_t)chunks[c].dc * 4);
            oo += ((size_t)chunks[c].dc + 63) & ~(size_t)63;
            p.mask = (uint32_t*)b; b += b_mask;
            p.keep = (uint64_t*)(slab + o_keeps + b_keep * (size_t)c);
            p.list = (int*)b; b += b_list;
            p.map = (int*)b; b += b_list;
            p.cov = (uint32_t*)b; b += b_cov;
            p.ptr = (int*)b;
            p.counts = (int*)(slab + o_counts) + 2 * (size_t)c;
        }
    }
    HIPCHK(hipMemcpyAsync(slab, plans.data(), (size_t)count * sizeof(nemk::ChunkPlan), hipMemcpyHostToDevice, M->stream));
    HIPCHK(hipMemcpyAsync(slab + b_plans, org_host.data(), org_total * 4, hipMemcpyHostToDevice, M->stream));
    nemk::launch_chunk_plan(M->dev, reinterpret_cast<const nemk::ChunkPlan*>(slab), count, max_dc, M->stream);
    HIPCHK(hipGetLastError());
    std::vector<int> counts((size_t)count * 2);
    std::vector<char> keeps;
    bool want_keep = false;
    for (int c = 0; c < count; c++) want_keep = want_keep || chunks[c].keep != nullptr;
    HIPCHK(hipMemcpyAsync(counts.data(), slab + o_counts, (size_t)count * 8, hipMemcpyDeviceToHost, M->stream));
    if (want_keep) { keeps.resize(b_keeps); HIPCHK(hipMemcpyAsync(keeps.data(), slab + o_keeps, b_keeps, hipMemcpyDeviceToHost, M->stream)); }
    HIPCHK(hipStreamSynchronize(M->stream));
    if (want_keep)
        for (int c = 0; c < count; c++) if (chunks[c].keep) memcpy(chunks[c].keep, keeps.data() + b_keep * (size_t)c, (size_t)nw64 * 8);
    const auto t_plan = std::chrono::steady_clock::now();
    // ---- the problems: sizes from phase 1, PPanGGOLiN-style initial parameters (one value per class and kind)
    std::vector<nemgpu_problem> P;
    std::vector<nemk::ChunkPlan> pplans;
    std::vector<int> nnzc, slot;                              // (per problem: the chunk it solves)
    std::vector<uint8_t*> labels;
    P.reserve((size_t)count); pplans.reserve((size_t)count); nnzc.reserve((size_t)count); slot.reserve((size_t)count); labels.reserve((size_t)count);
    std::map<int, std::vector<float>> init;                   // sample size -> prop | center | disp
    for (int c = 0; c < count; c++) {
        nemgpu_chunk& q = chunks[c];
        q.n = counts[(size_t)c * 2]; q.nnz = counts[(size_t)c * 2 + 1];
        if (q.n <= 0 && (votes != nullptr || tally != nullptr)) continue;
        if (q.n <= 0) { set_error("nemgpu_solve_chunks: chunk " + std::to_string(c) + " holds no family"); q.rc = NEMGPU_E_ARG; return NEMGPU_E_ARG; }
        pplans.push_back(plans[(size_t)c]);
        nnzc.push_back(q.nnz);
        slot.push_back(c);
        labels.push_back(q.labels);
        std::vector<float>& v = init[q.dc];
        if (v.empty()) {
            v.resize((size_t)k + 2 * (size_t)k * q.dc);
            for (int h = 0; h < k; h++) {
                v[(size_t)h] = prop[h];
                for (int o = 0; o < q.dc; o++) { v[(size_t)k + (size_t)h * q.dc + o] = center_k[h]; v[(size_t)k + (size_t)k * q.dc + (size_t)h * q.dc + o] = disp_k[h]; }
            }
        }
        P.emplace_back();
        nemgpu_problem& p = P.back();
        p.n = q.n; p.d = q.dc; p.k = k;
        p.prop = v.data(); p.center = v.data() + k; p.disp = v.data() + k + (size_t)k * q.dc;
        p.out_prop = q.out_prop; p.out_center = q.out_center; p.out_disp = q.out_disp; p.out_nbobs_k = q.out_nbobs_k; p.out_c = nullptr;
    }
    ChunkSource src;
    src.master = M; src.plans = pplans.data(); src.nnz = nnzc.data(); src.labels = labels.data();
    src.votes = votes; src.slot = slot.data(); src.tally = tally;
    const auto t_prep = std::chrono::steady_clock::now();
    const int np = (int)P.size();
    const int rc = np > 0 ? solve_many_one(P.data(), np, cfg, M->device, workers, group, &src) : NEMGPU_OK;
    for (int i = 0; i < np; i++) { chunks[slot[(size_t)i]].rc = P[(size_t)i].rc; chunks[slot[(size_t)i]].result = P[(size_t)i].result; }
    if (prof) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[solve_chunks] %d chunks: plans (which families, which edges; one wait) %.2f ms, problem records %.2f ms, pipeline %.2f ms\n",
                count, ms(t_begin, t_plan), ms(t_plan, t_prep), ms(t_prep, std::chrono::steady_clock::now()));
    }
    return rc;
}

int nemgpu_solve_chunks(nemgpu_master* M, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                        const float* disp_k, const nemgpu_config* cfg, int workers, int group)
{
    return solve_chunks_impl(M, chunks, count, k, prop, center_k, disp_k, cfg, workers, group, nullptr);
}

// ============================================================================================
// The sub-problem of a selection of families (`__write_nem_input_files(..., filter_by_partition="shell")`,
// ppanggolin.py:844 and :859: what partition_shell solves), formed on the device into an engine that random starts can
// run on: the formed bit rows also come back into the engine's host rows, where nemgpu_run_random draws its centres.
// ============================================================================================
int nemgpu_master_subproblem(nemgpu_master* M, const int32_t* organisms, int dc, const uint8_t* select_bytes, int edge_rule, int k,
                             nemgpu_engine** engine, int32_t* families_out, int* n_out, int* nnz_out, int* outside_entry)
{
    if (!M || !organisms || !select_bytes || !engine || !n_out || !nnz_out) return NEMGPU_E_FUNCARG;
    *engine = nullptr; *n_out = 0; *nnz_out = 0;
    if (outside_entry) *outside_entry = -1;
    // ---- everything that can be refused without a launch
    if (M->directed) {
        set_error("nemgpu_master_subproblem: the master was built directed (nx.all_neighbors of a DiGraph lists a family that is both "
                  "predecessor and successor twice, its row holds it once)");
        return NEMGPU_E_ARG;
    }
    if (k <= 0 || k > kMaxKernelK) { set_error("nemgpu_master_subproblem: 1 .. 32 classes"); return NEMGPU_E_ARG; }
    if (edge_rule != nemk::kEdgeInduced && edge_rule != nemk::kEdgeReference) { set_error("nemgpu_master_subproblem: edge_rule is 0 (induced) or 1 (reference)"); return NEMGPU_E_ARG; }
    if (dc <= 0 || dc > M->d) { set_error("nemgpu_master_subproblem: 1 .. d organisms are needed"); return NEMGPU_E_ARG; }
    {
        std::vector<char> seen((size_t)M->d, 0);
        for (int t = 0; t < dc; t++) {
            const int o = organisms[t];
            if (o < 0 || o >= M->d) { set_error("nemgpu_master_subproblem: organism index out of range"); return NEMGPU_E_ARG; }
            if (seen[(size_t)o]) { set_error("nemgpu_master_subproblem: organism " + std::to_string(o) + " is given twice"); return NEMGPU_E_ARG; }
            seen[(size_t)o] = 1;
        }
    }
    const int n = M->n, nw64 = M->nw64, wf = M->wf, nnz = M->nnz;
    if (std::all_of(select_bytes, select_bytes + n, [](uint8_t b) { return b == 0; })) {
        set_error("nemgpu_master_subproblem: the selection keeps no family"); return NEMGPU_E_ARG;
    }
    HIPCHK(hipSetDevice(M->device));
    // ---- phase 1 of one plan: the selection packed to bits, then which families, which edges, how many of each
    const size_t b_plan = a256(sizeof(nemk::ChunkPlan)), b_org = a256((size_t)dc * 4), b_cnt = 256, b_sel = a256((size_t)n),
                 b_keep = a256((size_t)nw64 * 8), b_mask = a256((size_t)wf * 4), b_list = a256((size_t)n * 4),
                 b_cov = a256((size_t)std::max(nnz, 1) * 4), b_ptr = a256(((size_t)n + 1) * 4);
    char* slab = nullptr;
    if (hipMalloc(&slab, b_plan + b_org + b_cnt + b_sel + 2 * b_keep + b_mask + 2 * b_list + b_cov + b_ptr) != hipSuccess) {
        (void)hipGetLastError(); set_error("nemgpu_master_subproblem: device memory for the plan"); return NEMGPU_E_MEMORY;
    }
    // (the fill kernels read the plan's arrays on the engine's stream: the slab goes once both streams are idle)
    struct SlabFree { char* p; hipStream_t a; hipStream_t b; ~SlabFree() { (void)hipStreamSynchronize(a); if (b) (void)hipStreamSynchronize(b); (void)hipFree(p); } } slab_free{slab, M->stream, nullptr};
    nemk::ChunkPlan plan;
    char* b = slab + b_plan;
    plan.organisms = (const int*)b; b += b_org; plan.dc = dc;
    plan.counts = (int*)b; plan.outside = plan.counts + 2; b += b_cnt;
    uint8_t* sel_bytes_dev = (uint8_t*)b; b += b_sel;
    uint64_t* sel_bits = (uint64_t*)b; b += b_keep;
    plan.select = sel_bits; plan.edge_rule = edge_rule;
    plan.keep = (uint64_t*)b; b += b_keep;
    plan.mask = (uint32_t*)b; b += b_mask;
    plan.list = (int*)b; b += b_list;
    plan.map = (int*)b; b += b_list;
    plan.cov = (uint32_t*)b; b += b_cov;
    plan.ptr = (int*)b;
    HIPCHK(hipMemcpyAsync(slab, &plan, sizeof(plan), hipMemcpyHostToDevice, M->stream));
    HIPCHK(hipMemcpyAsync(slab + b_plan, organisms, (size_t)dc * 4, hipMemcpyHostToDevice, M->stream));
    HIPCHK(hipMemcpyAsync(sel_bytes_dev, select_bytes, (size_t)n, hipMemcpyHostToDevice, M->stream));
    nemk::launch_select_pack(sel_bytes_dev, n, nw64, sel_bits, M->stream);
    nemk::launch_chunk_plan(M->dev, reinterpret_cast<const nemk::ChunkPlan*>(slab), 1, dc, M->stream);
    HIPCHK(hipGetLastError());
    int counts[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(counts, plan.counts, sizeof(counts), hipMemcpyDeviceToHost, M->stream));
    HIPCHK(hipStreamSynchronize(M->stream));
    *n_out = counts[0]; *nnz_out = counts[1];
    if (edge_rule == nemk::kEdgeReference && counts[2] != INT_MAX) {          // the writer's KeyError: no problem is formed
        if (outside_entry) *outside_entry = counts[2];
        return NEMGPU_OK;
    }
    if (counts[0] <= 0) { set_error("nemgpu_master_subproblem: the selection keeps no family (none is present in these organisms)"); return NEMGPU_E_ARG; }
    // ---- phase 2: the engine, its buffers filled in place, its rows brought back for the random starts
    nemgpu_engine* e = nullptr;
    int r = nemgpu_create(&e, counts[0], dc, k, 0, counts[0], M->device, nullptr);
    if (r != NEMGPU_OK) return r;
    slab_free.b = e->stream;
    r = adopt_chunk(e, M, plan, counts[1]);
    hipError_t err = hipSuccess;
    if (r == NEMGPU_OK) {
        const size_t words = (size_t)e->n * e->wf;
        uint32_t* rows = host_bits_reserve(e, words);
        err = hipMemcpyAsync(rows, e->xf_stage, words * 4, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess && families_out) err = hipMemcpyAsync(families_out, plan.list, (size_t)counts[0] * 4, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    }
    if (r == NEMGPU_OK && err != hipSuccess) { (void)hipGetLastError(); set_error(std::string("nemgpu_master_subproblem: ") + hipGetErrorString(err)); r = NEMGPU_E_DEVICE; }
    if (r != NEMGPU_OK) { slab_free.b = nullptr; (void)hipStreamSynchronize(e->stream); nemgpu_destroy(e); return r; }
    *engine = e;
    return NEMGPU_OK;
}

// the problem an engine holds as nemgpu_master_subproblem formed it: bit rows [n][ceil(d/32)], ptr [n + 1], idx and w [nnz]
int nemgpu_subproblem_fetch(nemgpu_engine* e, uint32_t* xbits, int32_t* ptr, int32_t* idx, float* w)
{
    if (!e) return NEMGPU_E_FUNCARG;
    if (!e->have_matrix || e->host_bits_words != (size_t)e->n * e->wf || !e->nei_ptr) { set_error("nemgpu_subproblem_fetch: not an engine of nemgpu_master_subproblem"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    if (xbits) memcpy(xbits, e->host_bits, e->host_bits_words * 4);
    if (ptr) HIPCHK(hipMemcpyAsync(ptr, e->nei_ptr, ((size_t)e->n + 1) * 4, hipMemcpyDeviceToHost, e->stream));
    if (idx && e->nnz > 0) HIPCHK(hipMemcpyAsync(idx, e->nei_idx, (size_t)e->nnz * 4, hipMemcpyDeviceToHost, e->stream));
    if (w && e->nnz > 0) HIPCHK(hipMemcpyAsync(w, e->nei_w, (size_t)e->nnz * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NEMGPU_OK;
}

// ============================================================================================
// The vote of partition()'s loop over the samples (validate_family, ppanggolin.py:1015-1037, and the loop around it,
// :1045-1105) on the device: nem_vote.hpp / nem_vote.hip.
// ============================================================================================
int nemgpu_votes_create(nemgpu_votes** out, nemgpu_master* M, const int32_t* organisms, int d_sel, int chunk_size, int batch)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!M || !organisms || d_sel <= 0 || chunk_size <= 0 || batch <= 0) { set_error("nemgpu_votes_create: a master, organisms, chunk size and batch are needed"); return NEMGPU_E_FUNCARG; }
    if (d_sel > M->d || batch > 4096) { set_error("nemgpu_votes_create: more organisms than the master's, or a batch above 4096"); return NEMGPU_E_ARG; }
    std::vector<uint8_t> seen((size_t)M->d, 0);
    for (int t = 0; t < d_sel; t++) {
        const int o = organisms[t];
        if (o < 0 || o >= M->d || seen[(size_t)o]) { set_error("nemgpu_votes_create: organism index out of range or repeated"); return NEMGPU_E_ARG; }
        seen[(size_t)o] = 1;
    }
    HIPCHK(hipSetDevice(M->device));
    const int n = M->n;
    const size_t b_cnt = a256((size_t)n * 16), b_st = a256((size_t)n), b_first = a256((size_t)n * 4), b_V = a256((size_t)batch * n),
                 b_maps = a256((size_t)batch * nemk::kVoteMapStride), b_desc = a256((size_t)batch * sizeof(nemk::VoteDesc)), b_words = 256,
                 b_sel = a256((size_t)d_sel * 4);
    nemgpu_votes* v = new nemgpu_votes();
    v->master = M; v->device = M->device; v->n = n; v->d_sel = d_sel; v->chunk_size = chunk_size; v->batch = batch;
    v->quotient = (double)d_sel / (double)chunk_size;
    auto fail = [&](const char* what) { nemgpu_votes_destroy(v); set_error(what); return NEMGPU_E_DEVICE; };
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    if (hipMalloc(&v->block, b_cnt + b_st + b_first + b_V + b_maps + b_desc + b_words + b_sel) != hipSuccess) return fail("nemgpu_votes_create: device memory");
    if (hipHostMalloc((void**)&v->words_host, 2 * sizeof(int), hipHostMallocDefault) != hipSuccess) { v->words_host = nullptr; return fail("nemgpu_votes_create: pinned memory"); }
    char* b = v->block;
    v->state.n = n;
    v->state.cnt = (int32_t*)b; b += b_cnt;
    v->state.st = (uint8_t*)b; b += b_st;
    v->state.first = (int32_t*)b; b += b_first;
    v->V = (uint8_t*)b; b += b_V;
    v->maps = (uint8_t*)b; b += b_maps;
    v->desc = (nemk::VoteDesc*)b; b += b_desc;
    v->words = (int*)b; b += b_words;
    int* sel = (int*)b;
    hipError_t err = hipMemcpyAsync(sel, organisms, (size_t)d_sel * 4, hipMemcpyHostToDevice, v->stream);
    if (err == hipSuccess) { nemk::launch_vote_init(v->state, M->dev.xt, M->nw64, sel, d_sel, v->stream); err = hipGetLastError(); }
    if (err == hipSuccess) err = hipStreamSynchronize(v->stream);
    if (err != hipSuccess) return fail("nemgpu_votes_create: initialisation failed");
    *out = v;
    return NEMGPU_OK;
}

void nemgpu_votes_destroy(nemgpu_votes* v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) { (void)hipStreamSynchronize(v->stream); (void)hipStreamDestroy(v->stream); }
    if (v->block) (void)hipFree(v->block);
    if (v->words_host) (void)hipHostFree(v->words_host);
    delete v;
}

// one group of nemgpu_solve_many's pipeline, run and waited for: every member's code map from its final parameters and
// its labels into its row of the vote matrix, straight from the engine's buffers (labels and parameters stay on the device)
static int vote_group(nemgpu_votes* v, const std::vector<nemgpu_engine*>& E, const std::vector<int>& who,
                      const std::vector<nemgpu_result>& R, const ChunkSource* src)
{
    const int B = (int)E.size();
    if (B > v->batch) { set_error("vote: a group larger than the vote batch"); return NEMGPU_E_INTERNAL; }
    std::vector<nemk::VoteDesc> d((size_t)B);
    int max_n = 0;
    for (int j = 0; j < B; j++) {
        const nemgpu_engine* e = E[(size_t)j];
        if (!e->ncem() || e->k != 3) { set_error("vote: NCEM runs of three classes are voted"); return NEMGPU_E_ARG; }
        const int i = who[(size_t)j];
        d[(size_t)j] = nemk::VoteDesc{e->lab[e->cur] + e->lo, src->plans[i].list, e->prop + e->par_o_center, e->prop + e->par_o_disp,
                                      e->n, e->d, R[(size_t)j].status, src->slot[i]};
        max_n = std::max(max_n, e->n);
    }
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMemcpyAsync(v->desc, d.data(), (size_t)B * sizeof(nemk::VoteDesc), hipMemcpyHostToDevice, v->stream));
    nemk::launch_vote_classmap(v->desc, B, 3, v->maps, v->stream);
    nemk::launch_vote_scatter(v->desc, B, max_n, v->maps, v->V, v->n, v->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(v->stream));          // (the engines go to the fetches next, and d goes out of scope)
    return NEMGPU_OK;
}

// the batch's `count` rows of V into the counts; *stop_index = the row after which every family is validated, or -1
static int vote_commit_batch(nemgpu_votes* v, int count, int* stop_index)
{
    HIPCHK(hipMemsetAsync(v->words, 0, 2 * sizeof(int), v->stream));
    nemk::launch_vote_scan(v->state, v->V, count, v->quotient, v->d_sel, v->samples_voted, v->words, v->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(v->words_host, v->words, 2 * sizeof(int), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipStreamSynchronize(v->stream));
    int stop = -1;
    if (v->words_host[0] == 0) { stop = v->words_host[1] - 1; v->done = true; }
    v->samples_voted += stop >= 0 ? stop + 1 : (v->done ? 0 : count);
    if (stop_index) *stop_index = stop;
    return NEMGPU_OK;
}

static int votes_begin(nemgpu_votes* v, int count, const char* who)
{
    if (count <= 0 || count > v->batch) { set_error(std::string(who) + ": 1 .. batch samples per call"); return NEMGPU_E_ARG; }
    if (v->done) { set_error(std::string(who) + ": every family is validated already"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMemsetAsync(v->V, nemk::kVoteNone, (size_t)count * v->n, v->stream));
    return NEMGPU_OK;
}

int nemgpu_votes_solve(nemgpu_votes* v, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                       const float* disp_k, const nemgpu_config* cfg, int workers, int group, int* stop_index)
{
    if (stop_index) *stop_index = -1;
    if (!v || !chunks || !cfg) return NEMGPU_E_FUNCARG;
    if (k != 3 || cfg->algo != NEMGPU_ALGO_NCEM) { set_error("nemgpu_votes_solve: the vote takes NCEM runs of three classes"); return NEMGPU_E_ARG; }
    int r = votes_begin(v, count, "nemgpu_votes_solve");
    if (r != NEMGPU_OK) return r;
    r = solve_chunks_impl(const_cast<nemgpu_master*>(v->master), chunks, count, k, prop, center_k, disp_k, cfg, workers, group, v);
    if (r != NEMGPU_OK) return r;
    return vote_commit_batch(v, count, stop_index);
}

int nemgpu_votes_add_host(nemgpu_votes* v, int count, const uint64_t* keep, const uint8_t* labels, const uint8_t* maps, int* stop_index)
{
    if (stop_index) *stop_index = -1;
    if (!v || !keep || !labels || !maps) return NEMGPU_E_FUNCARG;
    const int n = v->n, nw64 = (n + 63) / 64;
    for (int s = 0; s < count; s++)
        for (int c = 0; c < 3; c++) if (maps[(size_t)s * 3 + c] > 3) { set_error("nemgpu_votes_add_host: codes are 0 .. 3"); return NEMGPU_E_ARG; }
    int r = votes_begin(v, count, "nemgpu_votes_add_host");
    if (r != NEMGPU_OK) return r;
    // the samples as the pipeline leaves them on the device: per sample its kept families' master indices and labels
    std::vector<int> list((size_t)count * n);
    std::vector<uint8_t> lab((size_t)count * n), map4((size_t)count * nemk::kVoteMapStride);
    std::vector<int> nk((size_t)count, 0);
    for (int s = 0; s < count; s++) {
        int j = 0;
        for (int f = 0; f < n; f++) {
            if (!((keep[(size_t)s * nw64 + (f >> 6)] >> (f & 63)) & 1ull)) continue;
            const uint8_t l = labels[(size_t)s * n + j];
            if (l > 2) { set_error("nemgpu_votes_add_host: labels are 0 .. 2"); return NEMGPU_E_ARG; }
            list[(size_t)s * n + j] = f; lab[(size_t)s * n + j] = l; j++;
        }
        nk[(size_t)s] = j;
        for (int c = 0; c < nemk::kVoteMapStride; c++) map4[(size_t)s * nemk::kVoteMapStride + c] = c < 3 ? maps[(size_t)s * 3 + c] : 3;
    }
    char* tmp = nullptr;
    const size_t b_list = (size_t)count * n * 4;
    HIPCHK(hipMalloc(&tmp, b_list + (size_t)count * n));
    struct TmpFree { char* p; ~TmpFree() { (void)hipFree(p); } } tmp_free{tmp};
    std::vector<nemk::VoteDesc> d((size_t)count);
    int max_n = 0;
    for (int s = 0; s < count; s++) {
        d[(size_t)s] = nemk::VoteDesc{(const uint8_t*)(tmp + b_list) + (size_t)s * n, (const int*)tmp + (size_t)s * n, nullptr, nullptr,
                                      nk[(size_t)s], 0, 0, s};
        max_n = std::max(max_n, nk[(size_t)s]);
    }
    HIPCHK(hipMemcpyAsync(tmp, list.data(), b_list, hipMemcpyHostToDevice, v->stream));
    HIPCHK(hipMemcpyAsync(tmp + b_list, lab.data(), (size_t)count * n, hipMemcpyHostToDevice, v->stream));
    HIPCHK(hipMemcpyAsync(v->maps, map4.data(), map4.size(), hipMemcpyHostToDevice, v->stream));
    HIPCHK(hipMemcpyAsync(v->desc, d.data(), (size_t)count * sizeof(nemk::VoteDesc), hipMemcpyHostToDevice, v->stream));
    nemk::launch_vote_scatter(v->desc, count, max_n, v->maps, v->V, n, v->stream);
    HIPCHK(hipGetLastError());
    r = vote_commit_batch(v, count, stop_index);      // (waits for the stream: the host arrays outlive their copies)
    return r;
}

int nemgpu_vote_classmap_host(int count, int k, const int* dc, const float* center, const float* disp, const int* status, uint8_t* maps)
{
    if (count <= 0 || !dc || !center || !disp || !status || !maps) return NEMGPU_E_FUNCARG;
    if (k != 3) { set_error("nemgpu_vote_classmap_host: the class map is PPanGGOLiN's, for three classes"); return NEMGPU_E_ARG; }
    size_t total = 0;
    for (int s = 0; s < count; s++) {
        if (dc[s] <= 0) { set_error("nemgpu_vote_classmap_host: a sample has organisms"); return NEMGPU_E_ARG; }
        total += (size_t)k * dc[s];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no usable HIP device: this library has no CPU fallback"); return NEMGPU_E_DEVICE; }
    g_hip_used.store(true);
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamFree { hipStream_t s; ~StreamFree() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } st_free{st};
    const size_t b_par = a256(total * 4), b_desc = a256((size_t)count * sizeof(nemk::VoteDesc));
    char* tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, 2 * b_par + b_desc + (size_t)count * nemk::kVoteMapStride));
    struct TmpFree { hipStream_t s; char* p; ~TmpFree() { (void)hipStreamSynchronize(s); (void)hipFree(p); } } tmp_free{st, tmp};
    float* dcen = (float*)tmp;
    float* ddis = (float*)(tmp + b_par);
    nemk::VoteDesc* ddesc = (nemk::VoteDesc*)(tmp + 2 * b_par);
    uint8_t* dmaps = (uint8_t*)(tmp + 2 * b_par + b_desc);
    std::vector<nemk::VoteDesc> d((size_t)count);
    size_t off = 0;
    for (int s = 0; s < count; s++) {
        d[(size_t)s] = nemk::VoteDesc{nullptr, nullptr, dcen + off, ddis + off, 0, dc[s], status[s], s};
        off += (size_t)k * dc[s];
    }
    std::vector<uint8_t> m4((size_t)count * nemk::kVoteMapStride);
    HIPCHK(hipMemcpyAsync(dcen, center, total * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ddis, disp, total * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ddesc, d.data(), (size_t)count * sizeof(nemk::VoteDesc), hipMemcpyHostToDevice, st));
    nemk::launch_vote_classmap(ddesc, count, k, dmaps, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(m4.data(), dmaps, m4.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < count; s++)
        for (int c = 0; c < 3; c++) maps[(size_t)s * 3 + c] = m4[(size_t)s * nemk::kVoteMapStride + c];
    return NEMGPU_OK;
}

int nemgpu_votes_result(nemgpu_votes* v, int32_t* cnt, uint8_t* final_code, int32_t* validated, int64_t* samples_voted)
{
    if (!v) return NEMGPU_E_FUNCARG;
    const int n = v->n;
    std::vector<int32_t> c((size_t)n * 4), first((size_t)n);
    std::vector<uint8_t> st((size_t)n);
    HIPCHK(hipSetDevice(v->device));
    HIPCHK(hipMemcpyAsync(c.data(), v->state.cnt, c.size() * 4, hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipMemcpyAsync(st.data(), v->state.st, st.size(), hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipMemcpyAsync(first.data(), v->state.first, first.size() * 4, hipMemcpyDeviceToHost, v->stream));
    HIPCHK(hipStreamSynchronize(v->stream));
    if (cnt) memcpy(cnt, c.data(), c.size() * 4);
    if (validated) memcpy(validated, first.data(), first.size() * 4);
    if (final_code)
        for (int f = 0; f < n; f++) {
            // max(cnt, key=cnt.get) in the order P, S, C, U (ppanggolin.py:1104-1105); a forced U is sys.maxsize votes
            uint8_t best = 0;
            for (uint8_t k = 1; k < 4; k++) if (c[(size_t)f * 4 + k] > c[(size_t)f * 4 + best]) best = k;
            final_code[f] = !(st[(size_t)f] & nemk::VOTE_IN_PAN) ? nemk::kVoteNone : (st[(size_t)f] & nemk::VOTE_FORCED_U) ? 3 : best;
        }
    if (samples_voted) *samples_voted = v->samples_voted;
    return NEMGPU_OK;
}

// ============================================================================================
// The evolution curve's resamples (command_line.py:262-281, 591-625): many samples of one master solved as
// nemgpu_solve_chunks solves them, each reduced on the device to the stats of partition(just_stats=True)
// (nem_resample.hpp / nem_resample.hip).
// ============================================================================================

// one group of nemgpu_solve_many's pipeline, run and waited for: every member's code map from its final parameters
// (launch_vote_classmap, as vote_group) and its labels counted into its stats row, straight from the engine's buffers
static int tally_group(ResampleTally* t, const std::vector<nemgpu_engine*>& E, const std::vector<int>& who,
                       const std::vector<nemgpu_result>& R, const ChunkSource* src)
{
    const int B = (int)E.size();
    if (B > kTallyGroupCap) { set_error("resamples: a group larger than the tally's"); return NEMGPU_E_INTERNAL; }
    std::vector<nemk::VoteDesc> d((size_t)B);
    for (int j = 0; j < B; j++) {
        const nemgpu_engine* e = E[(size_t)j];
        if (!e->ncem() || e->k != 3) { set_error("resamples: NCEM runs of three classes are counted"); return NEMGPU_E_ARG; }
        const int i = who[(size_t)j];
        d[(size_t)j] = nemk::VoteDesc{e->lab[e->cur] + e->lo, src->plans[i].list, e->prop + e->par_o_center, e->prop + e->par_o_disp,
                                      e->n, e->d, R[(size_t)j].status, src->slot[i]};
    }
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipMemcpyAsync(t->desc, d.data(), (size_t)B * sizeof(nemk::VoteDesc), hipMemcpyHostToDevice, t->stream));
    nemk::launch_vote_classmap(t->desc, B, 3, t->maps, t->stream);
    nemk::launch_resample_tally(t->desc, B, t->maps, t->stats, t->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(t->stream));          // (the engines go to the fetches next, and d goes out of scope)
    return NEMGPU_OK;
}

int nemgpu_resamples_solve(nemgpu_master* M, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                           const float* disp_k, const nemgpu_config* cfg, int workers, int group, int32_t* stats)
{
    if (!M || !chunks || count <= 0 || !prop || !center_k || !disp_k || !cfg || !stats) return NEMGPU_E_FUNCARG;
    if (k != 3 || cfg->algo != NEMGPU_ALGO_NCEM) { set_error("nemgpu_resamples_solve: the stats take NCEM runs of three classes"); return NEMGPU_E_ARG; }
    // every check before anything is launched; a resample is an ordered SET of organisms (the reference's OrderedSet)
    std::vector<int> seen((size_t)M->d, -1), off((size_t)count + 1, 0);
    for (int c = 0; c < count; c++) {
        const nemgpu_chunk& q = chunks[c];
        if (!q.organisms || q.dc <= 0 || q.dc > M->d) { set_error("nemgpu_resamples_solve: sample " + std::to_string(c) + ": 1 .. d organisms are needed"); return NEMGPU_E_FUNCARG; }
        for (int t = 0; t < q.dc; t++) {
            const int o = q.organisms[t];
            if (o < 0 || o >= M->d) { set_error("nemgpu_resamples_solve: sample " + std::to_string(c) + ": organism index out of range"); return NEMGPU_E_ARG; }
            if (seen[(size_t)o] == c) { set_error("nemgpu_resamples_solve: sample " + std::to_string(c) + ": organism " + std::to_string(o) + " repeated"); return NEMGPU_E_ARG; }
            seen[(size_t)o] = c;
        }
        off[(size_t)c + 1] = off[(size_t)c] + q.dc;
    }
    HIPCHK(hipSetDevice(M->device));
    const int total = off[(size_t)count];
    std::vector<int> org((size_t)total);
    for (int c = 0; c < count; c++) memcpy(org.data() + off[(size_t)c], chunks[c].organisms, (size_t)chunks[c].dc * 4);
    const size_t b_stats = a256((size_t)count * nemk::kResampleStats * 4), b_desc = a256((size_t)kTallyGroupCap * sizeof(nemk::VoteDesc)),
                 b_maps = a256((size_t)kTallyGroupCap * nemk::kVoteMapStride), b_off = a256(((size_t)count + 1) * 4), b_org = a256((size_t)total * 4);
    ResampleTally t;
    t.device = M->device;
    char* block = nullptr;
    struct Free {
        ResampleTally& t; char*& p;
        ~Free() { if (t.stream) { (void)hipStreamSynchronize(t.stream); (void)hipStreamDestroy(t.stream); } if (p) (void)hipFree(p); }
    } release{t, block};
    HIPCHK(hipStreamCreateWithFlags(&t.stream, hipStreamNonBlocking));
    if (hipMalloc(&block, b_stats + b_desc + b_maps + b_off + b_org) != hipSuccess) {
        (void)hipGetLastError(); block = nullptr; set_error("nemgpu_resamples_solve: device memory"); return NEMGPU_E_MEMORY;
    }
    t.stats = (int32_t*)block;
    t.desc = (nemk::VoteDesc*)(block + b_stats);
    t.maps = (uint8_t*)(block + b_stats + b_desc);
    int* d_off = (int*)(block + b_stats + b_desc + b_maps);
    int* d_org = (int*)(block + b_stats + b_desc + b_maps + b_off);
    // core_exact / accessory of every sample on the tally's stream, beside the chunk pipeline's phase 1
    HIPCHK(hipMemsetAsync(t.stats, 0, (size_t)count * nemk::kResampleStats * 4, t.stream));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), ((size_t)count + 1) * 4, hipMemcpyHostToDevice, t.stream));
    HIPCHK(hipMemcpyAsync(d_org, org.data(), (size_t)total * 4, hipMemcpyHostToDevice, t.stream));
    nemk::launch_resample_core(M->dev.xt, M->n, M->nw64, d_org, d_off, count, t.stats, t.stream);
    HIPCHK(hipGetLastError());
    const int rc = solve_chunks_impl(M, chunks, count, k, prop, center_k, disp_k, cfg, workers, group, nullptr, &t);
    if (rc != NEMGPU_OK) return rc;
    HIPCHK(hipMemcpyAsync(stats, t.stats, (size_t)count * nemk::kResampleStats * 4, hipMemcpyDeviceToHost, t.stream));
    HIPCHK(hipStreamSynchronize(t.stream));
    return NEMGPU_OK;
}

// Which device solves which problem when nemgpu_solve_many_devices deals the lock-step groups: group g (problems
// g*group .. g*group + group - 1) goes to slot g % n_devices of the device list.  Host arithmetic only.
int nemgpu_deal_groups(int count, int group, int n_devices, int* slot_of_problem)
{
    if (count < 0 || n_devices <= 0 || !slot_of_problem) return NEMGPU_E_FUNCARG;
    group = std::max(1, std::min(group, 256));
    for (int i = 0; i < count; i++) slot_of_problem[i] = (i / group) % n_devices;
    return NEMGPU_OK;
}

// nemgpu_solve_many over SEVERAL devices of this process: the reference's own form of parallelism -- independent chunk
// problems side by side (multiprocessing.Pool over 500-organism chunks, ppanggolin.py:1039-1095) -- with the devices in
// the role of the pool's workers.  The lock-step groups are dealt round-robin over `devices` (an entry may repeat: two
// pipelines on one device); every device runs its share through nemgpu_solve_many on a thread of its own, with its own
// worker threads, streams, lock-step contexts and resource pool; no device waits for another.  Every problem's result
// equals its own nemgpu_run.  Returns the first failure (each problem's own status is in its rc).
int nemgpu_solve_many_devices(nemgpu_problem* P, int count, const nemgpu_config* cfg, const int* devices, int n_devices,
                              int workers, int group)
{
    if (!P || count <= 0 || !cfg || !devices || n_devices <= 0) return NEMGPU_E_FUNCARG;
    if (n_devices == 1) return nemgpu_solve_many(P, count, cfg, devices[0], workers, group);
    const int ndev = nemgpu_device_count();
    for (int s = 0; s < n_devices; s++)
        if (devices[s] < 0 || devices[s] >= ndev) { set_error("nemgpu_solve_many_devices: bad device index in the list"); return NEMGPU_E_ARG; }
    group = std::max(1, std::min(group, 256));
    std::vector<int> slot((size_t)count);
    (void)nemgpu_deal_groups(count, group, n_devices, slot.data());
    std::vector<std::vector<nemgpu_problem>> sub((size_t)n_devices);
    std::vector<std::vector<int>> who((size_t)n_devices);
    for (int i = 0; i < count; i++) { sub[(size_t)slot[i]].push_back(P[i]); who[(size_t)slot[i]].push_back(i); }
    std::vector<int> rcs((size_t)n_devices, NEMGPU_OK);
    std::vector<std::string> errs((size_t)n_devices);
    const int wk = std::max(1, workers / n_devices);
    std::vector<std::thread> th;
    for (int s = 0; s < n_devices; s++) {
        if (sub[(size_t)s].empty()) continue;
        th.emplace_back([&, s] {
            tl_runner = true;
            rcs[(size_t)s] = nemgpu_solve_many(sub[(size_t)s].data(), (int)sub[(size_t)s].size(), cfg, devices[s], wk, group);
            if (rcs[(size_t)s] != NEMGPU_OK) errs[(size_t)s] = g_last_error;       // (the error text is per thread)
        });
    }
    for (std::thread& t : th) t.join();
    int rc = NEMGPU_OK;
    for (int s = 0; s < n_devices; s++) {
        for (size_t j = 0; j < sub[(size_t)s].size(); j++) {
            P[who[(size_t)s][j]].result = sub[(size_t)s][j].result;
            P[who[(size_t)s][j]].rc = sub[(size_t)s][j].rc;
        }
        if (rcs[(size_t)s] != NEMGPU_OK && rc == NEMGPU_OK) { rc = rcs[(size_t)s]; set_error(errs[(size_t)s]); }
    }
    return rc;
}

// ---- random starts in lock step -------------------------------------------------------------------------------
// A state-only twin of `p`: matrix layouts, graph and draw table are p's, everything else is carved from `slab`.
static int make_clone(nemgpu_engine* p, nemgpu_engine** out, char* slab, size_t slab_bytes, int* flags_host, float* par0)
{
    nemgpu_engine* c = new nemgpu_engine();
    c->n_total = p->n_total; c->n_true = p->n_true; c->d = p->d; c->k = p->k; c->lo = p->lo; c->hi = p->hi; c->n = p->n;
    c->npad = p->npad; c->dpad = p->dpad; c->W = p->W; c->wf = p->wf; c->nw64 = p->nw64; c->device = p->device;
    c->stream = p->stream; c->own_stream = false;
    c->cfg = p->cfg; c->have_matrix = true; c->have_params = true; c->has_graph = p->has_graph;
    c->xw = p->xw; c->xws = p->xws; c->perm = p->perm; c->xt = p->xt; c->use_sort = p->use_sort;
    c->nei_ptr = p->nei_ptr; c->nei_idx = p->nei_idx; c->nei_w = p->nei_w; c->nnz = p->nnz;
    c->use_graphs = p->use_graphs; c->ff_mode = p->ff_mode; c->ff_batch = p->ff_batch; c->map_margin = p->map_margin; c->round_batch = p->round_batch; c->rounds_iter = p->rounds_iter;
    c->parent = p; c->carve_all = true;
    c->chunks.push_back({slab, slab_bytes, 0, false});
    c->shared_chunk = 0;
    c->flags_host = flags_host; c->flags_host_borrowed = true;
    const size_t kd = (size_t)p->k * p->d;
    c->prop0 = par0; c->center0 = par0 + p->k; c->disp0 = par0 + p->k + kd;
    alloc_for(c);
    int r = alloc_model_buffers(c);
    if (r == NEMGPU_OK) r = ensure_state_buffers(c);
    if (r == NEMGPU_OK) r = ensure_crit_buffers(c);
    alloc_for(p);
    if (r != NEMGPU_OK) { nemgpu_destroy(c); return r; }
    c->draw_ctl = c->sweep_next + 8;
    *out = c;
    return NEMGPU_OK;
}

// `count` twins of e (kept for the next call)
static int ensure_clones(nemgpu_engine* e, int count)
{
    if ((int)e->clones.size() >= count) return NEMGPU_OK;
    HIPCHK(hipStreamSynchronize(e->stream));
    for (nemgpu_engine* c : e->clones) nemgpu_destroy(c);
    e->clones.clear();
    pool_put(e->device, false, e->clone_slab, e->clone_slab_size); e->clone_slab = nullptr;
    pool_put(e->device, true, (char*)e->clone_flags_host, e->clone_flags_size); e->clone_flags_host = nullptr;
    // what one twin carves: a dry run of its allocations
    {
        nemgpu_engine probe;
        probe.n_total = e->n_total; probe.d = e->d; probe.k = e->k; probe.n = e->n; probe.npad = e->npad; probe.dpad = e->dpad;
        probe.W = e->W; probe.nw64 = e->nw64; probe.cfg = e->cfg; probe.parent = e; probe.dry_run = true;
        alloc_for(&probe);
        int r = alloc_model_buffers(&probe);
        if (r == NEMGPU_OK) r = ensure_state_buffers(&probe);
        if (r == NEMGPU_OK) r = ensure_crit_buffers(&probe);
        alloc_for(e);
        if (r) return r;
        e->clone_bytes = probe.dry_bytes + 4096;
    }
    const size_t kd = (size_t)e->k * e->d;
    const size_t par_bytes = (((size_t)count * (e->k + 2 * kd) * sizeof(float)) + 255) & ~(size_t)255;
    HIPCHK(pool_get(e->device, false, par_bytes + (size_t)count * e->clone_bytes, &e->clone_slab, &e->clone_slab_size));
    HIPCHK(hipMemsetAsync(e->clone_slab, 0, par_bytes + (size_t)count * e->clone_bytes, e->stream));
    HIPCHK(pool_get(e->device, true, (size_t)count * e->flag_words() * sizeof(int), (char**)&e->clone_flags_host, &e->clone_flags_size));
    e->clone_par0 = reinterpret_cast<float*>(e->clone_slab);
    for (int i = 0; i < count; i++) {
        nemgpu_engine* c = nullptr;
        int r = make_clone(e, &c, e->clone_slab + par_bytes + (size_t)i * e->clone_bytes, e->clone_bytes,
                           e->clone_flags_host + (size_t)i * e->flag_words(), e->clone_par0 + (size_t)i * (e->k + 2 * kd));
        if (r) return r;
        e->clones.push_back(c);
    }
    return NEMGPU_OK;
}

// INIT_RANDOM: RandNemAlgo (nem_alg.c:1574-1742).  InitPara's whole-sample dispersion (:1200-1281) is one M-step
// with every family in class 0; every start draws its centres from the data (MakeRandomPara, :1381-1473), runs the
// INIT_PARAM_FILE pipeline on them and is ranked by criterion M (DEFAULT_CRIT, nem_typ.h:80); the best partition is
// restored and EstimPara run on it (:1703-1713).
// What of it does not depend on how the starts are run -- one after the other or in lock step:
struct RandomStarts {
    nemgpu_engine* e = nullptr;
    std::vector<float> dispsam;                                    // InitPara: the whole sample's dispersion
    GlibcRandom rng{1};
    int nbsucc = 0, best = -1, last_status = NEMGPU_OK;
    float best_crit[6] = {0, 0, 0, 0, 0, 0};
    nemgpu_result best_res{};

    int begin(nemgpu_engine* engine, uint32_t seed)
    {
        e = engine;
        int r;
        const int n = e->n, k = e->k, d = e->d;
        if ((r = ensure_state_buffers(e))) return r;
        // ---- InitPara: dispersion of the whole sample
        e->have_params = true;                                     // (the slots are (re)written by every start)
        if ((r = reset_state(e))) return r;
        if (e->ncem()) {
            HIPCHK(hipMemsetAsync(e->lab[0], 0, (size_t)e->n_total, e->stream));
        } else {
            std::vector<float> c1((size_t)n * k, 0.0f);
            for (int i = 0; i < n; i++) c1[(size_t)i * k] = 1.0f;
            HIPCHK(copy_sync(e, e->cbuf[0], c1.data(), c1.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        e->cur = 0; e->masks_valid = false;
        if ((r = do_mstep(e))) return r;
        if (!e->ncem() && (r = read_iter_flags(e))) return r;     // (a fuzzy M-step can report a fault)
        dispsam.resize((size_t)d);
        HIPCHK(copy_sync(e, dispsam.data(), e->disp, sizeof(float) * d, hipMemcpyDeviceToHost));
        rng.seed(seed);
        if (e->libc() && e->cfg.tie_seed != seed) { e->cfg.tie_seed = seed; e->draw_valid = false; }   // one stream (nem_exe.c:621)
        alloc_for(e);
        if (e->ncem()) { if (!e->best_lab && (r = dev_alloc(&e->best_lab, (size_t)e->n_total))) return r; }
        else { if (!e->best_c && (r = dev_alloc(&e->best_c, (size_t)e->n_total * k))) return r; }
        return NEMGPU_OK;
    }

    // RandomInteger (nem_rnd.c:40-63); with TIE_LIBC the starts' draws and the sweeps' tie draws are ONE stream
    int draw_integer(int mini, int maxi, int* out)
    {
        if (mini >= maxi) { *out = maxi; return NEMGPU_OK; }
        if (!e->libc()) { *out = rng.integer(mini, maxi); return NEMGPU_OK; }
        uint32_t v = 0;
        const int r = host_draw(e, &v);
        *out = (int)(v % (uint32_t)(maxi - mini + 1)) + mini;
        return r;
    }

    // MakeRandomPara, nem_alg.c:1381-1473, into the caller's arrays (TIE_LIBC: from where the stream stands)
    int make_random_para(float* prop, float* center, float* disp)
    {
        const int n = e->n, k = e->k, d = e->d, wf = e->wf;
        auto bit = [&](int i, int j) { return (float)((e->host_bits[(size_t)i * wf + (j >> 5)] >> (j & 31)) & 1u); };
        for (int h = 0; h < k; h++) for (int j = 0; j < d; j++) disp[(size_t)h * d + j] = dispsam[j] / k;      // :1400
        for (int h = 0; h < k; h++) prop[h] = (float)(1.0 / k);                                              // :1405
        for (int h = 0; h < k; h++) {
            int ipt = 0;
            bool again = true;
            for (int ndraw = 0; again && ndraw < 100; ndraw++) {                                             // :1419
                const int r = draw_integer(0, n - 1, &ipt);
                if (r) return r;
                again = false;
                for (int g = 0; g < h && !again; g++) {
                    bool different = false;
                    for (int j = 0; j < d && !different; j++) different = center[(size_t)g * d + j] != bit(ipt, j);
                    if (!different) again = true;
                }
            }
            for (int j = 0; j < d; j++) center[(size_t)h * d + j] = bit(ipt, j);                             // :1457
        }
        return NEMGPU_OK;
    }

    // a start's parameters into the engine's initial slots
    int upload(const float* prop, const float* center, const float* disp)
    {
        const size_t k = (size_t)e->k, kd = k * e->d;
        HIPCHK(copy_sync(e, e->prop0, prop, sizeof(float) * k, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(e, e->center0, center, sizeof(float) * kd, hipMemcpyHostToDevice));
        HIPCHK(copy_sync(e, e->disp0, disp, sizeof(float) * kd, hipMemcpyHostToDevice));
        return NEMGPU_OK;
    }

    // one start alone on the engine itself: ComputePartitionFromPara + NemAlgo + criteria, as nemgpu_run does
    int run_alone(const float* prop, const float* center, const float* disp, float crit[6])
    {
        int r;
        if ((r = upload(prop, center, disp)) || (r = iterate(e, e->cfg.it_max, true))) return r;
        if (e->iters == 0 && (r = finish_unstepped(e))) return r;
        return criteria(e, crit);
    }

    // A start that `src` (the engine or a twin of it) has run: the first that succeeds, or one with a strictly greater
    // criterion M, is the best so far -- its partition is set aside on the engine's stream
    int offer(nemgpu_engine* src, const float* crit, int start)
    {
        last_status = src->status;
        if (src->status != NEMGPU_OK) return NEMGPU_OK;
        nbsucc++;
        if (nbsucc == 1 || crit[3] > best_crit[3]) {                                                         // :1676-1697
            if (e->ncem()) HIPCHK(hipMemcpyAsync(e->best_lab, src->lab[src->cur], (size_t)e->n_total, hipMemcpyDeviceToDevice, e->stream));
            else HIPCHK(hipMemcpyAsync(e->best_c, src->cbuf[src->cur], sizeof(float) * (size_t)e->n_total * e->k, hipMemcpyDeviceToDevice, e->stream));
            for (int t = 0; t < 6; t++) best_crit[t] = crit[t];
            best = start;
            fill_result(src, &best_res);
        }
        return NEMGPU_OK;
    }

    // the best partition back in place and EstimPara on it; without a successful start, the last one's status
    int finish(nemgpu_result* res, int* best_start)
    {
        int r;
        if (nbsucc > 0) {
            if (e->ncem()) HIPCHK(hipMemcpyAsync(e->lab[e->cur], e->best_lab, (size_t)e->n_total, hipMemcpyDeviceToDevice, e->stream));
            else HIPCHK(hipMemcpyAsync(e->cbuf[e->cur], e->best_c, sizeof(float) * (size_t)e->n_total * e->k, hipMemcpyDeviceToDevice, e->stream));
            e->masks_valid = false; e->tables_fresh = false; e->density_fresh = false;
            if ((r = do_mstep(e)) || (!e->ncem() && (r = read_iter_flags(e)))) return r;                          // :1711
            e->status = NEMGPU_OK; e->emptyk = 0;
            e->iters = best_res.iters; e->converged = best_res.converged;
            if (res) { *res = best_res; res->status = NEMGPU_OK; res->tie_draws = e->draws; for (int t = 0; t < 6; t++) res->crit[t] = best_crit[t]; }
        } else if (res) {
            fill_result(e, res);
            res->status = last_status;
        }
        if (best_start) *best_start = best;
        HIPCHK(hipStreamSynchronize(e->stream));
        return NEMGPU_OK;
    }
};

// RandNemAlgo (nem_alg.c:1574-1742) with the starts in lock step.  TIE_LIBC: the starts' centre draws and the sweeps'
// tie draws are one stream, so where start s begins depends on the ties of the starts before it.  Where the ties ARE
// is what makes lock step possible: a random start gives every class the same dispersion (the whole sample's over K,
// nem_alg.c:1400) and the same proportion, so in the two initial sweeps every family that is as far from two centres
// ties exactly -- hundreds to thousands of draws per start -- while from the first M-step on the classes' parameters
// differ and a tie is an accident (profiles/r04_random_starts_draws.json: 100 starts, 0 draws behind the initial sweeps).
// So a round runs in two phases.  A: start by start, in stream order -- centres drawn, parameters up, density, the blind
// sweep and the beta sweep completed from the host (what the sequential form does for them), which leaves the stream
// where the next start's centres are drawn.  B: the EM iterations of all the round's starts in lock step, each from its
// own initial partition, on the assumption that none of them draws.  The assumption is checked: the first start whose
// iterations did draw is still right (its draws came from where they should) and everything behind it is redone from
// the position it left the stream at.
// Logged (fn), a start that drew behind its initial sweeps ends the call with kStartsNotInLockStep: nothing was handed to
// the writer, the caller runs the starts one after the other.
constexpr int kStartsNotInLockStep = -7001;
static int run_random_lockstep(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start, nemgpu_log_fn fn = nullptr, void* user = nullptr)
{
    int r;
    const int k = e->k;
    const size_t kd = (size_t)k * e->d, par = (size_t)k + 2 * kd;
    RandomStarts rs;
    if ((r = rs.begin(e, seed))) return r;
    const int group = std::min(n_starts, 64);
    // Starts per round.  TIE_LIBC: phase B bets that no start draws behind its initial sweeps.  Whether these data keep
    // the bet is not known ahead: start 0 runs ALONE, on this engine's own pipelined path (what the sequential form
    // does), and tells; if its iterations drew nothing the rest go as wide as the group allows.  After a start whose
    // iterations drew (alone, or one that voided the round behind it) the next runs alone, the width grows with the run
    // of clean starts behind it (4, 20, the rest), and after two voided rounds in a row every remaining start runs alone:
    // data whose every start draws in its iterations cost what the sequential form costs.
    const char* fa = getenv("NEM_MI355X_STARTS_FIRST_ALONE");      // (0: bet from the first start on -- tests of the losing path)
    int width = (e->libc() && !(fa && fa[0] == '0') && fn == nullptr) ? 1 : group;   // (a logged run bets from the first start on: a lost bet sends the whole call to the sequential form)
    int voided_in_a_row = 0, clean_run = 0; bool alone_for_good = false;
    if ((r = ensure_clones(e, group))) return r;
    for (nemgpu_engine* c : e->clones) { c->cfg = e->cfg; c->stream = e->stream; c->round_batch = e->round_batch; c->ff_mode = e->ff_mode; c->ff_batch = e->ff_batch; c->map_margin = e->map_margin; }

    e->rs_rounds = e->rs_lockstep = e->rs_alone = e->rs_redone = e->rs_two_waits = 0;
    // (random starts tie by the hundreds in their initial sweeps: the draw window is sized for that from the first start on,
    //  instead of growing -- and sliding away from the earlier starts' positions -- when the first heavy start is met)
    if (e->libc()) e->tie_heavy = true;
    std::vector<float> host_par;
    std::vector<int> start_pos;
    int next = 0;
    static const bool prof = getenv("NEM_MI355X_BATCH_PROF") != nullptr;
    while (next < n_starts) {
        const int M = std::min(width, n_starts - next);
        std::vector<nemgpu_engine*> E(e->clones.begin(), e->clones.begin() + M);
        host_par.assign((size_t)M * par, 0.0f);
        start_pos.assign((size_t)M, 0);
        // start j of the round
        auto make_random_para = [&](int j) -> int {
            float* prop = host_par.data() + (size_t)j * par;
            const int rr = rs.make_random_para(prop, prop + k, prop + k + kd);
            start_pos[j] = e->draws;                                 // where this start's sweeps begin to draw
            return rr;
        };
        if (e->libc() && M == 1) {
            // ---- one start alone: this engine's own run, as one after the other
            if ((r = make_random_para(0))) return r;
            float crit[6];
            e->draws_after_init = e->draws;
            if ((r = rs.run_alone(host_par.data(), host_par.data() + k, host_par.data() + k + kd, crit))) return r;
            const bool drew_late = e->draws != e->draws_after_init;  // (its iterations drew: phase B's bet would have been lost)
            if ((r = rs.offer(e, crit, next))) return r;
            next += 1; e->rs_alone++;
            clean_run = drew_late ? 0 : clean_run + 1;
            width = (alone_for_good || clean_run == 0) ? 1 : (voided_in_a_row == 0 ? group : std::min(group, 4 * clean_run));
            continue;
        }
        std::vector<LoopCursor> L((size_t)M);
        std::vector<int> after_init((size_t)M, 0);
        if (e->libc()) {
            // ---- phase A: the starts' initial partitions, one after the other in stream order
            const int pos_round_first = e->draws;
            using clk = std::chrono::steady_clock;
            const auto ta = clk::now();
            double seg[5] = {0, 0, 0, 0, 0};
            auto lap = [&](int which, clk::time_point& t) { if (prof) { const auto now = clk::now(); seg[which] += std::chrono::duration<double, std::micro>(now - t).count(); t = now; } };
            auto lend_window = [&](nemgpu_engine* c) {
                c->draw_tab = e->draw_tab; c->draw_cap = e->draw_cap; c->draw_tab0 = e->draw_tab0; c->draw_valid = true;
                c->draw_borrowed = true;                           // (a twin that outgrows the shared window builds its own)
            };
            // the starts' parameters go up from a pinned block, one slot per start: no wait for a copy
            const size_t par_bytes = par * sizeof(float);
            if (e->rs_par_host_size < (size_t)M * par_bytes) {
                HIPCHK(hipStreamSynchronize(e->stream));
                pool_put(e->device, true, e->rs_par_host, e->rs_par_host_size); e->rs_par_host = nullptr; e->rs_par_host_size = 0;
                HIPCHK(pool_get(e->device, true, (size_t)group * par_bytes, &e->rs_par_host, &e->rs_par_host_size));
            }
            for (int j = 0; j < M; j++) {
                nemgpu_engine* c = E[j];
                auto t = clk::now();
                if ((r = make_random_para(j))) return r;
                // (k_finish reads the start's parameters where the host wrote them: a pinned slot is device-visible, 12 KB
                //  cross the bus inside the launch; a copy command of its own was 2 us + two queue gaps of 4-5 us in the chain)
                float* slot = reinterpret_cast<float*>(e->rs_par_host + (size_t)j * par_bytes);
                memcpy(slot, host_par.data() + (size_t)j * par, par_bytes);
                float* const own_par[3] = {c->prop0, c->center0, c->disp0};
                c->prop0 = slot; c->center0 = slot + k; c->disp0 = slot + k + kd;
                struct ParBack { nemgpu_engine* c; float* const* own; ~ParBack() { c->prop0 = own[0]; c->center0 = own[1]; c->disp0 = own[2]; } } par_back{c, own_par};
                if ((r = ensure_draw_window(e, e->draws, draw_need(e)))) return r;
                lend_window(c);
                c->draws = e->draws; c->tie_heavy = e->tie_heavy;
                if ((r = loop_begin(c, L[j], e->cfg.it_max, true))) return r;
                lap(0, t);
                // The rounds a sweep needs are long-tailed: a start that ties at a few families is through in three or
                // four, one whose centres tie at thousands needs dozens (a draw's number depends on every tie before
                // it).  What goes out at once: what 90 % of the starts so far got by with for the blind sweep (three: a
                // round behind the fixed point still costs 4 us), 70 % for the beta sweep; a sweep that needs more gets
                // batches that double (libc_init).
                int rounds_beta = 0;
                bool redone = false;
                if ((r = libc_init(c, &rounds_beta, &redone))) return r;
                if (redone) e->rs_two_waits++;
                lap(1, t);
                if (prof && rounds_beta >= 16) fprintf(stderr, "[random starts]   start %d: beta sweep %d rounds, %d draws in its initial sweeps\n", next + j, rounds_beta, c->draws - start_pos[j]);
                HIPCHK(hipGetLastError());
                lap(4, t);
                L[j].first = false;
                c->draws_after_init = after_init[j] = c->draws;
                e->draws = c->draws; e->tie_heavy = e->tie_heavy || c->tie_heavy;
            }
            // (the parent's window may have slid or grown since a twin borrowed it: it is made to reach from the round's
            //  first start to what the last one may still draw, and every twin gets it as it is now -- a twin whose
            //  position it did not cover would build a table of its own at its first batch, generator run from the seed
            //  and 2 MB up: 0.3 ms per twin, 14.7 ms of a cold engine's first round)
            if ((r = ensure_draw_window(e, pos_round_first, (long)(e->draws - pos_round_first) + draw_need(e)))) return r;
            for (int j = 0; j < M; j++) { lend_window(E[j]); E[j]->tie_heavy = e->tie_heavy; }
            if (prof) {
                HIPCHK(hipStreamSynchronize(e->stream));
                fprintf(stderr, "[random starts] phase A, %d starts: %.0f us (centres + upload %.0f, blind sweep out %.0f + wait %.0f, beta sweep out %.0f + wait and masks %.0f), "
                                "%d of them sweep by sweep, stream at %d\n", M,
                        std::chrono::duration<double, std::micro>(clk::now() - ta).count(), seg[0], seg[1], seg[2], seg[3], seg[4], e->rs_two_waits, e->draws);
                for (int w = 0; w < 2; w++) {
                    fprintf(stderr, "[random starts]   rounds needed by the %s sweeps so far:", w ? "beta" : "blind");
                    for (int q = 1; q <= 16; q++) if (e->libc_init_hist[w][q]) fprintf(stderr, " %d%s x%d", q, q == 16 ? "+" : "", e->libc_init_hist[w][q]);
                    fprintf(stderr, "\n");
                }
            }
        } else {
            for (int j = 0; j < M; j++) if ((r = make_random_para(j))) return r;
            HIPCHK(copy_sync(e, e->clone_par0, host_par.data(), host_par.size() * sizeof(float), hipMemcpyHostToDevice));
            for (int j = 0; j < M; j++) if ((r = loop_begin(E[j], L[j], e->cfg.it_max, true))) return r;
        }
        // ---- the EM iterations in lock step (TIE_LIBC: phase B)
        std::vector<std::vector<StartLogLine>> logs((size_t)(fn ? M : 0));
        if (fn) {
            if (!e->libc()) {                                       // (the initial partitions first: a batch of no iterations)
                for (int j = 0; j < M; j++) L[j].remaining = 0;
                if ((r = iterate_many(E, L))) return r;
                for (int j = 0; j < M; j++) L[j].remaining = e->cfg.it_max;
            }
            if ((r = iterate_many_logged(E, L, host_par.data(), par, logs))) return r;
        } else if ((r = iterate_many(E, L))) return r;
        for (int j = 0; j < M; j++)
            if (E[j]->iters == 0 && (r = finish_unstepped(E[j]))) return r;
        std::vector<float> crits((size_t)M * 6);
        float (*crit)[6] = reinterpret_cast<float (*)[6]>(crits.data());
        if ((r = criteria_many(E, crit))) return r;                 // (waits for the twins' stream, which is e's)
        // the starts of this round that stand: all of them, or (TIE_LIBC) up to the first one whose iterations drew
        int valid = M;
        if (e->libc())
            for (int j = 0; j < M; j++) if (E[j]->draws != after_init[j]) { valid = j + 1; break; }
        if (fn && (valid < M || (e->libc() && E[M - 1]->draws != after_init[M - 1]))) return kStartsNotInLockStep;
        if (fn) {
            // the round's lines to the caller's writer, start by start in the reference's order
            for (int j = 0; j < M; j++) {
                emit(fn, user, next + j, LogLine{NEMGPU_LOG_START});
                for (const StartLogLine& ln : logs[(size_t)j]) emit(fn, user, next + j, ln.v);
            }
        }
        for (int j = 0; j < valid; j++)
            if ((r = rs.offer(E[j], crit[j], next + j))) return r;
        if (e->libc()) {
            e->draws = E[valid - 1]->draws;                        // the stream as start `valid - 1` left it
            e->tie_heavy = e->tie_heavy || E[valid - 1]->tie_heavy;
        } else if (valid < M) {
            set_error("internal: lock-step starts out of order"); return NEMGPU_E_FUNCARG;
        }
        next += valid; e->rs_rounds++; e->rs_lockstep += valid; e->rs_redone += M - valid;
        if (e->libc()) {
            if (valid < M || E[M - 1]->draws != after_init[M - 1]) { voided_in_a_row++; clean_run = 0; if (voided_in_a_row >= 2) alone_for_good = true; width = 1; }
            else { voided_in_a_row = 0; clean_run += M; width = group; }
        }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return rs.finish(res, best_start);
}

// fn != nullptr: the starts one after the other, one logged step per host round trip (nemgpu_iterate_logged's form)
static int run_random_impl(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start,
                           nemgpu_log_fn fn, void* user)
{
    if (!e || n_starts <= 0) return NEMGPU_E_FUNCARG;
    // (MakeRandomPara has a missing-data rule of its own, nem_alg.c:1436-1458, that this engine does not state)
    { const int mr = masked_refuse(e, "nemgpu_run_random"); if (mr) return mr; }
    if (e->lo != 0 || e->hi != e->n_total) { set_error("random starts need the whole problem on one engine"); return NEMGPU_E_FUNCARG; }
    if (!e->have_matrix || e->host_bits_words == 0) { set_error("the matrix must be set first"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    // whichever way the call is left, in either form: nothing of it is still queued on the engine's stream
    struct Drained { hipStream_t s; ~Drained() { (void)hipStreamSynchronize(s); } } drained{e->stream};
    { const int fr = flush_reset(e); if (fr) return fr; }
    int voided = 0;                                                // starts of a logged lock-step round that was thrown away whole
    {
        // the starts are independent EM runs on ONE matrix: by default they run in lock step, every launch serving all
        // of them (NEM_MI355X_BATCH_STARTS=0: one after the other on this engine)
        const char* g = getenv("NEM_MI355X_BATCH_STARTS");
        const bool lock_ok = n_starts > 1 && !(g && g[0] == '0') && !crit_test(e);
        if (!fn && lock_ok) return run_random_lockstep(e, n_starts, seed, res, best_start);
        // With the per-iteration log (fn): one iteration per lock-step step, the criteria of all starts side by side, the
        // lines handed over start by start afterwards (NEM_MI355X_BATCH_STARTS_LOGGED=0: one start after the other).  One
        // round only -- under TIE_LIBC a start that draws behind its initial sweeps sends the call to the sequential form
        // below before a line has been handed over.
        const char* gl = getenv("NEM_MI355X_BATCH_STARTS_LOGGED");
        if (fn && lock_ok && n_starts <= 64 && !(gl && gl[0] == '0')) {
            const int rr = run_random_lockstep(e, n_starts, seed, res, best_start, fn, user);
            if (rr != kStartsNotInLockStep) return rr;
            voided = n_starts;
        }
    }
    int r;
    const int k = e->k;
    const size_t kd = (size_t)k * e->d;
    RandomStarts rs;
    if ((r = rs.begin(e, seed))) return r;
    std::vector<float> prop((size_t)k), center(kd), disp(kd);
    e->rs_rounds = e->rs_lockstep = e->rs_two_waits = 0; e->rs_alone = n_starts;   // (one after the other)
    e->rs_redone = voided;                                         // (... after a round that lost its bet: the counters must tell)
    for (int s = 0; s < n_starts; s++) {
        if ((r = rs.make_random_para(prop.data(), center.data(), disp.data()))) return r;
        float crit[6];
        if (!fn) {
            if ((r = rs.run_alone(prop.data(), center.data(), disp.data(), crit))) return r;
        } else {
            // the same, step by step: a line per iteration
            if ((r = rs.upload(prop.data(), center.data(), disp.data()))) return r;
            bool have_crit = false;
            emit(fn, user, s, LogLine{NEMGPU_LOG_START});
            float cb[6], ca[6];
            std::vector<float> nb((size_t)k);
            nemgpu_result r1{};
            auto own = [&](int iter, const float* sizes) { return LogLine{NEMGPU_LOG_LINE, iter, 0, cb, ca, prop.data(), center.data(), disp.data(), sizes}; };
            if ((r = iterate_logged_impl(e, 1, true, &r1, cb, ca, prop.data(), center.data(), disp.data(), nullptr))) return r;
            emit(fn, user, s, own(0, nullptr));
            for (int iter = 1; iter <= e->cfg.it_max && !e->converged && e->status == NEMGPU_OK; iter++) {
                if ((r = iterate_logged_impl(e, 0, true, &r1, cb, ca, prop.data(), center.data(), disp.data(), nb.data()))) return r;
                if (e->status == NEMGPU_W_EMPTYCLASS) {
                    if ((r = estim_sizes_host(e, nb.data()))) return r;
                    emit(fn, user, s, LogLine::empty(iter, e->emptyk, nb.data()));
                    break;
                }
                emit(fn, user, s, own(iter, nb.data()));
                memcpy(crit, ca, sizeof crit);                     // (of the final partition, on the final densities, if the run ends here)
                have_crit = true;
            }
            if (e->status == NEMGPU_W_EMPTYCLASS) have_crit = false;
            if (e->iters == 0) {
                if ((r = finish_unstepped(e))) return r;
                have_crit = false;
            }
            if (!have_crit && (r = criteria(e, crit))) return r;
        }
        if ((r = rs.offer(e, crit, s))) return r;
    }
    return rs.finish(res, best_start);
}

int nemgpu_run_random(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start)
{
    return run_random_impl(e, n_starts, seed, res, best_start, nullptr, nullptr);
}

int nemgpu_run_random_logged(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start,
                             nemgpu_log_fn fn, void* user)
{
    if (!fn) return NEMGPU_E_FUNCARG;
    return run_random_impl(e, n_starts, seed, res, best_start, fn, user);
}

int nemgpu_glibc_random(uint32_t seed, int count, int32_t* out)
{
    if (!out || count < 0) return NEMGPU_E_FUNCARG;
    nemk::GlibcRandom rng(seed);
    for (int i = 0; i < count; i++) out[i] = (int32_t)rng.next();
    return NEMGPU_OK;
}

int nemgpu_density(nemgpu_engine* e)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = do_tables(e))) return r;
    if ((r = do_density(e))) return r;
    HIPCHK(hipStreamSynchronize(e->stream));
    return NEMGPU_OK;
}

int nemgpu_sweep(nemgpu_engine* e, float beta, int* rounds)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    if ((r = do_sweep(e, beta, rounds))) return r;
    e->cur = (e->cur + 1) % 3;
    e->masks_valid = false;
    return NEMGPU_OK;
}

int nemgpu_mstep(nemgpu_engine* e, int* emptyk)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    if ((r = do_mstep(e))) return r;
    if ((r = read_iter_flags(e))) return r;
    if (emptyk) *emptyk = e->h_iter()[FLAG_EMPTYK];
    return e->h_iter()[FLAG_EMPTYK] ? NEMGPU_W_EMPTYCLASS : NEMGPU_OK;
}

int nemgpu_criteria(nemgpu_engine* e, float crit6[6])
{
    if (!e || !crit6) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    return criteria(e, crit6);
}

// ---- multi-GPU (sharded) step pieces ----------------------------------------------------------
// Same kernels; the host driver (pangenomenem_amd/distributed.py) owns the all-gathered label arrays
// and the statistics buffer and runs the collectives between these calls.  Everything is
// asynchronous on the engine's stream; between nemgpu_shard_begin and nemgpu_shard_end the loop
// control lives on the device (k_ctrl), exactly like the single-GPU pipelined loop.
int nemgpu_stats_words(const nemgpu_engine* e) { return e ? e->k + e->k * e->d : 0; }

int nemgpu_shard_layout(nemgpu_engine* e, int world, int rank, int blk, int stride, int n_true)
{
    if (!e || world <= 0 || rank < 0 || rank >= world || blk <= 0 || stride < blk + 1 || n_true <= 0) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_layout"); if (mr) return mr; }
    if (e->lo != rank * stride || e->n > blk || e->n_total != world * stride) {
        set_error("shard layout does not match the engine's slot range");
        return NEMGPU_E_ARG;
    }
    if (stride % 4 != 0) { set_error("shard layout: stride must be a multiple of 4 bytes"); return NEMGPU_E_ARG; }
    e->sh_world = world; e->sh_rank = rank; e->sh_blk = blk; e->sh_stride = stride; e->n_true = n_true;
    return NEMGPU_OK;
}

namespace {
void shard_sweep_args(nemgpu_engine* e, SweepArgs& a, float beta, int sweep_id)
{
    sweep_args(e, a, beta, sweep_id >= 0 ? (uint32_t)sweep_id : 0u, sweep_id < 0);   // -1: the device keeps count (pipelined loop)
    a.stop = e->stop_ptr;
    a.n_ranks = e->sh_world; a.slot_stride = e->sh_stride; a.slot_pad = e->sh_stride - e->sh_blk;
    a.fold_ticket = e->sweep_next + 32;
    if (e->libc()) { sweep_draw_args(e, a, e->stop_ptr == nullptr); a.rank_index = e->sh_rank; }
}
uint8_t* own_flag_byte(nemgpu_engine* e, uint8_t* labels) { return labels + (size_t)e->sh_rank * e->sh_stride + e->sh_blk; }
int shard_buf(const nemgpu_engine* e, const uint8_t* p) { for (int b = 0; b < 3; b++) if (e->shard_lab[b] == p) return b; return -1; }
// TIE_LIBC: the draw counts that go with a round's guess and output buffers -- per block (the engine's, by buffer) and
// per rank (in the buffers' block tails, all-gathered with the labels)
int shard_tie_args(nemgpu_engine* e, SweepArgs& a, const uint8_t* guess, uint8_t* out)
{
    if (!e->libc()) return NEMGPU_OK;
    const int g = shard_buf(e, guess), o = shard_buf(e, out);
    if (g < 0 || o < 0) { set_error("TIE_LIBC in the sharded path: a label array that nemgpu_shard_set_labels was not told about"); return NEMGPU_E_FUNCARG; }
    a.tie_cnt_guess = e->tie_cnt[g]; a.tie_cnt_out = e->tie_cnt[o];
    a.rank_tot_in = guess + e->sh_tot_off();
    a.rank_tot_out = out + (size_t)e->sh_rank * e->sh_stride + e->sh_tot_off();
    return NEMGPU_OK;
}
void shard_round1_args(nemgpu_engine* e, SweepArgs& a, float beta, int sweep_id, const uint8_t* labels_old_dev,
                       const uint8_t* labels_guess_dev, uint8_t* labels_out_dev)
{
    shard_sweep_args(e, a, beta, sweep_id);
    a.lab_old = labels_old_dev; a.lab_guess = labels_guess_dev; a.lab_out = labels_out_dev;
    a.flags = e->round_flags(1);
    a.flags_in = labels_guess_dev + e->sh_blk;                     // rank 0's flag byte; stride = slot_stride
    a.publish_byte = own_flag_byte(e, labels_out_dev); a.publish_ticket = e->sweep_next + 32;
    // the verifying round also says whether one of THIS rank's labels moved in the sweep (its guess against the old
    // partition): the byte behind its flag byte, gathered with it -- the convergence test then needs no pass over the
    // whole label array on every rank
    a.post_on = 1; a.post_from_guess = 1; a.post_skip_guess = 1; a.post_moved = 1; a.post_no_masks = 1;
    a.post_nw64 = e->nw64; a.post_mask = e->mask; a.post_flags = e->iter_flags();
}
}  // namespace

static int shard_check(nemgpu_engine* e)
{
    if (!e) return NEMGPU_E_FUNCARG;
    if (!e->ncem()) { set_error("the sharded path is NCEM-only (SURVEY.md 8e)"); return NEMGPU_E_FUNCARG; }
    if (e->sh_stride == 0) { set_error("nemgpu_shard_layout must be called first"); return NEMGPU_E_FUNCARG; }
    if (e->libc() && (e->shard_lab[0] == nullptr || e->sh_tot_off() + 4 > e->sh_stride)) {
        set_error("TIE_LIBC in the sharded path: nemgpu_shard_set_labels first (and a block tail of at least 12 bytes)");
        return NEMGPU_E_FUNCARG;
    }
    if (crit_test(e)) {
        // (the criterion is an i-ordered float sum over ALL families: no sharded reduction reproduces it, and the loop
        //  control of this path only knows the clas test -- a run configured with crit would never converge)
        set_error("the family-sharded path implements the convergence tests none and clas only");
        return NEMGPU_E_FUNCARG;
    }
    return NEMGPU_OK;
}

int nemgpu_shard_begin(nemgpu_engine* e)
{
    { const int cr = shard_check(e); if (cr) return cr; }
    { const int mr = masked_refuse(e, "nemgpu_shard_begin"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    HIPCHK(hipMemsetAsync(e->ctrl(), 0, C_WORDS * sizeof(int), e->stream));
    if (e->libc()) {                                               // the stream's window and position, as every rank has them
        int r;
        if ((r = ensure_draw_window(e, e->draws, draw_need(e)))) return r;
        if ((r = publish_draw_ctl(e))) return r;
    }
    e->stop_ptr = e->ctrl() + C_STOP;
    return NEMGPU_OK;
}

// nemgpu_shard_begin for a batch that starts a run over: the reset (initial parameters back in place), the clearing of
// the loop control and the density tables in ONE launch (the head of the single engine's restart batches, enqueue_init)
// instead of a device-to-device copy, three fills and a tables launch
int nemgpu_shard_begin_restart(nemgpu_engine* e)
{
    { const int cr = shard_check(e); if (cr) return cr; }
    { const int mr = masked_refuse(e, "nemgpu_shard_begin_restart"); if (mr) return mr; }
    if (!e->have_matrix || !e->have_params) { set_error("matrix and parameters must be set first"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    int r;
    if ((r = reset_state(e, true))) return r;                      // host half; the device half is the launch below
    e->reset_pending = false;
    if ((r = clear_fault(e))) return r;
    FinishArgs t = finish_args(e, 0, nullptr);
    restart_head(e, t);
    finish_launch(e, t);
    HIPCHK(hipGetLastError());
    if (e->libc()) {                                               // (srandom(seed): the stream starts over)
        if ((r = ensure_draw_window(e, e->draws, draw_need(e)))) return r;
        if ((r = publish_draw_ctl(e))) return r;
    }
    e->stop_ptr = e->ctrl() + C_STOP;
    return NEMGPU_OK;
}

// this rank's partial counts of the labels relaxation round 0 just produced (its class masks were built by that
// launch) -> stats_dev, normally the statistics tail of this rank's block in the label array gathered next
int nemgpu_shard_counts(nemgpu_engine* e, int32_t* stats_dev)
{
    if (!e || !stats_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_counts"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    launch_mstep_counts(counts_args(e, stats_dev, nullptr), e->stream);
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// local class masks of the given labels + popcounts -> stats_dev (the explicit form of the above)
int nemgpu_shard_mstep_partial(nemgpu_engine* e, const uint8_t* labels_cur_dev, int32_t* stats_dev)
{
    if (!e || !labels_cur_dev || !stats_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_mstep_partial"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    launch_labels_post(labels_post_args(e, labels_cur_dev, nullptr, nullptr), e->stream);
    launch_mstep_counts(counts_args(e, stats_dev, nullptr), e->stream);
    HIPCHK(hipGetLastError());
    e->masks_valid = false;
    return NEMGPU_OK;
}

// [parameter update from the summed statistics] + density + relaxation round 0 (guess = old) + this rank's
// changed byte behind its label block (then: all-gather of labels_out)
int nemgpu_shard_estep_round0(nemgpu_engine* e, const int32_t* stats_dev, float beta, int sweep_id,
                              const uint8_t* labels_old_dev, uint8_t* labels_out_dev)
{
    if (!e || !labels_old_dev || !labels_out_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_estep_round0"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    const bool fused = stats_dev != nullptr && e->fused_update();
    if (fused) {
        // parameter update (per block, from the summed counts) + density in one launch
        FinishArgs t = finish_args(e, 1, stats_dev);
        shard_stats(e, t);
        density_launch(e, t);
        HIPCHK(hipGetLastError());
    } else {
        if (stats_dev != nullptr) {
            FinishArgs t = finish_args(e, 1, stats_dev);
            shard_stats(e, t);
            finish_launch(e, t);
            HIPCHK(hipGetLastError());
        } else if ((r = do_tables(e))) return r;
        if (e->density_fresh) { if (!e->flags_clean && (r = clear_sweep_flags(e))) return r; }   // same parameters as the last E1: keep pkfki
        else if ((r = do_density(e))) return r;                    // also clears MOVED + the round flag window
    }
    // the blind sweep of a start (beta = 0, sweep 0, the parameters as given): a flag slot of its own and no "moved"
    // flag, so that the sweep behind it -- same densities -- needs no clearing of the flags in between
    const bool blind = stats_dev == nullptr && sweep_id == 0 && beta == 0.0f;
    SweepArgs a;
    shard_sweep_args(e, a, beta, sweep_id);
    a.lab_old = labels_old_dev; a.lab_guess = labels_old_dev; a.lab_out = labels_out_dev;
    a.flags = e->round_flags(blind ? kRoundCap - 1 : 0);
    // the same launch builds the class masks of its output (for nemgpu_shard_counts) and publishes the flag byte
    a.post_on = 1; a.post_from_guess = 0; a.post_moved = blind ? 0 : 1; a.post_nw64 = e->nw64; a.post_mask = e->mask;
    a.post_flags = e->iter_flags();                                // ("moved" byte: final when this is the sweep's only round)
    a.publish_byte = own_flag_byte(e, labels_out_dev); a.publish_ticket = e->sweep_next + 32;
    if ((r = shard_tie_args(e, a, labels_old_dev, labels_out_dev))) return r;
    launch_sweep(a, true, e->stream);
    HIPCHK(hipGetLastError());
    e->flags_clean = blind && e->flags_clean;
    return NEMGPU_OK;
}

// relaxation round 1 (guess = round 0's all-gathered output); returns at once on every rank when no rank
// changed a label in round 0 (then: all-gather of labels_out, whose content is unused in that case)
int nemgpu_shard_estep_round1(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                              const uint8_t* labels_guess_dev, uint8_t* labels_out_dev)
{
    if (!e || !labels_old_dev || !labels_guess_dev || !labels_out_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_estep_round1"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    SweepArgs a;
    shard_round1_args(e, a, beta, sweep_id, labels_old_dev, labels_guess_dev, labels_out_dev);
    { const int tr = shard_tie_args(e, a, labels_guess_dev, labels_out_dev); if (tr) return tr; }
    launch_sweep(a, true, e->stream);
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// relaxation round 1 and this rank's partial counts of round 0's labels (nemgpu_shard_counts) in ONE launch where the
// shape has such a kernel (k_sweep_counts), else one after the other: the two do not depend on each other
int nemgpu_shard_estep_round1_counts(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                                     const uint8_t* labels_guess_dev, uint8_t* labels_out_dev, int32_t* stats_dev)
{
    if (!e || !labels_old_dev || !labels_guess_dev || !labels_out_dev || !stats_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_estep_round1_counts"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    SweepArgs a;
    shard_round1_args(e, a, beta, sweep_id, labels_old_dev, labels_guess_dev, labels_out_dev);
    { const int tr = shard_tie_args(e, a, labels_guess_dev, labels_out_dev); if (tr) return tr; }
    static const bool merge = !(getenv("NEM_DIST_MERGE") && getenv("NEM_DIST_MERGE")[0] == '0');
    const CountsArgs ca = counts_args(e, stats_dev, nullptr);
    if (!merge || !launch_sweep_counts(a, ca, e->stream)) {
        launch_sweep(a, true, e->stream);
        launch_mstep_counts(ca, e->stream);
    }
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// ---- fuzzy NEM on several GPUs (SURVEY.md 8e's exact alternative) ----------------------------------------------
// The fuzzy M-step's sums are i-ordered float accumulators (nem_mod.c:1303-1313, 1677-1686, 1448-1458): no reduction
// over family shards reproduces them.  So the E-step is sharded over FAMILIES (this engine: rows [lo, hi), the
// memberships of every family in caller-owned arrays float[n_total][K] that the caller all-gathers between relaxation
// rounds) and the M-step over ORGANISMS (a second engine per rank that holds ALL families x its slice of the
// organisms: every chain is summed on one device over the whole, gathered membership matrix, in family order).
// Host-driven, one step per call; pangenomenem_amd/distributed.py:ShardedFuzzyNem drives it.

// families of the whole problem when n_total carries padding (proportions divide by it, nem_mod.c:456-465)
int nemgpu_shard_fuzzy_layout(nemgpu_engine* e, int n_true)
{
    if (!e || n_true <= 0 || n_true > e->n_total) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_fuzzy_layout"); if (mr) return mr; }
    if (e->ncem()) { set_error("nemgpu_shard_fuzzy_*: the engine must be configured with algo = nem"); return NEMGPU_E_ARG; }
    e->n_true = n_true;
    return NEMGPU_OK;
}

// one relaxation round of the E-step sweep over this engine's families: c_out[lo..hi) from the guess c_guess (round 0:
// the old partition) -- the other families' rows of c_out are left alone (the caller's all-gather fills them).
// changed / nzero / firstzero (host): the round's flags (firstzero: global index of the first family whose densities
// all vanished, -1 if none).  Synchronises.
int nemgpu_shard_fuzzy_round(nemgpu_engine* e, float beta, int sweep_id, int round, const float* c_old_dev, const float* c_guess_dev,
                             float* c_out_dev, int* changed, int* nzero, int* firstzero)
{
    if (!e || !c_old_dev || !c_guess_dev || !c_out_dev || round < 0) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_fuzzy_round"); if (mr) return mr; }
    if (e->ncem()) { set_error("nemgpu_shard_fuzzy_round: the engine must be configured with algo = nem"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    const int slot = round % kRoundCap;
    HIPCHK(hipMemsetAsync(e->round_flags(slot), 0, FLAG_ROUND_STRIDE * sizeof(int), e->stream));
    SweepArgs a;
    sweep_args(e, a, beta, (uint32_t)sweep_id);                    // (host-driven: no stop word)
    a.c_old = c_old_dev; a.c_guess = c_guess_dev; a.c_out = c_out_dev;
    a.flags = e->round_flags(slot);
    a.fold_ticket = e->sweep_next + 32;
    launch_sweep(a, false, e->stream);
    HIPCHK(hipGetLastError());
    e->flags_clean = false;
    HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if ((r = check_fault(e))) return r;
    const int* f = e->h_round(slot);
    if (changed) *changed = f[FLAG_CHANGED];
    if (nzero) *nzero = f[FLAG_NZERO];
    if (firstzero) *firstzero = f[FLAG_NZERO] > 0 ? e->n_total - f[FLAG_FIRSTZERO] : -1;
    return NEMGPU_OK;
}

// EstimSizes / EstimLaplaceCenters / EstimLaplaceIner for THIS engine's organisms on the memberships of all its
// families (c_dev: float[n][K], the whole gathered matrix for an organism-slice engine): class sizes, centres and
// inertia to device arrays of the caller's (K, K * d, K * d floats).  Dispersions are not derived here: InerToDisp
// needs every organism (nemgpu_shard_fuzzy_finish).
int nemgpu_shard_fuzzy_mstep_cols(nemgpu_engine* e, const float* c_dev, float* nbobs_out_dev, float* center_out_dev, float* iner_out_dev)
{
    if (!e || !c_dev || !nbobs_out_dev || !center_out_dev || !iner_out_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_fuzzy_mstep_cols"); if (mr) return mr; }
    if (e->ncem()) { set_error("nemgpu_shard_fuzzy_mstep_cols: the engine must be configured with algo = nem"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    launch_mstep_fuzzy(fuzzy_args(e, c_dev, nullptr), e->stream);
    HIPCHK(hipGetLastError());
    const size_t kd = (size_t)e->k * e->d;
    HIPCHK(hipMemcpyAsync(nbobs_out_dev, e->nbobs_k, sizeof(float) * e->k, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(center_out_dev, e->center, sizeof(float) * kd, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(iner_out_dev, e->iner, sizeof(float) * kd, hipMemcpyDeviceToDevice, e->stream));
    e->tables_fresh = false; e->density_fresh = false;
    return read_iter_flags(e);                                     // (waits; a stalled hand-over of the M-step is an error)
}

// the rest of EstimPara on the gathered statistics of ALL organisms (device arrays: K, K * D, K * D floats): InerToDisp*
// (nem_mod.c:922-1174), proportions, the empty-class test, the density tables -- then E1 on this engine's families.
// emptyk (host): 0, or the class (1..K) EstimLaplaceCenters found empty (nothing else was updated for it).
int nemgpu_shard_fuzzy_finish(nemgpu_engine* e, const float* nbobs_dev, const float* center_dev, const float* iner_dev, int* emptyk)
{
    if (!e || !nbobs_dev || !center_dev || !iner_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_fuzzy_finish"); if (mr) return mr; }
    if (e->ncem()) { set_error("nemgpu_shard_fuzzy_finish: the engine must be configured with algo = nem"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    const size_t kd = (size_t)e->k * e->d;
    HIPCHK(hipMemcpyAsync(e->nbobs_k, nbobs_dev, sizeof(float) * e->k, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->center, center_dev, sizeof(float) * kd, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->iner, iner_dev, sizeof(float) * kd, hipMemcpyDeviceToDevice, e->stream));
    finish_launch(e, finish_args(e, 2, nullptr));
    HIPCHK(hipGetLastError());
    if ((r = read_iter_flags(e))) return r;
    const int ek = e->h_iter()[FLAG_EMPTYK];
    if (emptyk) *emptyk = ek;
    if (ek != 0) return NEMGPU_W_EMPTYCLASS;                       // nem_alg.c:1831-1838: the E-step does not run
    return do_density(e);
}

// HasConverged's CVTEST_CLAS (nem_alg.c:2075-2089) over this engine's families: moved (host) = some membership moved
// by the threshold or more
int nemgpu_shard_fuzzy_moved(nemgpu_engine* e, const float* c_new_dev, const float* c_old_dev, int* moved)
{
    if (!e || !c_new_dev || !c_old_dev || !moved) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_fuzzy_moved"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemsetAsync(e->iter_flags() + FLAG_MOVED, 0, sizeof(int), e->stream));
    launch_conv_fuzzy(conv_fuzzy_args(e, c_new_dev, c_old_dev, nullptr, nullptr), e->stream);
    HIPCHK(hipGetLastError());
    int r;
    if ((r = read_iter_flags(e))) return r;
    *moved = e->h_iter()[FLAG_MOVED];
    return NEMGPU_OK;
}

// convergence test over the whole label array + the device-side loop tests (k_ctrl logic)
int nemgpu_shard_finish_iteration(nemgpu_engine* e, float beta, int is_init, const uint8_t* labels_old_dev,
                                  const uint8_t* labels_q_dev, const uint8_t* labels_r_dev)
{
    if (!e || !labels_old_dev || !labels_q_dev || !labels_r_dev) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_finish_iteration"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    CtrlArgs ca = ctrl_args(e, 2, beta);                           // (the path is NCEM-only, shard_check)
    ca.q_flags = labels_q_dev + e->sh_blk; ca.r_flags = labels_r_dev + e->sh_blk;
    ca.n_ranks = e->sh_world; ca.flag_stride = e->sh_stride; ca.is_init = is_init;
    if (is_init) ca.blind = e->round_flags(kRoundCap - 1);         // (the blind sweep's zero-density tally)
    // every rank's "one of my labels moved" byte came with the gather of the sweep's last round: round 1's, or -- no
    // neighbours to verify against (beta = 0) -- round 0's
    // (the driver runs the verifying round whenever beta != 0, graph or no graph: here the rule is its own)
    const bool two_rounds = beta != 0.0f || e->libc();             // (the reference's tie stream couples the sites of a sweep without neighbours too)
    ca.use_nei = two_rounds ? 1 : 0;
    ca.moved_bytes = is_init ? 0 : (two_rounds ? 1 : 2);
    if (e->libc()) ca.q_tot = labels_q_dev + e->sh_tot_off();
    launch_ctrl(ca, e->stream);
    HIPCHK(hipGetLastError());
    return NEMGPU_OK;
}

// one host-checked relaxation round (fallback when a sweep needs more than two rounds): returns whether
// THIS rank changed a label; the caller all-gathers labels_out and max-reduces the flag
int nemgpu_shard_round_sync(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                            const uint8_t* labels_guess_dev, uint8_t* labels_out_dev, int* changed)
{
    if (!e || !labels_old_dev || !labels_guess_dev || !labels_out_dev || !changed) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_round_sync"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    const int* saved = e->stop_ptr;
    e->stop_ptr = nullptr;
    SweepArgs a;
    shard_sweep_args(e, a, beta, sweep_id);
    e->stop_ptr = saved;
    a.lab_old = labels_old_dev; a.lab_guess = labels_guess_dev; a.lab_out = labels_out_dev;
    a.flags = e->round_flags(2);
    if (e->libc()) {
        // (the window of the stream at the host's position; the rank's draws of this round go to its block's tail:
        //  the last block of the round writes them with the flag byte)
        int r;
        if ((r = ensure_draw_window(e, e->draws, draw_need(e)))) return r;
        sweep_draw_args(e, a, true);
        a.publish_byte = own_flag_byte(e, labels_out_dev); a.publish_ticket = e->sweep_next + 32;
        if ((r = shard_tie_args(e, a, labels_guess_dev, labels_out_dev))) return r;
    }
    HIPCHK(hipMemsetAsync(e->round_flags(2), 0, FLAG_ROUND_STRIDE * sizeof(int), e->stream));
    launch_sweep(a, true, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *changed = e->h_round(2)[FLAG_CHANGED] != 0;
    return NEMGPU_OK;
}

// TIE_LIBC in the sharded path, host side.  nemgpu_shard_set_labels: the driver's three all-gathered label arrays (the
// engine keeps each one's per-block draw counts).  nemgpu_shard_round_draws: after nemgpu_shard_round_sync -- this
// rank's draws in that round, and whether one of them fell outside the draw table (then the round is void on every
// rank: nemgpu_shard_grow_draws on all of them and the round again).  nemgpu_shard_book_draws: a sweep the host
// completed drew n numbers (the sum of the ranks' draws of its final round): the stream moves on.
int nemgpu_shard_set_labels(nemgpu_engine* e, const uint8_t* lab0, const uint8_t* lab1, const uint8_t* lab2)
{
    if (!e || !lab0 || !lab1 || !lab2) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_set_labels"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    e->shard_lab[0] = lab0; e->shard_lab[1] = lab1; e->shard_lab[2] = lab2;
    alloc_for(e);
    for (int b = 0; b < 3; b++)
        if (!e->tie_cnt[b]) { const int r = dev_alloc(&e->tie_cnt[b], (size_t)e->n / 256 + 2); if (r) return r; }
    drop_graphs(e);
    return NEMGPU_OK;
}
int nemgpu_shard_round_draws(nemgpu_engine* e, int* draws, int* table_short)
{
    if (!e) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_round_draws"); if (mr) return mr; }
    const int v = e->h_round(2)[FLAG_NTIES];
    if (draws) *draws = v & ((1 << 30) - 1);
    if (table_short) *table_short = (v >> 30) & 1;
    return NEMGPU_OK;
}
int nemgpu_shard_grow_draws(nemgpu_engine* e) { if (!e) return NEMGPU_E_FUNCARG; e->tie_heavy = true; return NEMGPU_OK; }
int nemgpu_shard_book_draws(nemgpu_engine* e, int n) { if (!e || n < 0) return NEMGPU_E_FUNCARG; e->draws += n; return NEMGPU_OK; }

// end of a batch: read the loop-control block back (one sync).  res->iters etc. are the batch's increments.
int nemgpu_shard_end_enqueue(nemgpu_engine* e)
{
    // last call of a batch's enqueue phase (may be inside a graph capture): copy the control block to the host
    if (!e) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_end_enqueue"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    e->stop_ptr = nullptr;
    HIPCHK(hipMemcpyAsync(e->flags_host, e->flags_dev, e->flag_words() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    return NEMGPU_OK;
}

int nemgpu_shard_end(nemgpu_engine* e, nemgpu_result* res, int* commits, int* need_rounds)
{
    // wait for the batch and report; call after nemgpu_shard_end_enqueue (or after replaying a captured batch)
    if (!e) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_end"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    e->stop_ptr = nullptr;
    HIPCHK(hipStreamSynchronize(e->stream));
    const int* c = e->h_ctrl();
    if (res) {
        res->status = c[C_STATUS]; res->iters = c[C_ITERS]; res->converged = c[C_CONVERGED]; res->emptyk = c[C_EMPTYK];
        res->zero_density_sites = c[C_NZERO];
        res->first_zero_density_site = c[C_NZERO] > 0 ? e->n_total - c[C_FIRSTZERO] : -1;
        res->sweep_rounds = c[C_SWEEP_ROUNDS];
    }
    if (commits) *commits = c[C_COMMITS];
    if (need_rounds) *need_rounds = c[C_NEED_ROUNDS];
    if (e->libc()) {
        e->draws += c[C_DRAWS];                                    // (the committed sweeps' draws: where the next one starts)
        for (int q = 0; q < 2; q++) if (e->h_round(q)[FLAG_NTIES] & (1 << 30)) e->tie_heavy = true;
    }
    e->flags_clean = false;
    return NEMGPU_OK;
}

// ---- RCCL called directly (no Python between the launches of a batch) ------------------------------------------
// The sharded EM needs one collective, an in-place all-gather of label blocks.  Issued through torch.distributed
// every call costs tens of microseconds of host time, more than the iteration's kernels; issued from here the whole
// batch -- kernels and all-gathers -- is enqueued by one C call.  librccl.so (the one PyTorch ships and has already
// loaded) is bound at run time; torch.distributed stays the bootstrap (it carries the ncclUniqueId) and the fallback.
struct nccl_uid_t { char internal[128]; };                                     // ncclUniqueId, rccl.h:40-43
namespace {
struct RcclApi {
    void* handle = nullptr;
    int (*get_unique_id)(nccl_uid_t*) = nullptr;                               // ncclGetUniqueId
    int (*comm_init_rank)(void**, int, nccl_uid_t, int) = nullptr;             // ncclCommInitRank(comm*, nranks, id, rank)
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    int (*comm_count)(const void*, int*) = nullptr;                            // ncclCommCount
    int (*comm_abort)(void*) = nullptr;                                        // ncclCommAbort
    const char* (*error_string)(int) = nullptr;
};
RcclApi g_rccl;
int rccl_fail(const char* what, int code)
{
    set_error(std::string(what) + " failed: " + (g_rccl.error_string ? g_rccl.error_string(code) : "?"));
    return NEMGPU_E_DEVICE;
}
}  // namespace

int nemgpu_rccl_open(const char* librccl_path)
{
    if (g_rccl.handle) return NEMGPU_OK;
    void* h = dlopen(librccl_path && librccl_path[0] ? librccl_path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { set_error(std::string("dlopen(librccl) failed: ") + dlerror()); return NEMGPU_E_DEVICE; }
    g_rccl.get_unique_id = (int (*)(nccl_uid_t*))dlsym(h, "ncclGetUniqueId");
    g_rccl.comm_init_rank = (int (*)(void**, int, nccl_uid_t, int))dlsym(h, "ncclCommInitRank");
    g_rccl.all_gather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.comm_destroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    g_rccl.error_string = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    g_rccl.comm_count = (int (*)(const void*, int*))dlsym(h, "ncclCommCount");
    g_rccl.comm_abort = (int (*)(void*))dlsym(h, "ncclCommAbort");
    if (!g_rccl.get_unique_id || !g_rccl.comm_init_rank || !g_rccl.all_gather || !g_rccl.comm_destroy) {
        set_error("librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy");
        dlclose(h);
        return NEMGPU_E_DEVICE;
    }
    g_rccl.handle = h;
    return NEMGPU_OK;
}

int nemgpu_rccl_unique_id(uint8_t id128[128])
{
    if (!id128) return NEMGPU_E_FUNCARG;
    if (!g_rccl.handle) { set_error("nemgpu_rccl_open first"); return NEMGPU_E_FUNCARG; }
    nccl_uid_t id;
    int rc = g_rccl.get_unique_id(&id);
    if (rc != 0) return rccl_fail("ncclGetUniqueId", rc);
    memcpy(id128, id.internal, 128);
    return NEMGPU_OK;
}

void rccl_release(nemgpu_engine* e)
{
    if (e->rccl_comm && g_rccl.comm_destroy) (void)g_rccl.comm_destroy(e->rccl_comm);
    e->rccl_comm = nullptr;
}

// collective: every rank of the job calls it with the id rank 0 produced
int nemgpu_rccl_attach(nemgpu_engine* e, const uint8_t id128[128], int world, int rank)
{
    if (!e || !id128 || world <= 0 || rank < 0 || rank >= world) return NEMGPU_E_FUNCARG;
    if (!g_rccl.handle) { set_error("nemgpu_rccl_open first"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    nccl_uid_t id;
    memcpy(id.internal, id128, 128);
    void* comm = nullptr;
    int rc = g_rccl.comm_init_rank(&comm, world, id, rank);
    if (rc != 0) return rccl_fail("ncclCommInitRank", rc);
    e->rccl_comm = comm;
    return NEMGPU_OK;
}

// ranks of the engine's native communicator as RCCL itself reports them (ncclCommCount); 0 when none is attached
int nemgpu_rccl_ranks(const nemgpu_engine* e)
{
    if (!e || !e->rccl_comm || !g_rccl.comm_count) return 0;
    int n = 0;
    if (g_rccl.comm_count(e->rccl_comm, &n) != 0) return 0;
    return n;
}

namespace {
int rccl_allgather_blocks(nemgpu_engine* e, uint8_t* buf)
{
    if (e->sh_world == 1) return NEMGPU_OK;                        // (a rank alone holds every block already)
    const size_t stride = (size_t)e->sh_stride;
    int rc = g_rccl.all_gather(buf + (size_t)e->sh_rank * stride, buf, stride, /*ncclUint8*/ 1, e->rccl_comm, e->stream);
    if (rc != 0) return rccl_fail("ncclAllGather", rc);
    return NEMGPU_OK;
}
}  // namespace

// One in-place all-gather of `stride`-byte blocks through the engine's own communicator, waited for with a deadline:
// the caller (every rank, collectively) compares the result with the same gather through torch.distributed before
// trusting the native path with the EM.  On a timeout the communicator is aborted and detached (the engine then has
// no native path) and NEMGPU_E_DEVICE is returned.
int nemgpu_rccl_selftest(nemgpu_engine* e, uint8_t* buf_dev, int stride, int timeout_ms)
{
    if (!e || !buf_dev || stride <= 0) return NEMGPU_E_FUNCARG;
    if (!e->rccl_comm) { set_error("nemgpu_rccl_attach first"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    int rc = g_rccl.all_gather(buf_dev + (size_t)e->sh_rank * stride, buf_dev, (size_t)stride, /*ncclUint8*/ 1,
                               e->rccl_comm, e->stream);
    if (rc != 0) return rccl_fail("ncclAllGather (self-test)", rc);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(e->stream);
        if (q == hipSuccess) return NEMGPU_OK;
        if (q != hipErrorNotReady) { set_error(std::string("self-test: ") + hipGetErrorString(q)); return NEMGPU_E_DEVICE; }
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > timeout_ms) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (g_rccl.comm_abort) (void)g_rccl.comm_abort(e->rccl_comm);
    e->rccl_comm = nullptr;
    set_error("native RCCL self-test timed out: communicator aborted");
    return NEMGPU_E_DEVICE;
}

// One whole batch of the sharded EM -- [the two initial sweeps +] n_iters iterations, all-gathers included --
// enqueued on the engine's stream without returning to the caller in between (what ShardedNem._enqueue_batch
// does through torch.distributed).  lab[3]: the all-gathered label arrays; stats_off: byte offset of a rank's
// statistics inside its block; base: buffer of the current partition (2 after an init).
static int shard_batch_body(nemgpu_engine* e, int with_init, int n_iters, int base, float beta, int want_stats,
                            uint8_t* lab0, uint8_t* lab1, uint8_t* lab2, int stats_off)
{
    uint8_t* L[3] = {lab0, lab1, lab2};
    const bool use_nei = beta != 0.0f || e->libc();                // two rounds: neighbours to verify against, or the shared draw stream
    auto own_stats = [&](uint8_t* buf) { return (int32_t*)(buf + (size_t)e->sh_rank * e->sh_stride + stats_off); };
    auto all_stats = [&](uint8_t* buf) { return (const int32_t*)(buf + stats_off); };
    int r;
#define NEM_TRY(call) do { if ((r = (call)) != NEMGPU_OK) return r; } while (0)
    NEM_TRY(with_init ? nemgpu_shard_begin_restart(e) : nemgpu_shard_begin(e));
    if (with_init) {
        NEM_TRY(nemgpu_shard_estep_round0(e, nullptr, 0.0f, 0, L[0], L[1]));       // blind sweep
        NEM_TRY(rccl_allgather_blocks(e, L[1]));
        NEM_TRY(nemgpu_shard_estep_round0(e, nullptr, beta, 1, L[1], L[2]));
        if (want_stats && !use_nei) NEM_TRY(nemgpu_shard_counts(e, own_stats(L[2])));
        NEM_TRY(rccl_allgather_blocks(e, L[2]));
        if (use_nei) {
            if (want_stats) NEM_TRY(nemgpu_shard_estep_round1_counts(e, beta, 1, L[1], L[2], L[0], own_stats(L[0])));
            else NEM_TRY(nemgpu_shard_estep_round1(e, beta, 1, L[1], L[2], L[0]));
            NEM_TRY(rccl_allgather_blocks(e, L[0]));
        }
        NEM_TRY(nemgpu_shard_finish_iteration(e, beta, 1, L[1], L[2], L[0]));
    }
    for (int j = 0; j < n_iters; j++) {
        const int P = (base + j) % 3, Q = (P + 1) % 3, R = (P + 2) % 3;
        const int S = use_nei ? Q : P;                                             // where P's statistics were gathered
        NEM_TRY(nemgpu_shard_estep_round0(e, want_stats ? all_stats(L[S]) : nullptr, beta, -1, L[P], L[Q]));
        if (want_stats && !use_nei) NEM_TRY(nemgpu_shard_counts(e, own_stats(L[Q])));
        NEM_TRY(rccl_allgather_blocks(e, L[Q]));
        if (use_nei) {
            if (want_stats) NEM_TRY(nemgpu_shard_estep_round1_counts(e, beta, -1, L[P], L[Q], L[R], own_stats(L[R])));
            else NEM_TRY(nemgpu_shard_estep_round1(e, beta, -1, L[P], L[Q], L[R]));
            NEM_TRY(rccl_allgather_blocks(e, L[R]));
        }
        NEM_TRY(nemgpu_shard_finish_iteration(e, beta, 0, L[P], L[Q], L[R]));
    }
#undef NEM_TRY
    return nemgpu_shard_end_enqueue(e);
}

int nemgpu_shard_enqueue_batch(nemgpu_engine* e, int with_init, int n_iters, int base, float beta, int want_stats,
                               uint8_t* lab0, uint8_t* lab1, uint8_t* lab2, int stats_off)
{
    if (!e || !lab0 || !lab1 || !lab2 || n_iters < 0 || base < 0 || base > 2) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_enqueue_batch"); if (mr) return mr; }
    if (!e->rccl_comm) { set_error("nemgpu_rccl_attach first"); return NEMGPU_E_FUNCARG; }
    // A rank alone has no collective inside its batches: they go out as hipGraphs of the library's own, captured the
    // second time a shape is enqueued (as the single engine's batches are).  With more ranks the batch holds RCCL
    // calls and is issued launch by launch -- one C call either way.
    if (e->sh_world == 1 && e->use_graphs && !e->libc()) {        // (TIE_LIBC: the stream's position is a launch argument)
        //  Everything that decides WHICH launches the body issues is part of the key: besides the call's
        // arguments, the host state the body branches on.  So a pending reset is flushed here, outside the capture, and
        // a restart clears a reported fault and does the host half of its reset here: a replay only launches the graph,
        // and a reset left pending would later copy the initial parameters over the estimated ones.  (The body does the
        // same again, to the same effect; besides that it changes only the freshness flags: no rewind of its own.)
        { const int cr = shard_check(e); if (cr) return cr; }
        HIPCHK(hipSetDevice(e->device));
        if (with_init == 0) { const int fr = flush_reset(e); if (fr) return fr; }
        else {
            if (!e->have_matrix || !e->have_params) { set_error("matrix and parameters must be set first"); return NEMGPU_E_FUNCARG; }
            const int rr = reset_state(e, true);
            if (rr) return rr;
            e->reset_pending = false;                              // (the device half is the batch's first launch)
            const int cf = clear_fault(e);
            if (cf) return cf;
        }
        e->stop_ptr = nullptr;                                     // (where the body's last call leaves it)
        uint32_t bb; memcpy(&bb, &beta, 4);
        const std::vector<uint64_t> desc = {(uint64_t)with_init, (uint64_t)n_iters, (uint64_t)base, (uint64_t)bb, (uint64_t)want_stats,
                                            (uint64_t)(uintptr_t)lab0, (uint64_t)(uintptr_t)lab1, (uint64_t)(uintptr_t)lab2, (uint64_t)stats_off,
                                            (uint64_t)((with_init ? 0 : ((e->tables_fresh ? 1 : 0) | (e->density_fresh ? 2 : 0) | (e->flags_clean ? 4 : 0) |
                                                                         (e->masks_valid ? 8 : 0))))};
        Graphed how;
        const int r = run_graphed(e, &e->shard_graphs, desc, 2, e->stream, [&]() {
            return shard_batch_body(e, with_init, n_iters, base, beta, want_stats, lab0, lab1, lab2, stats_off);
        }, []() {}, &how);
        e->n_plain += how == Graphed::plain;
        e->n_captured += how == Graphed::captured;
        e->n_replayed += how == Graphed::replayed;
        return r;
    }
    e->n_plain++;
    return shard_batch_body(e, with_init, n_iters, base, beta, want_stats, lab0, lab1, lab2, stats_off);
}

// host-side completion of an iteration whose sweep needed extra rounds: count it like k_ctrl would have
int nemgpu_shard_set_sweep_number(nemgpu_engine* e, int next_sweep)
{
    if (!e) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_shard_set_sweep_number"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)e->sweep_next, next_sweep, 1, e->stream));
    return NEMGPU_OK;
}

// Criteria of the partition the last sweep started from (buffer cur+2: the sweep's ping/pong leave it intact),
// evaluated with the current densities -- what the reference logs "after the M-step" of an iteration
// (WriteLogCrit at the top of ComputePartitionNEM, nem_alg.c:2361).
int nemgpu_criteria_previous(nemgpu_engine* e, float crit6[6])
{
    if (!e || !crit6) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    return criteria(e, crit6, (e->cur + 2) % 3);
}

int nemgpu_set_partition(nemgpu_engine* e, const float* c_nk)
{
    // test hook: load a partition (row-major [n_total x k], HOST) as the current state
    if (!e || !c_nk) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    if (e->ncem()) {
        std::vector<uint8_t> lab((size_t)e->n_total);
        for (int i = 0; i < e->n_total; i++) {
            int best = 0;
            for (int k = 1; k < e->k; k++) if (c_nk[(size_t)i * e->k + k] > c_nk[(size_t)i * e->k + best]) best = k;
            lab[i] = (uint8_t)best;
        }
        HIPCHK(copy_sync(e, e->lab[e->cur], lab.data(), lab.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(e->tie_cnt[e->cur], 0, ((size_t)e->n / 256 + 2) * sizeof(int), e->stream));
    } else {
        HIPCHK(copy_sync(e, e->cbuf[e->cur], c_nk, sizeof(float) * (size_t)e->n_total * e->k, hipMemcpyHostToDevice));
    }
    e->masks_valid = false;
    return NEMGPU_OK;
}

int nemgpu_get_labels(nemgpu_engine* e, uint8_t* labels)
{
    if (!e || !labels) return NEMGPU_E_FUNCARG;
    if (!e->ncem() || !e->lab[e->cur]) { set_error("labels exist only for ncem runs"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(copy_sync(e, labels, e->lab[e->cur] + e->lo, (size_t)e->n, hipMemcpyDeviceToHost));
    for (int i = 0; i < e->n; i++) labels[i] &= 0x7F;              // (bit 7: the site drew, TIE_LIBC)
    return NEMGPU_OK;
}

// the final partition and parameters in one round trip: every piece is copied into one pinned block, one wait
int nemgpu_get_results(nemgpu_engine* e, float* prop, float* center, float* disp, float* nbobs_k, float* c_nk)
{
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    const size_t n = (size_t)e->n, k = (size_t)e->k;
    if (c_nk) {
        if (e->ncem() ? !e->lab[e->cur] : !e->cbuf[e->cur]) { set_error("no partition yet"); return NEMGPU_E_FUNCARG; }
    }
    const size_t b_part = c_nk ? (e->ncem() ? (n + 3) & ~(size_t)3 : sizeof(float) * n * k) : 0;
    const bool want_par = prop || center || disp || nbobs_k;
    const size_t o_prop = b_part, total = o_prop + (want_par ? sizeof(float) * e->par_words : 0);
    char* st = nullptr; size_t got = 0;
    std::vector<char> own;
    const bool pinned = total <= kStageMax && pool_get(e->device, true, total, &st, &got) == hipSuccess;
    if (!pinned) { (void)hipGetLastError(); own.resize(total); st = own.data(); }
    hipError_t err = hipSuccess;
    auto D2H = [&](size_t off, const void* src, size_t bytes) {
        if (err == hipSuccess && bytes) err = hipMemcpyAsync(st + off, src, bytes, hipMemcpyDeviceToHost, e->stream);
    };
    if (c_nk) {
        if (e->ncem()) D2H(0, e->lab[e->cur] + e->lo, n);
        else D2H(0, e->cbuf[e->cur] + (size_t)e->lo * k, sizeof(float) * n * k);
    }
    if (want_par) D2H(o_prop, e->prop, sizeof(float) * e->par_words);   // prop | center | disp | nbobs_k: one block
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess) result_unpack(e, st, b_part, prop, center, disp, nbobs_k, c_nk);
    if (pinned) pool_put(e->device, true, st, got);
    HIPCHK(err);
    return NEMGPU_OK;
}

int nemgpu_get_partition(nemgpu_engine* e, float* c_nk)
{
    if (!e || !c_nk) return NEMGPU_E_FUNCARG;
    return nemgpu_get_results(e, nullptr, nullptr, nullptr, nullptr, c_nk);
}

int nemgpu_get_params(nemgpu_engine* e, float* prop, float* center, float* disp, float* nbobs_k)
{
    if (!e) return NEMGPU_E_FUNCARG;
    return nemgpu_get_results(e, prop, center, disp, nbobs_k, nullptr);
}

int nemgpu_get_observed_counts(nemgpu_engine* e, float* nbobs_kd)
{
    if (!e || !nbobs_kd) return NEMGPU_E_FUNCARG;
    if (!e->has_obs) { set_error("nemgpu_get_observed_counts: the engine has no observed mask"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(copy_sync(e, nbobs_kd, e->nbobs_kd, sizeof(float) * e->k * e->d, hipMemcpyDeviceToHost));
    return NEMGPU_OK;
}

int nemgpu_get_density(nemgpu_engine* e, double* pkfki_nk, float* logpkfki_nk)
{
    // device layout is class-major [k][npad]; hand back the reference's row-major [n][k]
    if (!e) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t m = (size_t)e->k * e->npad;
    if (pkfki_nk) {
        std::vector<double> t(m);
        HIPCHK(copy_sync(e, t.data(), e->pkfki, sizeof(double) * m, hipMemcpyDeviceToHost));
        for (int i = 0; i < e->n; i++) for (int k = 0; k < e->k; k++) pkfki_nk[(size_t)i * e->k + k] = t[(size_t)k * e->npad + i];
    }
    if (logpkfki_nk) {
        std::vector<float> t(m);
        HIPCHK(copy_sync(e, t.data(), e->logpkfki, sizeof(float) * m, hipMemcpyDeviceToHost));
        for (int i = 0; i < e->n; i++) for (int k = 0; k < e->k; k++) logpkfki_nk[(size_t)i * e->k + k] = t[(size_t)k * e->npad + i];
    }
    return NEMGPU_OK;
}

// Kernel-duration probe for bench.py: `reps` launches of the E1 density kernel on the current parameters,
// each bracketed by HIP events recorded on the engine's stream; returns the average duration and the
// algorithmic bytes one launch moves.
int nemgpu_profile_density(nemgpu_engine* e, int reps, double* avg_ms, double* algorithmic_bytes_per_launch,
                           int* used_fused_kernel)
{
    if (!e || reps <= 0) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_profile_density"); if (mr) return mr; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = do_tables(e))) return r;
    if (!e->ev0) { HIPCHK(hipEventCreate(&e->ev0)); HIPCHK(hipEventCreate(&e->ev1)); }
    double total = 0.0;
    // measure the kernel the EM loop actually launches: the fused one (parameter update + density) when it applies
    const bool fused = !e->cfg.param_fix && e->ncem() && e->fused_update() && e->iters > 0;
    for (int i = 0; i < reps; i++) {
        HIPCHK(hipEventRecord(e->ev0, e->stream));
        if (fused) {
            density_launch(e, finish_args(e, 1, e->stats_last), nullptr, false);
            HIPCHK(hipGetLastError());
        } else if ((r = do_density(e))) return r;
        HIPCHK(hipEventRecord(e->ev1, e->stream));
        HIPCHK(hipEventSynchronize(e->ev1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        total += ms;
    }
    if (avg_ms) *avg_ms = total / reps;
    if (used_fused_kernel) *used_fused_kernel = fused ? 1 : 0;
    if (algorithmic_bytes_per_launch) {
        // E1 per launch: the bit-packed matrix once, the (k,d) tables once, pk*fk (f64) and log (f32) out
        *algorithmic_bytes_per_launch = (double)e->n * e->wf * 4.0 + (double)e->k * e->d * 24.0 +
                                        (double)e->n * e->k * 12.0;
    }
    return NEMGPU_OK;
}

// E1 as a lock-step batch launches it: the density kernels of `count` engines (same shape) zipped into ONE launch
// (k_density_b, problem = blockIdx.z), `reps` such launches back to back between one pair of HIP events on the first
// engine's stream.  avg_ms: per launch (all members); bytes: algorithmic bytes of one launch (all members).  The engines
// must have run (their parameters and tables are what the last M-step left).
int nemgpu_profile_density_many(nemgpu_engine** engines, int count, int reps, double* avg_ms, double* algorithmic_bytes_per_launch)
{
    if (!engines || count <= 0 || reps <= 0) return NEMGPU_E_FUNCARG;
    nemgpu_engine* lead = engines[0];
    HIPCHK(hipSetDevice(lead->device));
    int r;
    for (int m = 0; m < count; m++) if (engines[m] && (r = masked_refuse(engines[m], "nemgpu_profile_density_many"))) return r;
    std::vector<Recorder> recs((size_t)count);
    double bytes = 0.0;
    for (int m = 0; m < count; m++) {
        nemgpu_engine* e = engines[m];
        if (!e || e->device != lead->device) { set_error("profile_density_many: engines of one device"); return NEMGPU_E_FUNCARG; }
        if ((r = flush_reset(e)) || (r = do_tables(e))) return r;
        HIPCHK(hipStreamSynchronize(e->stream));
        set_recorder(&recs[m]);
        r = do_density(e);
        set_recorder(nullptr);
        if (r) return r;
        if (recs[m].ops.size() != 1) { set_error("profile_density_many: one density launch per engine expected"); return NEMGPU_E_INTERNAL; }
        if (!same_sequence(recs[m], recs[0])) { set_error("profile_density_many: the engines' density launches differ in shape"); return NEMGPU_E_FUNCARG; }
        bytes += (double)e->n * e->wf * 4.0 + (double)e->k * e->d * 24.0 + (double)e->n * e->k * 12.0;
    }
    std::vector<std::vector<int>> all(1);
    for (int m = 0; m < count; m++) all[0].push_back(m);
    const size_t total = zip_pack(nullptr, recs.data(), all, nullptr);
    if ((r = zip_reserve(lead, total))) return r;
    nemgpu_engine::ZipContext* z = zip_context(lead);
    std::vector<ZipPos> pos;
    zip_pack(z->zip_host, recs.data(), all, &pos);
    HIPCHK(hipMemcpyAsync(z->zip_dev, z->zip_host, total, hipMemcpyHostToDevice, lead->stream));
    if (!lead->ev0) { HIPCHK(hipEventCreate(&lead->ev0)); HIPCHK(hipEventCreate(&lead->ev1)); }
    auto once = [&]() { zip_issue(pos[0], z->zip_dev, lead->stream); };
    once();                                                    // (warm)
    HIPCHK(hipEventRecord(lead->ev0, lead->stream));
    for (int i = 0; i < reps; i++) once();
    HIPCHK(hipEventRecord(lead->ev1, lead->stream));
    HIPCHK(hipEventSynchronize(lead->ev1));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, lead->ev0, lead->ev1));
    if (avg_ms) *avg_ms = (double)ms / reps;
    if (algorithmic_bytes_per_launch) *algorithmic_bytes_per_launch = bytes;
    return NEMGPU_OK;
}

// Kernel-duration probe for bench.py's roofline.kernels[]: the three kernels of a solo NCEM iteration -- E1 (with the
// parameter update when the loop launches it that way), one relaxation round of the E-step sweep, the M-step counts --
// each launched `reps` times back to back between ONE pair of HIP events on the engine's stream (an event pair per
// launch costs ~3 us, as much as the shorter kernels), on the state the engine is in (the launches are idempotent: same
// inputs, same outputs; the partition is not advanced).  avg_ms[3], bytes[3]: average duration and algorithmic bytes
// per launch of {E1, sweep round, counts}; which[0]: 1 when E1 is the fused kernel.
int nemgpu_profile_kernels(nemgpu_engine* e, int reps, double avg_ms[3], double bytes[3], int which[1])
{
    if (!e || reps <= 0 || !avg_ms || !bytes) return NEMGPU_E_FUNCARG;
    { const int mr = masked_refuse(e, "nemgpu_profile_kernels"); if (mr) return mr; }
    if (!e->ncem() || e->lo != 0 || e->hi != e->n_total) { set_error("the kernel probe times a whole NCEM problem on one engine"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    { const int fr = flush_reset(e); if (fr) return fr; }
    int r;
    if ((r = ensure_state_buffers(e))) return r;
    if ((r = do_tables(e))) return r;
    if (!e->masks_valid) { if ((r = do_labels_post(e, e->cur, -1))) return r; }
    if (!e->ev0) { HIPCHK(hipEventCreate(&e->ev0)); HIPCHK(hipEventCreate(&e->ev1)); }
    const bool fused = !e->cfg.param_fix && e->fused_update() && e->iters > 0;
    auto timed = [&](auto&& launch, double* out) -> int {
        launch();                                                  // (one untimed launch: code object, caches)
        HIPCHK(hipEventRecord(e->ev0, e->stream));
        for (int i = 0; i < reps; i++) launch();
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e->ev1, e->stream));
        HIPCHK(hipEventSynchronize(e->ev1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
        *out = (double)ms / reps;
        return NEMGPU_OK;
    };
    // M-step counts first: they leave the statistics the fused E1 derives its parameters from
    CountsArgs ca = counts_args(e, e->stats, nullptr);
    ca.stop = nullptr;                                             // (the timed launches read no stop word)
    if ((r = timed([&] { launch_mstep_counts(ca, e->stream); }, &avg_ms[2]))) return r;
    e->stats_last = e->stats;
    if ((r = timed([&] {
            if (fused) density_launch(e, finish_args(e, 1, e->stats), nullptr, false);
            else launch_density(finish_args(e, 0, nullptr), density_io(e), e->stream);
        }, &avg_ms[0]))) return r;
    e->density_fresh = true; e->flags_clean = true;
    if (fused) e->tables_fresh = false;
    // one relaxation round: round 0 of a sweep from the current partition (guess = old), into the next buffer
    {
        SweepCtx c;
        const uint32_t keep = e->sweep_counter;
        if ((r = sweep_setup(e, e->cfg.beta, c, true))) return r;
        e->sweep_counter = keep;
        const int P = e->cur, Q = (e->cur + 1) % 3;
        c.a.lab_old = e->lab[P]; c.a.lab_guess = e->lab[P]; c.a.lab_out = e->lab[Q];
        c.a.tie_cnt_guess = e->tie_cnt[P]; c.a.tie_cnt_out = e->tie_cnt[Q];
        c.a.flags = e->round_flags(0); c.a.fold_ticket = e->sweep_next + 32;
        if ((r = timed([&] { launch_sweep(c.a, true, e->stream); }, &avg_ms[1]))) return r;
        e->flags_clean = false;
    }
    const double n = e->n, d = e->d, k = e->k, nnz = e->nnz;
    bytes[0] = n * e->wf * 4.0 + k * d * 24.0 + n * k * 12.0;             // bit matrix once, (k,d) tables, pk*fk f64 + log f32 out
    bytes[1] = 8.0 * nnz + 4.0 * (n + 1) + nnz + 8.0 * n * k + 2.0 * n;   // CSR idx + w, row pointers, neighbour labels, densities, labels in/out
    bytes[2] = d * e->nw64 * 8.0 + k * e->nw64 * 8.0 + 4.0 * (k + k * d); // organism bit rows once, class masks once, counts out
    if (which) which[0] = fused ? 1 : 0;
    return NEMGPU_OK;
}

// `reps` in-place all-gathers of the sharded EM's label blocks (stride bytes per rank) back to back through the engine's
// own communicator, between one pair of HIP events: what ONE of the iteration's two collectives costs.  Collective.
int nemgpu_rccl_time_allgather(nemgpu_engine* e, uint8_t* buf_dev, int reps, double* avg_ms)
{
    if (!e || !buf_dev || reps <= 0 || !avg_ms) return NEMGPU_E_FUNCARG;
    if (!e->rccl_comm) { set_error("nemgpu_rccl_attach first"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(e->device));
    if (!e->ev0) { HIPCHK(hipEventCreate(&e->ev0)); HIPCHK(hipEventCreate(&e->ev1)); }
    const size_t stride = (size_t)e->sh_stride;
    auto gather = [&]() { return g_rccl.all_gather(buf_dev + (size_t)e->sh_rank * stride, buf_dev, stride, /*ncclUint8*/ 1, e->rccl_comm, e->stream); };
    for (int i = 0; i < 3; i++) { const int rc = gather(); if (rc != 0) return rccl_fail("ncclAllGather", rc); }
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    for (int i = 0; i < reps; i++) { const int rc = gather(); if (rc != 0) return rccl_fail("ncclAllGather", rc); }
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *avg_ms = (double)ms / reps;
    return NEMGPU_OK;
}

// FETCH_SIZE calibration helper (profiles/README.md): one launch that reads `bytes` of freshly written device
// memory with E1's dword-per-lane pattern.  Run it under `rocprofv3 --pmc FETCH_SIZE` and compare.
int nemgpu_calibrate_fetch(size_t bytes, int reps)
{
    if (bytes < 4096 || reps <= 0) return NEMGPU_E_FUNCARG;
    uint32_t* buf = nullptr; uint32_t* sink = nullptr;
    HIPCHK(hipMalloc((void**)&buf, bytes));
    HIPCHK(hipMalloc((void**)&sink, 64));
    HIPCHK(hipMemset(buf, 0x5A, bytes));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < reps; i++) launch_calib_read(buf, bytes / 4, sink, nullptr);
    hipError_t err = hipDeviceSynchronize();
    (void)hipFree(buf); (void)hipFree(sink);
    HIPCHK(err);
    return NEMGPU_OK;
}

// Re-target the engine to another HIP stream (e.g. the capturing stream of a torch.cuda.graph).
int nemgpu_set_fast_forward(nemgpu_engine* e, int on)
{
    if (!e) return NEMGPU_E_FUNCARG;
    const int mode = on < 0 ? -1 : (on != 0);
    if (e->ff_mode != mode) {
        HIPCHK(hipStreamSynchronize(e->stream));
        drop_graphs(e);                                            // captured launches carry the old setting
        e->ff_mode = mode;
        e->density_fresh = false;
        e->tables_fresh = false;                                   // (the increment tables are built with the density tables)
    }
    return NEMGPU_OK;
}

int nemgpu_ff_table(double l1, double l0, uint32_t* q0_256, uint32_t* q1_256)
{
    if (!q0_256 || !q1_256) return NEMGPU_E_FUNCARG;
    for (int E = 0; E < 256; E++) nemk::ff_entry(l1, -l0, E, q0_256[E], q1_256[E]);
    return NEMGPU_OK;
}

// capture_on_first != 0: a batch shape of the pipelined loop is captured into a hipGraph the FIRST time it is
// enqueued (default: the second time -- a nem() call's engine enqueues most shapes once and capturing costs more
// than it saves unless the batch is replayed).  Benchmarks prime every shape of their timed region with it.
int nemgpu_set_graph_policy(nemgpu_engine* e, int capture_on_first)
{
    if (!e) return NEMGPU_E_FUNCARG;
    e->capture_first = capture_on_first != 0;
    return NEMGPU_OK;
}

// out[0] batches enqueued as plain launches, out[1] batches captured + instantiated (one-off cost), out[2] graph
// replays, out[3] sweeps the host had to finish round by round (more than the two enqueued relaxation rounds)
int nemgpu_graph_counters(const nemgpu_engine* e, int out[4])
{
    if (!e || !out) return NEMGPU_E_FUNCARG;
    out[0] = e->n_plain; out[1] = e->n_captured; out[2] = e->n_replayed; out[3] = e->n_host_rounds;
    return NEMGPU_OK;
}

// starts that went out without a blind launch (blind_fold_on), replays of such a start's graph included; -1: no engine
int nemgpu_debug_blind_folds(const nemgpu_engine* e)
{
    return e ? e->n_blind_folds : -1;
}

int nemgpu_random_start_counters(const nemgpu_engine* e, int out[4])
{
    if (!e || !out) return NEMGPU_E_FUNCARG;
    out[0] = e->rs_rounds; out[1] = e->rs_lockstep; out[2] = e->rs_alone; out[3] = e->rs_redone;
    return NEMGPU_OK;
}

int nemgpu_set_stream(nemgpu_engine* e, void* hip_stream)
{
    if (!e || !hip_stream) return NEMGPU_E_FUNCARG;
    if (e->own_stream && e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    e->stream = (hipStream_t)hip_stream;
    e->own_stream = false;
    drop_graphs(e);
    return NEMGPU_OK;
}

}  // extern "C"

// ---- test hooks for the exact segmented chains (nem_chain.hpp) ----
// mode 0: plain sequential loop; 1: the host emulation of the device procedure.  No GPU needed.
extern "C" float nemgpu_repeat_add_host(float x, long long times, int mode)
{
    if (mode == 2) return (x > 0.0f && x < 16777216.0f && x == (float)(uint32_t)x) ? nemk::ff_repeat_add_u24((uint32_t)x, times) : nemk::ff_repeat_add(x, times);
    if (mode != 0) return nemk::ff_repeat_add(x, times);
    volatile float s = 0.0f;
    for (long long j = 0; j < times; j++) s = s + x;
    return s;
}

extern "C" float nemgpu_chain_host(const double* x, long long n, float init, int mode)
{
    return mode == 0 ? nemchain::run_sequential(x, n, init) : nemchain::run_segmented(x, n, init);
}

// the device procedure on device `device`; returns NEMGPU_OK or an error code
extern "C" int nemgpu_chain_device(const double* x, long long n, float init, int device, float* out)
{
    if (x == nullptr || out == nullptr || n < 0) { set_error("nemgpu_chain_device: bad argument"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(device));
    double* dx = nullptr; float* dout = nullptr;
    HIPCHK(hipMalloc(&dx, (size_t)std::max<long long>(n, 1) * sizeof(double)));
    HIPCHK(hipMalloc(&dout, sizeof(float)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (n > 0) HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    nemk::launch_chain_debug(dx, n, init, dout, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st); (void)hipFree(dx); (void)hipFree(dout);
    return NEMGPU_OK;
}

// ---- test hooks for the piecewise d-ordered chain of non-negative multiples of 1/2 (nem_halfsum.hpp) ----
// mode 0: the plain sequential loop; mode w = 1 .. 16: the host emulation of the device procedure with w wavefronts
// (stepped: how many of the n adds it took for real).  No GPU needed.
extern "C" float nemgpu_halfsum_host(const float* x, int n, int mode, int* stepped)
{
    if (stepped) *stepped = mode == 0 ? n : 0;
    if (x == nullptr || n <= 0 || mode < 0 || mode > nemk::kHsMaxWaves) return 0.0f;
    return mode == 0 ? nemk::halfsum_plain(x, n) : nemk::halfsum_host(x, n, mode, stepped);
}

// the device procedure (n <= 8192; waves = 16: the block of k_finish, 1: one wavefront) on device `device`
extern "C" int nemgpu_halfsum_device(const float* x, int n, int waves, int device, float* out)
{
    if (x == nullptr || out == nullptr || n < 0 || n > 8192 || (waves != 1 && waves != 16)) { set_error("nemgpu_halfsum_device: bad argument"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(device));
    float* dx = nullptr; float* dout = nullptr;
    HIPCHK(hipMalloc(&dx, (size_t)std::max(n, 1) * sizeof(float)));
    HIPCHK(hipMalloc(&dout, 2 * sizeof(float)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (n > 0) HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    nemk::launch_halfsum_debug(dx, n, waves, dout, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st); (void)hipFree(dx); (void)hipFree(dout);
    return NEMGPU_OK;
}

// ---- test hooks for the NCEM label from the unnormalised row (nem_map.hpp) ----
// n rows cinum[n][K] (K <= 32): out[i] = {the normalised row's first maximum, the later entries equal to it as floats,
// the unnormalised row's first maximum, whether the row is clear}.  No GPU needed.
extern "C" int nemgpu_map_margin_host(const double* cinum, int n, int K, int* out)
{
    if (cinum == nullptr || out == nullptr || n < 0 || K < 1 || K > nemk::kMaxKernelK) { set_error("nemgpu_map_margin_host: bad argument"); return NEMGPU_E_FUNCARG; }
    for (int i = 0; i < n; i++) {
        int* o = out + 4 * (size_t)i;
        o[3] = nemk::map_row_host(cinum + (size_t)i * K, K, &o[0], &o[1], &o[2]) ? 1 : 0;
    }
    return NEMGPU_OK;
}

// the same four per row from the device's arithmetic, rows given as a round has them: densities pkf[n][K] and class
// contexts ctx[n][K], cinum = pkf * exp(beta * ctx) when use_nei (else pkf); K <= 8
extern "C" int nemgpu_map_margin_device(const double* pkf, const float* ctx, int n, int K, float beta, int use_nei, int device, int* out)
{
    if (pkf == nullptr || ctx == nullptr || out == nullptr || n <= 0 || K < 1 || K > 8) { set_error("nemgpu_map_margin_device: bad argument"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(device));
    const size_t m = (size_t)n * K;
    double* dp = nullptr; float* dc = nullptr; int* dout = nullptr;
    HIPCHK(hipMalloc(&dp, m * sizeof(double)));
    HIPCHK(hipMalloc(&dc, m * sizeof(float)));
    HIPCHK(hipMalloc(&dout, (size_t)n * 4 * sizeof(int)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPCHK(hipMemcpyAsync(dp, pkf, m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dc, ctx, m * sizeof(float), hipMemcpyHostToDevice, st));
    nemk::launch_map_margin_debug(dp, dc, n, K, beta, use_nei, dout, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st); (void)hipFree(dp); (void)hipFree(dc); (void)hipFree(dout);
    return NEMGPU_OK;
}

// where the device procedure spends its time (in-kernel clock, 100 MHz): us[0..3] = prefix sums, classification + walk,
// scan + hand-over, ordered pass; us[4] = the same chain as plain dependent adds on one lane
extern "C" int nemgpu_halfsum_profile(const float* x, int n, int waves, int device, double us[5])
{
    if (x == nullptr || us == nullptr || n < 0 || n > 8192 || (waves != 1 && waves != 16)) { set_error("nemgpu_halfsum_profile: bad argument"); return NEMGPU_E_FUNCARG; }
    HIPCHK(hipSetDevice(device));
    float* dx = nullptr; float* dout = nullptr; long long* dst = nullptr;
    HIPCHK(hipMalloc(&dx, (size_t)std::max(n, 1) * sizeof(float)));
    HIPCHK(hipMalloc(&dout, 2 * sizeof(float)));
    HIPCHK(hipMalloc(&dst, 6 * sizeof(long long)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (n > 0) HIPCHK(hipMemcpyAsync(dx, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    long long h[6];
    for (int rep = 0; rep < 3; rep++) nemk::launch_halfsum_debug(dx, n, waves, dout, st, dst);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dst, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 5; i++) us[i] = (double)(h[i + 1] - h[i]) * 0.01;
    (void)hipStreamDestroy(st); (void)hipFree(dx); (void)hipFree(dout); (void)hipFree(dst);
    return NEMGPU_OK;
}
