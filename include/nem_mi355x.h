/*
 * nem_mi355x.h -- C ABI of the MI355X-native NEM partitioning engine.
 *
 * Two layers, both plain C (pointers and sizes, no torch/C++ types):
 *
 *  1. The DROP-IN entry `nem()`: same symbol, signature, argument meaning, file formats and
 *     return codes as the reference's only FFI entry point
 *         /root/reference/ppanggolin/NEM/nem_exe.h:23-35   (declaration)
 *         /root/reference/ppanggolin/NEM/nem_exe.c:239-704 (definition)
 *         /root/reference/ppanggolin/NEM/nem.pyx:1-14      (the Cython `cpdef` binding PPanGGOLiN uses)
 *     It reads <Fname>.str/.dat/.nei/.m, runs the EM loop on the GPU, writes <Fname>.uf|.cf, .mf,
 *     .stderr and (dolog) .log.
 *
 *  2. The in-memory engine `nemgpu_*`: the same EM loop without the ASCII files, for callers that
 *     already hold the presence/absence matrix (benchmarks, tests, the multi-GPU host driver).
 *     It replaces the in-memory path  ClassifyByNem()  nem_alg.h:10-18 / nem_alg.c:546-584.
 *
 * Every entry point fails loudly (non-zero return + message in nemgpu_last_error()) when no HIP
 * device is usable: there is no CPU fallback in this library.
 */
#ifndef NEM_MI355X_H
#define NEM_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * 1. Drop-in entry (reference: nem_exe.h:23-35).
 *
 *   Fname          base path; inputs <Fname>.str .dat .nei .m, outputs <Fname>.uf|.cf .mf .stderr .log
 *                  .dat: N*D values 0 or 1; a token strtof reads as NaN (nan, NaN, nan(...)) is a cell that was not
 *                  observed, as in the reference (nem_exe.c:477-490, nem_mod.c:654).  Files with such cells run under
 *                  algo "ncem" with init_mode 2 (nemgpu_set_observed_bits below); "nem" and init_mode 1 on them return
 *                  2 and say why in <Fname>.stderr.  Any other value is refused as a file error.
 *   nk             number of classes K (> 0)
 *   algo           "nem" | "ncem"            ("gem" is not reachable from PPanGGOLiN; rejected)
 *   beta           MRF weight of the neighbourhood term
 *   convergence    "none" | "clas" | "crit"
 *   convergence_th threshold: "clas" max |c - c_old| < th; "crit" |(M - M_old) / M| < th (nem_alg.c:2075-2105)
 *   format         "hard" (.cf) | "fuzzy" (.uf)
 *   it_max         maximum number of EM iterations (>= 0)
 *   dolog          non-zero: messages to <Fname>.stderr and the reference's iteration log <Fname>.log (criteria
 *                  before / after every E-step and all parameters per iteration; NEM_MI355X_LOG=0: header only)
 *   model_family   "bern" (the only family PPanGGOLiN uses; "norm"/"lapl" rejected)
 *   proportion     "p_" | "pk"
 *   dispersion     "s__" | "sk_" | "s_d" | "skd"
 *   init_mode      2 (INIT_PARAM_FILE, nem_typ.h:218: start from <Fname>.m) or 1 (INIT_RANDOM, :217: 50 random
 *                  starts, best by criterion M, <Fname>.m not read; what PPanGGOLiN's partition_shell uses,
 *                  ppanggolin.py:1207); modes 0, 3, 4 rejected
 *
 * Return value (ExitET, lib_io.h:22-34): 0 ok, 1 empty class (no output files, like the
 * reference), 2 bad arguments, 3 file error, 4 memory, 5 GPU/system error, 6 internal error.
 * ------------------------------------------------------------------------------------------ */
int nem(const char* Fname,
        const int nk,
        const char* algo,
        const float beta,
        const char* convergence,
        const float convergence_th,
        const char* format,
        const int it_max,
        const int dolog,
        const char* model_family,
        const char* proportion,
        const char* dispersion,
        const int init_mode);

/* ------------------------------------------------------------------------------------------
 * 2. In-memory engine.
 * ------------------------------------------------------------------------------------------ */
typedef struct nemgpu_engine nemgpu_engine;

/* numeric values follow the reference enums (nem_typ.h:121-128, 191-205, 271-277) */
enum { NEMGPU_ALGO_NEM = 0, NEMGPU_ALGO_NCEM = 1 };
enum { NEMGPU_DISP___ = 0, NEMGPU_DISP_K_ = 1, NEMGPU_DISP__D = 2, NEMGPU_DISP_KD = 3 };
enum { NEMGPU_PROP__ = 0, NEMGPU_PROP_K = 1 };
/* CRIT: HasConverged's CVTEST_CRIT (nem_alg.c:2090-2105) on criterion M, starting from 0 like a reference run
   without a log (Criteria = {0}, nem_exe.c:264); CRIT_LOGGED: starting from the criterion of the initial partition,
   like a reference run with dolog (WriteLogCrit, nem_alg.c:1980, 2398) */
enum { NEMGPU_CV_NONE = 0, NEMGPU_CV_CLAS = 1, NEMGPU_CV_CRIT = 2, NEMGPU_CV_CRIT_LOGGED = 3 };
/* NCEM tie rule (ComputeMAP, nem_alg.c:590-645; numeric values of TIE_RANDOM / TIE_FIRST follow TieET).
   LIBC = the reference's TIE_RANDOM: kmaxes[random() % (nequal+1)] on glibc's random() after srandom(tie_seed)
   (nem_exe.c:621; the reference seeds with time(NULL), :353), drawn in site order exactly as the sequential
   sweep draws them -- with the seed fixed, labels equal the reference's even where classes tie.
   FIRST = TIE_FIRST.  HASH: counter-based, kmaxes[mix32(seed, sweep, site) % (nequal+1)] (stateless; the
   family-sharded multi-GPU path uses it). */
enum { NEMGPU_TIE_LIBC = 0, NEMGPU_TIE_FIRST = 1, NEMGPU_TIE_HASH = 2 };
/* status codes = StatusET (nem_typ.h:106-117) */
enum { NEMGPU_OK = 0, NEMGPU_W_EMPTYCLASS = 2, NEMGPU_E_ARG = 3, NEMGPU_E_MEMORY = 4,
       NEMGPU_E_FILEIN = 5, NEMGPU_E_FILEOUT = 6, NEMGPU_E_FILE = 7, NEMGPU_E_FUNCARG = 8,
       NEMGPU_E_DEVICE = 9,
       /* a kernel reported that it could not finish its work (e.g. a producer/consumer hand-over of the fuzzy M-step
          that never completed): the results of the call are not to be used.  nem() returns 6 (EXIT_E_BUG). */
       NEMGPU_E_INTERNAL = 10 };

typedef struct {
    int   algo;        /* NEMGPU_ALGO_*  */
    float beta;
    int   disper;      /* NEMGPU_DISP_*  */
    int   propor;      /* NEMGPU_PROP_*  */
    int   cvtest;      /* NEMGPU_CV_*    */
    float cvthres;
    int   it_max;
    int   param_fix;   /* .m flag 2: never re-estimate parameters (nem_alg.c:1806) */
    int   tie_rule;    /* NEMGPU_TIE_*   */
    uint32_t tie_seed;
} nemgpu_config;

typedef struct {
    int   status;      /* NEMGPU_OK or NEMGPU_W_EMPTYCLASS */
    int   iters;       /* completed EM iterations */
    int   converged;
    int   emptyk;      /* 1..K, 0 if none */
    int   zero_density_sites;   /* E-step updates that hit cumnum == 0 (nem_alg.c:2603-2613) */
    int   first_zero_density_site;
    int   sweep_rounds;         /* total relaxation rounds spent in E-step sweeps */
    float crit[6];     /* D G U M L Z (ComputeCrit, nem_alg.c:2678-2757) */
    double loop_seconds;        /* wall time of the EM iteration loop (host clock, synchronised) */
    int   tie_draws;            /* TIE_LIBC: random() draws consumed so far (a .cf writer continues the stream there) */
} nemgpu_result;

const char* nemgpu_last_error(void);

/* Number of usable HIP devices (0 when none, and in a process forked from one that had already used the GPU). */
int nemgpu_device_count(void);
/* The device a call that was not given one runs on -- what the drop-in nem() uses.  NEM_MI355X_DEVICE = <index>: that
   device (anything but a valid index is NEMGPU_E_ARG); NEM_MI355X_DEVICE = auto: processes spread over the node's
   devices, LOCAL_RANK (a launcher's) when set, else the process id, modulo the device count (PPanGGOLiN runs its
   chunks in a multiprocessing.Pool, ppanggolin.py:1039-1095); unset: the calling thread's current HIP device, i.e.
   the one the embedding application selected (device 0 when it selected none).  Fails with NEMGPU_E_DEVICE, before
   any HIP call, in a forked child of a process that had used the GPU. */
int nemgpu_default_device(int* device);

/* Create an engine for n_total families x d organisms, k classes on `device`.
   [site_lo, site_hi) is the family shard this engine owns (0, n_total for a single GPU).
   `hip_stream` is a hipStream_t to run on, or NULL for an engine-owned stream. */
int nemgpu_create(nemgpu_engine** out, int n_total, int d, int k, int site_lo, int site_hi,
                  int device, void* hip_stream);
void nemgpu_destroy(nemgpu_engine* e);

/* Presence/absence rows of the owned shard, one byte per cell (0/1), row-major
   [(site_hi-site_lo) x d], HOST memory.  Bit-packs, uploads and builds both device layouts. */
int nemgpu_set_matrix_bytes(nemgpu_engine* e, const uint8_t* x_host);
/* Same, family-major bit-packed rows: word w of row i holds organisms 32w..32w+31 (bit b =
   organism 32w+b), ceil(d/32) words per row, HOST memory.  Bits above organism d-1 in a row's last word are
   padding: the library clears them in its own copy (the caller's buffer is not written), whatever they hold. */
int nemgpu_set_matrix_bits(nemgpu_engine* e, const uint32_t* xbits_host);
/* Missing cells (a `nan` in the .dat, which the reference's NEM treats as not observed: DensBernoulli nem_mod.c:654,
   EstimSizes :1310, ComputeMedian :1455, EstimLaplaceIner :1682, InerToDisp* in their MISSING_IGNORE branches).
   obits_host: the layout of nemgpu_set_matrix_bits, bit j of row i = 1 when organism j of family i was observed; bits
   above organism d-1 are ignored.  NULL removes the mask.  The matrix bit of an unobserved cell is don't-care (the
   masked kernels read every matrix word through the mask).  The mask stays with the engine when another matrix is
   uploaded (nemgpu_set_matrix_*): only NULL here removes it.  (An engine holds at most 2^24 families, nemgpu_create:
   the observed counts are exact as floats, as the reference's sums are.)  An engine with a mask -- even one of all ones -- runs
   NCEM on the masked path: k_density_masked, k_mstep_counts_masked and k_finish_masked (nem_missing.hip), one host
   round trip per EM iteration, no graphs, no pipelining.  nemgpu_run, nemgpu_iterate, nemgpu_run_logged,
   nemgpu_iterate_logged, nemgpu_init_partition and the single steps (nemgpu_density, _sweep, _mstep, _criteria) work on it; the fuzzy algorithm,
   nemgpu_run_many, nemgpu_run_random*, nemgpu_restart_iterate, every nemgpu_shard_* and the nemgpu_profile_* calls
   refuse it with NEMGPU_E_ARG before any launch.  An engine without a mask runs exactly what it ran before. */
int nemgpu_set_observed_bits(nemgpu_engine* e, const uint32_t* obits_host);
/* Neighbourhood graph of the owned shard in CSR, .nei file order inside a row; neighbour
   indices are GLOBAL family indices (0-based).  ptr has (site_hi-site_lo)+1 entries.  HOST memory. */
int nemgpu_set_graph(nemgpu_engine* e, const int32_t* ptr, const int32_t* idx, const float* w);
/* Initial parameters (the .m file content): prop[k], center[k*d], disp[k*d].  HOST memory. */
int nemgpu_set_params(nemgpu_engine* e, const float* prop, const float* center, const float* disp);
int nemgpu_configure(nemgpu_engine* e, const nemgpu_config* cfg);

/* Whole run: INIT_PARAM_FILE start + EM loop + final criteria (single-GPU engines only). */
int nemgpu_run(nemgpu_engine* e, nemgpu_result* res);

/* Several whole runs (nemgpu_run each) in LOCK STEP: every step of the EM -- M-step counts, density, relaxation
   rounds, criteria -- is ONE launch for all `count` problems (problem = blockIdx.z; every loop kernel has a twin that
   reads an array of argument blocks), and the host synchronises once per batch of iterations for everybody.  What
   PPanGGOLiN's chunk loop (ppanggolin.py:1045-1086) needs: many independent problems of one kind, each far too small
   to fill the chip.  The engines must be complete (matrix, graph, parameters, configuration), whole problems, on one
   device; sizes and configurations may differ (members whose launch sequences differ are grouped).  Each problem's
   result is bit-identical to its nemgpu_run.  results: `count` entries. */
int nemgpu_run_many(nemgpu_engine** engines, int count, nemgpu_result* results);

/* Many whole problems from host arrays to host arrays in ONE call -- PPanGGOLiN's chunk loop
   (ppanggolin.py:1045-1086) when the chunks are arrays: `workers` threads of the library build the engines (bit
   packing, asynchronous uploads), the calling thread runs each `group` of them in lock step (nemgpu_run_many) as soon
   as it is complete -- the run waits for its members' uploads by event, their device layouts ride in its first step,
   their partitions and parameters come back in one block with it -- and the workers unpack the results and recycle the
   engines while later groups are being built.  From four groups on (and six workers) the groups are dealt to two such
   runners on the device (NEM_MI355X_RUNNERS=n: n runners; 1: never split).  Every problem's result equals its own
   nemgpu_run; every element of a problem's out_* arrays is written when its rc is NEMGPU_OK.  Returns the first
   failure (each problem's own status is in rc). */
typedef struct {
    int n, d, k;
    const uint8_t*  x_bytes;     /* [n][d] values 0/1 ...                                   */
    const uint32_t* x_bits;      /* ... or [n][ceil(d/32)] bit rows: exactly one of the two */
    const int32_t*  nei_ptr;     /* CSR neighbourhood graph [n+1] (NULL: none) */
    const int32_t*  nei_idx;
    const float*    nei_w;
    const float *prop, *center, *disp;                                  /* initial parameters [k], [k][d], [k][d] */
    float *out_prop, *out_center, *out_disp, *out_nbobs_k, *out_c;      /* results, any may be NULL; out_c [n][k] */
    nemgpu_result result;
    int rc;
} nemgpu_problem;
int nemgpu_solve_many(nemgpu_problem* problems, int count, const nemgpu_config* cfg, int device, int workers, int group);

/* The same over several devices of this process -- independent chunk problems side by side, the reference's own form of
   parallelism (multiprocessing.Pool over 500-organism chunks, ppanggolin.py:1039-1095) with the devices in the role of
   the pool's workers: the lock-step groups are dealt round-robin over `devices` (nemgpu_deal_groups; an entry may
   repeat), every device runs its share on a thread of its own with its own worker threads (workers / n_devices each),
   streams, lock-step contexts and resource pool.  Every problem's result equals its own nemgpu_run. */
int nemgpu_solve_many_devices(nemgpu_problem* problems, int count, const nemgpu_config* cfg, const int* devices, int n_devices,
                              int workers, int group);
/* slot_of_problem[i] = index into the device list of the device that solves problem i (host arithmetic only) */
int nemgpu_deal_groups(int count, int group, int n_devices, int* slot_of_problem);

/* ---- The chunks of partition()'s voting loop, formed on the device ----------------------------------------------
   The reference solves a pangenome of more than 500 organisms as many NEM problems, each on a random sample of the
   organisms (ppanggolin.py:1045-1086: `orgs = sample(organisms, chunck_size)`), and writes every sample's input files
   from ONE graph (__write_nem_input_files, ppanggolin.py:821-930): columns = the sampled organisms in sample order
   (:850); families without a sampled organism dropped, the others numbered in the graph's order (:849-852); an edge's
   weight = its coverage, the SUM over the sampled organisms of the adjacency's occurrence count in that organism
   (graph[a][b][org], which __add_link increments, :451; for a directed graph sens + antisens, graph[a][b][org] +
   graph[b][a][org]), an edge of coverage 0 dropped (:866-878), a family's neighbours in the order the master lists them.
   nemgpu_master_create puts that ONE pangenome on the device: the presence/absence bit rows xbits[n][ceil(d/32)]
   (family-major, bit o of a row = organism o), the graph in CSR (nei_ptr[n + 1], nei_idx[nnz]) and, per directed edge,
   the bit set of the organisms that carry it (edge_bits[nnz][ceil(d/32)], count >= 1).  Such a bits-only master takes
   every count as 1: its weights are the reference's only where no adjacency occurs twice in an organism (no tandem
   duplicate, no repeated operon, no directed graph).  HOST memory, copied once. */
typedef struct nemgpu_master nemgpu_master;
int nemgpu_master_create(nemgpu_master** out, int device, int n, int d, const uint32_t* xbits, const int32_t* nei_ptr,
                         const int32_t* nei_idx, const uint32_t* edge_bits);
/* The same with the counts: count[e][o] = what the reference sums for (family i, neighbour nei_idx[e]) in organism o,
   whose presence bit edge_bits holds (count >= 1).  Only the pairs with count >= 2 are listed, in CSR over the directed
   edges: extra_ptr[nnz + 1] (from 0, non-decreasing), extra_org[extra_ptr[nnz]] (per edge strictly increasing, in
   [0, d), set in that edge's edge_bits), extra_count[extra_ptr[nnz]] (>= 2).  The coverage of edge e in a sample =
   popc(edge_bits[e] & sample) + the sum of (count - 1) over e's listed organisms in the sample.  An edge's total count
   over all organisms may not exceed 2^24 (its weight stays exact in float).  Every argument is checked on the host
   before any HIP call (NEMGPU_E_ARG, nemgpu_last_error says why).  extra_ptr NULL, or no pair listed: exactly
   nemgpu_master_create. */
int nemgpu_master_create_counts(nemgpu_master** out, int device, int n, int d, const uint32_t* xbits, const int32_t* nei_ptr,
                                const int32_t* nei_idx, const uint32_t* edge_bits, const int32_t* extra_ptr,
                                const int32_t* extra_org, const int32_t* extra_count);
/* The same master built ON THE DEVICE from the organisms' gene orders: exactly what nemgpu_master_create_counts makes of
   the graph that PPanGGOLiN's __neighborhood_computation (ppanggolin.py:463-530) builds from the same annotations, with
   no graph, no n x d byte matrix and no per-edge byte row on either side.  HOST arrays, copied once:
     genes[g]             the family id (0 <= id < f, the caller's numbering) of every gene in walk order: organisms in
                          the order of `annotations`, inside one its contigs, inside a contig its genes;
     contig_ptr[c + 1]    contig j is genes[contig_ptr[j] .. contig_ptr[j + 1]) (from 0 to g, non-decreasing);
     contig_org[c]        the contig's organism = its column of the master (< d; walk order is array order);
     contig_circular[c]   0 / 1;     repeated[f]: 0 / 1 per family id (families_repeted), or NULL;
     directed             0: nx.Graph (what PPanGGOLiN's CLI builds), 1: nx.DiGraph.
   A gene of a repeated family does not exist (links bridge over it); master family i is the i-th family id in the order
   of first kept gene (nemgpu_master_fetch's `order`), a family without a kept gene is not in the master; every kept
   gene but its contig's first links (its family, the previous kept gene's family, organism), a circular contig then
   (first kept, last kept, organism), also with one or two kept genes; counts as __add_link makes them; a family's
   neighbours in nx.all_neighbors order (chunks.master_arrays_from_graph's docstring is the rule).  Every argument is
   checked on the host before any HIP call (NEMGPU_E_ARG, nemgpu_last_error says why); g + c < 2^30; 2 bits(n) + bits(d)
   <= 63; the limits of nemgpu_master_create_counts.  The master is destroyed by nemgpu_master_destroy. */
int nemgpu_master_create_orders(nemgpu_master** out, int device, int d, int f, int directed, const int32_t* genes, int g,
                                const int32_t* contig_ptr, const int32_t* contig_org, const uint8_t* contig_circular, int c,
                                const uint8_t* repeated);
/* A master GROWN by new organisms on the device: PPanGGOLiN.add_organism (ppanggolin.py:342-358), which keeps the graph
   and walks only the new organisms (__neighborhood_computation(update=new_orgs), :463-530).  *out is a new master on
   m's device (its own allocation and stream) = m + the gene orders of the new organisms alone; m is only read and stays
   valid (a nemgpu_votes made for it or a nemgpu_solve_chunks running on it is not disturbed; the caller destroys it).
   m's arrays do not cross PCIe: the update's orders and m's numbering (4 n bytes) go up, the new sizes come back.
     d_new                the new organisms: columns d .. d + d_new - 1 behind m's d;
     f                    the caller's id space now (>= the f the master was made with; made from arrays: >= n, family i
                          is id i);     genes / contig_ptr / contig_circular as nemgpu_master_create_orders takes them;
     contig_org[c]        ABSOLUTE columns, in [d, d + d_new);
     repeated[f]          families_repeted as the caller holds it after add_organism (the union), or NULL.
   The rules are nemgpu_master_create_orders', undirected, on the update's genes, and nx.Graph's on what is there:
   an id the master has keeps its number (one repeated only from now on keeps its node and old edges; its new genes do
   not exist and are bridged over), the other ids with a kept gene are numbered n, n + 1, ... in order of first kept
   gene (ids below the old f that never had a kept gene among them); an existing (row, neighbour) keeps its place in its
   row, a new one goes behind the row's old entries in order of first occurrence in the update (nx.all_neighbors after
   add_edge); count[entry][new organism] = its half-edges, >= 1 sets the bit in edge_bits (stride now ceil((d + d_new) /
   32), old words copied, bits above an old row's organism d - 1 dropped), >= 2 lists count behind the entry's old extras;
   the presence rows are re-strided, new families absent from the old organisms.  With the same `repeated` for both
   parts, appending B to the master of A is nemgpu_master_create_orders of A + B, array for array.
   Refused on the host before any HIP call (NEMGPU_E_ARG, nemgpu_last_error says why): malformed orders (create's
   rules), f below the master's, a contig_org outside [d, d + d_new), d_new <= 0, more than 131 072 organisms in all, a
   master built with directed = 1 (a row's predecessor / successor order cannot be recovered from summed counts: rebuild),
   a bits-only master of nemgpu_master_create (its counts are not known).  After numbering: 2 bits(n') + bits(d') <= 63;
   an edge's old + new count may not exceed 2^24 (checked on the device, reported as create reports it).
   A master made from arrays (nemgpu_master_create_counts) is taken as an undirected graph: a SYMMETRIC CSR (entry
   (a, b) iff entry (b, a), equal counts) is the caller's contract and is not checked. */
int nemgpu_master_append_orders(nemgpu_master** out, const nemgpu_master* m, int d_new, int f, const int32_t* genes, int g,
                                const int32_t* contig_ptr, const int32_t* contig_org, const uint8_t* contig_circular, int c,
                                const uint8_t* repeated);
/* Two masters MERGED on the device: PPanGGOLiN's `+=` (__iadd__, ppanggolin.py:368-391, "add a pangenome to this
   pangenome"), which throws the graph away and walks every annotation of both pangenomes again.  *out is a new master on
   a's device (its own allocation and stream) = the union of the two graphs as nx.Graph would hold it had b's organisms
   been walked after a's; a and b are only read and stay valid (a nemgpu_votes made for them or a nemgpu_solve_chunks
   running on them is not disturbed; the caller destroys them).  Neither master's arrays cross PCIe: b's family ids and
   a's numbering go up, the new sizes and the new families' ids come back.
     ids_b[b's n]         HOST: the id of b's family j in a's id space, distinct, in [0, f); NULL: b's own numbering
                          (nemgpu_master_fetch's `order`), that is, one id space shared by both;
     f                    the id space of the merged master (>= the f a was made with, above every id of b).
   Organisms: a's columns, then b's as d_a .. d_a + d_b - 1.  Families: a's keep their numbers, b's whose id a lacks are
   numbered n_a, n_a + 1, ... in b's order.  Rows: an entry of a keeps its place; an entry of b that a lacks goes behind
   the row's entries of a, in the order b's row lists them; a self-loop stays one entry.  Per entry: edge_bits (stride
   ceil((d_a + d_b) / 32)) = a's words, the bits above organism d_a - 1 dropped, OR b's bits shifted up by d_a bits; the
   extras a's, then b's with organism + d_a; counts unchanged.  Presence: a's rows re-strided, b's with their family bits
   permuted.  chunks.master_arrays_merge states it in numpy.  With the same `repeated` for both parts, merging the master
   of B into the master of A is nemgpu_master_create_orders of A + B, array for array; a family repeated in one part
   alone keeps the node and the edges the other part gave it (nemgpu_master_append_orders' rule).
   Refused on the host before any HIP call (NEMGPU_E_ARG, nemgpu_last_error says why): f <= 0, a master built with
   directed = 1 or a bits-only master on either side, masters on different devices, f below a's id space or not above
   every id of b, an id of b out of range or used twice, more than 131 072 organisms in all.  After the numbering:
   2 bits(n) + bits(d) <= 63 (the merged master stays one that nemgpu_master_append_orders accepts); after the plan: at
   most 2^31 - 1 entries and extras; an entry's count in a + its count in b may not exceed 2^24 (checked on the device,
   reported as create reports it).  out, a or b NULL: NEMGPU_E_FUNCARG. */
int nemgpu_master_merge(nemgpu_master** out, const nemgpu_master* a, const nemgpu_master* b, const int32_t* ids_b, int f);
/* A partition PROJECTED onto the organisms from the master: what PPanGGOLiN.projection (ppanggolin.py:1698-1755; the
   CLI's -pr; the first step of partition_shell(Q = "auto"), :1190-1192) counts and writes, as arrays, with no graph and
   no per-gene loop on the host.  HOST arrays; m is only read and stays valid and unchanged; the work runs on m's stream
   (as nemgpu_master_fetch does: not next to another call on the same master from another thread).
     part[n]              every master family's class in the vote's codes: P 0, S 1, C 2, U 3 (nemgpu_votes_result's final);
     f, genes[g], contig_ptr[c + 1], contig_org[c], repeated[f] or NULL
                          the gene orders of the organisms to project as nemgpu_master_create_orders takes them (no
                          contig_circular): contig_org are m's columns, any subset of them in any order, an organism's
                          contigs need not be adjacent; ids in the numbering m was made with (nemgpu_master_fetch's
                          `order`); g = 0 (and c = 0) is allowed.
   Outputs, any may be NULL:
     gene_family[g]       the master family of every gene; -1 for a gene of a repeated family (projection() skips it,
                          :1719); -2 for an id that no master family has (the reference would raise KeyError).  The
                          other genes are KEPT;
     gene_copies[g]       for a kept gene the kept genes of its family in its organism among the contigs given
                          (len(node[family][organism]), :1731); 0 for the others;
     nei_counts[n][3]     per master family the entries of its CSR row whose neighbour is of class P, S, C
                          (nx.all_neighbors of an nx.Graph, :1723: a self-loop is one entry; class U counts nowhere);
     org_counts[d][7]     per master column over that organism's kept genes: persistent, shell, cloud, undefined (the
                          family's class), core_exact (the family is present in all d organisms of m) or accessory
                          (partition_exact, :1143-1148), pangenome (every kept gene); 0 for the organisms not given.
   All integer: the results do not depend on the order of the device's additions.
   Refused on the host before any launch (NEMGPU_E_ARG, nemgpu_last_error says why): malformed orders (create's rules:
   ids in [0, f), contig_ptr monotone from 0 to g, contig_org in [0, d), g + c < 2^30), a part value above 3, a master
   built with directed = 1 (nx.all_neighbors of a DiGraph lists a family that is both predecessor and successor of the
   node twice, the master's row holds it once with the summed count: the reference's neighbour counts cannot be
   recovered from it).  m == NULL: NEMGPU_E_FUNCARG. */
int nemgpu_master_project(const nemgpu_master* m, const uint8_t* part, int f, const int32_t* genes, int g,
                          const int32_t* contig_ptr, const int32_t* contig_org, int c, const uint8_t* repeated,
                          int32_t* org_counts, int32_t* nei_counts, int32_t* gene_family, int32_t* gene_copies);
/* The per-family TABLE of the pangenome matrix (PPanGGOLiN.write_matrix, ppanggolin.py:1400-1452: the Roary-style .csv
   and .Rtab), computed on the device from the master and the flat orders of ALL its organisms, and the .Rtab's cell
   block formatted there.  HOST arrays; m is only read and stays valid and unchanged; the work runs on m's stream.
     f, genes[g], contig_ptr[c + 1], contig_org[c], repeated[f] or NULL
                          the gene orders as nemgpu_master_project takes them (g > 0);
     gene_len[g]          END - START of every gene, what __add_gene receives (:497, :511); any int32.
   A gene of a repeated family is skipped, as in the build.  Per master family i (caller id order[i]):
     nb_genes[n]          its kept genes (node["nb_genes"], :418);      nb_org[n]  the organisms with at least one;
     len_min, len_max, len_distinct[n], len_sum[n] (int64)
                          over the DISTINCT lengths of its kept genes (node["length"] is a set, :426-430; min, max and
                          mean are taken over it, :1431, :1443-1445);
     multi_ptr[n + 1], multi_org[n_multi], multi_cnt[n_multi]
                          the (family, organism) cells whose copy count len(node[org]) (:1429) is 2 or more, in CSR
                          over the families, the organisms increasing per family; every other cell's count is its
                          presence bit in the master.
   The cells derived from the orders must equal the master's presence bits, every cell, both directions (checked on the
   device); if not -- the orders are not this master's; also a kept gene whose family the master lacks -- the call returns
   NEMGPU_E_ARG with nemgpu_last_error's text and makes no table.  Malformed orders are refused on the host before any
   launch by nemgpu_master_project's rules.  A master built with directed = 1 is fine: the adjacency is not read.
   The table stays on the device until nemgpu_family_table_destroy; it does not keep m alive.
   _rtab_size: the bytes of the text of families row0 .. row0 + rows - 1.
   _rtab: that text into text[capacity] (HOST): per family the d copy counts in decimal joined by '\t', then '\n' -- what
   the reference writes after column 14 of a line of the .Rtab -- and every line's end offset in line_end[rows];
   *needed (may be NULL) = the bytes the batch takes.  capacity below that: NEMGPU_E_ARG, *needed still set, nothing
   written.  m: the table's master. */
typedef struct nemgpu_family_table nemgpu_family_table;
int nemgpu_family_table_create(nemgpu_family_table** out, const nemgpu_master* m, int f, const int32_t* genes, const int32_t* gene_len,
                               int g, const int32_t* contig_ptr, const int32_t* contig_org, int c, const uint8_t* repeated);
int nemgpu_family_table_shape(const nemgpu_family_table* t, int* n, int* d, int* n_multi);
int nemgpu_family_table_fetch(const nemgpu_family_table* t, int32_t* nb_genes, int32_t* nb_org, int32_t* len_min, int32_t* len_max,
                              int32_t* len_distinct, int64_t* len_sum, int32_t* multi_ptr, int32_t* multi_org, int32_t* multi_cnt);
int nemgpu_family_table_rtab_size(const nemgpu_family_table* t, int row0, int rows, int64_t* bytes);
int nemgpu_family_table_rtab(nemgpu_family_table* t, const nemgpu_master* m, int row0, int rows, char* text, int64_t capacity,
                             int64_t* needed, int64_t* line_end);
void nemgpu_family_table_destroy(nemgpu_family_table* t);
/* The per-edge TABLE of the pangenome graph's GEXF export (PPanGGOLiN.export_to_GEXF, ppanggolin.py:1294-1362), computed
   on the device from the master and the flat orders of ALL its organisms, and the edges' organism <attvalue> lines
   formatted there.  HOST arrays; m is only read and stays valid and unchanged; the work runs on m's stream.
     f, genes[g], contig_ptr[c + 1], contig_org[c], repeated[f] or NULL
                          the gene orders as nemgpu_family_table_create takes them (g > 0), contig_org non-decreasing:
                          the organisms walked in column order;
     gene_start[g], gene_end[g]   the annotation's START and END;
     contig_size[c]       a circular contig's size (circular_contig_size), -1 for a linear contig.
   The links are the build's (__neighborhood_computation, :485-520): a kept gene and the previous kept gene of its
   contig, length START[gene] - END[previous]; per circular contig its first and last kept gene, length
   (size - END[last]) + START[first]; lengths in 64 bits, one outside int32 (a gene's END - START too) is refused.  The
   edges are the master's CSR entries with idx >= row, in CSR order: neighbors_graph.edges() of an nx.Graph.  Per edge:
     src, dst[E]          its families;          weight[E]  the organisms that carry it;
     len_min, len_max, len_distinct[E], len_sum[E] (int64), len_mid_lo, len_mid_hi[E]
                          over the DISTINCT lengths of its links (data["length"] is a set, :456-459): the two middle
                          elements of the sorted distinct lengths (equal when their number is odd) give the median;
   per family  fam_mid_lo, fam_mid_hi[n]  the same middles over the distinct lengths END - START of its kept genes;
   per organism  org_first_edge[d]  the first edge, in edge order, that carries it (E: none).
   The (edge, organism, count) triples derived from the links must equal the master's edge bits and extras, every one,
   both directions (a bits-only master: the bits alone); if not -- the orders are not this master's -- the call returns
   NEMGPU_E_ARG with nemgpu_last_error's text and makes no table.  Malformed orders are refused on the host before any
   launch; so is a master built with directed = 1.  The table does not keep m alive.
   _attvalues_size: the bytes of the text of edges row0 .. row0 + rows - 1 for these attribute ids (attr_id[d] >= 0).
   _attvalues: that text into text[capacity] (HOST): per edge, per organism on it in increasing column order, the line
   `          <attvalue for="ID" value="COUNT" />\n` (ten spaces; ID = attr_id[organism], COUNT the pair's count), and
   every edge's end offset in edge_end[rows]; *needed (may be NULL) = the bytes the batch takes.  capacity below that:
   NEMGPU_E_ARG, *needed still set, nothing written.  m: the table's master. */
typedef struct nemgpu_edge_table nemgpu_edge_table;
int nemgpu_edge_table_create(nemgpu_edge_table** out, const nemgpu_master* m, int f, const int32_t* genes, const int32_t* gene_start,
                             const int32_t* gene_end, int g, const int32_t* contig_ptr, const int32_t* contig_org, const int32_t* contig_size,
                             int c, const uint8_t* repeated);
int nemgpu_edge_table_shape(const nemgpu_edge_table* t, int* n, int* d, int* n_edges);
int nemgpu_edge_table_fetch(const nemgpu_edge_table* t, int32_t* src, int32_t* dst, int32_t* weight, int32_t* len_min, int32_t* len_max,
                            int32_t* len_distinct, int64_t* len_sum, int32_t* len_mid_lo, int32_t* len_mid_hi, int32_t* fam_mid_lo,
                            int32_t* fam_mid_hi, int32_t* org_first_edge);
int nemgpu_edge_table_attvalues_size(nemgpu_edge_table* t, const nemgpu_master* m, const int32_t* attr_id, int row0, int rows, int64_t* bytes);
int nemgpu_edge_table_attvalues(nemgpu_edge_table* t, const nemgpu_master* m, const int32_t* attr_id, int row0, int rows, char* text,
                                int64_t capacity, int64_t* needed, int64_t* edge_end);
/* The organisms' METADATA on the edges (export_to_GEXF's metadata=, ppanggolin.py:1339-1354): per edge and attribute the
   sorted set of the values of the organisms that carry the edge, joined by `|`.  The caller ranks every attribute's
   distinct values in sorted order and escapes them; the device ORs one-hot(rank) over an edge's organisms and writes
   the values present in increasing rank.
   _metadata: gives the table its metadata, uploaded once and kept until the next _metadata call or _destroy.  HOST:
     n_attr > 0;  attr_id[n_attr] >= 0   the attributes' ids, in the order their lines are written;
     value_rank[n_attr][d]   every organism's value as its rank in [0, n_values[a]);
     n_values[n_attr]        the attribute's distinct values, 1 .. 65536 (an edge's mask of one attribute is built in
                             8 KiB of LDS per wave);
     value_ptr[V + 1], value_text   V = the sum of n_values: the bytes of value (a, rank) are value_text[value_ptr[v]
                             .. value_ptr[v + 1]) with v = n_values[0] + .. + n_values[a - 1] + rank; value_ptr starts at 0
                             and ascends (an empty value is a value); value_ptr[V] + V <= 2^30.  A single value's length
                             has no bound of its own: no value is staged.
   Anything outside that is refused with NEMGPU_E_ARG before any launch, and the table keeps the metadata it had.
   _metamasks: for edges row0 .. row0 + rows - 1 the present-value bit masks into masks[rows][W] (HOST), W = the sum over
   the attributes of ceil(n_values[a] / 32): an edge's words are the attributes' one after the other, bit (rank & 31) of
   word (rank >> 5) set where an organism of the edge has that value.
   _metavalues_size / _metavalues: as _attvalues_size / _attvalues, the same contract (*needed always set, a capacity
   below it NEMGPU_E_ARG and nothing written): per edge, per attribute in order, the line
   `          <attvalue for="ID" value="V1|V2|..." />\n`.  m is only read; the work runs on m's stream, its scratch is
   allocated for the call and freed.  Without metadata these three return NEMGPU_E_ARG. */
int nemgpu_edge_table_metadata(nemgpu_edge_table* t, int n_attr, const int32_t* attr_id, const int32_t* value_rank, const int32_t* n_values,
                               const int64_t* value_ptr, const char* value_text);
int nemgpu_edge_table_metamasks(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, uint32_t* masks);
int nemgpu_edge_table_metavalues_size(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, int64_t* bytes);
int nemgpu_edge_table_metavalues(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, char* text, int64_t capacity, int64_t* needed,
                                 int64_t* edge_end);
void nemgpu_edge_table_destroy(nemgpu_edge_table* t);
/* The NODES' <attvalue> lines of the same export, formatted on the device from the master, the flat orders of ALL its
   organisms and every gene's ID, NAME and PRODUCT given as (offset, length) spans of the load's text (the loader's
   SPAN_ID, SPAN_NAME, SPAN_PRODUCT; an absent NAME or PRODUCT is an empty span).  gexf.node_text_host (Python) states the
   bytes.  HOST arrays; m is the table's master in every call, only read; the work runs on m's stream, scratch is
   allocated for the call and freed.
   _create: f, genes[g], contig_ptr[c + 1], contig_org[c], repeated[f] or NULL as nemgpu_edge_table_create takes them
     (g > 0, at most (2^31 - 1) / 3; contig_org non-decreasing).  A gene is kept when its id is not flagged.  The kept
     genes' (family, organism) cells must be exactly the master's presence bits: if not, NEMGPU_E_ARG and no table.
     hash_bits (tests): 0, or the bits of the string hash that are kept, so that the probes collide.
   _text: once per batch of genes gene0 .. gene1 - 1, in order from 0 to g: text[bytes] is the part of the load's text the
     batch's spans lie in (a run of whole files), span_off[3][gene1 - gene0] offsets into it, span_len[3][gene1 - gene0]
     (ID, NAME, PRODUCT; a length at most 2^24).  A span past the end of the text is refused before any launch.  The
     device keeps the spans of the kept genes, escaped as ElementTree escapes an attribute, and not the text.
   _finish: after the last batch: the distinct names and products of every family (equal bytes), each at its first
     gene in walk order.
   _shape, _fetch: n, d, g; nb_genes[n] the families' kept genes, org_first_node[d] the first family, in master order,
     with a kept gene of the organism (n: none).  Either may be NULL.
   _ids: numbers the node attributes as networkx does when `tail` titles follow a node's organisms (partition,
     partition_exact, [the subpartition,] the four length_*): nb_genes 0, node 0's first organism, name, product, node
     0's other organisms, the tail, then every organism first met at a later node in (node, organism) order; in the
     light export nb_genes 0, name 1, product 2.  org_id[d] (-1: the organism has no kept gene), name_id[2] (light,
     full; product's is one more), node_end_full[n], node_end_light[n]: every node's end offset in the text of all
     nodes.  Any may be NULL.  The text calls format for the last numbering.
   _lines_size, _lines: the text of nodes row0 .. row0 + rows - 1 into text[capacity] (HOST): per node one slice -- full:
     the first organism's line, the name line, the product line, the other organisms' lines; light (full = 0): the name
     and product lines -- each line `          <attvalue for="ID" value="A|B|..." />\n`; node_end[rows]: every node's
     end offset in the batch; *needed (may be NULL) = the bytes the batch takes; capacity below that: NEMGPU_E_ARG,
     *needed still set, nothing written. */
typedef struct nemgpu_node_table nemgpu_node_table;
int nemgpu_node_table_create(nemgpu_node_table** out, const nemgpu_master* m, int f, const int32_t* genes, int g, const int32_t* contig_ptr,
                             const int32_t* contig_org, int c, const uint8_t* repeated, int hash_bits);
int nemgpu_node_table_text(nemgpu_node_table* t, const nemgpu_master* m, const char* text, int64_t bytes, int gene0, int gene1,
                           const int64_t* span_off, const int32_t* span_len);
int nemgpu_node_table_finish(nemgpu_node_table* t, const nemgpu_master* m);
int nemgpu_node_table_shape(const nemgpu_node_table* t, int* n, int* d, int* g);
int nemgpu_node_table_fetch(const nemgpu_node_table* t, int32_t* nb_genes, int32_t* org_first_node);
int nemgpu_node_table_ids(nemgpu_node_table* t, const nemgpu_master* m, int tail, int32_t* org_id, int32_t* name_id, int64_t* node_end_full,
                          int64_t* node_end_light);
int nemgpu_node_table_lines_size(const nemgpu_node_table* t, int full, int row0, int rows, int64_t* bytes);
int nemgpu_node_table_lines(nemgpu_node_table* t, const nemgpu_master* m, int full, int row0, int rows, char* text, int64_t capacity,
                            int64_t* needed, int64_t* node_end);
void nemgpu_node_table_destroy(nemgpu_node_table* t);
/* The pangenome graph LAID OUT on the device: PPanGGOLiN.compute_layout (ppanggolin.py:1250-1292), which hands the
   family graph to ForceAtlas2 (Jacomy et al. 2014) and puts the positions on the nodes.  The reference delegates to the
   external package fa2 (Barnes-Hut at theta 1.2); here the repulsion is the EXACT all-pairs sum, n^2 per iteration
   (nemgpu_layout_create_bh below: a Barnes-Hut sum), and
   what is computed is stated in numpy by pangenomenem_amd/layout.py's layout_arrays: no equality with fa2 is claimed.
   From the master (only read, and not needed after _create returns): an edge is a CSR entry with idx > row, its weight
   the popcount of the entry's bit row; a self-loop attracts nothing; mass[i] = 1 + the entries of row i.  A bits-only
   master is fine (the weights are popcounts); n = 0 gives an empty layout.
     cfg     compute_layout's parameters; lin_log, adjust_sizes and strong_gravity == 0 are refused;
     pos     the start positions, double [n][2], finite.
   float64 throughout, IEEE division and square root, no float atomics: every term is the statement's, bit for bit, only
   the order of the sums is the device's own (the slices of a node's j range in order, a row's entries in order, fixed
   trees for S and T), so a result is a function of the inputs alone.  Positions, forces and the speed control's state
   stay on the device: _run(3) then _run(2) is _run(5).  _run enqueues `iterations` iterations on the layout's stream and
   does not wait for them; _fetch does.
   _fetch: pos [n][2], forces [n][2] (the last iteration's), state [5] = speed, eff (the speed efficiency), S, T (the
   last iteration's global swinging and traction), iterations done; any may be NULL.
   Refused on the host before any launch (NEMGPU_E_ARG, nemgpu_last_error says why): the modes above, a parameter or a
   start position that is not finite, iterations < 0, a master built with directed = 1 (a DiGraph's weight is per
   direction, the master holds only the sum).
   _slices: the slices a node's j range is cut into for n families (a function of n alone), the repulsion kernel's tile
   width and the least slice length; host only. */
typedef struct nemgpu_layout nemgpu_layout;
typedef struct {
    double scaling_ratio;                 /* 50000 */
    double gravity;                       /* 1 */
    double edge_weight_influence;         /* 1; 0: every edge counts 1; else weight ** influence */
    double jitter_tolerance;              /* 1 */
    int strong_gravity;                   /* 1 (0 is refused) */
    int outbound_attraction_distribution; /* 1 */
    int lin_log, adjust_sizes;            /* 0 (anything else is refused) */
} nemgpu_layout_config;
int nemgpu_layout_create(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos);
int nemgpu_layout_run(nemgpu_layout* l, int iterations);
int nemgpu_layout_fetch(nemgpu_layout* l, double* pos, double* forces, double* state);
void nemgpu_layout_destroy(nemgpu_layout* l);
int nemgpu_layout_slices(int n, int* tile, int* slice_grain);
/* The same layout with the repulsion as a BARNES-HUT sum, what compute_layout asks of fa2 (barnesHutOptimize=True,
   barnesHutTheta=1.2): O(n log n) per iteration.  The tree is this project's own, stated rule by rule in numpy by
   pangenomenem_amd/layout_bh.py (tree_arrays, walk, layout_bh_arrays) -- a square around the bodies, 32-bit Morton keys
   on a 2^16 grid, the bodies sorted by (key, index), a cell per run of equal key prefix under a run of more than LEAF
   bodies, moments summed left to right, a depth-first walk that accepts an inner cell not holding the body iff
   theta^2 d2 > size^2 -- and the device is held to it bit for bit: keys, order, cells, moments and every force; only the
   order of S and T is the device's.  How fa2 splits its regions and sizes them could not be checked: no equality with
   fa2 is claimed.  nemgpu_layout_create and its exact sum stay the default; this is the opt-in.
   _create_bh: nemgpu_layout_create's arguments and theta >= 0, finite (0: every cell is opened, the exact pair set in
   tree order).  The same handle: _run, _fetch and _destroy work on it.  Refused on the host before any HIP call
   (NEMGPU_E_ARG, nemgpu_last_error says why): a theta that is negative or not finite, and all that _create refuses.
   Everything is allocated here, for the statement's bound on the cells, 1 + DEPTH min(n, 4 (n / (LEAF + 1))): _run only
   enqueues.
   _bh_shape: DEPTH and LEAF; host only.
   _bh_tree: the tree of the CURRENT positions, built and copied to host buffers, any of them NULL: *n_cells; box [3] = x0,
   y0, side; keys, order [n] in sorted order (order: sorted position -> family); level, lo, hi, M, Sx, Sy with room for
   the bound above (n_cells are written); accepted, visited [n] per family: the cells its walk accepted and the bodies
   of the leaves it opened.  It changes no state (a run continued after it gives the same bits) and waits for the
   layout's stream.  A layout made by nemgpu_layout_create is refused (NEMGPU_E_ARG). */
int nemgpu_layout_create_bh(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos, double theta);
int nemgpu_layout_bh_shape(int* depth, int* leaf);
int nemgpu_layout_bh_tree(nemgpu_layout* l, int* n_cells, double* box, uint32_t* keys, int32_t* order, int32_t* level, int32_t* lo, int32_t* hi,
                          double* M, double* Sx, double* Sy, int32_t* accepted, int32_t* visited);
/* The organisms CLUSTERED for the presence/absence plot: what the R script of PPanGGOLiN's CLI computes with
   hclust(dist(t(binary_matrix), method = "binary")) (command_line.py:57, :79) and the raster it draws (:84-101), from the
   master's presence bits; pangenomenem_amd/tileplot.py states every step in numpy.  m is only read (its presence rows;
   the adjacency is not: a bits-only master and one built with directed = 1 are fine) and MUST OUTLIVE the handle, which
   reads its rows again in _cells; the work runs on m's stream.
   _create: the distances of all pairs of organisms, resident until _destroy as the full symmetric square double [d][d]
     (8 d^2 bytes): with A, B the family sets of organisms i, j, inter = |A & B|, uni = |A| + |B| - inter,
     dist = (double)(uni - inter) / uni, 0 where uni == 0 (R_dist_binary; both empty: 0; the diagonal is 0).  Exact
     integer counts and one IEEE division: no tolerance.  d <= 32768 (_tile_info's max_organisms); more is refused
     before any allocation.
   _distances: rows i0 .. i0 + rows - 1 of the square into out[rows][d] (HOST).
   _run: R's hclust(method = "complete") as Murtagh's nearest-neighbour algorithm (hclust.f; tileplot.
     hclust_complete_host is the statement, ties included: every minimum is found with a strict <, the lowest index
     wins): merge s joins the clusters of organisms i2[s] < j2[s] (the merged cluster goes on under i2[s], j2[s] is
     retired) at height[s]; d - 1 merges (HOST arrays of d - 1; d == 1: nothing is written, they may be NULL).
     The merges run on a copy (another 8 d^2 bytes, for the call): _distances gives the same rows afterwards.  The loop
     runs on the device without a host round trip per merge.
   _cells: the raster's rows row0 .. row0 + rows - 1 into out[rows][d] (HOST, uint8 0 / 1): cell (r, c) = family
     fam_order[row0 + r] present in organism org_order[c].  fam_order[n] and org_order[d] are permutations.
   _tile_info: the distance kernel's tile (organisms per side), the 64-bit words of a row it stages per step, and the
     most organisms _create takes; host only; any may be NULL.
   NEMGPU_E_ARG before any launch (nemgpu_last_error says why): a NULL pointer, rows out of range (rows <= 0 too), an
   order that is not a permutation, d above the limit. */
typedef struct nemgpu_orgclust nemgpu_orgclust;
int nemgpu_orgclust_create(nemgpu_orgclust** out, const nemgpu_master* m);
int nemgpu_orgclust_shape(const nemgpu_orgclust* h, int* n, int* d);
int nemgpu_orgclust_distances(const nemgpu_orgclust* h, int i0, int rows, double* out);
int nemgpu_orgclust_run(nemgpu_orgclust* h, int32_t* i2, int32_t* j2, double* height);
int nemgpu_orgclust_cells(nemgpu_orgclust* h, const int32_t* fam_order, const int32_t* org_order, int row0, int rows, uint8_t* out);
void nemgpu_orgclust_destroy(nemgpu_orgclust* h);
int nemgpu_orgdist_tile_info(int* tile, int* chunk_words, int* max_organisms);
/* What a master holds, of whichever constructor: sizes (n families, d organisms, nnz CSR entries, n_extra pairs with
   count >= 2; any pointer may be NULL), and the arrays as nemgpu_master_create_counts takes them, read back from the
   device: xbits[n][ceil(d/32)], nei_ptr[n + 1], nei_idx[nnz], edge_bits[nnz][ceil(d/32)], extra_ptr[nnz + 1],
   extra_org[n_extra], extra_count[n_extra], order[n] (master family i = caller id order[i]; 0, 1, ... for a master
   made from arrays).  HOST buffers; any may be NULL. */
int nemgpu_master_shape(const nemgpu_master* m, int* n, int* d, int* nnz, int* n_extra);
int nemgpu_master_fetch(const nemgpu_master* m, uint32_t* xbits, int32_t* nei_ptr, int32_t* nei_idx, uint32_t* edge_bits,
                        int32_t* extra_ptr, int32_t* extra_org, int32_t* extra_count, int32_t* order);
void nemgpu_master_destroy(nemgpu_master* m);
/* One sample.  in: organisms[dc] (indices into the master's, the chunk's column order).  out: n = families with at least
   one sampled organism, nnz = directed edges of the chunk's graph; optional arrays (NULL: not wanted): keep[ceil(n_master
   / 64)] (bit i: master family i is in the chunk -- the chunk's family j is the j-th set bit), labels[n] (NCEM: class of
   the chunk's family j; room for n_master bytes), out_prop[k], out_center[k][dc], out_disp[k][dc], out_nbobs_k[k]. */
typedef struct {
    const int32_t* organisms;
    int dc;
    int n, nnz;
    uint64_t* keep;
    uint8_t* labels;
    float *out_prop, *out_center, *out_disp, *out_nbobs_k;
    nemgpu_result result;
    int rc;
} nemgpu_chunk;
/* All samples in ONE call: the device decides which families and edges each sample keeps (one pass over all samples,
   one wait), then every sample goes through nemgpu_solve_many's pipeline -- `workers` builder threads, lock-step groups
   of `group` problems, results unpacked while later groups are built -- with its matrix rows, lane order and graph
   written by the device straight into its engine's buffers: per sample only the initial parameters (k values per kind:
   prop[k], and ONE centre and ONE dispersion per class for every organism, as PPanGGOLiN's default .m has them,
   ppanggolin.py:893-901) and the results cross PCIe.  Every sample's result equals nemgpu_solve_many on the same
   sample formed on the host (tests/test_gpu_chunks.py). */
int nemgpu_solve_chunks(nemgpu_master* m, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                        const float* disp_k, const nemgpu_config* cfg, int workers, int group);

/* ---- The sub-problem of a selection of families (partition_shell) ------------------------------------------------
   partition_shell (ppanggolin.py:1175-1248, the CLI's -ss) solves the NEM problem of the shell families alone:
   `__write_nem_input_files(dir, organisms, init, filter_by_partition="shell")` keeps the nodes whose partition is
   "shell" (:844), in node order, and runs INIT_RANDOM (50 starts) or a parameter file on them.
   nemgpu_master_subproblem forms that problem on the device from the resident master and hands back an ENGINE of
   n x dc and k classes that holds it: organisms[dc] are the columns (distinct indices of the master's organisms),
   select_bytes[n_master] the selection (non-zero: selected; packed to bits on the device).  A family is kept iff it is
   selected and present in one of the organisms; families_out[n] (room for n_master; may be NULL) lists the kept
   families' master indices, *n and *nnz the problem's sizes.  edge_rule:
     0, induced:   an edge is kept iff its coverage over the organisms is positive and both ends are kept (the writer's
                   evident intent: what it writes, unfiltered, for neighbors_graph.subgraph(shell));
     1, reference: the writer as written.  Its test at :859 is inverted: a neighbour that IS shell is skipped, one that
                   is NOT reaches index_fam[neighbor] without an entry (KeyError).  No edge is kept; when a kept family
                   has an entry of positive coverage to a family that is not selected, *outside_entry is the smallest
                   such CSR entry of the master, NO engine is made (*engine stays NULL) and the call returns NEMGPU_OK:
                   the caller raises the KeyError naming nei_idx[*outside_entry].  Else *outside_entry is -1.
   The formed bit rows also come back into the engine's host rows, so that nemgpu_run_random (which draws its centres
   from them), nemgpu_set_params + nemgpu_run and nemgpu_get_results work on the engine as on any other; the caller
   configures it, runs it and destroys it (nemgpu_destroy).  The master is only read.
   NEMGPU_E_ARG, before any launch: an organism out of range or given twice, k <= 0 or k > 32, a selection without a
   family, a master built directed (nx.all_neighbors of a DiGraph is not its row).  NEMGPU_E_ARG after phase 1: no
   selected family is present in the organisms.
   nemgpu_subproblem_fetch reads the formed problem back (HOST buffers; any may be NULL): xbits[n][ceil(dc/32)],
   ptr[n + 1], idx[nnz], w[nnz]. */
int nemgpu_master_subproblem(nemgpu_master* m, const int32_t* organisms, int dc, const uint8_t* select_bytes, int edge_rule, int k,
                             nemgpu_engine** engine, int32_t* families_out, int* n, int* nnz, int* outside_entry);
int nemgpu_subproblem_fetch(nemgpu_engine* e, uint32_t* xbits, int32_t* ptr, int32_t* idx, float* w);

/* ---- The vote of partition()'s loop over the samples ----------------------------------------------------------
   partition() (ppanggolin.py:1015-1105) counts, per family of the pangenome, the P/S/C/U votes of the samples' runs
   (run_partitioning, :1886-1980: P/S/C if the class with the most non-zero centres is class 0 and the one with the
   largest sum of dispersions class 1, else everything U; a run that emptied a class: everything U), sample after sample.
   A family is validated by the vote that makes its total exceed len(organisms) / chunk_size with an absolute majority,
   or exceed len(organisms) (U is forced if it then has no majority); votes after validation still count.  The loop
   stops after the sample that validates the last family; the final class is the first largest count in the order
   P, S, C, U.  A nemgpu_votes holds those counts on the device for one master and one selection organisms[d_sel]
   (distinct indices into the master's organisms; the pangenome = the families with a selected organism). */
typedef struct nemgpu_votes nemgpu_votes;
int nemgpu_votes_create(nemgpu_votes** out, nemgpu_master* m, const int32_t* organisms, int d_sel, int chunk_size, int batch);
void nemgpu_votes_destroy(nemgpu_votes* v);
/* count <= batch samples solved as nemgpu_solve_chunks solves them (k = 3, NCEM; labels / out_* may be NULL) and voted
   in order on the device, straight from the runs' labels and parameters.  *stop_index: the sample of this call after
   which every family is validated (the samples after it are solved, not counted), or -1.  A sample that keeps no family
   votes nothing (rc NEMGPU_OK, n = 0).  An engine error is returned and nothing of the call is counted. */
int nemgpu_votes_solve(nemgpu_votes* v, nemgpu_chunk* chunks, int count, int k, const float* prop, const float* center_k,
                       const float* disp_k, const nemgpu_config* cfg, int workers, int group, int* stop_index);
/* Synthetic samples through the same vote: keep[count][ceil(n_master / 64)] (the kept families, as nemgpu_chunk.keep),
   labels[count][n_master] (label 0 .. 2 of the sample's kept family j at j), maps[count][3] (the code, 0 .. 3, that
   each label votes). */
int nemgpu_votes_add_host(nemgpu_votes* v, int count, const uint64_t* keep, const uint8_t* labels, const uint8_t* maps, int* stop_index);
/* The code map of `count` runs of k = 3 classes from their final parameters: center / disp = per sample [k][dc[s]],
   the samples one after another; status[s] = the run's status.  maps[count][3]. */
int nemgpu_vote_classmap_host(int count, int k, const int* dc, const float* center, const float* disp, const int* status, uint8_t* maps);
/* cnt[n_master][4] (votes P, S, C, U), final_code[n_master] (0 .. 3; 0xFF: not in the pangenome), validated[n_master]
   (the sample, counted over all calls, whose vote validated the family; -1: not validated), samples_voted.  Any may be
   NULL. */
int nemgpu_votes_result(nemgpu_votes* v, int32_t* cnt, uint8_t* final_code, int32_t* validated, int64_t* samples_voted);

/* PPanGGOLiN's evolution curve (command_line.py:262-281): count samples of the master solved as nemgpu_solve_chunks
   solves them (k = 3, NCEM), each reduced on the device to the stats of partition(just_stats=True):
   stats[count][6] = persistent, shell, cloud, undefined, core_exact, accessory.  labels / out_* of the chunks may be
   NULL (no label crosses PCIe then).  A sample that keeps no family is not solved: its stats are all 0, its rc
   NEMGPU_OK.  A sample is a set: an organism repeated in it, or out of range, is refused (NEMGPU_E_ARG) before anything
   is launched. */
int nemgpu_resamples_solve(nemgpu_master* m, nemgpu_chunk* chunks, int count, int k, const float* prop,
                           const float* center_k, const float* disp_k, const nemgpu_config* cfg, int workers,
                           int group, int32_t* stats);

/* Whole run from random starts (the reference's init_mode = INIT_RANDOM, RandNemAlgo nem_alg.c:1574-1742): n_starts
   starts (the reference uses 50), centres drawn from the data with the reference's generator -- glibc random()
   after srandom(seed), restated in csrc/nem_rng.hpp -- best start by criterion M, EstimPara on the best partition.
   With the same seed and tie-free data the result equals the reference's (which seeds with time(NULL)).
   best_start: 0-based index of the chosen start, -1 if every start ended with an empty class. */
int nemgpu_run_random(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start);
/* The same run with what the reference writes to <Fname>.log for INIT_RANDOM (nem_alg.c:1632-1636, 1662-1669: "Random
   initialization %d :", the start's line 0, then NemAlgo's line per iteration): `fn` is called on the calling thread for
   every event, in the reference's order -- start by start, though up to 64 starts run in lock step underneath (their
   lines are kept and handed over when the round is through; more starts, the `crit` convergence test or
   NEM_MI355X_BATCH_STARTS_LOGGED=0: one start after the other, events as they happen).  The pointers of an event are
   host arrays that are valid during the call only. */
typedef struct nemgpu_log_event {
    int kind;                     /* NEMGPU_LOG_START | _LINE | _EMPTY */
    int start;                    /* 0-based start */
    int iter;                     /* _LINE: 0 = the start's initial partition, else the iteration; _EMPTY: the iteration */
    int emptyk;                   /* _EMPTY: the class (1..K) */
    const float* crit_before;     /* _LINE: D,G,U,M,L,Z of the partition the E-step sweep started from (WriteLogCrit, :2361) */
    const float* crit_after;      /* _LINE: ... of the partition it left (:2398) */
    const float* prop;            /* _LINE: K */
    const float* center;          /* _LINE: K*D */
    const float* disp;            /* _LINE: K*D */
    const float* nbobs_k;         /* _LINE, iter > 0: K class sizes of this iteration's EstimPara; _EMPTY: EstimSizes'
                                     sizes of the partition that emptied a class (the next start's line 0 prints them,
                                     nothing resets NbObs_KD between starts); _LINE, iter 0: NULL */
} nemgpu_log_event;
enum { NEMGPU_LOG_START = 0, NEMGPU_LOG_LINE = 1, NEMGPU_LOG_EMPTY = 2 };
typedef void (*nemgpu_log_fn)(const nemgpu_log_event* ev, void* user);
/* nemgpu_run (INIT_PARAM_FILE: ComputePartitionFromPara + NemAlgo, nem_alg.c:1160, 1746-1879) with what the reference writes
   to <Fname>.log when dolog is set (WriteLogCrit, nem_alg.c:2361, 2398): `fn` gets a _LINE event for the initial partition
   (iter 0) and one per EM iteration, or _EMPTY for the iteration that emptied a class; `start` is 0.  The iterations run
   pipelined, seven per wait, and the criteria of a batch's iterations are evaluated together afterwards (NCEM with the
   `clas` / `none` tests; otherwise, or with NEM_MI355X_LOG_BATCHED=0, one iteration per wait as nemgpu_iterate_logged).
   res->crit: the criteria of the final partition when the last line carried them, else crit[0] = NaN (the caller asks
   nemgpu_criteria, after nemgpu_mstep + nemgpu_density if no iteration ran, nem_alg.c:1845-1852). */
int nemgpu_run_logged(nemgpu_engine* e, nemgpu_result* res, nemgpu_log_fn fn, void* user);
int nemgpu_run_random_logged(nemgpu_engine* e, int n_starts, uint32_t seed, nemgpu_result* res, int* best_start,
                             nemgpu_log_fn fn, void* user);
/* Test hook: the first `count` values random() returns after srandom(seed), from the restated generator. */
int nemgpu_glibc_random(uint32_t seed, int count, int32_t* out);

/* Step-level entry points (same kernels; used by tests, bench.py and the multi-GPU host driver). */
int nemgpu_init_partition(nemgpu_engine* e);              /* ComputePartitionFromPara(Needinit=1) */
int nemgpu_iterate(nemgpu_engine* e, int n_iters, nemgpu_result* res);  /* up to n_iters EM iterations */
int nemgpu_reset(nemgpu_engine* e);                       /* back to the initial parameters, zero partition */
/* One EM iteration -- or, with_init != 0, the start: reset + the two initial sweeps, no iteration -- plus what a line
   of the reference's log needs (the criteria of the partition the sweep started from and of the new one, the
   parameters), all in one stream submission and one wait (HOST buffers; the parameter pointers may be NULL).
   res->loop_seconds covers the criteria as well. */
int nemgpu_iterate_logged(nemgpu_engine* e, int with_init, nemgpu_result* res, float crit_before[6], float crit_after[6],
                          float* prop, float* center, float* disp, float* nbobs_k);
int nemgpu_restart_iterate(nemgpu_engine* e, int n_iters, nemgpu_result* res);  /* reset + init + n iterations, one pipeline */
int nemgpu_density(nemgpu_engine* e);                     /* E1 only */
int nemgpu_sweep(nemgpu_engine* e, float beta, int* rounds);  /* E2 only (one full Gauss-Seidel sweep) */
int nemgpu_mstep(nemgpu_engine* e, int* emptyk);          /* M only */
int nemgpu_criteria(nemgpu_engine* e, float crit6[6]);    /* C1 only */
/* C1 on the partition the last E-step sweep started from, with the current densities: the "after the M-step"
   criteria of the reference's <Fname>.log (WriteLogCrit, nem_alg.c:2361, 2620-2646) */
int nemgpu_criteria_previous(nemgpu_engine* e, float crit6[6]);

/* Multi-GPU step pieces (NCEM; families sharded across engines in contiguous blocks).  The host
   driver (pangenomenem_amd/distributed.py) owns the all-gathered label arrays (device memory) and
   the statistics buffer and runs the collectives (RCCL through torch.distributed) between these
   calls.  All calls are asynchronous on the engine's stream; between nemgpu_shard_begin and
   nemgpu_shard_end the loop tests run on the device, as in the single-GPU pipelined loop.

   Label arrays are uint8[world * stride]: rank r owns slots [r*stride, r*stride + blk) (its families,
   in order); the byte at r*stride + blk carries its "a label changed in this round" flag, the byte behind it "one
   of my labels moved in this sweep" (the verifying round's, or round 0's when there are no neighbours to verify
   against: every rank then runs the convergence test on the gathered bytes) and, further
   behind (4-byte aligned, the driver picks the offset), its partial M-step statistics, so ONE
   all-gather per relaxation round moves labels, flags and statistics together -- there is no separate
   all-reduce.  The engine is created with n_total = world*stride, site_lo = rank*stride,
   site_hi = site_lo + (families of the shard) and the graph's neighbour indices are slot indices.
   stats: int32[k + k*d] = { N_k, S1[k][j] = #{i in shard : label_i = k, x_ij = 1} } per rank; readers
   sum the world partial arrays (stride bytes apart), integer sums being exact in any order.          */
int nemgpu_stats_words(const nemgpu_engine* e);
int nemgpu_shard_layout(nemgpu_engine* e, int world, int rank, int blk, int stride, int n_families_total);
int nemgpu_shard_begin(nemgpu_engine* e);
/* partial counts of this rank's families under the given labels -> stats_dev (own statistics tail) */
int nemgpu_shard_mstep_partial(nemgpu_engine* e, const uint8_t* labels_cur_dev, int32_t* stats_dev);
/* the same for the labels the last nemgpu_shard_estep_round0 produced (their class masks already exist) */
int nemgpu_shard_counts(nemgpu_engine* e, int32_t* stats_dev);
/* stats_dev = rank 0's partial statistics inside an all-gathered label array (rank r's are r*stride bytes
   further) -> parameters, or NULL to keep them; density; round 0 (+ class masks of its output, + this rank's
   flag byte); sweep_id < 0 = device counter */
int nemgpu_shard_estep_round0(nemgpu_engine* e, const int32_t* stats_dev, float beta, int sweep_id,
                              const uint8_t* labels_old_dev, uint8_t* labels_out_dev);
int nemgpu_shard_estep_round1(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                              const uint8_t* labels_guess_dev, uint8_t* labels_out_dev);
/* round 1 and nemgpu_shard_counts(stats_dev) together: one launch where the shape has a kernel for it (the two do not
   depend on each other), else the two launches */
int nemgpu_shard_estep_round1_counts(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                                     const uint8_t* labels_guess_dev, uint8_t* labels_out_dev, int32_t* stats_dev);
/* Fuzzy NEM (algo = nem) on several GPUs -- SURVEY.md 8e's exact alternative to an all-reduce, which cannot reproduce
   the reference's i-ordered float sums (nem_mod.c:1303-1313, 1677-1686): the E-step sharded over FAMILIES, the M-step
   over ORGANISMS.  Per rank two engines: a row engine (its families x all organisms; site range [lo, hi) of n_total)
   and a column engine (all families x its organisms).  The membership matrix lives in caller-owned device arrays
   float[n_total][K] that the caller all-gathers after every relaxation round; the statistics of the organism slices
   are all-gathered into arrays of K, K*D, K*D floats.  One step per call, every call synchronises
   (pangenomenem_amd/distributed.py: ShardedFuzzyNem).  Results equal the single engine's bit for bit. */
int nemgpu_shard_fuzzy_layout(nemgpu_engine* e, int n_true);      /* families of the whole problem (n_total may be padded) */
int nemgpu_shard_fuzzy_round(nemgpu_engine* e, float beta, int sweep_id, int round, const float* c_old_dev, const float* c_guess_dev,
                             float* c_out_dev, int* changed, int* nzero, int* firstzero);
int nemgpu_shard_fuzzy_mstep_cols(nemgpu_engine* e, const float* c_dev, float* nbobs_out_dev, float* center_out_dev, float* iner_out_dev);
int nemgpu_shard_fuzzy_finish(nemgpu_engine* e, const float* nbobs_dev, const float* center_dev, const float* iner_dev, int* emptyk);
int nemgpu_shard_fuzzy_moved(nemgpu_engine* e, const float* c_new_dev, const float* c_old_dev, int* moved);

/* nemgpu_shard_begin for a batch that starts the run over: nemgpu_reset, the cleared loop control and the density
   tables in one launch */
int nemgpu_shard_begin_restart(nemgpu_engine* e);
int nemgpu_shard_finish_iteration(nemgpu_engine* e, float beta, int is_init, const uint8_t* labels_old_dev,
                                  const uint8_t* labels_q_dev, const uint8_t* labels_r_dev);
int nemgpu_shard_round_sync(nemgpu_engine* e, float beta, int sweep_id, const uint8_t* labels_old_dev,
                            const uint8_t* labels_guess_dev, uint8_t* labels_out_dev, int* changed);
/* NEMGPU_TIE_LIBC in the sharded path (nem_alg.c:617-637 -> nem_rnd.c:53-61): a tied site draws random() number
   `draws before the sweep + sites below it that drew in this sweep`, and the sites of the ranks below come first.  Every
   rank's draws of the round that produced a label array ride in its block's tail (an int32, nemgpu_shard_layout's
   blk rounded up to 4, + 4), all-gathered with the labels; every rank holds the same window of the same stream.
   nemgpu_shard_set_labels: the driver's three label arrays (the engine keeps each one's per-block draw counts).
   A start under this rule is completed from the host, sweep by sweep (the blind sweep's ties come first in the
   stream): nemgpu_shard_round_sync rounds until no rank changes anything, nemgpu_shard_round_draws after each (this
   rank's draws; table_short: a draw fell outside the table -- the round is void everywhere: nemgpu_shard_grow_draws on
   every rank, then the round again), nemgpu_shard_book_draws(sum over the ranks of the final round's draws). */
int nemgpu_shard_set_labels(nemgpu_engine* e, const uint8_t* lab0, const uint8_t* lab1, const uint8_t* lab2);
int nemgpu_shard_round_draws(nemgpu_engine* e, int* draws, int* table_short);
int nemgpu_shard_grow_draws(nemgpu_engine* e);
int nemgpu_shard_book_draws(nemgpu_engine* e, int n);
int nemgpu_shard_end_enqueue(nemgpu_engine* e);   /* async copy of the control block; last call of a batch */
int nemgpu_shard_end(nemgpu_engine* e, nemgpu_result* res, int* commits, int* need_rounds);   /* sync + report */
int nemgpu_shard_set_sweep_number(nemgpu_engine* e, int next_sweep);

/* RCCL called directly: the sharded EM's one collective (the in-place all-gather of label blocks) issued from C, so
   that a whole batch -- kernels and all-gathers -- is enqueued by ONE call instead of a Python round trip per
   launch.  librccl.so is bound at run time (pass the path of the library PyTorch ships; NULL: the loader's default);
   torch.distributed remains the bootstrap (it carries the 128-byte ncclUniqueId from rank 0) and the fallback.
   nemgpu_rccl_attach is collective over the job's ranks.  nemgpu_shard_enqueue_batch = nemgpu_shard_begin,
   [the two initial sweeps], n_iters iterations (round 0, all-gather, round 1 + counts, all-gather, convergence +
   loop control), nemgpu_shard_end_enqueue; follow with nemgpu_shard_end.  lab0..2: the three all-gathered label
   arrays; stats_off: byte offset of a rank's statistics inside its block; base: buffer of the current partition. */
int nemgpu_rccl_open(const char* librccl_path);
int nemgpu_rccl_unique_id(uint8_t id128[128]);
int nemgpu_rccl_attach(nemgpu_engine* e, const uint8_t id128[128], int world, int rank);
int nemgpu_shard_enqueue_batch(nemgpu_engine* e, int with_init, int n_iters, int base, float beta, int want_stats,
                               uint8_t* lab0, uint8_t* lab1, uint8_t* lab2, int stats_off);
/* One in-place all-gather of `stride`-byte blocks of buf_dev (world * stride bytes, device memory) through the
   engine's own communicator, waited for with a deadline; collective.  The caller compares the result with the same
   gather through torch.distributed before trusting the native path.  A timeout aborts and detaches the communicator. */
int nemgpu_rccl_selftest(nemgpu_engine* e, uint8_t* buf_dev, int stride, int timeout_ms);
/* ranks of the engine's native communicator as RCCL reports them (ncclCommCount); 0 when none is attached */
int nemgpu_rccl_ranks(const nemgpu_engine* e);

/* Test hook: load a partition (row-major [n_total x k], HOST) as the current state
   (argmax labels for ncem engines). */
int nemgpu_set_partition(nemgpu_engine* e, const float* c_nk);

/* Results (HOST buffers; any pointer may be NULL).  c_nk is row-major [(site_hi-site_lo) x k].
   nemgpu_get_results: parameters and partition in one device round trip. */
int nemgpu_get_results(nemgpu_engine* e, float* prop, float* center, float* disp, float* nbobs_k, float* c_nk);
int nemgpu_get_partition(nemgpu_engine* e, float* c_nk);
int nemgpu_get_labels(nemgpu_engine* e, uint8_t* labels);
int nemgpu_get_params(nemgpu_engine* e, float* prop, float* center, float* disp, float* nbobs_k);
int nemgpu_get_density(nemgpu_engine* e, double* pkfki_nk, float* logpkfki_nk);
/* An engine with an observed mask: NbObs_KD [k*d] of its last M-step, the class's observed families per organism
   (EstimSizes, nem_mod.c:1310; what the reference's log prints behind the dispersions).  NEMGPU_E_ARG without a mask. */
int nemgpu_get_observed_counts(nemgpu_engine* e, float* nbobs_kd);
/* ------------------------------------------------------------------------------------------
 * 3. File layer (host only; what nem() uses on either side of the engine).  Readers follow
 *    ReadStrFile / ReadMatrixFile / ReadPtsNeighs / ReadParamFile (nem_exe.c:739-1091, 1278-1478),
 *    writers follow SaveResults (nem_exe.c:1596-1781).  Return values are StatusET codes.
 * ------------------------------------------------------------------------------------------ */
typedef struct nemio_inputs nemio_inputs;
/* Parse <Fname>.str/.dat/.nei/.m for nk classes. */
int nemio_read(const char* Fname, int nk, nemio_inputs** out);
void nemio_free(nemio_inputs* in);
/* sizes: n families, d organisms, nnz neighbour entries, max_neighs, param_mode (1 init / 2 fixed), type 'S'|'N' */
int nemio_sizes(const nemio_inputs* in, int* n, int* d, int* nnz, int* max_neighs, int* param_mode, int* type);
/* copy out: xbits [n * ceil(d/32)], nei_ptr [n+1], nei_idx/nei_w [nnz], prop [k], center/disp [k*d]; NULL skips */
int nemio_copy(const nemio_inputs* in, uint32_t* xbits, int32_t* nei_ptr, int32_t* nei_idx, float* nei_w,
               float* prop, float* center, float* disp);
/* the .dat file's observed mask: obits [n * ceil(d/32)] (bit = 1: the cell held a number, 0: a `nan` token; padding
   bits 0), n_missing = the number of nan cells (nem_exe.c:477-490); NULL skips */
int nemio_observed(const nemio_inputs* in, uint32_t* obits, int* n_missing);
int nemio_write_uf(const char* path, const float* c_nk, int n, int k);
/* Test hook: " %<width>.<dec>f" (dec <= 3) of a float exactly as printf prints it -- the formatter behind the
   per-iteration <Fname>.log lines (WriteLogClasses' " %5.3f", " %7.3f", " %7.1f").  out: at least 64 bytes;
   returns the length written, -1 on bad arguments. */
int nemio_format_fixed(float v, int width, int dec, char* out);
int nemio_write_cf(const char* path, const float* c_nk, int n, int k, int tie_rule, uint32_t seed);
int nemio_write_mf(const char* path, const float crit6[6], float beta, int d, int k, const float* center,
                   const float* prop, const float* disp);

/* Kernel-duration probe for bench.py: `reps` launches of the E1 density kernel on the current
   parameters, each bracketed by HIP events on the engine's stream; average duration (ms) and the
   algorithmic bytes one launch moves. */
int nemgpu_profile_density(nemgpu_engine* e, int reps, double* avg_ms, double* algorithmic_bytes_per_launch,
                           int* used_fused_kernel);
/* The same for the three kernels of a solo NCEM iteration -- {E1, one relaxation round of the E-step sweep, the M-step
   counts} -- each launched `reps` times back to back between ONE pair of HIP events (an event pair per launch costs as
   much as the shorter kernels).  avg_ms[3], bytes[3]; which[0] = 1 when E1 is the fused kernel.  The engine's partition
   is not advanced. */
int nemgpu_profile_kernels(nemgpu_engine* e, int reps, double avg_ms[3], double bytes[3], int which[1]);
/* E1 (DensBernoulli over the whole matrix, nem_mod.c:619-690) as a lock-step batch launches it: the density kernels of
   `count` same-shaped engines of one device in ONE launch, `reps` launches back to back between one pair of HIP events.
   avg_ms: one launch (all members); algorithmic_bytes_per_launch: all members' bit-packed matrices, tables and outputs. */
int nemgpu_profile_density_many(nemgpu_engine** engines, int count, int reps, double* avg_ms, double* algorithmic_bytes_per_launch);
/* `reps` in-place all-gathers of the sharded EM's label blocks through the engine's own communicator between one pair
   of HIP events: the cost of ONE of an iteration's two collectives.  Collective over the job's ranks. */
int nemgpu_rccl_time_allgather(nemgpu_engine* e, uint8_t* buf_dev, int reps, double* avg_ms);
/* FETCH_SIZE calibration helper: `reps` launches reading `bytes` of device memory 16 bytes per lane (E1's
   pattern); run under `rocprofv3 --pmc FETCH_SIZE` and compare with the known byte count (profiles/README.md). */
int nemgpu_calibrate_fetch(size_t bytes, int reps);

/* E1 fast-forward (pangenomenem_amd/csrc/nem_ff.hpp): inside one float binade the reference's chain
   dk = (float)(((double)dk + |x-mu|*L1) - L0)  (nem_mod.c:661) adds a constant to the accumulator's bit pattern, so
   whole 32-organism words advance with one popcount; bit-identical to stepping.  on: 1 always, 0 never,
   -1 (default) automatic -- on from 256 organisms.  The
   environment variable NEM_MI355X_FF=0|1 sets the mode at creation.  The tests compare the two code paths. */
int nemgpu_set_fast_forward(nemgpu_engine* e, int on);
/* The increment tables that fast-forward uses for class constants L1 = log((1-eps)/eps), L0 = log(1-eps):
   q0[E] / q1[E] = bit-pattern increment of a match / mismatch step while the accumulator's exponent field is E
   (2^23 = "step exactly").  Host-only, needs no GPU. */
int nemgpu_ff_table(double l1, double l0, uint32_t* q0_256, uint32_t* q1_256);

/* The criteria of ComputeCrit (nem_alg.c:2727-2745) are i-ordered float accumulators
   acc = (float)((double)acc + x_i); the library evaluates them exactly but in parallel: between two powers of two
   the accumulator moves on a fixed grid and the chain is a prefix sum of integers
   (pangenomenem_amd/csrc/nem_chain.hpp).  Test hooks for that procedure on arbitrary doubles:
   nemgpu_chain_host -- mode 0: the plain sequential loop, mode 1: the host emulation of the device procedure
   (no GPU needed); nemgpu_chain_device -- the device procedure itself. */
float nemgpu_chain_host(const double* x, long long n, float init, int mode);
/* s = 0; `times` times s += x in float: mode 0 the loop, mode 1 its closed form per binade, mode 2 the integer form of
   that for integer x below 2^24 (csrc/nem_ff.hpp) */
float nemgpu_repeat_add_host(float x, long long times, int mode);
int nemgpu_chain_device(const double* x, long long n, float init, int device, float* out);
/* InerToDispK_'s d-ordered float sum of a class's inertia values (nem_mod.c:1054-1058): under NCEM they are
   non-negative multiples of 1/2 below 2^24, and the library evaluates the chain in pieces, all threads of a block at
   once (pangenomenem_amd/csrc/nem_halfsum.hpp).  Test hooks on arbitrary such values: nemgpu_halfsum_host -- mode 0:
   the plain loop, mode w = 1..16: the host emulation of the device procedure with w wavefronts (stepped: adds it took
   for real; no GPU needed); nemgpu_halfsum_device -- the device procedure itself (n <= 8192, waves 1 or 16);
   nemgpu_halfsum_profile -- its in-kernel timing: us[0..3] = prefix sums, classification + walk, scan + hand-over,
   ordered pass; us[4] = the same chain as plain dependent adds on one lane. */
float nemgpu_halfsum_host(const float* x, int n, int mode, int* stepped);
int nemgpu_halfsum_device(const float* x, int n, int waves, int device, float* out);
int nemgpu_halfsum_profile(const float* x, int n, int waves, int device, double us[5]);
/* An NCEM round takes a site's label from the unnormalised row cinum[k] = pkf[k] * exp(beta ctx[k]) where the row's
   maximum is clear, and normalises only the other rows (pangenomenem_amd/csrc/nem_map.hpp; NEM_MI355X_MAP_MARGIN=0:
   every row).  Test hooks, out[i] = {the normalised row's first maximum, the later entries equal to it as floats, the
   unnormalised row's first maximum, 1 if the row is clear}: nemgpu_map_margin_host -- rows cinum[n][K], K <= 32, on
   the CPU (no GPU needed); nemgpu_map_margin_device -- rows as a round has them (pkf[n][K], ctx[n][K]; use_nei = 0:
   cinum = pkf), K <= 8, with the device's arithmetic. */
int nemgpu_map_margin_host(const double* cinum, int n, int K, int* out);
int nemgpu_map_margin_device(const double* pkf, const float* ctx, int n, int K, float beta, int use_nei, int device, int* out);

/* nemgpu_destroy parks an engine's stream, first 16 MB of device memory and pinned control block (up to 16 sets
   per process) for the next nemgpu_create on the same device -- a nem() call creates and destroys an engine, and
   creating these costs as much as a small EM run.  This frees whatever is parked. */
void nemgpu_release_cached(void);

/* hipGraph policy of the pipelined EM loop.  By default a batch shape (initial sweeps or not, buffer phase, number of
   iterations) goes out as plain launches the first time and is captured + instantiated the second time it is
   enqueued; capture_on_first != 0 captures at once (benchmarks prime every shape of their timed region this way). */
int nemgpu_set_graph_policy(nemgpu_engine* e, int capture_on_first);
/* out[0] batches sent as plain launches, out[1] batches captured + instantiated, out[2] graph replays,
   out[3] sweeps the host had to finish round by round */
int nemgpu_graph_counters(const nemgpu_engine* e, int out[4]);
/* debug: starts of this engine that went out without a blind launch -- the first round of the start's beta sweep
   labelled the blind partition itself (NEM_MI355X_BLIND_FOLD, default on) --, graph replays included; -1: no engine */
int nemgpu_debug_blind_folds(const nemgpu_engine* e);
/* how the last nemgpu_run_random went (RandNemAlgo, nem_alg.c:1574-1742, starts in lock step): out = {lock-step rounds,
   starts that stood in them, starts run alone on the engine's own path, starts thrown away and redone because a start
   before them drew tie-breaks behind its initial sweeps (TIE_LIBC: one random() stream for all starts)}.  A logged
   call whose lock-step round lost that bet hands nothing over and runs every start again, alone: {0, 0, n, n}. */
int nemgpu_random_start_counters(const nemgpu_engine* e, int out[4]);

/* Re-target the engine to another HIP stream (e.g. the capturing stream of a torch.cuda.graph). */
int nemgpu_set_stream(nemgpu_engine* e, void* hip_stream);

/* The organisms' GFF files and the families table (PPanGGOLiN("file", ...), ppanggolin.py:180-315; csrc/nem_gff.hpp;
   loader.py's _batch_host and families_table_host state every array).
   _create: the families table's text (HOST, bytes < 2 GiB): tokens split at ASCII whitespace (str.isspace() below 0x80),
     the first of a line the family, every later one a gene; a gene named twice keeps the later line's family.  The
     distinct family names are numbered by their first line (*n_families of them; _family_spans: their (offset, length)
     in the text, HOST int32 [n_families][2]).  hash_bits: 0 for the full 64-bit string hash, else how many of its bits
     to keep (every table compares the bytes in full; tests make the probes collide with it).
   _batch: the bytes of n_files whole files joined by one '\n' (HOST, < 2 GiB), file f at [file_start[f], file_end[f]).
     The CDS lines before each file's ##FASTA become genes, ordered by (file, contig by first appearance, START, line);
     *n_genes, *n_contigs; *error = the least ((file << 40) | (line << 8) | code) of a refused line (line 0-based within
     its file; codes: 1 fewer than 3 fields, 2 a CDS with fewer than 9, 3 an attribute that is not key=value, 4 no ID,
     5 an ID the table does not have and infer_singletons == 0, 6 START, 7 END not an int32 in ASCII digits, 8 an ID
     twice in one file), all ones if none.  Nothing of a batch goes through the host between its upload and its result
     but the counts that size its arrays.
   _fetch: the last batch's genes (HOST, any may be NULL): file, start, end, fam (the family's number, -1 for an ID
     the table does not have), contig (dense over the batch) int32 [n_genes]; span_off, span_len int32 [5][n_genes]: ID,
     NAME (else GENE), PRODUCT, strand, contig name, stripped (an absent one: the empty span at the ID);
     fasta_off int32 [n_files]: where the file's ##FASTA line starts, its end if it has none.
   _number: after all the batches, the families' ids and the repeated ones.  name[g], org[g] (HOST): every gene's family
     name (a number in 0 .. n_names - 1: the table's families, then the inferred singletons' names as the caller numbered
     them) and organism, in the walk's order.  genes[g] = the ids dense by first occurrence in the walk, order[id] =
     the name of id (*n_used of them; room for n_names), repeated[id] = 1 where the family occurs more than
     lim_occurence > 0 times in ONE organism (room for max(n_names, 1)).
   _stage_ms: the last batch's device time by stage, float [6]: upload, lines, parse, contigs and IDs, sort, gather.
   _info: the byte kernels' tile in bytes and the contig sizes at which the sort changes its path (*n_thresholds of
     them, at most 8 written): one radix sort serves every size, so there are none.  Host only; any may be NULL. */
typedef struct nemgpu_gff nemgpu_gff;
int nemgpu_gff_info(int* tile_bytes, int* n_thresholds, int* thresholds);
int nemgpu_gff_create(nemgpu_gff** out, int device, const char* families_text, long long bytes, int hash_bits, int* n_families);
int nemgpu_gff_family_spans(const nemgpu_gff* h, int32_t* spans);
int nemgpu_gff_batch(nemgpu_gff* h, const char* text, long long bytes, const int32_t* file_start, const int32_t* file_end, int n_files,
                     int infer_singletons, int* n_genes, int* n_contigs, unsigned long long* error);
int nemgpu_gff_fetch(const nemgpu_gff* h, int32_t* file, int32_t* start, int32_t* end, int32_t* span_off, int32_t* span_len, int32_t* fam,
                     int32_t* contig, int32_t* fasta_off);
int nemgpu_gff_number(nemgpu_gff* h, const int32_t* name, const int32_t* org, int g, int n_names, int n_orgs, int lim_occurence, int32_t* genes,
                      int32_t* order, uint8_t* repeated, int* n_used);
int nemgpu_gff_stage_ms(const nemgpu_gff* h, float* ms);
void nemgpu_gff_destroy(nemgpu_gff* h);

#ifdef __cplusplus
}
#endif
#endif /* NEM_MI355X_H */
