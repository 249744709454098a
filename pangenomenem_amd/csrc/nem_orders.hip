// nem_orders.hip -- see nem_orders.hpp.
#include "nem_orders.hpp"
#include "nem_scan.hpp"

#include <algorithm>

namespace nemk {

namespace {

using namespace seg;
constexpr uint32_t kNoPos = 0xffffffffu;          // first position of a family without a kept gene
constexpr uint32_t kSuccBit = 0x80000000u;        // a successor record's time (sorts after every predecessor's)

// ---- stage 1 ----------------------------------------------------------------------------------------------------
// last[p] = p for a kept gene, -1 for one of a repeated family; the first kept position of every family id
// (seed, an append: the number every id of the old master has already; such an id takes no new number)
__global__ __launch_bounds__(kThreads) void k_orders_kept(const int* __restrict__ genes, int g, const uint8_t* __restrict__ repeated,
                                                         const int* __restrict__ seed, int* __restrict__ last, uint32_t* firstpos)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const int fam = genes[p];
    const bool kept = !(repeated && repeated[fam]);
    last[p] = kept ? p : -1;
    if (kept && !(seed && seed[fam] >= 0) && firstpos[fam] > (uint32_t)p) atomicMin(&firstpos[fam], (uint32_t)p);   // (the plain read only ever errs high)
}

// seed[order[i]] = i: the old master's numbering by caller id (order null: the identity)
__global__ __launch_bounds__(kThreads) void k_orders_seed(const int* __restrict__ order, int n_old, int* __restrict__ seed)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_old) seed[order ? order[i] : i] = i;
}

__global__ __launch_bounds__(kThreads) void k_orders_iota(uint32_t* __restrict__ v, int n)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// families by first kept position: newid of every caller id (-1: no kept gene), *n = the families with one; an append
// numbers them from n_old on and leaves the old master's ids their numbers
__global__ __launch_bounds__(kThreads) void k_orders_number(const uint32_t* __restrict__ pos_sorted, const uint32_t* __restrict__ fam_sorted, int f,
                                                           const int* __restrict__ seed, int n_old, int* __restrict__ newid,
                                                           int* __restrict__ n_out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= f) return;
    const bool has = pos_sorted[i] != kNoPos;
    const int fam = (int)fam_sorted[i];
    newid[fam] = has ? n_old + i : (seed ? seed[fam] : -1);
    if (has && (i + 1 == f || pos_sorted[i + 1] == kNoPos)) *n_out = i + 1;
}

struct KeyBits { int bn, bd; };
__device__ inline uint64_t make_key(KeyBits kb, int row, int nbr, int org)
{
    return ((uint64_t)(uint32_t)row << (kb.bn + kb.bd)) | ((uint64_t)(uint32_t)nbr << kb.bd) | (uint64_t)(uint32_t)org;
}

// the two record slots of every gene (2p, 2p + 1); an unused slot's key is 1 << (2 bn + bd): it sorts behind all
__global__ __launch_bounds__(kThreads) void k_orders_records(const int* __restrict__ genes, int g, const int* __restrict__ last,
                                                            const int* __restrict__ cptr, int c, const int* __restrict__ corg,
                                                            const uint8_t* __restrict__ circ, const int* __restrict__ newid, int directed,
                                                            KeyBits kb, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            int* __restrict__ gene_org)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const uint64_t none = (uint64_t)1 << (2 * kb.bn + kb.bd);
    uint64_t k0 = none, k1 = none;
    uint32_t v0 = 0, v1 = 0;
    int org = -1;
    if (last[p] == p) {
        const int j = last_le(cptr, c, p), start = cptr[j], end = cptr[j + 1];   // the contig: cptr[j] <= p < cptr[j + 1]
        org = corg[j];
        const int prev = p > 0 ? last[p - 1] : -1;
        int other = -1;
        uint32_t t = 0;
        if (prev >= start) { other = prev; t = (uint32_t)p + (uint32_t)j; }                       // ppanggolin.py:513
        else if (circ[j]) { other = last[end - 1]; t = (uint32_t)end + (uint32_t)j; }             // :518-519 (p is the contig's first kept gene)
        if (other >= 0) {
            const int a = newid[genes[p]], b = newid[genes[other]];
            if (directed) { k0 = make_key(kb, a, b, org); v0 = t | kSuccBit; k1 = make_key(kb, b, a, org); v1 = t; }
            else { k0 = make_key(kb, a, b, org); v0 = t; if (a != b) { k1 = make_key(kb, b, a, org); v1 = t; } }
        }
    }
    gene_org[p] = org;
    keys[2 * (size_t)p] = k0; keys[2 * (size_t)p + 1] = k1;
    vals[2 * (size_t)p] = v0; vals[2 * (size_t)p + 1] = v1;
}

// per sorted record: (starts an edge) << 32 | (starts an (edge, organism) pair)
__global__ __launch_bounds__(kThreads) void k_orders_heads(const uint64_t* __restrict__ keys, int n2, KeyBits kb, uint64_t* __restrict__ flags)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n2) return;
    const uint64_t none = (uint64_t)1 << (2 * kb.bn + kb.bd);
    const uint64_t k = keys[i];
    uint64_t fl = 0;
    if (k < none) {
        const uint64_t kp = i > 0 ? keys[i - 1] : ~(uint64_t)0;
        fl = ((uint64_t)(i == 0 || (kp >> kb.bd) != (k >> kb.bd)) << 32) | (uint64_t)(i == 0 || kp != k);
    }
    flags[i] = fl;
}

// the runs: where every pair starts and which edge it belongs to, where every edge's pairs start, an edge's first time
__global__ __launch_bounds__(kThreads) void k_orders_runs(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int n2, KeyBits kb,
                                                         const uint64_t* __restrict__ pos, int* __restrict__ trip_start,
                                                         int* __restrict__ trip_edge, int* __restrict__ edge_tstart, uint32_t* edge_min)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const uint64_t none = (uint64_t)1 << (2 * kb.bn + kb.bd);
    const uint64_t k = i < n2 ? keys[i] : none;
    const bool valid = k < none;
    int e = -1;
    uint32_t v = 0xffffffffu;
    if (valid) {
        const uint64_t kp = i > 0 ? keys[i - 1] : ~(uint64_t)0;
        const bool hp = i == 0 || (kp >> kb.bd) != (k >> kb.bd), ht = i == 0 || kp != k;
        const uint64_t before = pos[i];
        e = (int)(before >> 32) + (hp ? 1 : 0) - 1;
        const int t = (int)(uint32_t)before + (ht ? 1 : 0) - 1;
        if (ht) { trip_start[t] = i; trip_edge[t] = e; }
        if (hp) edge_tstart[e] = t;
        if (i + 1 == n2 || keys[i + 1] >= none) { trip_start[t + 1] = i + 1; edge_tstart[e + 1] = t + 1; }   // (the last record)
        v = vals[i];
    }
    bool tail;
    v = wave_segment(e, v, OpMin(), tail);
    if (valid && tail) atomicMin(&edge_min[e], v);
}

// pairs with count >= 2
__global__ __launch_bounds__(kThreads) void k_orders_multi(const int* __restrict__ trip_start, int tn, int* __restrict__ flag)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < tn) flag[t] = trip_start[t + 1] - trip_start[t] >= 2 ? 1 : 0;
}

// (row << 32 | first time, edge) of every edge
__global__ __launch_bounds__(kThreads) void k_orders_edge_keys(const uint64_t* __restrict__ keys, KeyBits kb, const int* __restrict__ trip_start,
                                                              const int* __restrict__ edge_tstart, const uint32_t* __restrict__ edge_min, int nnz,
                                                              uint64_t* __restrict__ ekeys, uint32_t* __restrict__ evals)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nnz) return;
    const uint64_t row = keys[trip_start[edge_tstart[e]]] >> (kb.bn + kb.bd);
    ekeys[e] = (row << 32) | edge_min[e];
    evals[e] = (uint32_t)e;
}

// ---- stage 2 ----------------------------------------------------------------------------------------------------
// CSR entry f = edge perm[f]: its neighbour, its number of multi-copy pairs (into extra_ptr, scanned next)
__global__ __launch_bounds__(kThreads) void k_orders_entries(const uint32_t* __restrict__ perm, int nnz, const uint64_t* __restrict__ keys, KeyBits kb,
                                                            const int* __restrict__ trip_start, const int* __restrict__ edge_tstart,
                                                            const int* __restrict__ xs, int* __restrict__ inv, int* __restrict__ idx,
                                                            int* __restrict__ xdeg, int* over)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= nnz) return;
    const int e = (int)perm[f];
    const int t0 = edge_tstart[e], t1 = edge_tstart[e + 1];
    inv[e] = f;
    idx[f] = (int)((keys[trip_start[t0]] >> kb.bd) & (((uint64_t)1 << kb.bn) - 1));
    if (xdeg) xdeg[f] = xs[t1] - xs[t0];
    if (trip_start[t1] - trip_start[t0] > (1 << 24)) *over = 1;
}

// ptr[r] = the first CSR entry of a row >= r
__global__ __launch_bounds__(kThreads) void k_orders_ptr(const uint64_t* __restrict__ ekeys_sorted, int nnz, int n, int* __restrict__ ptr)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r > n) return;
    int lo = 0, hi = nnz;
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if ((int)(ekeys_sorted[mid] >> 32) < r) lo = mid + 1; else hi = mid; }
    ptr[r] = lo;
}

// every (edge, organism) pair: its bit in the edge's organism set, and its entry of the extras when its count is >= 2
__global__ __launch_bounds__(kThreads) void k_orders_pairs(const uint64_t* __restrict__ keys, KeyBits kb, const int* __restrict__ trip_start,
                                                          const int* __restrict__ trip_edge, int tn, const int* __restrict__ edge_tstart,
                                                          const int* __restrict__ inv, const int* __restrict__ xs, int wf, uint32_t* edge_bits,
                                                          const int* __restrict__ extra_ptr, const int* __restrict__ skip,
                                                          int* __restrict__ extra_org, int* __restrict__ extra_add)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const bool valid = t < tn;
    long long word = -1;
    uint32_t bit = 0;
    if (valid) {
        const int e = trip_edge[t], f = inv[e];
        const int i0 = trip_start[t], cnt = trip_start[t + 1] - i0;
        const int org = (int)(keys[i0] & (((uint64_t)1 << kb.bd) - 1));
        word = (long long)f * wf + (org >> 5);
        bit = 1u << (org & 31);
        if (cnt >= 2) {
            const int dst = extra_ptr[f] + (skip ? skip[f] : 0) + (xs[t] - xs[edge_tstart[e]]);   // (skip: an append, behind the entry's old extras)
            extra_org[dst] = org;
            extra_add[dst] = cnt - 1;
        }
    }
    bool tail;
    bit = wave_segment(word, bit, OpOr(), tail);
    if (valid && tail) atomicOr(&edge_bits[word], bit);
}

// x[family][organism] = 1 for every kept gene, into the organism-major rows
__global__ __launch_bounds__(kThreads) void k_orders_presence(const int* __restrict__ genes, int g, const int* __restrict__ gene_org,
                                                             const int* __restrict__ newid, int nw64, unsigned long long* xt)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const int org = gene_org[p];
    if (org < 0) return;
    const int fam = newid[genes[p]];
    unsigned long long* w = xt + (size_t)org * nw64 + (fam >> 6);
    const unsigned long long bit = 1ull << (fam & 63);
    if (!(*w & bit)) atomicOr(w, bit);                        // (a stale read only costs the atomic)
}

__global__ __launch_bounds__(64) void k_master_rows(const uint64_t* __restrict__ xt, int n, int wf, int d, int nw64, uint32_t* __restrict__ xf)
{
    const int g = blockIdx.x, w = blockIdx.y, lane = threadIdx.x;
    const int o = w * 32 + lane;
    const uint64_t x = (lane < 32 && o < d) ? xt[(size_t)o * nw64 + g] : 0ull;
    uint32_t mine = 0;
#pragma unroll
    for (int b = 0; b < 64; b++) {
        const uint64_t bal = __ballot((x >> b) & 1ull);
        if (lane == b) mine = (uint32_t)bal;
    }
    const int i = g * 64 + lane;
    if (i < n) xf[(size_t)i * wf + w] = mine;
}

// ---- an append (orders_append_plan / orders_append_fill) ---------------------------------------------------------
__device__ inline void edge_of_run(const uint64_t* keys, KeyBits kb, const int* trip_start, const int* edge_tstart, int e, int* row, int* nbr)
{
    const uint64_t k = keys[trip_start[edge_tstart[e]]];
    *row = (int)(k >> (kb.bn + kb.bd));
    *nbr = (int)((k >> kb.bd) & (((uint64_t)1 << kb.bn) - 1));
}

// every edge of the update: its entry in the old master's row (a walk of the row), or -1
__global__ __launch_bounds__(kThreads) void k_append_lookup(const uint64_t* __restrict__ keys, KeyBits kb, const int* __restrict__ trip_start,
                                                           const int* __restrict__ edge_tstart, int nnz_u, int n_old,
                                                           const int* __restrict__ old_ptr, const int* __restrict__ old_idx, int* __restrict__ oldpos)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nnz_u) return;
    int row, nbr, pos = -1;
    edge_of_run(keys, kb, trip_start, edge_tstart, e, &row, &nbr);
    if (row < n_old && nbr < n_old)
        for (int t = old_ptr[row], t1 = old_ptr[row + 1]; t < t1; t++) if (old_idx[t] == nbr) { pos = t; break; }
    oldpos[e] = pos;
}

// in (row, first time) order: 1 for an edge the old master does not have
__global__ __launch_bounds__(kThreads) void k_append_isnew(const uint32_t* __restrict__ perm, const int* __restrict__ oldpos, int nnz_u,
                                                          int* __restrict__ flag)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < nnz_u) flag[i] = oldpos[perm[i]] < 0 ? 1 : 0;
}

// a row's new degree: its old entries + its new edges (rank: the scanned flags, ptr_u: the update's rows in sorted order)
__global__ __launch_bounds__(kThreads) void k_append_degree(int n, int n_old, const int* __restrict__ old_ptr, const int* __restrict__ ptr_u,
                                                           const int* __restrict__ rank, int* __restrict__ deg)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    deg[r] = (r < n_old ? old_ptr[r + 1] - old_ptr[r] : 0) + rank[ptr_u[r + 1]] - rank[ptr_u[r]];
}

// old entry t keeps its place in its row: fwd[t] = where; there its neighbour, its source and its number of old extras
__global__ __launch_bounds__(kThreads) void k_append_old_entries(int nnz_old, int n_old, const int* __restrict__ old_ptr,
                                                                const int* __restrict__ old_idx, const int* __restrict__ old_xptr,
                                                                const int* __restrict__ ptr, int* __restrict__ idx, int* __restrict__ src,
                                                                int* __restrict__ oldx, int* __restrict__ fwd, int* __restrict__ xdeg)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz_old) return;
    const int r = last_le(old_ptr, n_old, t);                 // the entry's row
    const int f = ptr[r] + (t - old_ptr[r]);
    const int x = old_xptr ? old_xptr[t + 1] - old_xptr[t] : 0;
    idx[f] = old_idx[t];
    src[f] = t;
    oldx[f] = x;
    fwd[t] = f;
    if (xdeg) xdeg[f] = x;
}

// the update's edges (sorted position i = edge perm[i]): inv[e] = its entry of the grown master -- an old edge's own, a
// new one behind its row's old entries by rank among the row's new ones; a new entry's neighbour; the entry's extras
// (old + the update's pairs with count >= 2); the 2^24 bound on old + new count
__global__ __launch_bounds__(kThreads) void k_append_new_entries(const uint32_t* __restrict__ perm, int nnz_u, const uint64_t* __restrict__ keys,
                                                                KeyBits kb, const int* __restrict__ trip_start,
                                                                const int* __restrict__ edge_tstart, const int* __restrict__ xs,
                                                                const int* __restrict__ oldpos, const int* __restrict__ rank,
                                                                const int* __restrict__ ptr_u, int n_old, const int* __restrict__ old_ptr,
                                                                const uint32_t* __restrict__ old_bits, int wf_old, uint32_t last_mask,
                                                                const int* __restrict__ old_xptr, const int* __restrict__ old_xadd,
                                                                const int* __restrict__ ptr, int* __restrict__ inv, int* __restrict__ idx,
                                                                int* __restrict__ src, int* __restrict__ oldx, int* __restrict__ xdeg, int* over)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nnz_u) return;
    const int e = (int)perm[i];
    const int t0 = edge_tstart[e], t1 = edge_tstart[e + 1];
    int row, nbr;
    edge_of_run(keys, kb, trip_start, edge_tstart, e, &row, &nbr);
    const int op = oldpos[e];
    long long total = trip_start[t1] - trip_start[t0];
    int f, x = 0;
    if (op >= 0) {
        f = ptr[row] + (op - old_ptr[row]);
        const uint32_t* w = old_bits + (size_t)op * wf_old;
        for (int j = 0; j < wf_old; j++) total += __popc(j == wf_old - 1 ? w[j] & last_mask : w[j]);
        if (old_xptr) { x = old_xptr[op + 1] - old_xptr[op]; for (int j = old_xptr[op]; j < old_xptr[op + 1]; j++) total += old_xadd[j]; }
    } else {
        f = ptr[row] + (row < n_old ? old_ptr[row + 1] - old_ptr[row] : 0) + (rank[i] - rank[ptr_u[row]]);
        idx[f] = nbr;
        src[f] = -1;
        oldx[f] = 0;
    }
    inv[e] = f;
    if (xdeg) xdeg[f] = x + (xs[t1] - xs[t0]);
    if (total > (1 << 24)) *over = 1;
}

// the grown edge_bits: an old entry's words (the bits above its last organism are not data), zero beyond and for new entries
__global__ __launch_bounds__(kThreads) void k_append_bits(long long words, int wf, int wf_old, uint32_t last_mask, const int* __restrict__ src,
                                                         const uint32_t* __restrict__ old_bits, uint32_t* __restrict__ bits)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= words) return;
    const long long f = i / wf;
    const int w = (int)(i - f * wf), s = src[f];
    uint32_t v = 0;
    if (s >= 0 && w < wf_old) { v = old_bits[(size_t)s * wf_old + w]; if (w == wf_old - 1) v &= last_mask; }
    bits[i] = v;
}

// old extra j of old entry t goes to the head of entry fwd[t]'s extras
__global__ __launch_bounds__(kThreads) void k_append_old_extras(int nx_old, int nnz_old, const int* __restrict__ old_xptr,
                                                               const int* __restrict__ old_xorg, const int* __restrict__ old_xadd,
                                                               const int* __restrict__ fwd, const int* __restrict__ xptr,
                                                               int* __restrict__ xorg, int* __restrict__ xadd)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= nx_old) return;
    const int t = last_le(old_xptr, nnz_old, j);              // the extra's entry
    const int dst = xptr[fwd[t]] + (j - old_xptr[t]);
    xorg[dst] = old_xorg[j];
    xadd[dst] = old_xadd[j];
}

// the grown organism-major rows: the old ones at the new stride, zero for the new organisms and the new families
__global__ __launch_bounds__(kThreads) void k_append_xt(long long words, int nw64, int d_old, int nw64_old, const uint64_t* __restrict__ old_xt,
                                                       uint64_t* __restrict__ xt)
{
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= words) return;
    const long long o = i / nw64;
    const int w = (int)(i - o * nw64);
    xt[i] = (o < d_old && w < nw64_old) ? old_xt[(size_t)o * nw64_old + w] : 0ull;
}

}  // namespace

struct OrdersBuild : Scratch {
    int d = 0, f = 0, g = 0, n = 0, nnz = 0, tn = 0, nx = 0, n2 = 0;
    int n_old = 0;                                            // an append: the old master's families (else 0)
    int *oldpos = nullptr, *rank = nullptr, *ptr_u = nullptr; // an append (orders_append_plan)
    KeyBits kb{1, 1};
    int *genes = nullptr, *gene_org = nullptr, *newid = nullptr;
    uint32_t* fam_sorted = nullptr;
    const uint64_t* keys = nullptr;                           // the sorted records
    int *trip_start = nullptr, *trip_edge = nullptr, *xs = nullptr, *edge_tstart = nullptr;
    const uint64_t* ekeys = nullptr;                          // the sorted edges
    const uint32_t* perm = nullptr;
    int* inv = nullptr;
    int* partial = nullptr;
    int* over = nullptr;
};

void orders_free(OrdersBuild* b) { delete b; }

bool orders_key_fits(int n, int d) { return 2 * bits_for(n) + bits_for(d) <= 63; }

#define ORD(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { delete b; return e_; } } while (0)

hipError_t orders_stage(const OrdersIn& in, hipStream_t s, OrdersBuild** out, int* n, int* nnz, int* nx)
{
    *out = nullptr; *n = 0; *nnz = 0; *nx = 0;
    OrdersBuild* b = new OrdersBuild();
    const int g = in.g, c = in.c, f = in.f;
    b->d = in.d; b->f = f; b->g = g; b->n2 = 2 * g; b->n_old = in.n_old;
    int *cptr, *corg, *last, *seed = nullptr;
    uint8_t *circ, *rep = nullptr;
    uint32_t *fp0, *fp1, *fi0, *fi1;
    uint64_t* totals;                                         // [0] the record flags' total, then int words: n, over
    ORD(b->alloc(&b->genes, g)); ORD(b->alloc(&cptr, c + 1)); ORD(b->alloc(&corg, c)); ORD(b->alloc(&circ, c));
    if (in.repeated) ORD(b->alloc(&rep, f));
    ORD(b->alloc(&last, g)); ORD(b->alloc(&b->gene_org, g)); ORD(b->alloc(&b->newid, f));
    ORD(b->alloc(&fp0, f)); ORD(b->alloc(&fp1, f)); ORD(b->alloc(&fi0, f)); ORD(b->alloc(&fi1, f));
    ORD(b->alloc(&totals, 4));
    uint64_t* partial64;
    ORD(b->alloc(&partial64, (size_t)b->n2 / kScanTile + 2));
    b->partial = (int*)partial64;
    int* n_dev = (int*)(totals + 1);
    b->over = n_dev + 1;
    ORD(hipMemcpyAsync(b->genes, in.genes, (size_t)g * 4, hipMemcpyHostToDevice, s));
    ORD(hipMemcpyAsync(cptr, in.contig_ptr, ((size_t)c + 1) * 4, hipMemcpyHostToDevice, s));
    ORD(hipMemcpyAsync(corg, in.contig_org, (size_t)c * 4, hipMemcpyHostToDevice, s));
    ORD(hipMemcpyAsync(circ, in.contig_circular, (size_t)c, hipMemcpyHostToDevice, s));
    if (rep) ORD(hipMemcpyAsync(rep, in.repeated, (size_t)f, hipMemcpyHostToDevice, s));
    ORD(hipMemsetAsync(totals, 0, 4 * sizeof(uint64_t), s));
    ORD(hipMemsetAsync(fp0, 0xff, (size_t)f * 4, s));          // (kNoPos)
    if (in.n_old > 0) {                                       // an append: the old numbering by caller id
        int* ord = nullptr;
        ORD(b->alloc(&seed, f));
        ORD(hipMemsetAsync(seed, 0xff, (size_t)f * 4, s));
        if (in.order_old) { ORD(b->alloc(&ord, in.n_old)); ORD(hipMemcpyAsync(ord, in.order_old, (size_t)in.n_old * 4, hipMemcpyHostToDevice, s)); }
        hipLaunchKernelGGL(k_orders_seed, dim3(blocks(in.n_old)), dim3(kThreads), 0, s, ord, in.n_old, seed);
    }
    // 1. kept genes, every gene's last kept gene at or before it
    hipLaunchKernelGGL(k_orders_kept, dim3(blocks(g)), dim3(kThreads), 0, s, b->genes, g, rep, seed, last, fp0);
    scan<int, OpMax, true>(last, last, g, OpMax(), -1, b->partial, (int*)nullptr, s);
    // 2. the numbering: the family ids by first kept position (those without one last)
    hipLaunchKernelGGL(k_orders_iota, dim3(blocks(f)), dim3(kThreads), 0, s, fi0, f);
    ORD(hipGetLastError());
    const uint32_t *fp_sorted, *fi_sorted;
    ORD(sort_pairs<uint32_t>(*b, fp0, fp1, fi0, fi1, f, 32, &fp_sorted, &fi_sorted, s));
    b->fam_sorted = const_cast<uint32_t*>(fi_sorted);
    hipLaunchKernelGGL(k_orders_number, dim3(blocks(f)), dim3(kThreads), 0, s, fp_sorted, fi_sorted, f, seed, in.n_old, b->newid, n_dev);
    ORD(hipGetLastError());
    ORD(hipMemcpyAsync(n, n_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    *n += in.n_old;
    b->n = *n;
    if (*n <= 0 || !orders_key_fits(*n, in.d)) { delete b; return hipErrorInvalidValue; }
    b->kb = KeyBits{bits_for(*n), bits_for(in.d)};
    // 3. the records
    uint64_t *k0, *k1, *pos;
    uint32_t *v0, *v1;
    const int n2 = b->n2;
    ORD(b->alloc(&k0, n2)); ORD(b->alloc(&k1, n2)); ORD(b->alloc(&v0, n2)); ORD(b->alloc(&v1, n2));
    hipLaunchKernelGGL(k_orders_records, dim3(blocks(g)), dim3(kThreads), 0, s, b->genes, g, last, cptr, c, corg, circ, b->newid, in.directed, b->kb,
                       k0, v0, b->gene_org);
    ORD(hipGetLastError());
    // 4. sorted; pairs and edges numbered by the scan of their first records
    const uint64_t* keys;
    const uint32_t* vals;
    ORD(sort_pairs<uint64_t>(*b, k0, k1, v0, v1, n2, 2 * b->kb.bn + b->kb.bd + 1, &keys, &vals, s));
    b->keys = keys;
    pos = keys == k0 ? k1 : k0;                               // (the sort's other buffer is free again)
    hipLaunchKernelGGL(k_orders_heads, dim3(blocks(n2)), dim3(kThreads), 0, s, keys, n2, b->kb, pos);
    scan<uint64_t, OpSum<uint64_t>, false>(pos, pos, n2, OpSum<uint64_t>(), (uint64_t)0, partial64, totals, s);
    ORD(hipGetLastError());
    uint64_t tot = 0;
    ORD(hipMemcpyAsync(&tot, totals, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    b->nnz = (int)(tot >> 32); b->tn = (int)(uint32_t)tot;
    uint32_t* edge_min;
    ORD(b->alloc(&b->trip_start, (size_t)b->tn + 1)); ORD(b->alloc(&b->trip_edge, b->tn)); ORD(b->alloc(&b->xs, (size_t)b->tn + 1));
    ORD(b->alloc(&b->edge_tstart, (size_t)b->nnz + 1)); ORD(b->alloc(&edge_min, b->nnz)); ORD(b->alloc(&b->inv, b->nnz));
    ORD(hipMemsetAsync(b->trip_start, 0, sizeof(int), s));    // (no record at all: the sentinels)
    ORD(hipMemsetAsync(b->edge_tstart, 0, sizeof(int), s));
    ORD(hipMemsetAsync(edge_min, 0xff, (size_t)std::max(b->nnz, 1) * 4, s));
    hipLaunchKernelGGL(k_orders_runs, dim3(blocks(n2)), dim3(kThreads), 0, s, keys, vals, n2, b->kb, (const uint64_t*)pos, b->trip_start,
                       b->trip_edge, b->edge_tstart, edge_min);
    if (b->tn > 0) hipLaunchKernelGGL(k_orders_multi, dim3(blocks(b->tn)), dim3(kThreads), 0, s, b->trip_start, b->tn, b->xs);
    scan<int, OpSum<int>, false>(b->xs, b->xs, b->tn, OpSum<int>(), 0, b->partial, b->xs + b->tn, s);
    ORD(hipGetLastError());
    // 5. the edges in CSR order
    if (b->nnz > 0) {
        uint64_t *e0, *e1;
        uint32_t *p0, *p1;
        ORD(b->alloc(&e0, b->nnz)); ORD(b->alloc(&e1, b->nnz)); ORD(b->alloc(&p0, b->nnz)); ORD(b->alloc(&p1, b->nnz));
        hipLaunchKernelGGL(k_orders_edge_keys, dim3(blocks(b->nnz)), dim3(kThreads), 0, s, keys, b->kb, b->trip_start, b->edge_tstart, edge_min,
                           b->nnz, e0, p0);
        ORD(hipGetLastError());
        ORD(sort_pairs<uint64_t>(*b, e0, e1, p0, p1, b->nnz, 32 + b->kb.bn, &b->ekeys, &b->perm, s));
    }
    ORD(hipMemcpyAsync(&b->nx, b->xs + b->tn, sizeof(int), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    *nnz = b->nnz; *nx = b->nx;
    *out = b;
    return hipSuccess;
}

#undef ORD
#define ORD(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

hipError_t orders_fill(OrdersBuild* b, uint64_t* xt, int nw64, int* ptr, int* idx, uint32_t* edge_bits, int wf, int* extra_ptr, int* extra_org,
                       int* extra_add, int32_t* order_host, int* over, hipStream_t s)
{
    const int n = b->n, nnz = b->nnz, tn = b->tn;
    *over = 0;
    ORD(hipMemsetAsync(xt, 0, (size_t)b->d * nw64 * 8, s));
    hipLaunchKernelGGL(k_orders_presence, dim3(blocks(b->g)), dim3(kThreads), 0, s, b->genes, b->g, b->gene_org, b->newid, nw64,
                       (unsigned long long*)xt);
    hipLaunchKernelGGL(k_orders_ptr, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, b->ekeys, nnz, n, ptr);
    if (nnz > 0) {
        int* xptr = b->nx > 0 ? extra_ptr : nullptr;          // (no multi-copy pair: no extras at all)
        ORD(hipMemsetAsync(edge_bits, 0, (size_t)nnz * wf * 4, s));
        hipLaunchKernelGGL(k_orders_entries, dim3(blocks(nnz)), dim3(kThreads), 0, s, b->perm, nnz, b->keys, b->kb, b->trip_start, b->edge_tstart,
                           b->xs, b->inv, idx, xptr, b->over);
        if (xptr) scan<int, OpSum<int>, false>(xptr, xptr, nnz, OpSum<int>(), 0, b->partial, xptr + nnz, s);
        hipLaunchKernelGGL(k_orders_pairs, dim3(blocks(tn)), dim3(kThreads), 0, s, b->keys, b->kb, b->trip_start, b->trip_edge, tn, b->edge_tstart,
                           b->inv, b->xs, wf, edge_bits, xptr, (const int*)nullptr, extra_org, extra_add);
    }
    ORD(hipGetLastError());
    ORD(hipMemcpyAsync(order_host, b->fam_sorted, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    ORD(hipMemcpyAsync(over, b->over, sizeof(int), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    return hipSuccess;
}

hipError_t orders_append_plan(OrdersBuild* b, const MasterDev& old, hipStream_t s, int* nnz_new)
{
    const int n = b->n, nnz_u = b->nnz;
    int* flag_total;                                          // rank[nnz_u]: the edges the old master does not have
    ORD(b->alloc(&b->oldpos, nnz_u)); ORD(b->alloc(&b->rank, (size_t)nnz_u + 1)); ORD(b->alloc(&b->ptr_u, (size_t)n + 1));
    flag_total = b->rank + nnz_u;
    if (nnz_u > 0) {
        hipLaunchKernelGGL(k_append_lookup, dim3(blocks(nnz_u)), dim3(kThreads), 0, s, b->keys, b->kb, b->trip_start, b->edge_tstart, nnz_u,
                           old.n, old.nei_ptr, old.nei_idx, b->oldpos);
        hipLaunchKernelGGL(k_append_isnew, dim3(blocks(nnz_u)), dim3(kThreads), 0, s, b->perm, b->oldpos, nnz_u, b->rank);
    }
    scan<int, OpSum<int>, false>(b->rank, b->rank, nnz_u, OpSum<int>(), 0, b->partial, flag_total, s);
    hipLaunchKernelGGL(k_orders_ptr, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, b->ekeys, nnz_u, n, b->ptr_u);
    ORD(hipGetLastError());
    int added = 0;
    ORD(hipMemcpyAsync(&added, flag_total, sizeof(int), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    if ((long long)old.nnz + added > 0x7fffffff) return hipErrorInvalidValue;
    *nnz_new = old.nnz + added;
    return hipSuccess;
}

hipError_t orders_append_fill(OrdersBuild* b, const MasterDev& old, int nx_old, int nnz, uint64_t* xt, int nw64, int* ptr, int* idx,
                              uint32_t* edge_bits, int wf, int* extra_ptr, int* extra_org, int* extra_add, int32_t* order_host, int* over,
                              hipStream_t s)
{
    const int n = b->n, nnz_u = b->nnz, tn = b->tn;
    const uint32_t last_mask = (old.d & 31) ? (1u << (old.d & 31)) - 1u : ~0u;
    const int* old_xptr = nx_old > 0 ? old.extra_ptr : nullptr;
    *over = 0;
    int *src, *oldx, *fwd, *partial;                          // (partial: the build's is sized by the update's genes alone)
    ORD(b->alloc(&src, nnz)); ORD(b->alloc(&oldx, nnz)); ORD(b->alloc(&fwd, old.nnz));
    ORD(b->alloc(&partial, (size_t)std::max(n, nnz) / kScanTile + 2));
    // the presence rows: the old ones at the new strides, the update's bits OR-ed in
    const long long xt_words = (long long)b->d * nw64;
    hipLaunchKernelGGL(k_append_xt, dim3(blocks(xt_words)), dim3(kThreads), 0, s, xt_words, nw64, old.d, old.nw64, old.xt, xt);
    hipLaunchKernelGGL(k_orders_presence, dim3(blocks(b->g)), dim3(kThreads), 0, s, b->genes, b->g, b->gene_org, b->newid, nw64,
                       (unsigned long long*)xt);
    // the rows: old degree + new edges
    hipLaunchKernelGGL(k_append_degree, dim3(blocks(n)), dim3(kThreads), 0, s, n, old.n, old.nei_ptr, b->ptr_u, b->rank, ptr);
    scan<int, OpSum<int>, false>(ptr, ptr, n, OpSum<int>(), 0, partial, ptr + n, s);
    if (nnz > 0) {
        if (old.nnz > 0)
            hipLaunchKernelGGL(k_append_old_entries, dim3(blocks(old.nnz)), dim3(kThreads), 0, s, old.nnz, old.n, old.nei_ptr, old.nei_idx, old_xptr,
                               ptr, idx, src, oldx, fwd, extra_ptr);
        if (nnz_u > 0)
            hipLaunchKernelGGL(k_append_new_entries, dim3(blocks(nnz_u)), dim3(kThreads), 0, s, b->perm, nnz_u, b->keys, b->kb, b->trip_start,
                               b->edge_tstart, b->xs, b->oldpos, b->rank, b->ptr_u, old.n, old.nei_ptr, old.edge_bits, old.wf, last_mask,
                               old_xptr, old.extra_add, ptr, b->inv, idx, src, oldx, extra_ptr, b->over);
        if (extra_ptr) scan<int, OpSum<int>, false>(extra_ptr, extra_ptr, nnz, OpSum<int>(), 0, partial, extra_ptr + nnz, s);
        const long long words = (long long)nnz * wf;
        hipLaunchKernelGGL(k_append_bits, dim3(blocks(words)), dim3(kThreads), 0, s, words, wf, old.wf, last_mask, src, old.edge_bits, edge_bits);
        if (nx_old > 0)
            hipLaunchKernelGGL(k_append_old_extras, dim3(blocks(nx_old)), dim3(kThreads), 0, s, nx_old, old.nnz, old.extra_ptr, old.extra_org,
                               old.extra_add, fwd, extra_ptr, extra_org, extra_add);
        if (tn > 0)
            hipLaunchKernelGGL(k_orders_pairs, dim3(blocks(tn)), dim3(kThreads), 0, s, b->keys, b->kb, b->trip_start, b->trip_edge, tn, b->edge_tstart,
                               b->inv, b->xs, wf, edge_bits, extra_ptr, (const int*)oldx, extra_org, extra_add);
    }
    ORD(hipGetLastError());
    if (n > old.n) ORD(hipMemcpyAsync(order_host, b->fam_sorted, (size_t)(n - old.n) * 4, hipMemcpyDeviceToHost, s));
    ORD(hipMemcpyAsync(over, b->over, sizeof(int), hipMemcpyDeviceToHost, s));
    ORD(hipStreamSynchronize(s));
    return hipSuccess;
}

#undef ORD

void launch_master_rows(const uint64_t* xt, int n, int wf, int d, int nw64, uint32_t* xf, hipStream_t s)
{
    hipLaunchKernelGGL(k_master_rows, dim3(nw64, wf), dim3(64), 0, s, xt, n, wf, d, nw64, xf);
}

}  // namespace nemk
