// nem_edges.hip -- see nem_edges.hpp.  The kernels, then the C entry points (nemgpu_edge_table_*): everything refused for
// its arguments alone is refused on the host before the first HIP call.
#include "nem_edges.hpp"

#include <string>
#include <vector>

#include "nem_table.hpp"

namespace nemk {

namespace {

using namespace seg;
constexpr int kNoFamily = -2;                     // a caller id that no master family has (nem_project.hip's)

__device__ inline bool fits_int32(long long v) { return v >= -2147483648ll && v <= 2147483647ll; }

// the valid bits of word w of a bit row over d organisms
__device__ inline uint32_t word_mask(int w, int d) { return (w == (d - 1) / 32 && (d & 31)) ? (1u << (d & 31)) - 1u : 0xffffffffu; }

// the count of (entry t, organism o), whose bit is set: 1 + its extra
__device__ inline int pair_count(const int* __restrict__ extra_ptr, const int* __restrict__ extra_org, const int* __restrict__ extra_add, int t, int o)
{
    if (!extra_ptr) return 1;
    const int a = extra_ptr[t], b = extra_ptr[t + 1];
    if (a == b) return 1;
    const int x = lower_bound(extra_org, a, b, o);
    return (x < b && extra_org[x] == o) ? 1 + extra_add[x] : 1;
}

// ---- the edges ---------------------------------------------------------------------------------------------------
// up[t] = 1 for a CSR entry with idx >= row: an edge of nx.Graph.edges()
__global__ __launch_bounds__(kThreads) void k_edges_up(const int* __restrict__ ptr, const int* __restrict__ idx, int n, int nnz, int* __restrict__ up)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < nnz) up[t] = idx[t] >= last_le(ptr, n, t) ? 1 : 0;
}

// every edge's ends and entry, and its key (src, dst) with its number (upx: the exclusive scan of up)
__global__ __launch_bounds__(kThreads) void k_edges_list(const int* __restrict__ ptr, const int* __restrict__ idx, int n, int nnz,
                                                        const int* __restrict__ up, const int* __restrict__ upx, int bn, uint64_t* __restrict__ ekey,
                                                        uint32_t* __restrict__ eval, int* __restrict__ src, int* __restrict__ dst,
                                                        int* __restrict__ entry)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= nnz || !up[t]) return;
    const int r = last_le(ptr, n, t), j = idx[t], e = upx[t];
    src[e] = r; dst[e] = j; entry[e] = t;
    ekey[e] = ((uint64_t)(uint32_t)r << bn) | (uint64_t)(uint32_t)j;
    eval[e] = (uint32_t)e;
}

// the set bits of the edges' rows and the number of their extras: totals[0], totals[1]
__global__ __launch_bounds__(kThreads) void k_edges_popcount(const uint32_t* __restrict__ bits, const int* __restrict__ up, long long words, int wf, int d,
                                                            const int* __restrict__ extra_ptr, unsigned long long* totals)
{
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    int cnt = 0, xs = 0;
    if (q < words) {
        const int t = (int)(q / wf), w = (int)(q % wf);
        if (up[t]) {
            cnt = __popc(bits[q] & word_mask(w, d));
            if (w == 0 && extra_ptr) xs = extra_ptr[t + 1] - extra_ptr[t];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { cnt += __shfl_down(cnt, off); xs += __shfl_down(xs, off); }
    if (lane_id() == 0 && cnt) atomicAdd(&totals[0], (unsigned long long)cnt);
    if (lane_id() == 0 && xs) atomicAdd(&totals[1], (unsigned long long)xs);
}

// ---- the links ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_edges_kept(const int* __restrict__ genes, int g, const uint8_t* __restrict__ repeated, int* __restrict__ last)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < g) last[p] = (repeated && repeated[genes[p]]) ? -1 : p;
}

// one lane per gene (last: the inclusive max-scan of k_edges_kept's): its family key (family, gene length) and, where it
// ends a link, the link's keys (edge, organism) and (edge, length); everything else sorts behind every edge / family
__global__ __launch_bounds__(kThreads) void k_edges_links(const int* __restrict__ genes, const int* __restrict__ gstart, const int* __restrict__ gend, int g,
                                                         const int* __restrict__ last, const int* __restrict__ cptr, int c,
                                                         const int* __restrict__ corg, const int* __restrict__ csize, const int* __restrict__ inv,
                                                         int n, const uint64_t* __restrict__ ekeys, const uint32_t* __restrict__ evals, int ne, int bn,
                                                         int bd, uint64_t* __restrict__ key_org, uint64_t* __restrict__ key_len,
                                                         uint64_t* __restrict__ key_fam, int* flags)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    uint64_t ko = (uint64_t)(uint32_t)ne << bd, kl = (uint64_t)(uint32_t)ne << 32, kf = (uint64_t)(uint32_t)n << 32;
    int bad = 0;
    if (last[p] == p) {
        const int fam = inv[genes[p]];
        if (fam == kNoFamily) {
            bad |= kEdgesNoFamily;
        } else {
            const long long glen = (long long)gend[p] - (long long)gstart[p];
            if (!fits_int32(glen)) bad |= kEdgesLength;
            else kf = ((uint64_t)(uint32_t)fam << 32) | (uint64_t)((uint32_t)(int)glen ^ kLenBias);
            const int j = last_le(cptr, c, p), start = cptr[j], end = cptr[j + 1];
            const int prev = p > 0 ? last[p - 1] : -1;
            int other = -1;
            long long len = 0;
            if (prev >= start) { other = prev; len = (long long)gstart[p] - (long long)gend[prev]; }                       // ppanggolin.py:513
            else if (csize[j] >= 0) { other = last[end - 1]; len = ((long long)csize[j] - (long long)gend[other]) + (long long)gstart[p]; }   // :518-519
            const int fb = other >= 0 ? inv[genes[other]] : kNoFamily;
            if (other >= 0 && fb != kNoFamily) {
                const int a = min(fam, fb), b = max(fam, fb);
                const uint64_t key = ((uint64_t)(uint32_t)a << bn) | (uint64_t)(uint32_t)b;
                const int at = lower_bound(ekeys, 0, ne, key);
                if (at >= ne || ekeys[at] != key) bad |= kEdgesNoEdge;
                else if (!fits_int32(len)) bad |= kEdgesLength;
                else {
                    const uint64_t e = evals[at];
                    ko = (e << bd) | (uint64_t)(uint32_t)corg[j];
                    kl = (e << 32) | (uint64_t)((uint32_t)(int)len ^ kLenBias);
                }
            }
        }
    }
    if (bad) atomicOr(flags, bad);
    key_org[p] = ko; key_len[p] = kl; key_fam[p] = kf;
}

// per sorted (edge, organism) key: head[p] = 1 where a pair starts, ehead[p] = 1 where an edge starts, multi[p] = 1 where
// the pair's count is 2 or more; the pair must have its bit and (counts known) its count in the master
__global__ __launch_bounds__(kThreads) void k_edges_pairs(const uint64_t* __restrict__ keys, int g, uint64_t none, int bd, const int* __restrict__ entry,
                                                         const uint32_t* __restrict__ bits, int wf, const int* __restrict__ extra_ptr,
                                                         const int* __restrict__ extra_org, const int* __restrict__ extra_add, int bits_only,
                                                         int* flags, int* __restrict__ head, int* __restrict__ ehead, int* __restrict__ multi)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const uint64_t k = keys[p];
    const bool h = is_head(keys, p, none);
    const bool eh = k < none && (p == 0 || (keys[p - 1] >> bd) != (k >> bd));
    int copies = 0;
    if (h) {
        const int e = (int)(k >> bd), org = (int)(k & ((1ull << bd) - 1ull));
        const int t = entry[e];
        copies = lower_bound(keys, p, g, k + 1) - p;
        if (!((bits[(size_t)t * wf + (org >> 5)] >> (org & 31)) & 1u)) atomicOr(flags, (int)kEdgesNoBit);
        else if (!bits_only && pair_count(extra_ptr, extra_org, extra_add, t, org) != copies) atomicOr(flags, (int)kEdgesCount);
    }
    head[p] = h ? 1 : 0;
    ehead[p] = eh ? 1 : 0;
    multi[p] = copies >= 2 ? 1 : 0;
}

// the two middle distinct lengths of the segment at sorted positions [a, b) of (segment, length) keys (didx: the scan of
// their distinct flags): the m-th distinct length (from 0) starts at the first position whose inclusive count is
// base + m + 1; no length: zeros
__device__ inline void middles(const uint64_t* __restrict__ key_len, const int* __restrict__ didx, int a, int b, int* lo, int* hi)
{
    const int base = before(didx, a), cnt = before(didx, b) - base;
    const int plo = lower_bound(didx, a, b, base + (cnt - 1) / 2 + 1);
    const int phi = lower_bound(didx, plo, b, base + cnt / 2 + 1);
    *lo = cnt > 0 ? (int)((uint32_t)key_len[plo] ^ kLenBias) : 0;
    *hi = cnt > 0 ? (int)((uint32_t)key_len[phi] ^ kLenBias) : 0;
}

// per edge its row of the table from the scans at its segment's ends (rid: the scan of the pairs' heads, for the weight)
__global__ __launch_bounds__(kThreads) void k_edges_rows(const int* __restrict__ sstart, const int* __restrict__ rid, const int* __restrict__ didx,
                                                        const long long* __restrict__ dsum, const uint64_t* __restrict__ key_len, EdgeTableDev t)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= t.ne) return;
    const int a = sstart[i], b = sstart[i + 1];
    t.weight[i] = before(rid, b) - before(rid, a);
    length_stats(key_len, didx, dsum, a, b, &t.len_distinct[i], &t.len_sum[i], &t.len_min[i], &t.len_max[i]);
    middles(key_len, didx, a, b, &t.len_mid_lo[i], &t.len_mid_hi[i]);
}

// per family the middles of its genes' distinct lengths
__global__ __launch_bounds__(kThreads) void k_edges_family(int n, const int* __restrict__ sstart, const int* __restrict__ didx,
                                                          const uint64_t* __restrict__ key_fam, int* __restrict__ mid_lo, int* __restrict__ mid_hi)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) middles(key_fam, didx, sstart[i], sstart[i + 1], &mid_lo[i], &mid_hi[i]);
}

// one block per word of 32 organisms: the first edge, in edge order, that carries each
__global__ __launch_bounds__(kThreads) void k_edges_first(const int* __restrict__ entry, int ne, const uint32_t* __restrict__ bits, int wf, int d,
                                                         int* __restrict__ first)
{
    __shared__ uint32_t s_tot[kThreads / 64];
    const int w = blockIdx.x;
    const uint32_t full = word_mask(w, d);
    if (threadIdx.x < 32 && w * 32 + (int)threadIdx.x < d) first[w * 32 + threadIdx.x] = ne;
    __syncthreads();
    uint32_t carry = 0;
    for (int base = 0; base < ne && carry != full; base += kThreads) {
        const int e = base + threadIdx.x;
        const uint32_t v = e < ne ? bits[(size_t)entry[e] * wf + w] & full : 0u;
        uint32_t all;
        const uint32_t ex = block_exclusive(v, OpOr(), 0u, s_tot, &all);
        uint32_t fresh = v & ~(carry | ex);
        while (fresh) { first[w * 32 + (__ffs((int)fresh) - 1)] = e; fresh &= fresh - 1u; }
        carry |= all;
    }
}

// ---- the <attvalue> text -----------------------------------------------------------------------------------------
// a line: 10 spaces, <attvalue for=", the id, " value=", the count, " />, a newline
constexpr int kLineFixed = 39, kLineMax = kLineFixed + 20;
constexpr int kStageWords = (64 * kLineMax + 8 + 7) / 8;      // a wave's 64 lines in LDS, at the global alignment

__device__ inline int line_width(int id, int cnt) { return kLineFixed + digits_of(id) + digits_of(cnt); }

// one wave per edge: the bytes of its lines
__global__ __launch_bounds__(kThreads) void k_att_sizes(const int* __restrict__ entry, const uint32_t* __restrict__ bits, int wf, int d,
                                                       const int* __restrict__ extra_ptr, const int* __restrict__ extra_org,
                                                       const int* __restrict__ extra_add, const int* __restrict__ attr_id, int row0, int rows,
                                                       long long* __restrict__ sizes)
{
    const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = lane_id();
    if (r >= rows) return;
    const int t = entry[row0 + r];
    long long sum = 0;
    for (int w = lane; w < wf; w += 64) {
        uint32_t v = bits[(size_t)t * wf + w] & word_mask(w, d);
        while (v) {
            const int o = w * 32 + __ffs((int)v) - 1;
            v &= v - 1u;
            sum += line_width(attr_id[o], pair_count(extra_ptr, extra_org, extra_add, t, o));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if (lane == 0) sizes[r] = sum;
}

// one wave per edge: its lines, 64 organisms at a time (everything but the lane's own line is uniform over the wave)
__global__ __launch_bounds__(kThreads) void k_att_text(const int* __restrict__ entry, const uint32_t* __restrict__ bits, int wf, int d,
                                                      const int* __restrict__ extra_ptr, const int* __restrict__ extra_org,
                                                      const int* __restrict__ extra_add, const int* __restrict__ attr_id, int row0, int rows,
                                                      const long long* __restrict__ ends, char* __restrict__ text)
{
    __shared__ uint64_t s_txt[kThreads / 64][kStageWords];
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int r = blockIdx.x * (kThreads / 64) + wv;
    if (r >= rows) return;
    const int t = entry[row0 + r];
    long long at = r > 0 ? ends[r - 1] : 0ll;
    char* stage = (char*)s_txt[wv];
    for (int o0 = 0; o0 < d; o0 += 64) {
        const int o = o0 + lane;
        const bool has = o < d && ((bits[(size_t)t * wf + (o >> 5)] >> (o & 31)) & 1u);
        if (!__ballot(has)) continue;
        int id = 0, cnt = 0, width = 0;
        if (has) { id = attr_id[o]; cnt = pair_count(extra_ptr, extra_org, extra_add, t, o); width = line_width(id, cnt); }
        int inc = width;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
        const int len = __shfl(inc, 63);
        if (has) {
            char* q = stage + (int)(at & 7) + (inc - width);
            const char* a = "          <attvalue for=\"";
            for (int k = 0; k < 25; k++) q[k] = a[k];
            q = put_digits(q + 25, id);
            const char* b = "\" value=\"";
            for (int k = 0; k < 9; k++) q[k] = b[k];
            q = put_digits(q + 9, cnt);
            const char* e = "\" />\n";
            for (int k = 0; k < 5; k++) q[k] = e[k];
        }
        store_run(text, at, len, true, [&](int k, int) { return s_txt[wv][k]; });
        at += len;
    }
}

}  // namespace

hipError_t edge_table(const MasterDev& m, const EdgesIn& in, EdgeTableDev* t, int* mismatch, hipStream_t s)
{
    const int n = m.n, d = m.d, nnz = m.nnz, wf = m.wf, g = in.o.g, c = in.o.c;
    *mismatch = kEdgesOk;
    t->n = n; t->d = d; t->ne = 0;
    Scratch mem;
    // the edges
    int *up, *upx, *partial, *totals;
    unsigned long long* ones;
    HIPTRY(mem.alloc(&up, nnz)); HIPTRY(mem.alloc(&upx, nnz)); HIPTRY(mem.alloc(&partial, (size_t)std::max(nnz, g) / kScanTile + 2)); HIPTRY(mem.alloc(&totals, 4));
    HIPTRY(mem.alloc(&ones, 2));
    HIPTRY(hipMemsetAsync(ones, 0, 16, s));
    HIPTRY(hipMemsetAsync(totals, 0, 16, s));
    if (nnz > 0) hipLaunchKernelGGL(k_edges_up, dim3(blocks(nnz)), dim3(kThreads), 0, s, m.nei_ptr, m.nei_idx, n, nnz, up);
    scan<int, OpSum<int>, false>(up, upx, nnz, OpSum<int>(), 0, partial, totals, s);
    HIPTRY(hipGetLastError());
    int ne = 0;
    HIPTRY(hipMemcpyAsync(&ne, totals, 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    t->ne = ne;
    HIPTRY(dev_alloc(&t->src, ne)); HIPTRY(dev_alloc(&t->dst, ne)); HIPTRY(dev_alloc(&t->entry, ne));
    const int bn = bits_for(n), bd = bits_for(d), be = bits_for(ne + 1), bn1 = bits_for(n + 1);
    uint64_t *ek0, *ek1;
    uint32_t *ev0, *ev1;
    HIPTRY(mem.alloc(&ek0, ne)); HIPTRY(mem.alloc(&ek1, ne)); HIPTRY(mem.alloc(&ev0, ne)); HIPTRY(mem.alloc(&ev1, ne));
    const uint64_t* ekeys = ek0;
    const uint32_t* evals = ev0;
    if (ne > 0) {
        hipLaunchKernelGGL(k_edges_list, dim3(blocks(nnz)), dim3(kThreads), 0, s, m.nei_ptr, m.nei_idx, n, nnz, (const int*)up, (const int*)upx, bn, ek0, ev0,
                           t->src, t->dst, t->entry);
        const long long words = (long long)nnz * wf;
        hipLaunchKernelGGL(k_edges_popcount, dim3(blocks(words)), dim3(kThreads), 0, s, m.edge_bits, (const int*)up, words, wf, d, m.extra_ptr, ones);
        HIPTRY(hipGetLastError());
        HIPTRY(sort_pairs<uint64_t>(mem, ek0, ek1, ev0, ev1, ne, 2 * bn, &ekeys, &evals, s));
    }
    // the links
    GeneOrdersDev o;
    int *gstart, *gend, *csize, *last, *flags;
    HIPTRY(mem.alloc(&gstart, g)); HIPTRY(mem.alloc(&gend, g)); HIPTRY(mem.alloc(&csize, c)); HIPTRY(mem.alloc(&last, g)); HIPTRY(mem.alloc(&flags, 1));
    HIPTRY(hipMemcpyAsync(gstart, in.gene_start, (size_t)g * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(gend, in.gene_end, (size_t)g * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(csize, in.contig_size, (size_t)c * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemsetAsync(flags, 0, 4, s));
    HIPTRY(upload_orders(mem, in.o, n, s, &o));                   // (last: its kernels behind every copy, as before)
    hipLaunchKernelGGL(k_edges_kept, dim3(blocks(g)), dim3(kThreads), 0, s, (const int*)o.genes, g, (const uint8_t*)o.rep, last);
    scan<int, OpMax, true>(last, last, g, OpMax(), -1, partial, (int*)nullptr, s);
    uint64_t *ka0, *ka1, *kb0, *kb1, *kc0, *kc1;
    HIPTRY(mem.alloc(&ka0, g)); HIPTRY(mem.alloc(&ka1, g)); HIPTRY(mem.alloc(&kb0, g));
    HIPTRY(mem.alloc(&kb1, g)); HIPTRY(mem.alloc(&kc0, g)); HIPTRY(mem.alloc(&kc1, g));
    hipLaunchKernelGGL(k_edges_links, dim3(blocks(g)), dim3(kThreads), 0, s, (const int*)o.genes, (const int*)gstart, (const int*)gend, g, (const int*)last,
                       (const int*)o.cptr, c, (const int*)o.corg, (const int*)csize, (const int*)o.inv, n, ekeys, evals, ne, bn, bd, ka0, kb0, kc0, flags);
    HIPTRY(hipGetLastError());
    const uint64_t *ks_org, *ks_len, *ks_fam;
    HIPTRY(sort_keys<uint64_t>(mem, ka0, ka1, g, bd + be, &ks_org, s));
    HIPTRY(sort_keys<uint64_t>(mem, kb0, kb1, g, 32 + be, &ks_len, s));
    HIPTRY(sort_keys<uint64_t>(mem, kc0, kc1, g, 32 + bn1, &ks_fam, s));
    // the (edge, organism, count) triples against the master's
    const uint64_t none_org = (uint64_t)(uint32_t)ne << bd, none_len = (uint64_t)(uint32_t)ne << 32, none_fam = (uint64_t)(uint32_t)n << 32;
    int *head, *ehead, *multi, *rid;
    HIPTRY(mem.alloc(&head, g)); HIPTRY(mem.alloc(&ehead, g)); HIPTRY(mem.alloc(&multi, g)); HIPTRY(mem.alloc(&rid, g));
    hipLaunchKernelGGL(k_edges_pairs, dim3(blocks(g)), dim3(kThreads), 0, s, ks_org, g, none_org, bd, (const int*)t->entry, m.edge_bits, wf, m.extra_ptr,
                       m.extra_org, m.extra_add, in.bits_only ? 1 : 0, flags, head, ehead, multi);
    scan<int, OpSum<int>, true>(head, rid, g, OpSum<int>(), 0, partial, totals + 1, s);
    scan<int, OpSum<int>, true>(ehead, ehead, g, OpSum<int>(), 0, partial, totals + 2, s);
    scan<int, OpSum<int>, true>(multi, multi, g, OpSum<int>(), 0, partial, totals + 3, s);
    HIPTRY(hipGetLastError());
    int h_flags = 0, h_totals[4] = {0, 0, 0, 0};
    unsigned long long h_ones[2] = {0, 0};
    HIPTRY(hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(h_totals, totals, 16, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(h_ones, ones, 16, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    if ((unsigned long long)h_totals[1] != h_ones[0] || h_totals[2] != ne) h_flags |= kEdgesMissing;
    if (!in.bits_only && (unsigned long long)h_totals[3] != h_ones[1]) h_flags |= kEdgesCount;
    if (h_flags) { *mismatch = h_flags; return hipSuccess; }
    // the table's arrays
    HIPTRY(dev_alloc(&t->weight, ne)); HIPTRY(dev_alloc(&t->len_min, ne)); HIPTRY(dev_alloc(&t->len_max, ne)); HIPTRY(dev_alloc(&t->len_distinct, ne));
    HIPTRY(dev_alloc(&t->len_sum, ne)); HIPTRY(dev_alloc(&t->len_mid_lo, ne)); HIPTRY(dev_alloc(&t->len_mid_hi, ne));
    HIPTRY(dev_alloc(&t->fam_mid_lo, n)); HIPTRY(dev_alloc(&t->fam_mid_hi, n)); HIPTRY(dev_alloc(&t->org_first_edge, d));
    int* sstart;
    SegLengths sl;
    HIPTRY(mem.alloc(&sstart, (size_t)std::max(ne, n) + 1)); HIPTRY(sl.alloc(mem, g));
    // per edge
    hipLaunchKernelGGL(k_seg_starts<uint64_t>, dim3(blocks((long long)ne + 1)), dim3(kThreads), 0, s, ks_org, g, bd, ne, sstart);
    sl.run(ks_len, g, none_len, true, s);
    if (ne > 0)
        hipLaunchKernelGGL(k_edges_rows, dim3(blocks(ne)), dim3(kThreads), 0, s, (const int*)sstart, (const int*)rid, (const int*)sl.didx,
                           (const long long*)sl.dsum, ks_len, *t);
    // per family (the kept genes' positions in the family keys; the stream orders the reuse of the scans' buffers)
    hipLaunchKernelGGL(k_seg_starts<uint64_t>, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, ks_fam, g, 32, n, sstart);
    sl.run(ks_fam, g, none_fam, false, s);
    hipLaunchKernelGGL(k_edges_family, dim3(blocks(n)), dim3(kThreads), 0, s, n, (const int*)sstart, (const int*)sl.didx, ks_fam, t->fam_mid_lo,
                       t->fam_mid_hi);
    // per organism
    hipLaunchKernelGGL(k_edges_first, dim3(wf), dim3(kThreads), 0, s, (const int*)t->entry, ne, m.edge_bits, wf, d, t->org_first_edge);
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(s));
    return hipSuccess;
}

void launch_att_sizes(const MasterDev& m, const EdgeTableDev& t, const int* attr_id, int row0, int rows, long long* sizes, hipStream_t s)
{
    hipLaunchKernelGGL(k_att_sizes, dim3((rows + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, (const int*)t.entry, m.edge_bits, m.wf, m.d,
                       m.extra_ptr, m.extra_org, m.extra_add, attr_id, row0, rows, sizes);
}

void launch_att_text(const MasterDev& m, const EdgeTableDev& t, const int* attr_id, int row0, int rows, const long long* ends, char* text,
                     hipStream_t s)
{
    hipLaunchKernelGGL(k_att_text, dim3((rows + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, (const int*)t.entry, m.edge_bits, m.wf, m.d,
                       m.extra_ptr, m.extra_org, m.extra_add, attr_id, row0, rows, ends, text);
}

}  // namespace nemk

using namespace nemk;

// An edge table on the device with the buffers of its text calls, kept for the next call
struct nemgpu_edge_table {
    int device = 0;
    EdgeTableDev dev{};
    int* attr = nullptr;                              // [d]
    long long* ends = nullptr;                        // [ends_cap + 1]: a batch's edge ends, then its size
    long long* partial = nullptr;
    size_t ends_cap = 0;
    TableText txt;
    EdgeMetaDev meta{};                               // nemgpu_edge_table_metadata's; n_attr 0: none
};

namespace {

void meta_free(EdgeMetaDev* v)
{
    void* all[] = {v->attr_id, v->n_values, v->rank, v->mask_off, v->val_base, v->val_ptr, v->blob};
    for (void* p : all) if (p) (void)hipFree(p);
    *v = EdgeMetaDev{};
}

void table_free(nemgpu_edge_table* t)
{
    EdgeTableDev& v = t->dev;
    void* all[] = {v.src, v.dst, v.entry, v.weight, v.len_min, v.len_max, v.len_distinct, v.len_sum, v.len_mid_lo, v.len_mid_hi, v.fam_mid_lo,
                   v.fam_mid_hi, v.org_first_edge, t->attr, t->ends, t->partial, t->txt.text};
    for (void* p : all) if (p) (void)hipFree(p);
    meta_free(&t->meta);
    delete t;
}

// room for a batch's edge ends and their scan's tile totals
int ends_room(nemgpu_edge_table* t, int rows)
{
    if (t->ends_cap >= (size_t)rows) return NEMGPU_OK;
    if (t->ends) (void)hipFree(t->ends);
    if (t->partial) (void)hipFree(t->partial);
    t->ends = nullptr; t->partial = nullptr; t->ends_cap = 0;
    HIPCHK(hipMalloc((void**)&t->ends, ((size_t)rows + 1) * 8));
    HIPCHK(hipMalloc((void**)&t->partial, ((size_t)rows / seg::kScanTile + 2) * 8));
    t->ends_cap = (size_t)rows;
    return NEMGPU_OK;
}

// what both text calls check and compute: the batch's edge ends on the device (t->ends) and its size
int batch_sizes(const std::string& who, nemgpu_edge_table* t, const nemgpu_master* m, const int32_t* attr_id, int row0, int rows, int64_t* bytes)
{
    { const int r = check_batch(who, m, t->dev.n, t->dev.d, t->device, row0, rows, t->dev.ne); if (r != NEMGPU_OK) return r; }
    for (int o = 0; o < t->dev.d; o++)
        if (attr_id[o] < 0) { set_error(who + ": attr_id " + std::to_string(o) + " is negative"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(t->device));
    if (!t->attr) HIPCHK(hipMalloc((void**)&t->attr, (size_t)t->dev.d * 4));
    { const int r = ends_room(t, rows); if (r != NEMGPU_OK) return r; }
    HIPCHK(hipMemcpyAsync(t->attr, attr_id, (size_t)t->dev.d * 4, hipMemcpyHostToDevice, m->stream));
    launch_att_sizes(m->dev, t->dev, t->attr, row0, rows, t->ends, m->stream);
    seg::scan<long long, seg::OpSum<long long>, true>(t->ends, t->ends, rows, seg::OpSum<long long>(), 0ll, t->partial, t->ends + rows, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bytes, t->ends + rows, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return NEMGPU_OK;
}

// what the metadata calls check and compute: the batch's present-value masks (*masks, mem's), from them its edge ends
// on the device (t->ends) and its size
int meta_batch(const std::string& who, nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, seg::Scratch& mem, uint32_t** masks,
               int64_t* bytes)
{
    { const int r = check_batch(who, m, t->dev.n, t->dev.d, t->device, row0, rows, t->dev.ne); if (r != NEMGPU_OK) return r; }
    if (!t->meta.n_attr) { set_error(who + ": the table has no metadata (nemgpu_edge_table_metadata)"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(t->device));
    { const int r = ends_room(t, rows); if (r != NEMGPU_OK) return r; }
    HIPCHK(mem.alloc(masks, (size_t)rows * t->meta.mask_words));
    launch_meta_masks(m->dev, t->dev, t->meta, row0, rows, *masks, m->stream);
    if (!bytes) return NEMGPU_OK;
    launch_meta_sizes(t->meta, rows, *masks, t->ends, m->stream);
    seg::scan<long long, seg::OpSum<long long>, true>(t->ends, t->ends, rows, seg::OpSum<long long>(), 0ll, t->partial, t->ends + rows, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bytes, t->ends + rows, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return NEMGPU_OK;
}

template <class T> hipError_t upload(T** dev, const T* host, size_t count)
{
    HIPTRY(seg::dev_alloc(dev, count));
    return count ? hipMemcpy(*dev, host, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}

}  // namespace

int nemgpu_edge_table_create(nemgpu_edge_table** out, const nemgpu_master* m, int f, const int32_t* genes, const int32_t* gene_start,
                             const int32_t* gene_end, int g, const int32_t* contig_ptr, const int32_t* contig_org, const int32_t* contig_size,
                             int c, const uint8_t* repeated)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!m) return NEMGPU_E_FUNCARG;
    if (f <= 0 || g <= 0 || c <= 0 || !genes || !gene_start || !gene_end || !contig_ptr || !contig_org || !contig_size) {
        set_error("nemgpu_edge_table_create: f > 0, the genes, their starts and ends, the contigs and their sizes are needed"); return NEMGPU_E_FUNCARG;
    }
    { const int r = check_orders(true, m->d, f, g, c, genes, contig_ptr, contig_org, nullptr); if (r != NEMGPU_OK) return r; }
    for (int j = 1; j < c; j++)
        if (contig_org[j] < contig_org[j - 1]) {
            set_error("orders: contig " + std::to_string(j) + ": contig_org must be non-decreasing (the organisms walked in column order)");
            return NEMGPU_E_ARG;
        }
    if (m->directed) {
        set_error("nemgpu_edge_table_create: the master was built directed (edges() of a DiGraph is another walk, and the master cannot tell "
                  "sens from antisens)");
        return NEMGPU_E_ARG;
    }
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    nemgpu_edge_table* t = new nemgpu_edge_table();
    t->device = m->device;
    const EdgesIn in{{f, g, c, genes, contig_ptr, contig_org, repeated, m->order.empty() ? nullptr : m->order.data()}, gene_start, gene_end,
                     contig_size, m->bits_only};
    int mismatch = 0;
    const hipError_t err = edge_table(m->dev, in, &t->dev, &mismatch, m->stream);
    if (err != hipSuccess) { table_free(t); return device_status("nemgpu_edge_table_create", err); }
    if (mismatch & kEdgesLength) {
        table_free(t);
        set_error("nemgpu_edge_table_create: a link's or a gene's length is outside int32");
        return NEMGPU_E_ARG;
    }
    if (mismatch) {
        table_free(t);
        set_error(std::string("nemgpu_edge_table_create: these orders are not this master's: ") +
                  ((mismatch & kEdgesNoFamily) ? "a kept gene's family is not in the master"
                   : (mismatch & kEdgesNoEdge) ? "two adjacent kept genes' families are not an edge of the master"
                   : (mismatch & kEdgesNoBit)  ? "an edge has a link in an organism where the master's edge bit is clear"
                   : (mismatch & kEdgesCount)  ? "an (edge, organism) pair's number of links is not the master's count"
                                               : "the master has an edge, or an edge bit, where the orders have no link"));
        return NEMGPU_E_ARG;
    }
    *out = t;
    return NEMGPU_OK;
}

int nemgpu_edge_table_shape(const nemgpu_edge_table* t, int* n, int* d, int* n_edges)
{
    if (!t) return NEMGPU_E_FUNCARG;
    if (n) *n = t->dev.n;
    if (d) *d = t->dev.d;
    if (n_edges) *n_edges = t->dev.ne;
    return NEMGPU_OK;
}

int nemgpu_edge_table_fetch(const nemgpu_edge_table* t, int32_t* src, int32_t* dst, int32_t* weight, int32_t* len_min, int32_t* len_max,
                            int32_t* len_distinct, int64_t* len_sum, int32_t* len_mid_lo, int32_t* len_mid_hi, int32_t* fam_mid_lo,
                            int32_t* fam_mid_hi, int32_t* org_first_edge)
{
    if (!t) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(t->device));
    const EdgeTableDev& v = t->dev;
    const size_t ne = (size_t)v.ne, n = (size_t)v.n, d = (size_t)v.d;
    if (src && ne) HIPCHK(hipMemcpy(src, v.src, ne * 4, hipMemcpyDeviceToHost));
    if (dst && ne) HIPCHK(hipMemcpy(dst, v.dst, ne * 4, hipMemcpyDeviceToHost));
    if (weight && ne) HIPCHK(hipMemcpy(weight, v.weight, ne * 4, hipMemcpyDeviceToHost));
    if (len_min && ne) HIPCHK(hipMemcpy(len_min, v.len_min, ne * 4, hipMemcpyDeviceToHost));
    if (len_max && ne) HIPCHK(hipMemcpy(len_max, v.len_max, ne * 4, hipMemcpyDeviceToHost));
    if (len_distinct && ne) HIPCHK(hipMemcpy(len_distinct, v.len_distinct, ne * 4, hipMemcpyDeviceToHost));
    if (len_sum && ne) HIPCHK(hipMemcpy(len_sum, v.len_sum, ne * 8, hipMemcpyDeviceToHost));
    if (len_mid_lo && ne) HIPCHK(hipMemcpy(len_mid_lo, v.len_mid_lo, ne * 4, hipMemcpyDeviceToHost));
    if (len_mid_hi && ne) HIPCHK(hipMemcpy(len_mid_hi, v.len_mid_hi, ne * 4, hipMemcpyDeviceToHost));
    if (fam_mid_lo) HIPCHK(hipMemcpy(fam_mid_lo, v.fam_mid_lo, n * 4, hipMemcpyDeviceToHost));
    if (fam_mid_hi) HIPCHK(hipMemcpy(fam_mid_hi, v.fam_mid_hi, n * 4, hipMemcpyDeviceToHost));
    if (org_first_edge) HIPCHK(hipMemcpy(org_first_edge, v.org_first_edge, d * 4, hipMemcpyDeviceToHost));
    return NEMGPU_OK;
}

int nemgpu_edge_table_attvalues_size(nemgpu_edge_table* t, const nemgpu_master* m, const int32_t* attr_id, int row0, int rows, int64_t* bytes)
{
    if (!t || !m || !attr_id || !bytes) return NEMGPU_E_FUNCARG;
    int64_t size = 0;
    const int r = batch_sizes("nemgpu_edge_table_attvalues_size", t, m, attr_id, row0, rows, &size);
    if (r == NEMGPU_OK) *bytes = size;
    return r;
}

int nemgpu_edge_table_attvalues(nemgpu_edge_table* t, const nemgpu_master* m, const int32_t* attr_id, int row0, int rows, char* text,
                                int64_t capacity, int64_t* needed, int64_t* edge_end)
{
    if (!t || !m || !attr_id || !text || !edge_end) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_edge_table_attvalues";
    int64_t bytes = 0;
    { const int r = batch_sizes(who, t, m, attr_id, row0, rows, &bytes); if (r != NEMGPU_OK) return r; }
    { const int r = text_room(who, &t->txt, capacity, bytes, needed); if (r != NEMGPU_OK) return r; }
    launch_att_text(m->dev, t->dev, t->attr, row0, rows, t->ends, t->txt.text, m->stream);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(edge_end, t->ends, (size_t)rows * 8, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(text, t->txt.text, (size_t)bytes, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    return device_status(who, err);
}

int nemgpu_edge_table_metadata(nemgpu_edge_table* t, int n_attr, const int32_t* attr_id, const int32_t* value_rank, const int32_t* n_values,
                               const int64_t* value_ptr, const char* value_text)
{
    if (!t || !attr_id || !value_rank || !n_values || !value_ptr) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_edge_table_metadata";
    const int d = t->dev.d;
    if (n_attr <= 0) { set_error(who + ": n_attr > 0"); return NEMGPU_E_ARG; }
    std::vector<int> mask_off((size_t)n_attr + 1, 0), val_base((size_t)n_attr, 0);
    long long values = 0, words = 0;
    for (int a = 0; a < n_attr; a++) {
        if (attr_id[a] < 0) { set_error(who + ": attr_id " + std::to_string(a) + " is negative"); return NEMGPU_E_ARG; }
        if (n_values[a] < 1 || n_values[a] > kMetaValuesMax) {
            set_error(who + ": attribute " + std::to_string(a) + " has " + std::to_string(n_values[a]) + " values, 1 .. " +
                      std::to_string(kMetaValuesMax) + " are held");
            return NEMGPU_E_ARG;
        }
        for (int o = 0; o < d; o++) {
            const int v = value_rank[(size_t)a * d + o];
            if (v < 0 || v >= n_values[a]) {
                set_error(who + ": attribute " + std::to_string(a) + ", organism " + std::to_string(o) + ": rank " + std::to_string(v) + " outside its " +
                          std::to_string(n_values[a]) + " values");
                return NEMGPU_E_ARG;
            }
        }
        val_base[a] = (int)values;
        values += n_values[a];
        words += (n_values[a] + 31) / 32;
        if (values > kMetaTextMax) { set_error(who + ": too many values"); return NEMGPU_E_ARG; }
        mask_off[(size_t)a + 1] = (int)words;
    }
    if (value_ptr[0] != 0) { set_error(who + ": value_ptr must start at 0"); return NEMGPU_E_ARG; }
    for (long long v = 0; v < values; v++)
        if (value_ptr[v + 1] < value_ptr[v]) { set_error(who + ": value_ptr must ascend (value " + std::to_string(v) + ")"); return NEMGPU_E_ARG; }
    const long long bytes = value_ptr[values];
    if (bytes + values > kMetaTextMax) {
        set_error(who + ": the values take " + std::to_string(bytes) + " bytes, with their number at most " + std::to_string(kMetaTextMax));
        return NEMGPU_E_ARG;
    }
    if (bytes && !value_text) return NEMGPU_E_FUNCARG;
    std::vector<int> ptr((size_t)values + 1);
    for (long long v = 0; v <= values; v++) ptr[(size_t)v] = (int)value_ptr[v];
    note_hip_used();
    HIPCHK(hipSetDevice(t->device));
    meta_free(&t->meta);
    EdgeMetaDev v;
    v.mask_words = (int)words;
    hipError_t err = upload(&v.attr_id, (const int*)attr_id, (size_t)n_attr);
    if (err == hipSuccess) err = upload(&v.n_values, (const int*)n_values, (size_t)n_attr);
    if (err == hipSuccess) err = upload(&v.rank, (const int*)value_rank, (size_t)n_attr * d);
    if (err == hipSuccess) err = upload(&v.mask_off, (const int*)mask_off.data(), mask_off.size());
    if (err == hipSuccess) err = upload(&v.val_base, (const int*)val_base.data(), val_base.size());
    if (err == hipSuccess) err = upload(&v.val_ptr, (const int*)ptr.data(), ptr.size());
    if (err == hipSuccess) err = upload(&v.blob, value_text, (size_t)bytes);
    if (err != hipSuccess) { meta_free(&v); return device_status(who, err); }
    v.n_attr = n_attr;
    t->meta = v;
    return NEMGPU_OK;
}

int nemgpu_edge_table_metamasks(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, uint32_t* masks)
{
    if (!t || !m || !masks) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_edge_table_metamasks";
    seg::Scratch mem;
    uint32_t* dev = nullptr;
    { const int r = meta_batch(who, t, m, row0, rows, mem, &dev, nullptr); if (r != NEMGPU_OK) return r; }
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(masks, dev, (size_t)rows * t->meta.mask_words * 4, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    return device_status(who, err);
}

int nemgpu_edge_table_metavalues_size(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, int64_t* bytes)
{
    if (!t || !m || !bytes) return NEMGPU_E_FUNCARG;
    seg::Scratch mem;
    uint32_t* masks = nullptr;
    int64_t size = 0;
    const int r = meta_batch("nemgpu_edge_table_metavalues_size", t, m, row0, rows, mem, &masks, &size);
    if (r == NEMGPU_OK) *bytes = size;
    return r;
}

int nemgpu_edge_table_metavalues(nemgpu_edge_table* t, const nemgpu_master* m, int row0, int rows, char* text, int64_t capacity, int64_t* needed,
                                 int64_t* edge_end)
{
    if (!t || !m || !text || !edge_end) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_edge_table_metavalues";
    seg::Scratch mem;
    uint32_t* masks = nullptr;
    int64_t bytes = 0;
    { const int r = meta_batch(who, t, m, row0, rows, mem, &masks, &bytes); if (r != NEMGPU_OK) return r; }
    { const int r = text_room(who, &t->txt, capacity, bytes, needed); if (r != NEMGPU_OK) return r; }
    launch_meta_text(t->meta, rows, masks, t->ends, t->txt.text, m->stream);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(edge_end, t->ends, (size_t)rows * 8, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(text, t->txt.text, (size_t)bytes, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    return device_status(who, err);
}

void nemgpu_edge_table_destroy(nemgpu_edge_table* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    table_free(t);
}
