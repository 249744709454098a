// nem_matrix.hip -- see nem_matrix.hpp.  The kernels, then the C entry points (nemgpu_family_table_*): everything refused
// for its arguments alone is refused on the host before the first HIP call.
#include "nem_matrix.hpp"

#include <string>
#include <vector>

#include "nem_table.hpp"

namespace nemk {

namespace {

using namespace seg;
constexpr int kNoFamily = -2;                     // a caller id that no master family has (nem_project.hip's)
constexpr int kRepeated = -1;                     // a gene of a repeated family

// ---- the family table ------------------------------------------------------------------------------------------
// one lane per gene: its organism (its contig's), its master family, its two keys; a gene that is not kept sorts behind
// every family in both
__global__ __launch_bounds__(kThreads) void k_matrix_keys(const int* __restrict__ genes, const int* __restrict__ glen, int g,
                                                         const int* __restrict__ cptr, int c, const int* __restrict__ corg,
                                                         const uint8_t* __restrict__ repeated, const int* __restrict__ inv, int n, int bd,
                                                         uint64_t* __restrict__ key_org, uint64_t* __restrict__ key_len, int* flags)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const int org = corg[last_le(cptr, c, p)];
    const int id = genes[p];
    const int fam = (repeated && repeated[id]) ? kRepeated : inv[id];
    if (fam == kNoFamily) atomicOr(flags, (int)kMatrixNoFamily);
    const bool kept = fam >= 0;
    key_org[p] = kept ? (((uint64_t)(uint32_t)fam << bd) | (uint64_t)(uint32_t)org) : ((uint64_t)(uint32_t)n << bd);
    key_len[p] = kept ? (((uint64_t)(uint32_t)fam << 32) | (uint64_t)((uint32_t)glen[p] ^ kLenBias)) : ((uint64_t)(uint32_t)n << 32);
}

// the set bits of the master's presence rows (families below n only)
__global__ __launch_bounds__(kThreads) void k_matrix_popcount(const uint64_t* __restrict__ xt, long long words, int nw64, int n,
                                                             unsigned long long* total)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    int cnt = 0;
    if (t < words) {
        uint64_t v = xt[t];
        if ((n & 63) && (int)(t % nw64) == nw64 - 1) v &= (1ull << (n & 63)) - 1ull;
        cnt = __popcll(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane_id() == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);
}

// per sorted (family, organism) key: head[p] = 1 where a cell starts, cnt[p] = the cell's genes there (0 elsewhere),
// multi[p] = 1 where that is 2 or more; a cell whose bit the master does not have is flagged
__global__ __launch_bounds__(kThreads) void k_matrix_cells(const uint64_t* __restrict__ keys, int g, uint64_t none, int bd,
                                                          const uint64_t* __restrict__ xt, int nw64, int* flags, int* __restrict__ head,
                                                          int* __restrict__ cnt, int* __restrict__ multi)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    const uint64_t k = keys[p];
    const bool h = is_head(keys, p, none);
    int copies = 0;
    if (h) {
        const int fam = (int)(k >> bd), org = (int)(k & ((1ull << bd) - 1ull));
        if (!((xt[(size_t)org * nw64 + (fam >> 6)] >> (fam & 63)) & 1ull)) atomicOr(flags, (int)kMatrixNotPresent);
        copies = lower_bound(keys, p, g, k + 1) - p;
    }
    head[p] = h ? 1 : 0;
    cnt[p] = copies;
    multi[p] = copies >= 2 ? 1 : 0;
}

// the cells of 2 or more, compacted in sorted order (midx: the inclusive scan of multi): organism, count, digits - 1
__global__ __launch_bounds__(kThreads) void k_matrix_multi(const uint64_t* __restrict__ keys, int g, int bd, const int* __restrict__ cnt,
                                                          const int* __restrict__ midx, int* __restrict__ multi_org,
                                                          int* __restrict__ multi_cnt, long long* __restrict__ multi_x)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g || cnt[p] < 2) return;
    const int t = midx[p] - 1;
    multi_org[t] = (int)(keys[p] & ((1ull << bd) - 1ull));
    multi_cnt[t] = cnt[p];
    multi_x[t] = digits_of(cnt[p]) - 1;
}

// per family its row of the table from the scans at its segment's ends; i = n closes multi_ptr and fam_xpre
__global__ __launch_bounds__(kThreads) void k_matrix_family(int n, const int* __restrict__ fstart, const int* __restrict__ rid,
                                                           const int* __restrict__ midx, const int* __restrict__ didx,
                                                           const long long* __restrict__ dsum, const uint64_t* __restrict__ key_len,
                                                           FamilyTableDev t)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    const int a = fstart[i];
    const int mp = before(midx, a);
    t.multi_ptr[i] = mp;
    t.fam_xpre[i] = t.multi_xpre[mp];
    if (i == n) return;
    const int b = fstart[i + 1];
    t.nb_genes[i] = b - a;
    t.nb_org[i] = before(rid, b) - before(rid, a);
    length_stats(key_len, didx, dsum, a, b, &t.len_distinct[i], &t.len_sum[i], &t.len_min[i], &t.len_max[i]);
}

// ---- the .Rtab cell block ---------------------------------------------------------------------------------------
constexpr int kTileFam = 256, kTileOrg = 256;     // a block's families (4 words of the presence rows) and organisms
constexpr int kTileWords = kTileFam / 64;
constexpr int kCellMax = 11;                      // a count below 2^30 and its separator
constexpr int kStageWords = (kTileOrg * kCellMax + 8 + 7) / 8;   // a wave's segment in LDS, at the global alignment

__global__ __launch_bounds__(kThreads) void k_rtab(const uint64_t* __restrict__ xt, int d, int nw64, const int* __restrict__ multi_ptr,
                                                  const int* __restrict__ multi_org, const int* __restrict__ multi_cnt,
                                                  const long long* __restrict__ multi_xpre, const long long* __restrict__ fam_xpre,
                                                  int row0, int rows, int tile0, char* __restrict__ text)
{
    __shared__ uint64_t s_raw[kTileOrg][kTileWords];          // organism-major, as loaded
    __shared__ uint64_t s_fam[kTileFam][kTileOrg / 64];       // family-major: bit o of a family's row = organism o0 + o
    __shared__ uint64_t s_txt[kThreads / 64][kStageWords];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int w0 = (tile0 + (int)blockIdx.x) * kTileWords;
    const int o0 = (int)blockIdx.y * kTileOrg;
    const int ncell = min(kTileOrg, d - o0);
    // adjacent lanes read adjacent words: 4 lanes per organism row
    for (int r = threadIdx.x / kTileWords; r < kTileOrg; r += kThreads / kTileWords) {
        const int w = w0 + (threadIdx.x % kTileWords), o = o0 + r;
        s_raw[r][threadIdx.x % kTileWords] = (o < d && w < nw64) ? xt[(size_t)o * nw64 + w] : 0ull;
    }
    __syncthreads();
    // the transposition: thread = family (its wave's word, its lane's bit); the reads are wave-uniform broadcasts
#pragma unroll
    for (int ow = 0; ow < kTileOrg / 64; ow++) {
        uint64_t acc = 0;
#pragma unroll 8
        for (int ob = 0; ob < 64; ob++) acc |= ((s_raw[ow * 64 + ob][wv] >> lane) & 1ull) << ob;
        s_fam[threadIdx.x][ow] = acc;
    }
    __syncthreads();
    const bool last_seg = o0 + ncell == d;
    char* stage = (char*)s_txt[wv];
    for (int j = 0; j < 64; j++) {                            // (everything below is uniform over the wave)
        const int i = (w0 + wv) * 64 + j;
        if (i < row0 || i >= row0 + rows) continue;
        const uint64_t* bits = s_fam[wv * 64 + j];
        const int pi = multi_ptr[i], pe = multi_ptr[i + 1];
        int t0 = pi, t1 = pi;                                 // the family's cells of 2 or more in this segment
        if (pe > pi) { t0 = lower_bound(multi_org, pi, pe, o0); t1 = lower_bound(multi_org, t0, pe, o0 + ncell); }
        const long long start = (long long)(i - row0) * 2 * d + (fam_xpre[i] - fam_xpre[row0]) + 2ll * o0 + (multi_xpre[t0] - multi_xpre[pi]);
        const int len = 2 * ncell + (int)(multi_xpre[t1] - multi_xpre[t0]);
        const int mis = (int)(start & 7);
        if (t0 != t1) {
            // lay the segment out in LDS at the global alignment: per cell its position, its digits, its separator
            for (int cell = lane; cell < ncell; cell += 64) {
                const int o = o0 + cell;
                const int t = lower_bound(multi_org, t0, t1, o);
                char* q = stage + mis + 2 * cell + (int)(multi_xpre[t] - multi_xpre[t0]);
                if (t < t1 && multi_org[t] == o) q = put_digits(q, multi_cnt[t]);
                else *q++ = (char)('0' + (int)((bits[cell >> 6] >> (cell & 63)) & 1ull));
                *q = (last_seg && cell == ncell - 1) ? '\n' : '\t';
            }
        }
        store_run(text, start, len, t0 != t1, [&](int k, int r0) {
            if (t0 != t1) return s_txt[wv][k];
            // every cell is one character: the word straight from the bits (cells c0 .. c0 + 4 at the most)
            const int c0 = max(r0, 0) >> 1, q = c0 >> 6, sh = c0 & 63;
            const uint64_t lo = bits[min(q, kTileOrg / 64 - 1)], hi = q + 1 < kTileOrg / 64 ? bits[q + 1] : 0ull;
            const uint64_t win = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
            uint64_t word = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const int r = r0 + b, cell = max(r, 0) >> 1;
                const int ch = (r & 1) ? ((last_seg && cell == ncell - 1) ? '\n' : '\t') : '0' + (int)((win >> (cell - c0)) & 1ull);
                word |= (uint64_t)(uint32_t)ch << (8 * b);
            }
            return word;
        });
    }
}

}  // namespace

hipError_t family_table(const MasterDev& m, const MatrixIn& in, FamilyTableDev* t, int* mismatch, hipStream_t s)
{
    const int n = m.n, d = m.d, g = in.o.g, c = in.o.c;
    *mismatch = kMatrixOk;
    t->n = n; t->d = d; t->nm = 0;
    Scratch mem;
    GeneOrdersDev o;
    int *glen, *flags;
    unsigned long long* ones;
    HIPTRY(mem.alloc(&glen, g)); HIPTRY(mem.alloc(&flags, 1)); HIPTRY(mem.alloc(&ones, 1));
    HIPTRY(hipMemcpyAsync(glen, in.gene_len, (size_t)g * 4, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemsetAsync(flags, 0, 4, s));
    HIPTRY(hipMemsetAsync(ones, 0, 8, s));
    HIPTRY(upload_orders(mem, in.o, n, s, &o));                   // (last: its kernels behind every copy, as before)
    const int bd = bits_for(d), bn = bits_for(n + 1);         // (the family field also holds n: not kept)
    const uint64_t none_org = (uint64_t)(uint32_t)n << bd, none_len = (uint64_t)(uint32_t)n << 32;
    uint64_t *ka0, *ka1, *kb0, *kb1;
    HIPTRY(mem.alloc(&ka0, g)); HIPTRY(mem.alloc(&ka1, g)); HIPTRY(mem.alloc(&kb0, g)); HIPTRY(mem.alloc(&kb1, g));
    hipLaunchKernelGGL(k_matrix_keys, dim3(blocks(g)), dim3(kThreads), 0, s, o.genes, glen, g, o.cptr, c, o.corg, o.rep, o.inv, n, bd, ka0, kb0, flags);
    const long long words = (long long)d * m.nw64;
    hipLaunchKernelGGL(k_matrix_popcount, dim3(blocks(words)), dim3(kThreads), 0, s, m.xt, words, m.nw64, n, ones);
    HIPTRY(hipGetLastError());
    const uint64_t *ks_org, *ks_len;
    HIPTRY(sort_keys<uint64_t>(mem, ka0, ka1, g, bd + bn, &ks_org, s));
    HIPTRY(sort_keys<uint64_t>(mem, kb0, kb1, g, 32 + bn, &ks_len, s));
    // the cells
    int *head, *cnt, *multi, *rid, *midx, *partial, *totals, *fstart;
    HIPTRY(mem.alloc(&head, g)); HIPTRY(mem.alloc(&cnt, g)); HIPTRY(mem.alloc(&multi, g)); HIPTRY(mem.alloc(&rid, g)); HIPTRY(mem.alloc(&midx, g));
    HIPTRY(mem.alloc(&partial, (size_t)g / kScanTile + 2)); HIPTRY(mem.alloc(&totals, 2)); HIPTRY(mem.alloc(&fstart, (size_t)n + 1));
    hipLaunchKernelGGL(k_matrix_cells, dim3(blocks(g)), dim3(kThreads), 0, s, ks_org, g, none_org, bd, m.xt, m.nw64, flags, head, cnt, multi);
    scan<int, OpSum<int>, true>(head, rid, g, OpSum<int>(), 0, partial, totals, s);
    scan<int, OpSum<int>, true>(multi, midx, g, OpSum<int>(), 0, partial, totals + 1, s);
    hipLaunchKernelGGL(k_seg_starts<uint64_t>, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, ks_org, g, bd, n, fstart);
    HIPTRY(hipGetLastError());
    int h_flags = 0, h_totals[2] = {0, 0};
    unsigned long long h_ones = 0;
    HIPTRY(hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(h_totals, totals, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(&h_ones, ones, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    if ((unsigned long long)h_totals[0] != h_ones) h_flags |= kMatrixCount;
    if (h_flags) { *mismatch = h_flags; return hipSuccess; }
    // the table's arrays
    const int nm = h_totals[1];
    t->nm = nm;
    HIPTRY(dev_alloc(&t->nb_genes, n)); HIPTRY(dev_alloc(&t->nb_org, n)); HIPTRY(dev_alloc(&t->len_min, n)); HIPTRY(dev_alloc(&t->len_max, n));
    HIPTRY(dev_alloc(&t->len_distinct, n)); HIPTRY(dev_alloc(&t->len_sum, n)); HIPTRY(dev_alloc(&t->multi_ptr, (size_t)n + 1));
    HIPTRY(dev_alloc(&t->multi_org, nm)); HIPTRY(dev_alloc(&t->multi_cnt, nm)); HIPTRY(dev_alloc(&t->multi_xpre, (size_t)nm + 1));
    HIPTRY(dev_alloc(&t->fam_xpre, (size_t)n + 1));
    long long* multi_x;
    SegLengths sl;
    HIPTRY(mem.alloc(&multi_x, nm)); HIPTRY(sl.alloc(mem, g));
    hipLaunchKernelGGL(k_matrix_multi, dim3(blocks(g)), dim3(kThreads), 0, s, ks_org, g, bd, (const int*)cnt, (const int*)midx, t->multi_org, t->multi_cnt, multi_x);
    scan<long long, OpSum<long long>, false>(multi_x, t->multi_xpre, nm, OpSum<long long>(), 0ll, sl.lpartial, t->multi_xpre + nm, s);
    // the distinct lengths
    sl.run(ks_len, g, none_len, true, s);
    hipLaunchKernelGGL(k_matrix_family, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, n, (const int*)fstart, (const int*)rid, (const int*)midx,
                       (const int*)sl.didx, (const long long*)sl.dsum, ks_len, *t);
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(s));
    return hipSuccess;
}

void launch_rtab(const MasterDev& m, const FamilyTableDev& t, int row0, int rows, char* text, hipStream_t s)
{
    const int tile0 = row0 / kTileFam, tiles = (row0 + rows - 1) / kTileFam - tile0 + 1;
    hipLaunchKernelGGL(k_rtab, dim3(tiles, (m.d + kTileOrg - 1) / kTileOrg), dim3(kThreads), 0, s, m.xt, m.d, m.nw64, (const int*)t.multi_ptr,
                       (const int*)t.multi_org, (const int*)t.multi_cnt, (const long long*)t.multi_xpre, (const long long*)t.fam_xpre, row0, rows, tile0, text);
}

}  // namespace nemk

using namespace nemk;

// A family table on the device with what the host needs of it: the lines' extra digits (fam_xpre), the text buffer
struct nemgpu_family_table {
    int device = 0;
    FamilyTableDev dev{};
    std::vector<long long> fam_xpre;                  // [n + 1]
    TableText txt;                                    // the last batch's text on the device, kept for the next
};

namespace {

void table_free(nemgpu_family_table* t)
{
    FamilyTableDev& v = t->dev;
    void* all[] = {v.nb_genes, v.nb_org, v.len_min, v.len_max, v.len_distinct, v.len_sum, v.multi_ptr, v.multi_org, v.multi_cnt,
                   v.multi_xpre, v.fam_xpre, t->txt.text};
    for (void* p : all) if (p) (void)hipFree(p);
    delete t;
}

// the end of every line of the batch, relative to its start; returns the batch's size
long long batch_ends(const nemgpu_family_table* t, int row0, int rows, int64_t* line_end)
{
    long long end = 0;
    for (int r = 0; r < rows; r++) {
        end = (long long)(r + 1) * 2 * t->dev.d + (t->fam_xpre[(size_t)row0 + r + 1] - t->fam_xpre[(size_t)row0]);
        if (line_end) line_end[r] = end;
    }
    return end;
}

}  // namespace

int nemgpu_family_table_create(nemgpu_family_table** out, const nemgpu_master* m, int f, const int32_t* genes, const int32_t* gene_len,
                               int g, const int32_t* contig_ptr, const int32_t* contig_org, int c, const uint8_t* repeated)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!m) return NEMGPU_E_FUNCARG;
    if (f <= 0 || g <= 0 || c <= 0 || !genes || !gene_len || !contig_ptr || !contig_org) {
        set_error("nemgpu_family_table_create: f > 0, the genes, their lengths and the contigs are needed"); return NEMGPU_E_FUNCARG;
    }
    { const int r = check_orders(true, m->d, f, g, c, genes, contig_ptr, contig_org, nullptr); if (r != NEMGPU_OK) return r; }
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    nemgpu_family_table* t = new nemgpu_family_table();
    t->device = m->device;
    const MatrixIn in{{f, g, c, genes, contig_ptr, contig_org, repeated, m->order.empty() ? nullptr : m->order.data()}, gene_len};
    int mismatch = 0;
    hipError_t err = family_table(m->dev, in, &t->dev, &mismatch, m->stream);
    if (err == hipSuccess && !mismatch) {
        t->fam_xpre.resize((size_t)m->n + 1);
        err = hipMemcpy(t->fam_xpre.data(), t->dev.fam_xpre, ((size_t)m->n + 1) * 8, hipMemcpyDeviceToHost);
    }
    if (err != hipSuccess) { table_free(t); return device_status("nemgpu_family_table_create", err); }
    if (mismatch) {
        table_free(t);
        set_error(std::string("nemgpu_family_table_create: these orders are not this master's: ") +
                  ((mismatch & kMatrixNoFamily) ? "a kept gene's family is not in the master"
                   : (mismatch & kMatrixNotPresent) ? "a family has a kept gene in an organism where the master's presence bit is clear"
                                                    : "the master has a presence bit where the orders have no kept gene"));
        return NEMGPU_E_ARG;
    }
    *out = t;
    return NEMGPU_OK;
}

int nemgpu_family_table_shape(const nemgpu_family_table* t, int* n, int* d, int* n_multi)
{
    if (!t) return NEMGPU_E_FUNCARG;
    if (n) *n = t->dev.n;
    if (d) *d = t->dev.d;
    if (n_multi) *n_multi = t->dev.nm;
    return NEMGPU_OK;
}

int nemgpu_family_table_fetch(const nemgpu_family_table* t, int32_t* nb_genes, int32_t* nb_org, int32_t* len_min, int32_t* len_max,
                              int32_t* len_distinct, int64_t* len_sum, int32_t* multi_ptr, int32_t* multi_org, int32_t* multi_cnt)
{
    if (!t) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(t->device));
    const FamilyTableDev& v = t->dev;
    const size_t n = (size_t)v.n, nm = (size_t)v.nm;
    if (nb_genes) HIPCHK(hipMemcpy(nb_genes, v.nb_genes, n * 4, hipMemcpyDeviceToHost));
    if (nb_org) HIPCHK(hipMemcpy(nb_org, v.nb_org, n * 4, hipMemcpyDeviceToHost));
    if (len_min) HIPCHK(hipMemcpy(len_min, v.len_min, n * 4, hipMemcpyDeviceToHost));
    if (len_max) HIPCHK(hipMemcpy(len_max, v.len_max, n * 4, hipMemcpyDeviceToHost));
    if (len_distinct) HIPCHK(hipMemcpy(len_distinct, v.len_distinct, n * 4, hipMemcpyDeviceToHost));
    if (len_sum) HIPCHK(hipMemcpy(len_sum, v.len_sum, n * 8, hipMemcpyDeviceToHost));
    if (multi_ptr) HIPCHK(hipMemcpy(multi_ptr, v.multi_ptr, (n + 1) * 4, hipMemcpyDeviceToHost));
    if (multi_org && nm) HIPCHK(hipMemcpy(multi_org, v.multi_org, nm * 4, hipMemcpyDeviceToHost));
    if (multi_cnt && nm) HIPCHK(hipMemcpy(multi_cnt, v.multi_cnt, nm * 4, hipMemcpyDeviceToHost));
    return NEMGPU_OK;
}

int nemgpu_family_table_rtab_size(const nemgpu_family_table* t, int row0, int rows, int64_t* bytes)
{
    if (!t || !bytes) return NEMGPU_E_FUNCARG;
    if (row0 < 0 || rows <= 0 || (long long)row0 + rows > t->dev.n) { set_error("nemgpu_family_table_rtab_size: rows outside the table"); return NEMGPU_E_ARG; }
    *bytes = batch_ends(t, row0, rows, nullptr);
    return NEMGPU_OK;
}

int nemgpu_family_table_rtab(nemgpu_family_table* t, const nemgpu_master* m, int row0, int rows, char* text, int64_t capacity,
                             int64_t* needed, int64_t* line_end)
{
    if (!t || !m || !text || !line_end) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_family_table_rtab";
    { const int r = check_batch(who, m, t->dev.n, t->dev.d, t->device, row0, rows, t->dev.n); if (r != NEMGPU_OK) return r; }
    const long long bytes = batch_ends(t, row0, rows, nullptr);
    HIPCHK(hipSetDevice(t->device));
    { const int r = text_room(who, &t->txt, capacity, bytes, needed); if (r != NEMGPU_OK) return r; }
    (void)batch_ends(t, row0, rows, line_end);
    launch_rtab(m->dev, t->dev, row0, rows, t->txt.text, m->stream);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(text, t->txt.text, (size_t)bytes, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    return device_status(who, err);
}

void nemgpu_family_table_destroy(nemgpu_family_table* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    table_free(t);
}
