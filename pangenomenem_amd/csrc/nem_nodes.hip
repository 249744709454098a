// nem_nodes.hip -- see nem_nodes.hpp.  The kernels, then the C entry points (nemgpu_node_table_*): everything refused for
// its arguments alone is refused on the host before the first HIP call.
#include "nem_nodes.hpp"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "nem_project.hpp"
#include "nem_table.hpp"

namespace nemk {

namespace {

using namespace seg;
constexpr int kNoFamily = -2;                     // a caller id that no master family has (nem_project.hip's)

// ---- escaping: gexf.escape's seven replacements (ElementTree's _escape_attrib) -------------------------------------------
__device__ inline const char* esc_of(unsigned char ch, int* width)
{
    switch (ch) {
    case '&': *width = 5; return "&amp;";
    case '<': *width = 4; return "&lt;";
    case '>': *width = 4; return "&gt;";
    case '"': *width = 6; return "&quot;";
    case '\r': *width = 5; return "&#13;";
    case '\n': *width = 5; return "&#10;";
    case '\t': *width = 5; return "&#09;";
    default: *width = 1; return nullptr;
    }
}

__device__ inline int esc_width(unsigned char ch) { int w; (void)esc_of(ch, &w); return w; }

__device__ inline char* esc_put(char* q, unsigned char ch)
{
    int w;
    const char* r = esc_of(ch, &w);
    if (!r) { *q = (char)ch; return q + 1; }
    for (int k = 0; k < w; k++) q[k] = r[k];
    return q + w;
}

// ---- create --------------------------------------------------------------------------------------------------------------
// a lane per gene: its family as the sort key (n: not kept), its organism
__global__ __launch_bounds__(kThreads) void k_nodes_keys(const int* __restrict__ genes, int g, const uint8_t* __restrict__ rep, const int* __restrict__ inv,
                                                        const int* __restrict__ cptr, int c, const int* __restrict__ corg, int n,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ val, int* __restrict__ gfam,
                                                        int* __restrict__ gorg, int* flags)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= g) return;
    int fam = n;
    if (!(rep && rep[genes[p]])) {
        fam = inv[genes[p]];
        if (fam == kNoFamily) { atomicOr(flags, (int)kNodesNoFamily); fam = n; }
    }
    key[p] = (uint32_t)fam; val[p] = (uint32_t)p; gfam[p] = fam;
    gorg[p] = corg[last_le(cptr, c, p)];
}

// a lane per sorted gene: its organism, whether it starts a (family, organism) run; a run's presence bit, the organism's
// first family
__global__ __launch_bounds__(kThreads) void k_nodes_runs(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sgene, const int* __restrict__ gorg,
                                                        int g, int n, const uint64_t* __restrict__ xt, int nw64, int* first, int* __restrict__ sorg,
                                                        int* __restrict__ head, int* flags)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= g) return;
    const int i = (int)skey[s];
    if (i >= n) { head[s] = 0; sorg[s] = -1; return; }
    const int o = gorg[sgene[s]];
    const bool h = s == 0 || (int)skey[s - 1] != i || gorg[sgene[s - 1]] != o;
    sorg[s] = o; head[s] = h ? 1 : 0;
    if (h) {
        if (!((xt[(size_t)o * nw64 + (i >> 6)] >> (i & 63)) & 1ull)) atomicOr(flags, (int)kNodesNoBit);
        atomicMin(&first[o], i);
    }
}

// the master's presence bits (families below n)
__global__ __launch_bounds__(kThreads) void k_nodes_popcount(const uint64_t* __restrict__ xt, long long words, int nw64, int n, unsigned long long* total)
{
    const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
    int cnt = 0;
    if (q < words) {
        const int w = (int)(q % nw64);
        uint64_t v = xt[q];
        if ((long long)w * 64 + 64 > n) v &= (long long)w * 64 >= n ? 0ull : (~0ull >> (64 - (n - w * 64)));
        cnt = __popcll(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane_id() == 0 && cnt) atomicAdd(total, (unsigned long long)cnt);
}

__global__ __launch_bounds__(kThreads) void k_nodes_fill(int* __restrict__ a, int count, int v)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < count) a[i] = v;
}

// ---- text ----------------------------------------------------------------------------------------------------------------
// a lane per (span, gene of the batch): the escaped width of a kept gene's span, 0 for a gene that is not kept
__global__ __launch_bounds__(kThreads) void k_nodes_widths(const char* __restrict__ text, const long long* __restrict__ off, const int* __restrict__ len,
                                                          const int* __restrict__ gfam, int gene0, int cnt, int n, long long* __restrict__ w)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= 3 * cnt) return;
    long long sum = 0;
    if (gfam[gene0 + t % cnt] < n) {
        const char* q = text + off[t];
        for (int k = 0; k < len[t]; k++) sum += esc_width((unsigned char)q[k]);
    }
    w[t] = sum;
}

// the same lane: its span, escaped, at wx[t] of the batch's part; the piece's place in the blob
__global__ __launch_bounds__(kThreads) void k_nodes_gather(const char* __restrict__ text, const long long* __restrict__ off, const int* __restrict__ len,
                                                          const long long* __restrict__ w, const long long* __restrict__ wx, int gene0, int cnt, int g,
                                                          char* __restrict__ part, long long base, long long* __restrict__ eoff,
                                                          int* __restrict__ elen)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= 3 * cnt) return;
    const size_t at = (size_t)(t / cnt) * g + gene0 + t % cnt;
    eoff[at] = base + wx[t]; elen[at] = (int)w[t];
    if (w[t] == 0) return;
    const char* q = text + off[t];
    char* out = part + wx[t];
    for (int k = 0; k < len[t]; k++) out = esc_put(out, (unsigned char)q[k]);
}

// ---- distinct names and products -----------------------------------------------------------------------------------------
__device__ inline uint64_t hash_bytes(const char* __restrict__ t, int len, uint32_t salt, uint64_t keep)
{
    uint64_t h = 0xcbf29ce484222325ull ^ ((uint64_t)salt * 0x9E3779B97F4A7C15ull);
    for (int j = 0; j < len; j++) { h ^= (unsigned char)t[j]; h *= 0x100000001b3ull; }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    return h & keep;
}

__device__ inline bool same_bytes(const char* __restrict__ a, const char* __restrict__ b, int len)
{
    for (int j = 0; j < len; j++) if (a[j] != b[j]) return false;
    return true;
}

// sorted gene s enters the table under (its family, its piece's bytes): its class's slot afterwards holds the class's
// least sorted gene.  The table has at least twice as many slots as genes, so a probe ends.
__global__ __launch_bounds__(kThreads) void k_nodes_insert(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sgene, int g, int n,
                                                          const char* __restrict__ blob, const long long* __restrict__ eoff, const int* __restrict__ elen,
                                                          int* tbl, uint32_t mask, uint64_t keep, int* __restrict__ slot_of)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= g) return;
    const uint32_t fam = skey[s];
    if ((int)fam >= n) { slot_of[s] = -1; return; }
    const int p = (int)sgene[s], len = elen[p];
    const char* mine = blob + eoff[p];
    uint32_t slot = (uint32_t)hash_bytes(mine, len, fam, keep) & mask;
    int found = -1;
    for (uint32_t probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        const int cur = atomicCAS(&tbl[slot], -1, s);
        if (cur == -1 || cur == s) { found = (int)slot; break; }
        const int q = (int)sgene[cur];
        if (skey[cur] == fam && elen[q] == len && same_bytes(blob + eoff[q], mine, len)) {
            atomicMin(&tbl[slot], s);
            found = (int)slot;
            break;
        }
    }
    slot_of[s] = found;
}

__global__ __launch_bounds__(kThreads) void k_nodes_emit(const int* __restrict__ tbl, const int* __restrict__ slot_of, int g, uint8_t* __restrict__ emit)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s < g) emit[s] = slot_of[s] >= 0 && tbl[slot_of[s]] == s ? 1 : 0;
}

// ---- the layout ----------------------------------------------------------------------------------------------------------
struct NodesDev {
    int n, g;
    const uint32_t *skey, *sgene;                 // [g] the genes sorted by family: the family (n: not kept), the gene
    const int* sorg;                              // [g] the sorted gene's organism
    const int* fstart;                            // [n + 1] a family's first sorted gene
    const char* blob;
    const long long* eoff;                        // [3][g] per gene its ID, NAME and PRODUCT, escaped, in the blob
    const int* elen;                              // [3][g]
    const uint8_t* emit;                          // [2][g] per sorted gene: the least of its name's / product's class
    const int* org_id;                            // [d]
    const long long *ca, *cn, *cp;                // [g] inclusive scans of the sorted genes' bytes: ids, names, products
    const int* r1;                                // [n] the end of the family's first run
    const long long *nlv, *plv;                   // [n] the bytes of the family's name and product values
    const long long* end[2];                      // [n] the nodes' ends: light, full
    int name_id[2];                               // light, full (the product's is one more)
};

__device__ inline bool run_end(const NodesDev& v, int s, int i)
{
    return s + 1 >= v.g || (int)v.skey[s + 1] != i || v.sorg[s + 1] != v.sorg[s];
}

// per sorted gene the bytes it adds to its organism's line, to the name line and to the product line
__global__ __launch_bounds__(kThreads) void k_nodes_contrib(NodesDev v, long long* __restrict__ ca, long long* __restrict__ cn, long long* __restrict__ cp)
{
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s >= v.g) return;
    const int i = (int)v.skey[s];
    if (i >= v.n) { ca[s] = 0; cn[s] = 0; cp[s] = 0; return; }
    const int p = (int)v.sgene[s], a = v.fstart[i];
    const bool h = s == a || v.sorg[s - 1] != v.sorg[s];
    ca[s] = (h ? kNodesLineHead + digits_of(v.org_id[v.sorg[s]]) : 1) + v.elen[p] + (run_end(v, s, i) ? 5 : 0);
    cn[s] = v.emit[s] ? (s == a ? 0 : 1) + v.elen[(size_t)v.g + p] : 0;
    cp[s] = v.emit[(size_t)v.g + s] ? (s == a ? 0 : 1) + v.elen[2 * (size_t)v.g + p] : 0;
}

// per family the end of its first run, its values' bytes and its node's bytes, light and full
__global__ __launch_bounds__(kThreads) void k_nodes_sizes(NodesDev v, int* __restrict__ r1, long long* __restrict__ nlv, long long* __restrict__ plv,
                                                         long long* __restrict__ size_light, long long* __restrict__ size_full)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= v.n) return;
    const int a = v.fstart[i], b = v.fstart[i + 1];
    r1[i] = b > a ? lower_bound(v.sorg, a, b, v.sorg[a] + 1) : a;
    const long long nv = before(v.cn, b) - before(v.cn, a), pv = before(v.cp, b) - before(v.cp, a);
    nlv[i] = nv; plv[i] = pv;
    size_light[i] = 2 * kNodesLineFixed + digits_of(v.name_id[0]) + digits_of(v.name_id[0] + 1) + nv + pv;
    size_full[i] = 2 * kNodesLineFixed + digits_of(v.name_id[1]) + digits_of(v.name_id[1] + 1) + nv + pv + before(v.ca, b) - before(v.ca, a);
}

__device__ inline char* put_head(char* q, int id)
{
    const char* a = "          <attvalue for=\"";
    for (int k = 0; k < 25; k++) q[k] = a[k];
    q = put_digits(q + 25, id);
    const char* b = "\" value=\"";
    for (int k = 0; k < 9; k++) q[k] = b[k];
    return q + 9;
}

__device__ inline void put_tail(char* q)
{
    const char* e = "\" />\n";
    for (int k = 0; k < 5; k++) q[k] = e[k];
}

__device__ inline char* put_piece(char* q, const NodesDev& v, int kind, int p)
{
    const size_t at = (size_t)kind * v.g + p;
    const char* from = v.blob + v.eoff[at];
    const int len = v.elen[at];
    for (int k = 0; k < len; k++) q[k] = from[k];
    return q + len;
}

// where family i's name line starts in the batch's text (base: the batch's first byte among all nodes')
__device__ inline long long name_line_at(const NodesDev& v, int full, int i, long long base)
{
    const int a = v.fstart[i];
    return (i > 0 ? v.end[full][i - 1] : 0ll) - base + (full ? before(v.ca, v.r1[i]) - before(v.ca, a) : 0ll);
}

// a lane per sorted gene in [s0, s1): its pieces
__global__ __launch_bounds__(kThreads) void k_nodes_pieces(NodesDev v, int full, int s0, int s1, long long base, char* __restrict__ text)
{
    const int s = s0 + blockIdx.x * kThreads + threadIdx.x;
    if (s >= s1) return;
    const int i = (int)v.skey[s], p = (int)v.sgene[s], a = v.fstart[i];
    const long long name_at = name_line_at(v, full, i, base);
    const int dn = digits_of(v.name_id[full]), dp = digits_of(v.name_id[full] + 1);
    const long long name_line = kNodesLineFixed + dn + v.nlv[i], product_line = kNodesLineFixed + dp + v.plv[i];
    if (full) {
        const bool h = s == a || v.sorg[s - 1] != v.sorg[s];
        const long long node_at = (i > 0 ? v.end[1][i - 1] : 0ll) - base;
        char* q = text + node_at + (before(v.ca, s) - before(v.ca, a)) + (s >= v.r1[i] ? name_line + product_line : 0ll);
        if (h) q = put_head(q, v.org_id[v.sorg[s]]); else *q++ = '|';
        q = put_piece(q, v, 0, p);
        if (run_end(v, s, i)) put_tail(q);
    }
    if (v.emit[s]) {
        char* q = text + name_at + kNodesLineHead + dn + (before(v.cn, s) - before(v.cn, a));
        if (s != a) *q++ = '|';
        (void)put_piece(q, v, 1, p);
    }
    if (v.emit[(size_t)v.g + s]) {
        char* q = text + name_at + name_line + kNodesLineHead + dp + (before(v.cp, s) - before(v.cp, a));
        if (s != a) *q++ = '|';
        (void)put_piece(q, v, 2, p);
    }
}

// a lane per family row0 .. row0 + rows - 1: the head and the tail of its name line and of its product line
__global__ __launch_bounds__(kThreads) void k_nodes_frames(NodesDev v, int full, int row0, int rows, long long base, char* __restrict__ text)
{
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= rows) return;
    const int i = row0 + r, id = v.name_id[full];
    char* q = put_head(text + name_line_at(v, full, i, base), id) + v.nlv[i];
    put_tail(q);
    q = put_head(q + 5, id + 1) + v.plv[i];
    put_tail(q);
}

}  // namespace

}  // namespace nemk

using namespace nemk;

// A node table on the device: the sorted genes, the escaped blob, the layout of the current numbering, and the buffer of
// its text calls, kept for the next call
struct nemgpu_node_table {
    int device = 0, n = 0, d = 0, g = 0;
    uint64_t keep = ~0ull;                            // the bits of the hash that are kept (tests: a few)
    uint32_t* sortbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    const uint32_t *skey = nullptr, *sgene = nullptr; // (two of sortbuf)
    int *gfam = nullptr, *sorg = nullptr, *fstart = nullptr;
    std::vector<int> fstart_h, first_h;               // [n + 1], [d] (n: the organism has no kept gene)
    long long* eoff = nullptr;                        // [3][g]
    int* elen = nullptr;                              // [3][g]
    int next_gene = 0;                                // the genes below it have their text
    long long blob_bytes = 0;
    std::vector<std::pair<char*, long long>> parts;   // the batches' parts of the blob until finish joins them
    char* blob = nullptr;
    bool finished = false;
    uint8_t* emit = nullptr;                          // [2][g]
    int tail = -1;                                    // the numbering the layout was made for (-1: none yet)
    int name_id[2] = {1, 1};
    std::vector<int> org_id_h;
    int *org_id = nullptr, *r1 = nullptr;
    long long *ca = nullptr, *cn = nullptr, *cp = nullptr, *nlv = nullptr, *plv = nullptr, *end[2] = {nullptr, nullptr};
    std::vector<long long> end_h[2];
    TableText txt;
};

namespace {

void table_free(nemgpu_node_table* t)
{
    void* all[] = {t->sortbuf[0], t->sortbuf[1], t->sortbuf[2], t->sortbuf[3], t->gfam, t->sorg, t->fstart, t->eoff, t->elen, t->blob, t->emit,
                   t->org_id, t->r1, t->ca, t->cn, t->cp, t->nlv, t->plv, t->end[0], t->end[1], t->txt.text};
    for (void* p : all) if (p) (void)hipFree(p);
    for (auto& part : t->parts) if (part.first) (void)hipFree(part.first);
    delete t;
}

NodesDev view(const nemgpu_node_table* t)
{
    NodesDev v{};
    v.n = t->n; v.g = t->g; v.skey = t->skey; v.sgene = t->sgene; v.sorg = t->sorg; v.fstart = t->fstart; v.blob = t->blob; v.eoff = t->eoff;
    v.elen = t->elen; v.emit = t->emit; v.org_id = t->org_id; v.ca = t->ca; v.cn = t->cn; v.cp = t->cp; v.r1 = t->r1; v.nlv = t->nlv; v.plv = t->plv;
    v.end[0] = t->end[0]; v.end[1] = t->end[1]; v.name_id[0] = t->name_id[0]; v.name_id[1] = t->name_id[1];
    return v;
}

int check_master(const std::string& who, const nemgpu_node_table* t, const nemgpu_master* m)
{
    if (m->n != t->n || m->d != t->d || m->device != t->device) { set_error(who + ": not the table's master"); return NEMGPU_E_ARG; }
    return NEMGPU_OK;
}

hipError_t create(nemgpu_node_table* t, const nemgpu_master* m, const GeneOrdersIn& in, int* mismatch)
{
    const int n = m->n, d = m->d, g = in.g;
    hipStream_t s = m->stream;
    Scratch mem;
    GeneOrdersDev o;
    int *gorg, *head, *partial, *flags, *first, *heads;
    unsigned long long* ones;
    for (int k = 0; k < 4; k++) HIPTRY(dev_alloc(&t->sortbuf[k], g));
    HIPTRY(dev_alloc(&t->gfam, g)); HIPTRY(dev_alloc(&t->sorg, g)); HIPTRY(dev_alloc(&t->fstart, (size_t)n + 1));
    HIPTRY(mem.alloc(&gorg, g)); HIPTRY(mem.alloc(&head, g)); HIPTRY(mem.alloc(&partial, (size_t)g / kScanTile + 2)); HIPTRY(mem.alloc(&flags, 1));
    HIPTRY(mem.alloc(&first, d)); HIPTRY(mem.alloc(&heads, 1)); HIPTRY(mem.alloc(&ones, 1));
    HIPTRY(hipMemsetAsync(flags, 0, 4, s));
    HIPTRY(hipMemsetAsync(ones, 0, 8, s));
    HIPTRY(upload_orders(mem, in, n, s, &o));
    hipLaunchKernelGGL(k_nodes_keys, dim3(blocks(g)), dim3(kThreads), 0, s, (const int*)o.genes, g, (const uint8_t*)o.rep, (const int*)o.inv, (const int*)o.cptr,
                       in.c, (const int*)o.corg, n, t->sortbuf[0], t->sortbuf[2], t->gfam, gorg, flags);
    HIPTRY(hipGetLastError());
    HIPTRY(sort_pairs<uint32_t>(mem, t->sortbuf[0], t->sortbuf[1], t->sortbuf[2], t->sortbuf[3], g, bits_for(n + 1), &t->skey, &t->sgene, s));
    hipLaunchKernelGGL(k_seg_starts<uint32_t>, dim3(blocks((long long)n + 1)), dim3(kThreads), 0, s, t->skey, g, 0, n, t->fstart);
    hipLaunchKernelGGL(k_nodes_fill, dim3(blocks(d)), dim3(kThreads), 0, s, first, d, n);
    hipLaunchKernelGGL(k_nodes_runs, dim3(blocks(g)), dim3(kThreads), 0, s, t->skey, t->sgene, (const int*)gorg, g, n, m->dev.xt, m->dev.nw64, first, t->sorg,
                       head, flags);
    scan<int, OpSum<int>, true>(head, head, g, OpSum<int>(), 0, partial, heads, s);
    const long long words = (long long)d * m->dev.nw64;
    if (words > 0) hipLaunchKernelGGL(k_nodes_popcount, dim3(blocks(words)), dim3(kThreads), 0, s, m->dev.xt, words, m->dev.nw64, n, ones);
    HIPTRY(hipGetLastError());
    int h_flags = 0, h_heads = 0;
    unsigned long long h_ones = 0;
    t->fstart_h.assign((size_t)n + 1, 0); t->first_h.assign((size_t)d, n);
    HIPTRY(hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(&h_heads, heads, 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(&h_ones, ones, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(t->fstart_h.data(), t->fstart, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipMemcpyAsync(t->first_h.data(), first, (size_t)d * 4, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    if ((unsigned long long)h_heads != h_ones) h_flags |= kNodesMissing;
    *mismatch = h_flags;
    if (h_flags) return hipSuccess;
    HIPTRY(dev_alloc(&t->eoff, 3 * (size_t)g)); HIPTRY(dev_alloc(&t->elen, 3 * (size_t)g)); HIPTRY(dev_alloc(&t->emit, 2 * (size_t)g));
    HIPTRY(dev_alloc(&t->org_id, d)); HIPTRY(dev_alloc(&t->r1, n)); HIPTRY(dev_alloc(&t->ca, g)); HIPTRY(dev_alloc(&t->cn, g)); HIPTRY(dev_alloc(&t->cp, g));
    HIPTRY(dev_alloc(&t->nlv, n)); HIPTRY(dev_alloc(&t->plv, n)); HIPTRY(dev_alloc(&t->end[0], n)); HIPTRY(dev_alloc(&t->end[1], n));
    return hipSuccess;
}

hipError_t text_batch(nemgpu_node_table* t, hipStream_t s, const char* text, long long bytes, int gene0, int cnt, const int64_t* span_off,
                      const int32_t* span_len)
{
    Scratch mem;
    char* dtext;
    long long *off, *w, *wx, *partial, *total;
    int* len;
    const int lanes = 3 * cnt;
    HIPTRY(mem.alloc(&dtext, (size_t)bytes)); HIPTRY(mem.alloc(&off, lanes)); HIPTRY(mem.alloc(&len, lanes)); HIPTRY(mem.alloc(&w, lanes));
    HIPTRY(mem.alloc(&wx, lanes)); HIPTRY(mem.alloc(&partial, (size_t)lanes / kScanTile + 2)); HIPTRY(mem.alloc(&total, 1));
    if (bytes) HIPTRY(hipMemcpyAsync(dtext, text, (size_t)bytes, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(off, span_off, (size_t)lanes * 8, hipMemcpyHostToDevice, s));
    HIPTRY(hipMemcpyAsync(len, span_len, (size_t)lanes * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_nodes_widths, dim3(blocks(lanes)), dim3(kThreads), 0, s, (const char*)dtext, (const long long*)off, (const int*)len,
                       (const int*)t->gfam, gene0, cnt, t->n, w);
    scan<long long, OpSum<long long>, false>(w, wx, lanes, OpSum<long long>(), 0ll, partial, total, s);
    HIPTRY(hipGetLastError());
    long long part_bytes = 0;
    HIPTRY(hipMemcpyAsync(&part_bytes, total, 8, hipMemcpyDeviceToHost, s));
    HIPTRY(hipStreamSynchronize(s));
    if (t->blob_bytes + part_bytes > kNodesBlobMax) return hipErrorOutOfMemory;
    char* part = nullptr;
    HIPTRY(dev_alloc(&part, (size_t)part_bytes));
    t->parts.push_back({part, part_bytes});
    hipLaunchKernelGGL(k_nodes_gather, dim3(blocks(lanes)), dim3(kThreads), 0, s, (const char*)dtext, (const long long*)off, (const int*)len,
                       (const long long*)w, (const long long*)wx, gene0, cnt, t->g, part, t->blob_bytes, t->eoff, t->elen);
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(s));                              // (the call's scratch is freed behind it)
    t->blob_bytes += part_bytes;
    t->next_gene = gene0 + cnt;
    return hipSuccess;
}

hipError_t finish(nemgpu_node_table* t, hipStream_t s)
{
    const int g = t->g;
    HIPTRY(dev_alloc(&t->blob, (size_t)t->blob_bytes));
    long long at = 0;
    for (auto& part : t->parts) {
        if (part.second) HIPTRY(hipMemcpyAsync(t->blob + at, part.first, (size_t)part.second, hipMemcpyDeviceToDevice, s));
        at += part.second;
    }
    Scratch mem;
    uint32_t slots = 2;
    while (slots < 2u * (uint32_t)g) slots <<= 1;                // (g <= kNodesGenesMax: at most 2^31)
    int *tbl, *slot_of;
    HIPTRY(mem.alloc(&tbl, slots)); HIPTRY(mem.alloc(&slot_of, g));
    for (int kind = 1; kind <= 2; kind++) {
        HIPTRY(hipMemsetAsync(tbl, 0xff, (size_t)slots * 4, s));
        hipLaunchKernelGGL(k_nodes_insert, dim3(blocks(g)), dim3(kThreads), 0, s, t->skey, t->sgene, g, t->n, (const char*)t->blob,
                           (const long long*)t->eoff + (size_t)kind * g, (const int*)t->elen + (size_t)kind * g, tbl, slots - 1, t->keep, slot_of);
        hipLaunchKernelGGL(k_nodes_emit, dim3(blocks(g)), dim3(kThreads), 0, s, (const int*)tbl, (const int*)slot_of, g, t->emit + (size_t)(kind - 1) * g);
    }
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(s));
    for (auto& part : t->parts) if (part.first) (void)hipFree(part.first);
    t->parts.clear();
    t->finished = true;
    return hipSuccess;
}

// the ids as networkx numbers them (gexf.node_attribute_ids states the same): nb_genes 0, node 0's first organism, name,
// product, node 0's other organisms, `tail` titles, then the organisms first met at later nodes in (node, organism) order
void number(nemgpu_node_table* t, int tail)
{
    const int n = t->n, d = t->d;
    std::vector<int> by;
    for (int o = 0; o < d; o++) if (t->first_h[o] < n) by.push_back(o);
    std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return t->first_h[a] < t->first_h[b]; });
    t->org_id_h.assign((size_t)d, -1);
    int k = 1;
    size_t j = 0;
    if (j < by.size() && t->first_h[by[j]] == 0) t->org_id_h[by[j++]] = k++;
    t->name_id[1] = k; t->name_id[0] = 1;
    k += 2;
    while (j < by.size() && t->first_h[by[j]] == 0) t->org_id_h[by[j++]] = k++;
    k += tail;
    for (; j < by.size(); j++) t->org_id_h[by[j]] = k++;
}

hipError_t layout(nemgpu_node_table* t, hipStream_t s)
{
    const int n = t->n, g = t->g, d = t->d;
    Scratch mem;
    long long *partial, *size;
    HIPTRY(mem.alloc(&partial, (size_t)std::max(g, n) / kScanTile + 2)); HIPTRY(mem.alloc(&size, 2 * (size_t)n));
    std::vector<int> ids(t->org_id_h);
    for (int& v : ids) v = std::max(v, 0);
    if (d) HIPTRY(hipMemcpyAsync(t->org_id, ids.data(), (size_t)d * 4, hipMemcpyHostToDevice, s));
    const NodesDev v = view(t);
    hipLaunchKernelGGL(k_nodes_contrib, dim3(blocks(g)), dim3(kThreads), 0, s, v, t->ca, t->cn, t->cp);
    scan<long long, OpSum<long long>, true>(t->ca, t->ca, g, OpSum<long long>(), 0ll, partial, (long long*)nullptr, s);
    scan<long long, OpSum<long long>, true>(t->cn, t->cn, g, OpSum<long long>(), 0ll, partial, (long long*)nullptr, s);
    scan<long long, OpSum<long long>, true>(t->cp, t->cp, g, OpSum<long long>(), 0ll, partial, (long long*)nullptr, s);
    t->end_h[0].assign((size_t)n, 0); t->end_h[1].assign((size_t)n, 0);
    if (n > 0) {
        hipLaunchKernelGGL(k_nodes_sizes, dim3(blocks(n)), dim3(kThreads), 0, s, v, t->r1, t->nlv, t->plv, size, size + n);
        scan<long long, OpSum<long long>, true>(size, t->end[0], n, OpSum<long long>(), 0ll, partial, (long long*)nullptr, s);
        scan<long long, OpSum<long long>, true>(size + n, t->end[1], n, OpSum<long long>(), 0ll, partial, (long long*)nullptr, s);
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(t->end_h[0].data(), t->end[0], (size_t)n * 8, hipMemcpyDeviceToHost, s));
        HIPTRY(hipMemcpyAsync(t->end_h[1].data(), t->end[1], (size_t)n * 8, hipMemcpyDeviceToHost, s));
    }
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(s));                              // (ids is the vector's own copy: wait before it goes)
    return hipSuccess;
}

int check_lines(const std::string& who, const nemgpu_node_table* t, int row0, int rows)
{
    if (!t->finished || t->tail < 0) { set_error(who + ": the table has no layout yet (nemgpu_node_table_finish, then _ids)"); return NEMGPU_E_ARG; }
    if (row0 < 0 || rows <= 0 || (long long)row0 + rows > t->n) { set_error(who + ": rows outside the table"); return NEMGPU_E_ARG; }
    return NEMGPU_OK;
}

long long batch_base(const nemgpu_node_table* t, int full, int row0) { return row0 > 0 ? t->end_h[full][(size_t)row0 - 1] : 0ll; }

}  // namespace

int nemgpu_node_table_create(nemgpu_node_table** out, const nemgpu_master* m, int f, const int32_t* genes, int g, const int32_t* contig_ptr,
                             const int32_t* contig_org, int c, const uint8_t* repeated, int hash_bits)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!m) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_node_table_create";
    if (f <= 0 || g <= 0 || c <= 0 || !genes || !contig_ptr || !contig_org || hash_bits < 0 || hash_bits > 64) {
        set_error(who + ": f > 0, the genes, the contigs and hash_bits in 0 .. 64 are needed"); return NEMGPU_E_FUNCARG;
    }
    if (g > kNodesGenesMax) { set_error(who + ": " + std::to_string(g) + " genes, at most " + std::to_string(kNodesGenesMax)); return NEMGPU_E_ARG; }
    { const int r = check_orders(true, m->d, f, g, c, genes, contig_ptr, contig_org, nullptr); if (r != NEMGPU_OK) return r; }
    for (int j = 1; j < c; j++)
        if (contig_org[j] < contig_org[j - 1]) {
            set_error("orders: contig " + std::to_string(j) + ": contig_org must be non-decreasing (the organisms walked in column order)");
            return NEMGPU_E_ARG;
        }
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    nemgpu_node_table* t = new nemgpu_node_table();
    t->device = m->device; t->n = m->n; t->d = m->d; t->g = g;
    t->keep = hash_bits == 0 || hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1;
    const GeneOrdersIn in{f, g, c, genes, contig_ptr, contig_org, repeated, m->order.empty() ? nullptr : m->order.data()};
    int mismatch = 0;
    const hipError_t err = create(t, m, in, &mismatch);
    if (err != hipSuccess) { table_free(t); return device_status(who, err); }
    if (mismatch) {
        table_free(t);
        set_error(who + ": these orders are not this master's: " +
                  ((mismatch & kNodesNoFamily) ? "a kept gene's family is not in the master"
                   : (mismatch & kNodesNoBit)  ? "a family has a kept gene in an organism where the master's presence bit is clear"
                                               : "the master has a presence bit where the orders have no kept gene"));
        return NEMGPU_E_ARG;
    }
    *out = t;
    return NEMGPU_OK;
}

int nemgpu_node_table_text(nemgpu_node_table* t, const nemgpu_master* m, const char* text, int64_t bytes, int gene0, int gene1,
                           const int64_t* span_off, const int32_t* span_len)
{
    if (!t || !m || !span_off || !span_len || (bytes > 0 && !text)) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_node_table_text";
    { const int r = check_master(who, t, m); if (r != NEMGPU_OK) return r; }
    if (t->finished) { set_error(who + ": the table is finished"); return NEMGPU_E_ARG; }
    if (bytes < 0 || bytes > kNodesBlobMax || gene0 != t->next_gene || gene1 <= gene0 || gene1 > t->g) {
        set_error(who + ": the batches are runs of genes in order: genes " + std::to_string(gene0) + " .. " + std::to_string(gene1) + ", the next is " +
                  std::to_string(t->next_gene) + " of " + std::to_string(t->g));
        return NEMGPU_E_ARG;
    }
    const int cnt = gene1 - gene0;
    for (long long k = 0; k < 3ll * cnt; k++)
        if (span_len[k] < 0 || span_len[k] > kNodesSpanMax || span_off[k] < 0 || span_off[k] > bytes - span_len[k]) {
            set_error(who + ": span " + std::to_string(k / cnt) + " of gene " + std::to_string(gene0 + k % cnt) + " (" + std::to_string(span_off[k]) +
                      ", " + std::to_string(span_len[k]) + ") is past the end of the batch's " + std::to_string(bytes) + " bytes, or longer than " +
                      std::to_string(kNodesSpanMax));
            return NEMGPU_E_ARG;
        }
    HIPCHK(hipSetDevice(t->device));
    return device_status(who, text_batch(t, m->stream, text, bytes, gene0, cnt, span_off, span_len));
}

int nemgpu_node_table_finish(nemgpu_node_table* t, const nemgpu_master* m)
{
    if (!t || !m) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_node_table_finish";
    { const int r = check_master(who, t, m); if (r != NEMGPU_OK) return r; }
    if (t->finished) { set_error(who + ": the table is finished"); return NEMGPU_E_ARG; }
    if (t->next_gene != t->g) {
        set_error(who + ": the genes from " + std::to_string(t->next_gene) + " on have no text yet"); return NEMGPU_E_ARG;
    }
    HIPCHK(hipSetDevice(t->device));
    return device_status(who, finish(t, m->stream));
}

int nemgpu_node_table_shape(const nemgpu_node_table* t, int* n, int* d, int* g)
{
    if (!t) return NEMGPU_E_FUNCARG;
    if (n) *n = t->n;
    if (d) *d = t->d;
    if (g) *g = t->g;
    return NEMGPU_OK;
}

int nemgpu_node_table_fetch(const nemgpu_node_table* t, int32_t* nb_genes, int32_t* org_first_node)
{
    if (!t) return NEMGPU_E_FUNCARG;
    if (nb_genes) for (int i = 0; i < t->n; i++) nb_genes[i] = t->fstart_h[(size_t)i + 1] - t->fstart_h[(size_t)i];
    if (org_first_node) for (int o = 0; o < t->d; o++) org_first_node[o] = t->first_h[(size_t)o];
    return NEMGPU_OK;
}

int nemgpu_node_table_ids(nemgpu_node_table* t, const nemgpu_master* m, int tail, int32_t* org_id, int32_t* name_id, int64_t* node_end_full,
                          int64_t* node_end_light)
{
    if (!t || !m) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_node_table_ids";
    { const int r = check_master(who, t, m); if (r != NEMGPU_OK) return r; }
    if (!t->finished) { set_error(who + ": the table is not finished (nemgpu_node_table_finish)"); return NEMGPU_E_ARG; }
    if (tail < 0 || tail > 0x7fffffff - 16 - t->d) { set_error(who + ": tail >= 0, and ids that fit an int"); return NEMGPU_E_ARG; }
    if (tail != t->tail) {
        HIPCHK(hipSetDevice(t->device));
        number(t, tail);
        t->tail = -1;
        const hipError_t err = layout(t, m->stream);
        if (err != hipSuccess) return device_status(who, err);
        t->tail = tail;
    }
    if (org_id) for (int o = 0; o < t->d; o++) org_id[o] = t->org_id_h[(size_t)o];
    if (name_id) { name_id[0] = t->name_id[0]; name_id[1] = t->name_id[1]; }
    if (node_end_full) for (int i = 0; i < t->n; i++) node_end_full[i] = t->end_h[1][(size_t)i];
    if (node_end_light) for (int i = 0; i < t->n; i++) node_end_light[i] = t->end_h[0][(size_t)i];
    return NEMGPU_OK;
}

int nemgpu_node_table_lines_size(const nemgpu_node_table* t, int full, int row0, int rows, int64_t* bytes)
{
    if (!t || !bytes) return NEMGPU_E_FUNCARG;
    full = full ? 1 : 0;
    { const int r = check_lines("nemgpu_node_table_lines_size", t, row0, rows); if (r != NEMGPU_OK) return r; }
    *bytes = t->end_h[full][(size_t)row0 + rows - 1] - batch_base(t, full, row0);
    return NEMGPU_OK;
}

int nemgpu_node_table_lines(nemgpu_node_table* t, const nemgpu_master* m, int full, int row0, int rows, char* text, int64_t capacity,
                            int64_t* needed, int64_t* node_end)
{
    if (!t || !m || !text || !node_end) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_node_table_lines";
    full = full ? 1 : 0;
    { const int r = check_master(who, t, m); if (r != NEMGPU_OK) return r; }
    { const int r = check_lines(who, t, row0, rows); if (r != NEMGPU_OK) return r; }
    const long long base = batch_base(t, full, row0), bytes = t->end_h[full][(size_t)row0 + rows - 1] - base;
    HIPCHK(hipSetDevice(t->device));
    { const int r = text_room(who, &t->txt, capacity, bytes, needed); if (r != NEMGPU_OK) return r; }
    const int s0 = t->fstart_h[(size_t)row0], s1 = t->fstart_h[(size_t)row0 + rows];
    const NodesDev v = view(t);
    if (s1 > s0) hipLaunchKernelGGL(k_nodes_pieces, dim3(blocks(s1 - s0)), dim3(kThreads), 0, m->stream, v, full, s0, s1, base, t->txt.text);
    hipLaunchKernelGGL(k_nodes_frames, dim3(blocks(rows)), dim3(kThreads), 0, m->stream, v, full, row0, rows, base, t->txt.text);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(text, t->txt.text, (size_t)bytes, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    for (int r = 0; r < rows; r++) node_end[r] = t->end_h[full][(size_t)row0 + r] - base;
    return device_status(who, err);
}

void nemgpu_node_table_destroy(nemgpu_node_table* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    table_free(t);
}
