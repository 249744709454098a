// nem_edge_meta.hip -- the edges' metadata <attvalue> lines of the GEXF export: see nem_edges.hpp.  The kernels and their
// launchers; the C entry points (nemgpu_edge_table_metadata, _metamasks, _metavalues[_size]) are nem_edges.hip's, which
// owns the table's handle and refuses on the host whatever is outside the bounds these kernels rely on.
#include "nem_edges.hpp"

#include "nem_scan.hpp"

namespace nemk {

namespace {

using namespace seg;

// a line: 10 spaces, <attvalue for=", the id, " value=", the present values joined by |, " />, a newline
constexpr int kMetaHead = 25, kMetaMid = 9, kMetaTail = 5, kMetaFixed = kMetaHead + kMetaMid + kMetaTail;

// the wave's lanes have written LDS that other lanes of the wave read next
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave per edge: per attribute the OR over the edge's organisms of one-hot(rank), made in LDS
__global__ __launch_bounds__(kThreads) void k_meta_masks(const int* __restrict__ entry, const uint32_t* __restrict__ bits, int wf, int d, EdgeMetaDev meta,
                                                        int row0, int rows, uint32_t* __restrict__ masks)
{
    __shared__ uint32_t s_mask[kThreads / 64][kMetaValuesMax / 32];
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int r = blockIdx.x * (kThreads / 64) + wv;
    if (r >= rows) return;
    const int t = entry[row0 + r];
    uint32_t* mine = s_mask[wv];
    uint32_t* out = masks + (size_t)r * meta.mask_words;
    for (int a = 0; a < meta.n_attr; a++) {
        const int off = meta.mask_off[a], nw = meta.mask_off[a + 1] - off;
        const int* __restrict__ rank = meta.rank + (size_t)a * d;
        for (int k = lane; k < nw; k += 64) mine[k] = 0u;     // (word k is read below, and zeroed again, by this same lane)
        wave_sync();
        for (int o0 = 0; o0 < d; o0 += 64) {
            const int o = o0 + lane;
            if (o < d && ((bits[(size_t)t * wf + (o >> 5)] >> (o & 31)) & 1u)) {
                const int v = rank[o];                        // (in [0, n_values[a]): checked on the host)
                atomicOr(&mine[v >> 5], 1u << (v & 31));
            }
        }
        wave_sync();
        for (int k = lane; k < nw; k += 64) out[off + k] = mine[k];
    }
}

// the bytes of attribute a's line of an edge whose words of that attribute are `mask`: the wave computes it together,
// every lane gets it.  What both k_meta_sizes and k_meta_text take a line's width from.
__device__ inline int meta_line_width(const EdgeMetaDev& meta, int a, const uint32_t* __restrict__ mask)
{
    const int nw = meta.mask_off[a + 1] - meta.mask_off[a];
    const int* __restrict__ ptr = meta.val_ptr + meta.val_base[a];
    int sum = 0;                                              // every present value and its separator
    for (int k = lane_id(); k < nw; k += 64) {
        uint32_t m = mask[k];
        while (m) {
            const int v = k * 32 + __ffs((int)m) - 1;
            m &= m - 1u;
            sum += ptr[v + 1] - ptr[v] + 1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    return kMetaFixed + digits_of(meta.attr_id[a]) + (sum > 0 ? sum - 1 : 0);
}

// one wave per edge: the bytes of its lines
__global__ __launch_bounds__(kThreads) void k_meta_sizes(EdgeMetaDev meta, int rows, const uint32_t* __restrict__ masks, long long* __restrict__ sizes)
{
    const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint32_t* mine = masks + (size_t)r * meta.mask_words;
    long long sum = 0;
    for (int a = 0; a < meta.n_attr; a++) sum += meta_line_width(meta, a, mine + meta.mask_off[a]);
    if (lane_id() == 0) sizes[r] = sum;
}

// byte k of a line's head: the opening, the id's nd digits, the middle
__device__ inline char head_byte(int k, int id, int nd)
{
    const char* open = "          <attvalue for=\"";
    const char* mid = "\" value=\"";
    if (k < kMetaHead) return open[k];
    if (k >= kMetaHead + nd) return mid[k - kMetaHead - nd];
    for (int q = kMetaHead + nd - 1 - k; q > 0; q--) id /= 10;
    return (char)('0' + id % 10);
}

// one wave per edge: its lines; a line's values in increasing rank, a value's bytes a lane each
__global__ __launch_bounds__(kThreads) void k_meta_text(EdgeMetaDev meta, int rows, const uint32_t* __restrict__ masks, const long long* __restrict__ ends,
                                                       char* __restrict__ text)
{
    const int lane = lane_id();
    const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint32_t* mine = masks + (size_t)r * meta.mask_words;
    long long at = r > 0 ? ends[r - 1] : 0ll;
    for (int a = 0; a < meta.n_attr; a++) {
        const uint32_t* mask = mine + meta.mask_off[a];
        const int nw = meta.mask_off[a + 1] - meta.mask_off[a];
        const int* __restrict__ ptr = meta.val_ptr + meta.val_base[a];
        const int width = meta_line_width(meta, a, mask);
        const int id = meta.attr_id[a], nd = digits_of(id), head = kMetaHead + nd + kMetaMid;     // (head <= 44: one lane per byte)
        if (lane < head) text[at + lane] = head_byte(lane, id, nd);
        long long p = at + head;
        bool first = true;
        for (int w0 = 0; w0 < nw; w0 += 64) {
            const uint32_t word = w0 + lane < nw ? mask[w0 + lane] : 0u;
            unsigned long long busy = __ballot(word != 0u);
            while (busy) {                                    // (uniform over the wave, as everything below but the byte's lane)
                const int j = __ffsll((long long)busy) - 1;
                busy &= busy - 1ull;
                uint32_t m = __shfl(word, j);
                while (m) {
                    const int v = (w0 + j) * 32 + __ffs((int)m) - 1;
                    m &= m - 1u;
                    if (!first) { if (lane == 0) text[p] = '|'; p++; }
                    first = false;
                    const int from = ptr[v], len = ptr[v + 1] - from;
                    for (int k = lane; k < len; k += 64) text[p + k] = meta.blob[from + k];
                    p += len;
                }
            }
        }
        const char* tail = "\" />\n";
        if (lane < kMetaTail) text[at + width - kMetaTail + lane] = tail[lane];
        at += width;
    }
}

int waves(int rows) { return (rows + kThreads / 64 - 1) / (kThreads / 64); }

}  // namespace

void launch_meta_masks(const MasterDev& m, const EdgeTableDev& t, const EdgeMetaDev& meta, int row0, int rows, uint32_t* masks, hipStream_t s)
{
    hipLaunchKernelGGL(k_meta_masks, dim3(waves(rows)), dim3(kThreads), 0, s, (const int*)t.entry, m.edge_bits, m.wf, m.d, meta, row0, rows, masks);
}

void launch_meta_sizes(const EdgeMetaDev& meta, int rows, const uint32_t* masks, long long* sizes, hipStream_t s)
{
    hipLaunchKernelGGL(k_meta_sizes, dim3(waves(rows)), dim3(kThreads), 0, s, meta, rows, masks, sizes);
}

void launch_meta_text(const EdgeMetaDev& meta, int rows, const uint32_t* masks, const long long* ends, char* text, hipStream_t s)
{
    hipLaunchKernelGGL(k_meta_text, dim3(waves(rows)), dim3(kThreads), 0, s, meta, rows, masks, ends, text);
}

}  // namespace nemk
