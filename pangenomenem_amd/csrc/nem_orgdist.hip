// nem_orgdist.hip -- see nem_orgdist.hpp.  The kernels, then the C entry points (nemgpu_orgclust_*): everything refused
// for its arguments alone is refused on the host before the first HIP call.
#include "nem_orgdist.hpp"

#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "nem_table.hpp"

namespace nemk {

namespace {

constexpr int kDistThreads = 256;                 // 16 x 16 lanes, a 4 x 4 micro-tile each
constexpr int kRowPad = kOrgChunk + 1;            // 64-bit words per staged row: 66 dwords, so 16 rows fall on 16 bank pairs
constexpr int kOrgSuper = 16;                     // tiles per side of the square of tiles that neighbouring blocks share
constexpr int kTilePad = kOrgTile + 1;            // doubles per row of the finished tile
constexpr int kStageWords = 2 * kOrgTile * kRowPad;
constexpr int kStagePerLane = kOrgTile * kOrgChunk / kDistThreads;   // words of one tile a lane stages per step
static_assert(kOrgTile == 64 && kDistThreads == 256, "a lane's rows are lane / 16 + 16 r, its columns lane % 16 + 16 c");
static_assert(kOrgChunk == 32, "a lane stages word lane % 32 of rows lane / 32 + 8 it");
static_assert(kOrgTile * kTilePad <= kStageWords, "the finished tile reuses the staging words");
static_assert(kOrgMax % 32 == 0, "the live set is whole words");

__device__ inline uint64_t last_word_mask(int n) { return (n & 63) ? ((1ull << (n & 63)) - 1ull) : ~0ull; }

// one wave per organism
__global__ __launch_bounds__(256) void k_org_popcount(const uint64_t* __restrict__ xt, int n, int d, int nw64, int* __restrict__ pop)
{
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= d) return;
    const uint64_t* row = xt + (size_t)o * nw64;
    int cnt = 0;
    for (int w = lane; w < nw64; w += 64) {
        uint64_t v = row[w];
        if (w == nw64 - 1) v &= last_word_mask(n);
        cnt += __popcll(v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0) pop[o] = cnt;
}

// acc += the set bits of x in ONE instruction: the bit count instruction adds its second operand, which hipcc leaves 0
// and follows with an add of its own (five instructions per word pair instead of four)
__device__ inline void add_bits(int& acc, uint32_t x) { asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x)); }

// word k of a lane's four rows of each staged tile
__device__ inline void lds_words(const uint64_t* sa, const uint64_t* sb, int ty, int tx, int k, uint64_t (&a)[4], uint64_t (&b)[4])
{
#pragma unroll
    for (int r = 0; r < 4; r++) a[r] = sa[(ty + 16 * r) * kRowPad + k];
#pragma unroll
    for (int c = 0; c < 4; c++) b[c] = sb[(tx + 16 * c) * kRowPad + k];
}

// what a lane stages of one step: word w of rows r0 + 8 it of both tiles (absent rows and words are zero)
__device__ inline void stage_load(const uint64_t* __restrict__ xt, int n, int d, int nw64, int i0, int j0, int r0, int w,
                                  uint64_t (&va)[kStagePerLane], uint64_t (&vb)[kStagePerLane])
{
    const uint64_t mask = (w == nw64 - 1) ? last_word_mask(n) : ~0ull;
#pragma unroll
    for (int it = 0; it < kStagePerLane; it++) {
        const int oi = i0 + r0 + 8 * it, oj = j0 + r0 + 8 * it;
        va[it] = (w < nw64 && oi < d) ? (xt[(size_t)oi * nw64 + w] & mask) : 0ull;
        vb[it] = (w < nw64 && oj < d) ? (xt[(size_t)oj * nw64 + w] & mask) : 0ull;
    }
}

// (LDS admits four workgroups per CU: the registers are held to the same four waves per SIMD)
__global__ __launch_bounds__(kDistThreads, 4) void k_org_dist(const uint64_t* __restrict__ xt, int n, int d, int nw64, int tiles, int supers,
                                                             const int* __restrict__ pop, double* __restrict__ dist)
{
    // Blocks that run together take the tiles of one kOrgSuper x kOrgSuper square of tiles: they share 2 kOrgSuper tiles'
    // rows in L2 and the Infinity Cache instead of reading a whole row of tiles from HBM for every tile row.
    const int sid = blockIdx.x / (kOrgSuper * kOrgSuper), in = blockIdx.x % (kOrgSuper * kOrgSuper);
    const int bi = (sid / supers) * kOrgSuper + in / kOrgSuper, bj = (sid % supers) * kOrgSuper + in % kOrgSuper;
    if (bj < bi || bj >= tiles) return;           // the tiles below the diagonal are the mirror stores of those above
    __shared__ uint64_t s_mem[kStageWords];
    uint64_t* sa = s_mem;
    uint64_t* sb = s_mem + kOrgTile * kRowPad;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int lw = t & 31, lr = t >> 5;
    const int i0 = bi * kOrgTile, j0 = bj * kOrgTile;
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0;
    uint64_t va[kStagePerLane], vb[kStagePerLane];
    stage_load(xt, n, d, nw64, i0, j0, lr, lw, va, vb);
    for (int w0 = 0; w0 < nw64; w0 += kOrgChunk) {
#pragma unroll
        for (int it = 0; it < kStagePerLane; it++) {
            sa[(lr + 8 * it) * kRowPad + lw] = va[it];
            sb[(lr + 8 * it) * kRowPad + lw] = vb[it];
        }
        __syncthreads();
        if (w0 + kOrgChunk < nw64) stage_load(xt, n, d, nw64, i0, j0, lr, w0 + kOrgChunk + lw, va, vb);   // the next step's, in flight
        // word k + 1's LDS reads are issued before word k's counts: a wave has its next operands on the way while it counts
        uint64_t a[2][4], b[2][4];
        lds_words(sa, sb, ty, tx, 0, a[0], b[0]);
#pragma unroll 1
        for (int k = 0; k < kOrgChunk; k += 2) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (h == 0 || k + 2 < kOrgChunk) lds_words(sa, sb, ty, tx, k + h + 1, a[h ^ 1], b[h ^ 1]);
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        add_bits(acc[r][c], (uint32_t)a[h][r] & (uint32_t)b[h][c]);
                        add_bits(acc[r][c], (uint32_t)(a[h][r] >> 32) & (uint32_t)(b[h][c] >> 32));
                    }
            }
        }
        __syncthreads();
    }
    // the tile as doubles in LDS, then whole rows out: as it stands and, off the diagonal, transposed
    double* tile = reinterpret_cast<double*>(s_mem);
    int pa[4], pb[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int gi = i0 + ty + 16 * r, gj = j0 + tx + 16 * r;
        pa[r] = gi < d ? pop[gi] : 0;
        pb[r] = gj < d ? pop[gj] : 0;
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int inter = acc[r][c], uni = pa[r] + pb[c] - inter;
            tile[(ty + 16 * r) * kTilePad + tx + 16 * c] = uni > 0 ? (double)(uni - inter) / (double)uni : 0.0;
        }
    __syncthreads();
    const int c = t & 63;
    for (int r = t >> 6; r < kOrgTile; r += kDistThreads / 64) {
        if (i0 + r < d && j0 + c < d) dist[(size_t)(i0 + r) * d + j0 + c] = tile[r * kTilePad + c];
        if (bi != bj && j0 + r < d && i0 + c < d) dist[(size_t)(j0 + r) * d + i0 + c] = tile[c * kTilePad + r];
    }
}

// ---- the merges ------------------------------------------------------------------------------------------------------
constexpr int kNone = INT_MAX;                    // no candidate yet: behind every index

// the lexicographic (value, index) order: the first, lowest index wins a tie, as a serial scan with a strict < has it
__device__ inline bool before(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

__device__ inline bool is_live(const uint32_t* live, int k) { return (live[k >> 5] >> (k & 31)) & 1u; }

// lane 0 gets the wave's minimum
__device__ inline void wave_min(double& v, int& i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int oi = __shfl_down(i, off);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// NN and DISNN of every row before the first merge (all live): one wave per row i < d - 1
__global__ __launch_bounds__(256) void k_org_nn_init(const double* __restrict__ W, int d, int* __restrict__ nn, double* __restrict__ disnn)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= d - 1) return;
    const double* row = W + (size_t)i * d;
    double bv = INFINITY;
    int bj = kNone;
    for (int j = i + 1 + lane; j < d; j += 64) {
        const double v = row[j];
        if (before(v, j, bv, bj)) { bv = v; bj = j; }
    }
    wave_min(bv, bj);
    if (lane == 0) { nn[i] = bj; disnn[i] = bv; }
}

// the workgroup's minimum of (v, i) into s_v[0], s_i[0]: thread 0, which wrote them, may read them at once
__device__ inline void block_min(double v, int i, double* s_v, int* s_i)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_min(v, i);
    __syncthreads();                              // (the last reader of s_v, s_i is done)
    if (lane == 0) { s_v[wave] = v; s_i[wave] = i; }
    __syncthreads();
    if (wave == 0) {
        v = lane < kMergeThreads / 64 ? s_v[lane] : INFINITY;
        i = lane < kMergeThreads / 64 ? s_i[lane] : kNone;
        wave_min(v, i);
        if (lane == 0) { s_v[0] = v; s_i[0] = i; }
    }
}

// The loops below keep kInFlight loads of a lane in flight: a row is 8 d bytes in HBM and one workgroup walks it, so what a
// merge costs is the round trips it waits for, not the bytes.
constexpr int kInFlight = 4;

// the minimum of row[k] over the live k in [k0, d), the share of lane `me` of `lanes`
__device__ inline void row_min(const double* row, const uint32_t* live, int k0, int d, int me, int lanes, double& v, int& j)
{
    for (int k = k0 + me; k < d; k += kInFlight * lanes) {
        double x[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; u++) x[u] = k + u * lanes < d ? row[k + u * lanes] : INFINITY;
#pragma unroll
        for (int u = 0; u < kInFlight; u++) {
            const int ku = k + u * lanes;
            if (ku < d && is_live(live, ku) && before(x[u], ku, v, j)) { v = x[u]; j = ku; }
        }
    }
}

__global__ __launch_bounds__(kMergeThreads) void k_org_merges(double* W, int d, int* nn, double* disnn, int* list, int* __restrict__ i2o,
                                                             int* __restrict__ j2o, double* __restrict__ ho)
{
    constexpr int kWaves = kMergeThreads / 64, kStride = kInFlight * kMergeThreads;
    __shared__ uint32_t s_live[kOrgMax / 32];
    __shared__ double s_v[kWaves];
    __shared__ int s_i[kWaves];
    __shared__ int s_pair[2], s_cnt;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int w = t; w < kOrgMax / 32; w += kMergeThreads) {
        const int lo = w * 32;
        s_live[w] = lo + 32 <= d ? ~0u : (lo >= d ? 0u : ((1u << (d - lo)) - 1u));
    }
    if (t == 0) i2o[d - 2] = -1;                  // until the last merge is recorded
    __syncthreads();
    for (int step = 0; step < d - 1; step++) {
        // the live i of least DISNN
        double bv = INFINITY;
        int bi = kNone;
        for (int i = t; i < d - 1; i += kStride) {
            double x[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) x[u] = i + u * kMergeThreads < d - 1 ? disnn[i + u * kMergeThreads] : INFINITY;
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int iu = i + u * kMergeThreads;
                if (iu < d - 1 && is_live(s_live, iu) && before(x[u], iu, bv, bi)) { bv = x[u]; bi = iu; }
            }
        }
        block_min(bv, bi, s_v, s_i);
        if (t == 0) {
            const int im = s_i[0], jm = im < d - 1 ? nn[im] : -1;
            const int a = im < jm ? im : jm, b = im < jm ? jm : im;
            s_pair[0] = a; s_pair[1] = b; s_cnt = 0;
            if (a >= 0 && b < d) {
                i2o[step] = a; j2o[step] = b; ho[step] = s_v[0];
                s_live[b >> 5] &= ~(1u << (b & 31));
            }
        }
        __syncthreads();
        const int I2 = s_pair[0], J2 = s_pair[1];
        if (I2 < 0 || J2 >= d) return;            // (cannot be: the lowest live row has a live neighbour; i2o[d - 2] stays -1)
        // d(I2, k) = max(d(I2, k), d(J2, k)), both halves of the square; the nearest k > I2
        double* rowI = W + (size_t)I2 * d;
        const double* rowJ = W + (size_t)J2 * d;
        bv = INFINITY; bi = kNone;
        for (int k = t; k < d; k += kStride) {
            double xa[kInFlight], xb[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int ku = k + u * kMergeThreads;
                xa[u] = ku < d ? rowI[ku] : 0.0;
                xb[u] = ku < d ? rowJ[ku] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int ku = k + u * kMergeThreads;
                if (ku < d && ku != I2 && is_live(s_live, ku)) {
                    double a = xa[u];
                    if (xb[u] > a) { a = xb[u]; rowI[ku] = a; W[(size_t)ku * d + I2] = a; }
                    if (ku > I2 && before(a, ku, bv, bi)) { bv = a; bi = ku; }
                }
            }
        }
        block_min(bv, bi, s_v, s_i);
        if (t == 0) { nn[I2] = s_i[0] == kNone ? -1 : s_i[0]; disnn[I2] = s_v[0]; }
        __syncthreads();
        // the live rows whose NN was I2 or J2 ...
        for (int i = t; i < d - 1; i += kStride) {
            int q[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) q[u] = i + u * kMergeThreads < d - 1 ? nn[i + u * kMergeThreads] : -1;
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int iu = i + u * kMergeThreads;
                if (iu < d - 1 && (q[u] == I2 || q[u] == J2) && is_live(s_live, iu)) list[atomicAdd(&s_cnt, 1)] = iu;
            }
        }
        __syncthreads();
        // ... searched again: `group` waves to a row (all of them for one row, one for sixteen rows or more), their
        // minima joined through LDS
        const int cnt = s_cnt;
        int group = kWaves;
        while (group > 1 && group * cnt > kWaves) group >>= 1;
        const int per_round = kWaves / group;
        for (int base = 0; base < cnt; base += per_round) {
            const int q = base + wave / group;
            double v = INFINITY;
            int j = kNone, i = -1;
            if (q < cnt) {
                i = list[q];
                row_min(W + (size_t)i * d, s_live, i + 1, d, (wave % group) * 64 + lane, group * 64, v, j);
                wave_min(v, j);
            }
            if (group > 1) {
                if (lane == 0) { s_v[wave] = v; s_i[wave] = j; }
                __syncthreads();
                if (q < cnt && wave % group == 0) {
                    v = lane < group ? s_v[wave + lane] : INFINITY;
                    j = lane < group ? s_i[wave + lane] : kNone;
                    wave_min(v, j);
                }
            }
            if (q < cnt && wave % group == 0 && lane == 0) { nn[i] = j == kNone ? -1 : j; disnn[i] = v; }
            if (group > 1) __syncthreads();       // (s_v, s_i are free for the next round)
        }
        __syncthreads();
    }
}

// ---- the raster ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_org_cells(const uint64_t* __restrict__ xt, int d, int nw64, const int* __restrict__ fam,
                                                  const int* __restrict__ org, int col_blocks, uint8_t* __restrict__ out)
{
    const int r = blockIdx.x / col_blocks, c = (blockIdx.x % col_blocks) * 256 + threadIdx.x;
    if (c >= d) return;
    const int f = fam[r];
    out[(size_t)r * d + c] = (uint8_t)((xt[(size_t)org[c] * nw64 + (f >> 6)] >> (f & 63)) & 1ull);
}

}  // namespace

void launch_org_popcount(const MasterDev& m, int* pop, hipStream_t s)
{
    hipLaunchKernelGGL(k_org_popcount, dim3((m.d + 3) / 4), dim3(256), 0, s, m.xt, m.n, m.d, m.nw64, pop);
}

void launch_org_distances(const MasterDev& m, const int* pop, double* dist, hipStream_t s)
{
    const int tiles = (m.d + kOrgTile - 1) / kOrgTile, supers = (tiles + kOrgSuper - 1) / kOrgSuper;
    hipLaunchKernelGGL(k_org_dist, dim3(supers * supers * kOrgSuper * kOrgSuper), dim3(kDistThreads), 0, s, m.xt, m.n, m.d, m.nw64, tiles, supers,
                       pop, dist);
}

void launch_org_merges(double* work, int d, int* nn, double* disnn, int* list, int* i2, int* j2, double* height, hipStream_t s)
{
    hipLaunchKernelGGL(k_org_nn_init, dim3((d - 1 + 3) / 4), dim3(256), 0, s, (const double*)work, d, nn, disnn);
    hipLaunchKernelGGL(k_org_merges, dim3(1), dim3(kMergeThreads), 0, s, work, d, nn, disnn, list, i2, j2, height);
}

void launch_org_cells(const MasterDev& m, const int* fam, const int* org, int rows, uint8_t* out, hipStream_t s)
{
    const int col_blocks = (m.d + 255) / 256;
    hipLaunchKernelGGL(k_org_cells, dim3((unsigned)((size_t)rows * col_blocks)), dim3(256), 0, s, m.xt, m.d, m.nw64, fam, org, col_blocks, out);
}

}  // namespace nemk

using namespace nemk;

// The organisms' distances on the device, with the raster's buffers kept between batches.  It reads its master's rows:
// the master must outlive it.
struct nemgpu_orgclust {
    int device = 0, n = 0, d = 0;
    const nemgpu_master* m = nullptr;
    double* dist = nullptr;                           // [d][d]
    int* pop = nullptr;                               // [d]
    int *fam = nullptr, *org = nullptr;               // a batch's families, the organisms' order
    uint8_t* cells = nullptr;
    size_t fam_cap = 0, cells_cap = 0;
};

namespace {

constexpr int kCellsRowsMax = 1 << 22;                // families per raster batch (rows x column blocks stays a grid size)

void orgclust_free(nemgpu_orgclust* h)
{
    void* all[] = {h->dist, h->pop, h->fam, h->org, h->cells};
    for (void* p : all) if (p) (void)hipFree(p);
    delete h;
}

// order[count] is a permutation of 0 .. count - 1
bool is_permutation(const int32_t* order, int count)
{
    std::vector<uint8_t> seen((size_t)count, 0);
    for (int i = 0; i < count; i++) {
        const int v = order[i];
        if (v < 0 || v >= count || seen[(size_t)v]) return false;
        seen[(size_t)v] = 1;
    }
    return true;
}

int arg_error(const std::string& msg) { set_error(msg); return NEMGPU_E_ARG; }

}  // namespace

int nemgpu_orgdist_tile_info(int* tile, int* chunk_words, int* max_organisms)
{
    if (tile) *tile = kOrgTile;
    if (chunk_words) *chunk_words = kOrgChunk;
    if (max_organisms) *max_organisms = kOrgMax;
    return NEMGPU_OK;
}

int nemgpu_orgclust_create(nemgpu_orgclust** out, const nemgpu_master* m)
{
    if (!out) return arg_error("nemgpu_orgclust_create: out is NULL");
    *out = nullptr;
    if (!m) return arg_error("nemgpu_orgclust_create: a master is needed");
    if (m->d > kOrgMax) return arg_error("nemgpu_orgclust_create: " + std::to_string(m->d) + " organisms, more than " + std::to_string(kOrgMax));
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    nemgpu_orgclust* h = new nemgpu_orgclust();
    h->device = m->device; h->n = m->n; h->d = m->d; h->m = m;
    const size_t d = (size_t)m->d;
    hipError_t err = hipMalloc((void**)&h->dist, a256(d * d * 8));
    if (err == hipSuccess) err = hipMalloc((void**)&h->pop, a256(d * 4));
    if (err == hipSuccess) err = hipMalloc((void**)&h->org, a256(d * 4));
    if (err != hipSuccess) { (void)hipGetLastError(); orgclust_free(h); set_error("nemgpu_orgclust_create: device memory"); return NEMGPU_E_MEMORY; }
    launch_org_popcount(m->dev, h->pop, m->stream);
    launch_org_distances(m->dev, h->pop, h->dist, m->stream);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    if (err != hipSuccess) { orgclust_free(h); return device_status("nemgpu_orgclust_create", err); }
    *out = h;
    return NEMGPU_OK;
}

int nemgpu_orgclust_shape(const nemgpu_orgclust* h, int* n, int* d)
{
    if (!h) return arg_error("nemgpu_orgclust_shape: the handle is NULL");
    if (n) *n = h->n;
    if (d) *d = h->d;
    return NEMGPU_OK;
}

int nemgpu_orgclust_distances(const nemgpu_orgclust* h, int i0, int rows, double* out)
{
    if (!h || !out) return arg_error("nemgpu_orgclust_distances: a NULL pointer");
    if (i0 < 0 || rows <= 0 || (long long)i0 + rows > h->d) return arg_error("nemgpu_orgclust_distances: rows outside the square");
    HIPCHK(hipSetDevice(h->device));
    return device_status("nemgpu_orgclust_distances",
                         hipMemcpy(out, h->dist + (size_t)i0 * h->d, (size_t)rows * h->d * 8, hipMemcpyDeviceToHost));
}

int nemgpu_orgclust_run(nemgpu_orgclust* h, int32_t* i2, int32_t* j2, double* height)
{
    if (!h) return arg_error("nemgpu_orgclust_run: the handle is NULL");
    if (h->d < 2) return NEMGPU_OK;                   // one organism: no merge
    if (!i2 || !j2 || !height) return arg_error("nemgpu_orgclust_run: a NULL pointer");
    HIPCHK(hipSetDevice(h->device));
    const size_t d = (size_t)h->d, sq = a256(d * d * 8), b8 = a256(d * 8), b4 = a256(d * 4);
    char* block = nullptr;                            // work | disnn | height | nn | list | i2 | j2
    if (hipMalloc((void**)&block, sq + 2 * b8 + 4 * b4) != hipSuccess) {
        (void)hipGetLastError(); set_error("nemgpu_orgclust_run: device memory for the merges' copy of the distances"); return NEMGPU_E_MEMORY;
    }
    double* work = (double*)block;
    double* disnn = (double*)(block + sq);
    double* hd = (double*)(block + sq + b8);
    int* nn = (int*)(block + sq + 2 * b8);
    int* list = (int*)(block + sq + 2 * b8 + b4);
    int* i2d = (int*)(block + sq + 2 * b8 + 2 * b4);
    int* j2d = (int*)(block + sq + 2 * b8 + 3 * b4);
    hipStream_t s = h->m->stream;
    hipError_t err = hipMemcpyAsync(work, h->dist, d * d * 8, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess) { launch_org_merges(work, h->d, nn, disnn, list, i2d, j2d, hd, s); err = hipGetLastError(); }
    if (err == hipSuccess) err = hipMemcpyAsync(i2, i2d, (d - 1) * 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipMemcpyAsync(j2, j2d, (d - 1) * 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipMemcpyAsync(height, hd, (d - 1) * 8, hipMemcpyDeviceToHost, s);
    const hipError_t waited = hipStreamSynchronize(s);
    if (err == hipSuccess) err = waited;
    (void)hipFree(block);
    if (err == hipSuccess && i2[d - 2] < 0) { set_error("nemgpu_orgclust_run: the merge loop met a row without a live neighbour"); return NEMGPU_E_INTERNAL; }
    return device_status("nemgpu_orgclust_run", err);
}

int nemgpu_orgclust_cells(nemgpu_orgclust* h, const int32_t* fam_order, const int32_t* org_order, int row0, int rows, uint8_t* out)
{
    if (!h || !fam_order || !org_order || !out) return arg_error("nemgpu_orgclust_cells: a NULL pointer");
    if (row0 < 0 || rows <= 0 || (long long)row0 + rows > h->n) return arg_error("nemgpu_orgclust_cells: rows outside the families");
    if (rows > kCellsRowsMax) return arg_error("nemgpu_orgclust_cells: more than " + std::to_string(kCellsRowsMax) + " rows in a batch");
    if (!is_permutation(fam_order, h->n)) return arg_error("nemgpu_orgclust_cells: fam_order is not a permutation of the families");
    if (!is_permutation(org_order, h->d)) return arg_error("nemgpu_orgclust_cells: org_order is not a permutation of the organisms");
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)rows * h->d;
    if (h->fam_cap < (size_t)rows) {
        if (h->fam) (void)hipFree(h->fam);
        h->fam = nullptr; h->fam_cap = 0;
        HIPCHK(hipMalloc((void**)&h->fam, a256((size_t)rows * 4)));
        h->fam_cap = (size_t)rows;
    }
    if (h->cells_cap < bytes) {
        if (h->cells) (void)hipFree(h->cells);
        h->cells = nullptr; h->cells_cap = 0;
        HIPCHK(hipMalloc((void**)&h->cells, a256(bytes)));
        h->cells_cap = bytes;
    }
    hipStream_t s = h->m->stream;
    hipError_t err = hipMemcpyAsync(h->fam, fam_order + row0, (size_t)rows * 4, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemcpyAsync(h->org, org_order, (size_t)h->d * 4, hipMemcpyHostToDevice, s);
    if (err == hipSuccess) { launch_org_cells(h->m->dev, h->fam, h->org, rows, h->cells, s); err = hipGetLastError(); }
    if (err == hipSuccess) err = hipMemcpyAsync(out, h->cells, bytes, hipMemcpyDeviceToHost, s);
    const hipError_t waited = hipStreamSynchronize(s);
    if (err == hipSuccess) err = waited;
    return device_status("nemgpu_orgclust_cells", err);
}

void nemgpu_orgclust_destroy(nemgpu_orgclust* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    orgclust_free(h);
}
