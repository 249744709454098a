// nem_layout_bh.hip -- see nem_layout_bh.hpp.  The kernels in the order they run, then the C entry points
// (nemgpu_layout_create_bh, _bh_shape, _bh_tree): what is refused for its arguments alone is refused on the host before
// the first HIP call.  Every lane tests its index before it touches a per-body or per-cell array.
#include "nem_layout_bh.hpp"

#include <cmath>
#include <string>
#include <vector>

#include "nem_internal.hpp"
#include "nem_master.hpp"
#include "nem_scan.hpp"
#include "nem_table.hpp"

namespace nemk {

namespace {

constexpr int kT = kLayoutTile;
constexpr int kLevels = kBhDepth + 1;

// ---- the square: per block of bodies, then over the blocks (min and max: any order gives the same) ------------------
__device__ inline void block_min_max(double (*s)[kT], double lo_x, double hi_x, double lo_y, double hi_y)
{
    s[0][threadIdx.x] = lo_x; s[1][threadIdx.x] = hi_x; s[2][threadIdx.x] = lo_y; s[3][threadIdx.x] = hi_y;
    __syncthreads();
    for (int half = kT / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            s[0][threadIdx.x] = fmin(s[0][threadIdx.x], s[0][threadIdx.x + half]);
            s[1][threadIdx.x] = fmax(s[1][threadIdx.x], s[1][threadIdx.x + half]);
            s[2][threadIdx.x] = fmin(s[2][threadIdx.x], s[2][threadIdx.x + half]);
            s[3][threadIdx.x] = fmax(s[3][threadIdx.x], s[3][threadIdx.x + half]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kT) void k_bh_box_blocks(const double* __restrict__ x, const double* __restrict__ y, int n, double* __restrict__ part)
{
    __shared__ double s[4][kT];
    const int i = blockIdx.x * kT + threadIdx.x;
    const bool mine = i < n;
    const double xi = mine ? x[i] : 0.0, yi = mine ? y[i] : 0.0;
    block_min_max(s, mine ? xi : INFINITY, mine ? xi : -INFINITY, mine ? yi : INFINITY, mine ? yi : -INFINITY);
    if (threadIdx.x < 4) part[4 * (size_t)blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kT) void k_bh_box(const double* __restrict__ part, int nb, BhBox* __restrict__ box)
{
    __shared__ double s[4][kT];
    double lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += kT) {
        lo_x = fmin(lo_x, part[4 * (size_t)b]);     hi_x = fmax(hi_x, part[4 * (size_t)b + 1]);
        lo_y = fmin(lo_y, part[4 * (size_t)b + 2]); hi_y = fmax(hi_y, part[4 * (size_t)b + 3]);
    }
    block_min_max(s, lo_x, hi_x, lo_y, hi_y);
    if (threadIdx.x != 0) return;
    const double side = fmax(s[1][0] - s[0][0], s[3][0] - s[2][0]);
    box->x0 = s[0][0];
    box->y0 = s[2][0];
    box->side = side;
    box->live = side > 0.0 ? 1 : 0;
    box->pad = 0;
}

// ---- the keys ---------------------------------------------------------------------------------------------------------
__device__ inline uint32_t spread16(uint32_t c)
{
    c = (c | (c << 8)) & 0x00FF00FFu;
    c = (c | (c << 4)) & 0x0F0F0F0Fu;
    c = (c | (c << 2)) & 0x33333333u;
    c = (c | (c << 1)) & 0x55555555u;
    return c;
}

__device__ inline uint32_t grid_cell(double v, double v0, double side)
{
    constexpr double G = (double)(1 << kBhDepth);
    const double t = (v - v0) / side;
    const double g = t * G;
    return g >= 0.0 ? (g >= G ? (uint32_t)(1 << kBhDepth) - 1u : (uint32_t)g) : 0u;        // (a NaN: 0)
}

__global__ __launch_bounds__(kT) void k_bh_keys(const double* __restrict__ x, const double* __restrict__ y, int n, const BhBox* __restrict__ box,
                                                uint32_t* __restrict__ key, uint32_t* __restrict__ val)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const BhBox b = *box;
    key[i] = b.live ? spread16(grid_cell(x[i], b.x0, b.side)) | (spread16(grid_cell(y[i], b.y0, b.side)) << 1) : 0u;
    val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kT) void k_bh_gather(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ mass, int n,
                                                  const uint32_t* __restrict__ order, double* __restrict__ sx, double* __restrict__ sy,
                                                  double* __restrict__ sm)
{
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const uint32_t o = order[p];
    sx[p] = x[o];
    sy[p] = y[o];
    sm[p] = mass[o];
}

// ---- the cells ----------------------------------------------------------------------------------------------------------
// the end of the run at level `l` (> 0) that holds sorted position p, searched in (p, hi)
__device__ inline int run_end(const uint32_t* skey, int p, int hi, uint32_t key, int l)
{
    const int shift = 2 * (kBhDepth - l);
    const uint64_t next = ((uint64_t)(key >> shift) + 1ull) << shift;
    return next > 0xffffffffull ? hi : seg::lower_bound(skey, p + 1, hi, (uint32_t)next);
}

// a lane per sorted position follows its runs down the levels: flag[l][p] = a cell of level l starts at p.  The run of
// level l lies inside the run of level l - 1, and a cell exists iff that one holds more than kBhLeaf bodies
__global__ __launch_bounds__(kT) void k_bh_heads(const uint32_t* __restrict__ skey, int n, const BhBox* __restrict__ box, int* __restrict__ flag)
{
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const uint32_t key = skey[p];
    int lo = 0, hi = n;
    bool more = box->live != 0;
    for (int l = 0; l < kLevels; l++) {
        int f = 0;
        if (more) {
            if (l > 0) {
                const int shift = 2 * (kBhDepth - l);
                lo = seg::lower_bound(skey, lo, p, (key >> shift) << shift);
                hi = run_end(skey, p, hi, key, l);
            }
            f = lo == p ? 1 : 0;
            more = hi - lo > kBhLeaf;
        }
        flag[(size_t)l * n + p] = f;
    }
}

// a lane per (level, sorted position): where a cell starts, its extent and its links.  cid = the exclusive scan of flag:
// the cells are numbered by level, then by run order.  The cell after one that ends at `hi` is the shallowest that starts
// there: at the first level at which the keys on both sides of `hi` differ
__global__ __launch_bounds__(kT) void k_bh_cells(const uint32_t* __restrict__ skey, int n, const int* __restrict__ flag, const int* __restrict__ cid,
                                                 long long cap, BhCell* __restrict__ cell, int* __restrict__ level)
{
    const int p = blockIdx.x * kT + threadIdx.x;
    const int l = blockIdx.y;
    if (p >= n || !flag[(size_t)l * n + p]) return;
    const int c = cid[(size_t)l * n + p];
    if (c >= cap) return;                                     // (the bound holds: no cell is ever dropped here)
    const int hi = l == 0 ? n : run_end(skey, p, n, skey[p], l);
    const bool leaf = hi - p <= kBhLeaf || l == kBhDepth;
    BhCell out;
    out.lo = p;
    out.hi = hi;
    out.child = leaf ? -1 : cid[(size_t)(l + 1) * n + p];
    out.rope = -1;
    const uint32_t diff = hi < n ? skey[hi - 1] ^ skey[hi] : 0u;      // (not 0 inside: the run ended where the key grew)
    if (diff) {
        const int top = 31 - __clz((int)diff);
        out.rope = cid[(size_t)(kBhDepth - (top >> 1)) * n + hi];
    }
    if (out.child >= cap) out.child = -1;                     // (as above: never taken)
    if (out.rope >= cap) out.rope = -1;
    cell[c] = out;
    level[c] = l;
}

// one launch per level, the deepest first: a lane per cell of the level sums its bodies (a leaf) or its children, left to right
__global__ __launch_bounds__(kT) void k_bh_moments(int l, int n, const int* __restrict__ cid, const int* __restrict__ cells, long long cap,
                                                   const BhBox* __restrict__ box, const BhCell* __restrict__ cell, const double* __restrict__ sx,
                                                   const double* __restrict__ sy, const double* __restrict__ sm, double* __restrict__ M,
                                                   double* __restrict__ Sx, double* __restrict__ Sy, BhCentre* __restrict__ centre)
{
    const long long total = min((long long)*cells, cap);
    const long long first = cid[(size_t)l * n];
    const long long end = l == kBhDepth ? total : min((long long)cid[(size_t)(l + 1) * n], total);
    const long long c = first + (long long)blockIdx.x * kT + threadIdx.x;
    if (c >= end) return;
    const BhCell me = cell[c];
    double m = 0.0, ax = 0.0, ay = 0.0;
    if (me.child < 0) {
        for (int j = me.lo; j < me.hi; j++) {
            const double mj = sm[j];
            m += mj;
            ax += mj * sx[j];
            ay += mj * sy[j];
        }
    } else {
        int k = me.child;
        for (int done = me.lo; done < me.hi && k < total; k++) {      // (the children partition their parent, in key order)
            m += M[k];
            ax += Sx[k];
            ay += Sy[k];
            done = cell[k].hi;
        }
    }
    M[c] = m;
    Sx[c] = ax;
    Sy[c] = ay;
    const double s = box->side / (double)(1 << l);
    centre[c] = BhCentre{ax / m, ay / m, m, s * s};
}

// ---- the walk: a lane per sorted body; neighbouring lanes are neighbours in space and walk alike --------------------
__global__ __launch_bounds__(kT) void k_layout_bh_walk(const uint32_t* __restrict__ order, const double* __restrict__ sx, const double* __restrict__ sy,
                                                       const double* __restrict__ sm, int n, const BhBox* __restrict__ box,
                                                       const BhCell* __restrict__ cell, const BhCentre* __restrict__ centre, double scaling,
                                                       double theta2, double* __restrict__ px, double* __restrict__ py, int* __restrict__ accepted,
                                                       int* __restrict__ visited)
{
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= n) return;
    const double xi = sx[p], yi = sy[p];
    const double smi = scaling * sm[p];
    double ax = 0.0, ay = 0.0;
    int na = 0, nv = 0;
    int c = box->live ? 0 : -1;                               // (no tree: no repulsion)
    while (c >= 0) {                                          // (a rope strictly advances in depth-first order)
        const BhCell me = cell[c];
        if (me.child < 0) {
            for (int j = me.lo; j < me.hi; j++) {
                const double dx = xi - sx[j], dy = yi - sy[j];
                const double d2 = dx * dx + dy * dy;
                const double coef = d2 > 0.0 ? (smi * sm[j]) / d2 : 0.0;      // j = i and a coincident pair: nothing
                ax += dx * coef;
                ay += dy * coef;
            }
            nv += me.hi - me.lo;
            c = me.rope;
            continue;
        }
        if (p >= me.lo && p < me.hi) { c = me.child; continue; }              // (its own cell is always opened)
        const BhCentre far = centre[c];
        const double dx = xi - far.cx, dy = yi - far.cy;
        const double d2 = dx * dx + dy * dy;
        if (theta2 * d2 > far.s2) {
            const double coef = (smi * far.M) / d2;
            ax += dx * coef;
            ay += dy * coef;
            na++;
            c = me.rope;
        } else {
            c = me.child;
        }
    }
    const uint32_t o = order[p];
    px[o] = ax;
    py[o] = ay;
    if (accepted) accepted[o] = na;
    if (visited) visited[o] = nv;
}

template <class T>
T* carve(char* base, size_t* at, size_t count)
{
    T* p = reinterpret_cast<T*>(base + *at);
    *at += a256(count * sizeof(T));
    return p;
}

hipError_t sort_bodies(LayoutBh* b, bool size_only, hipStream_t s)
{
    rocprim::double_buffer<uint32_t> keys(b->k0, b->k1), vals(b->v0, b->v1);
    const hipError_t err = rocprim::radix_sort_pairs(size_only ? nullptr : b->sort_tmp, b->sort_bytes, keys, vals, (unsigned)b->n, 0u,
                                                     2u * kBhDepth, s);
    if (err == hipSuccess && !size_only) { b->skey = keys.current(); b->order = vals.current(); }
    return err;
}

}  // namespace

hipError_t layout_bh_create(LayoutBh** out, int n, double theta, hipStream_t s)
{
    *out = nullptr;
    LayoutBh* b = new LayoutBh();
    b->n = n;
    b->theta = theta;
    b->theta2 = theta * theta;
    b->box_blocks = (n + kT - 1) / kT;
    b->cell_cap = bh_cell_bound(n);
    hipError_t err = n > 1 ? sort_bodies(b, true, s) : hipSuccess;             // (the size of the sort's temporary storage)
    if (err != hipSuccess) { delete b; return err; }
    const size_t un = (size_t)n, cap = (size_t)b->cell_cap, flat = (size_t)kLevels * un;
    const size_t bytes = a256(b->sort_bytes) + a256(4 * (size_t)b->box_blocks * 8) + a256(sizeof(BhBox)) + 4 * a256(un * 4) + 3 * a256(un * 8) +
                         2 * a256(flat * 4) + a256((flat / seg::kScanTile + 2) * 4) + a256(4) + a256(cap * sizeof(BhCell)) +
                         a256(cap * sizeof(BhCentre)) + a256(cap * 4) + 3 * a256(cap * 8) + 2 * a256(un * 4);
    err = hipMalloc((void**)&b->block, bytes);
    if (err != hipSuccess) { delete b; return err; }
    size_t at = 0;
    b->sort_tmp = carve<char>(b->block, &at, b->sort_bytes);
    b->part = carve<double>(b->block, &at, 4 * (size_t)b->box_blocks);
    b->box = carve<BhBox>(b->block, &at, 1);
    b->k0 = carve<uint32_t>(b->block, &at, un); b->k1 = carve<uint32_t>(b->block, &at, un);
    b->v0 = carve<uint32_t>(b->block, &at, un); b->v1 = carve<uint32_t>(b->block, &at, un);
    b->sx = carve<double>(b->block, &at, un); b->sy = carve<double>(b->block, &at, un); b->sm = carve<double>(b->block, &at, un);
    b->flag = carve<int>(b->block, &at, flat); b->cid = carve<int>(b->block, &at, flat);
    b->scan_partial = carve<int>(b->block, &at, flat / seg::kScanTile + 2);
    b->cells = carve<int>(b->block, &at, 1);
    b->cell = carve<BhCell>(b->block, &at, cap);
    b->centre = carve<BhCentre>(b->block, &at, cap);
    b->level = carve<int>(b->block, &at, cap);
    b->M = carve<double>(b->block, &at, cap); b->Sx = carve<double>(b->block, &at, cap); b->Sy = carve<double>(b->block, &at, cap);
    b->accepted = carve<int>(b->block, &at, un); b->visited = carve<int>(b->block, &at, un);
    b->skey = b->k0;
    b->order = b->v0;
    err = hipMemsetAsync(b->block, 0, bytes, s);
    if (err != hipSuccess) { layout_bh_free(b); return err; }
    *out = b;
    return hipSuccess;
}

void layout_bh_free(LayoutBh* b)
{
    if (!b) return;
    if (b->block) (void)hipFree(b->block);
    delete b;
}

hipError_t launch_layout_bh_repulse(const LayoutDev& l, const LayoutParams& p, LayoutBh* b, bool counters, hipStream_t s)
{
    const int n = l.n;
    if (n <= 0) return hipSuccess;
    const dim3 tile(kT), bodies(l.blocks);
    hipLaunchKernelGGL(k_bh_box_blocks, bodies, tile, 0, s, (const double*)l.x, (const double*)l.y, n, b->part);
    hipLaunchKernelGGL(k_bh_box, dim3(1), tile, 0, s, (const double*)b->part, b->box_blocks, b->box);
    hipLaunchKernelGGL(k_bh_keys, bodies, tile, 0, s, (const double*)l.x, (const double*)l.y, n, (const BhBox*)b->box, b->k0, b->v0);
    if (n > 1) {
        HIPTRY(sort_bodies(b, false, s));
    } else {
        b->skey = b->k0;
        b->order = b->v0;
    }
    hipLaunchKernelGGL(k_bh_gather, bodies, tile, 0, s, (const double*)l.x, (const double*)l.y, (const double*)l.mass, n, b->order, b->sx, b->sy, b->sm);
    hipLaunchKernelGGL(k_bh_heads, bodies, tile, 0, s, b->skey, n, (const BhBox*)b->box, b->flag);
    seg::scan<int, seg::OpSum<int>, false>(b->flag, b->cid, kLevels * n, seg::OpSum<int>(), 0, b->scan_partial, b->cells, s);
    hipLaunchKernelGGL(k_bh_cells, dim3(l.blocks, kLevels), tile, 0, s, b->skey, n, (const int*)b->flag, (const int*)b->cid, b->cell_cap, b->cell,
                       b->level);
    for (int lv = kBhDepth; lv >= 0; lv--) {
        const int most = lv == 0 ? 1 : bh_level_bound(n);
        if (most <= 0) continue;                              // (n <= kBhLeaf: the root alone)
        hipLaunchKernelGGL(k_bh_moments, dim3((most + kT - 1) / kT), tile, 0, s, lv, n, (const int*)b->cid, (const int*)b->cells, b->cell_cap,
                           (const BhBox*)b->box, (const BhCell*)b->cell, (const double*)b->sx, (const double*)b->sy, (const double*)b->sm, b->M,
                           b->Sx, b->Sy, b->centre);
    }
    hipLaunchKernelGGL(k_layout_bh_walk, bodies, tile, 0, s, b->order, (const double*)b->sx, (const double*)b->sy, (const double*)b->sm, n,
                       (const BhBox*)b->box, (const BhCell*)b->cell, (const BhCentre*)b->centre, p.scaling, b->theta2, l.px, l.py,
                       counters ? b->accepted : (int*)nullptr, counters ? b->visited : (int*)nullptr);
    return hipGetLastError();
}

}  // namespace nemk

using namespace nemk;

int nemgpu_layout_bh_shape(int* depth, int* leaf)
{
    if (depth) *depth = kBhDepth;
    if (leaf) *leaf = kBhLeaf;
    return NEMGPU_OK;
}

int nemgpu_layout_create_bh(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos, double theta)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!m || !cfg) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_layout_create_bh";
    if (!std::isfinite(theta) || theta < 0.0) { set_error(who + ": theta is finite and not negative"); return NEMGPU_E_ARG; }
    if ((long long)m->n * kLevels > 0x7fffffffll) { set_error(who + ": too many families for the (level, position) index"); return NEMGPU_E_ARG; }
    return layout_create(out, m, cfg, pos, who.c_str(), &theta);
}

int nemgpu_layout_bh_tree(nemgpu_layout* l, int* n_cells, double* box, uint32_t* keys, int32_t* order, int32_t* level, int32_t* lo, int32_t* hi,
                          double* M, double* Sx, double* Sy, int32_t* accepted, int32_t* visited)
{
    if (!l) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_layout_bh_tree";
    if (!l->bh) { set_error(who + ": a layout made by nemgpu_layout_create has no tree (nemgpu_layout_create_bh makes one)"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(l->device));
    LayoutBh* b = l->bh;
    const size_t n = (size_t)l->dev.n;
    hipStream_t s = l->stream;
    hipError_t err = launch_layout_bh_repulse(l->dev, l->par, b, true, s);   // (writes the tree's arrays and px, py: every iteration rewrites them)
    int cells = 0;
    BhBox hb{};
    if (err == hipSuccess && n) err = hipMemcpyAsync(&cells, b->cells, 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && n) err = hipMemcpyAsync(&hb, b->box, sizeof(hb), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return device_status(who, err);
    if (cells > b->cell_cap) { set_error(who + ": more cells than the bound allows"); return NEMGPU_E_DEVICE; }
    const size_t nc = (size_t)cells;
    std::vector<BhCell> hc((lo || hi) ? nc : 0);
    auto back = [&](void* dst, const void* src, size_t bytes) {
        if (err == hipSuccess && dst && bytes) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    };
    back(keys, b->skey, n * 4);
    back(order, b->order, n * 4);
    back(level, b->level, nc * 4);
    back(hc.empty() ? nullptr : hc.data(), b->cell, hc.size() * sizeof(BhCell));
    back(M, b->M, nc * 8);
    back(Sx, b->Sx, nc * 8);
    back(Sy, b->Sy, nc * 8);
    back(accepted, b->accepted, n * 4);
    back(visited, b->visited, n * 4);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return device_status(who, err);
    for (size_t c = 0; c < hc.size(); c++) {
        if (lo) lo[c] = hc[c].lo;
        if (hi) hi[c] = hc[c].hi;
    }
    if (n_cells) *n_cells = cells;
    if (box) { box[0] = hb.x0; box[1] = hb.y0; box[2] = hb.side; }
    return NEMGPU_OK;
}
