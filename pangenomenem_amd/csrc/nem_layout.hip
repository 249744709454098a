// nem_layout.hip -- see nem_layout.hpp.  The kernels, then the C entry points (nemgpu_layout_*): everything refused for
// its arguments alone is refused on the host before the first HIP call.
#include "nem_layout.hpp"

#include <cmath>
#include <string>
#include <vector>

#include "nem_internal.hpp"
#include "nem_layout_bh.hpp"
#include "nem_master.hpp"
#include "nem_table.hpp"

namespace nemk {

namespace {

constexpr int kInfluenceOne = 0, kInfluenceZero = 1, kInfluencePow = 2;

// ---- setup: one lane per node walks its row: the entry's weight is the popcount of its bit row --------------------
__global__ __launch_bounds__(kLayoutTile) void k_layout_setup(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                             const uint32_t* __restrict__ edge_bits, int n, int d, int wf, int distributed,
                                                             int influence_kind, const double* __restrict__ pow_w,
                                                             double* __restrict__ mass, double* __restrict__ efac)
{
    const int i = blockIdx.x * kLayoutTile + threadIdx.x;
    if (i >= n) return;
    const int a = ptr[i], b = ptr[i + 1];
    mass[i] = (double)(1 + (b - a));
    const double comp = distributed ? (double)((long long)n + ptr[n]) / (double)n : 1.0;      // mean(mass): the masses sum to n + nnz
    const uint32_t last = (d & 31) ? ((1u << (d & 31)) - 1u) : 0xffffffffu;
    for (int t = a; t < b; t++) {
        const int j = idx[t];
        int w = 0;
        for (int k = 0; k < wf; k++) w += __popc(edge_bits[(size_t)t * wf + k] & (k == wf - 1 ? last : 0xffffffffu));
        const double e = influence_kind == kInfluenceOne ? (double)w : influence_kind == kInfluenceZero ? 1.0 : pow_w[w];
        const int src = min(i, j);
        const double fac = (-comp) * e;
        efac[t] = distributed ? fac / (double)(1 + (ptr[src + 1] - ptr[src])) : fac;
    }
}

// ---- step 1: a lane owns node i; the block walks slice blockIdx.y of the j range in LDS tiles of x, y, mass ----------
__global__ __launch_bounds__(kLayoutTile) void k_layout_repulse(const double* __restrict__ x, const double* __restrict__ y,
                                                               const double* __restrict__ mass, int n, int slice_len, double scaling,
                                                               double* __restrict__ px, double* __restrict__ py)
{
    __shared__ double s_x[kLayoutTile], s_y[kLayoutTile], s_m[kLayoutTile];
    const int i = blockIdx.x * kLayoutTile + threadIdx.x;
    const int j0 = min(n, (int)blockIdx.y * slice_len), j1 = min(n, j0 + slice_len);
    const bool mine = i < n;
    const double xi = mine ? x[i] : 0.0, yi = mine ? y[i] : 0.0;
    const double smi = mine ? scaling * mass[i] : 0.0;
    double ax = 0.0, ay = 0.0;
    for (int t0 = j0; t0 < j1; t0 += kLayoutTile) {
        const int cnt = min(kLayoutTile, j1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            s_x[threadIdx.x] = x[t0 + threadIdx.x];
            s_y[threadIdx.x] = y[t0 + threadIdx.x];
            s_m[threadIdx.x] = mass[t0 + threadIdx.x];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < cnt; k++) {
            const double dx = xi - s_x[k], dy = yi - s_y[k];
            const double d2 = dx * dx + dy * dy;
            const double coef = d2 > 0.0 ? (smi * s_m[k]) / d2 : 0.0;      // j = i and a coincident pair: nothing
            ax += dx * coef;
            ay += dy * coef;
        }
    }
    if (mine) {
        px[(size_t)blockIdx.y * n + i] = ax;
        py[(size_t)blockIdx.y * n + i] = ay;
    }
}

// a block's 256 values summed in a fixed tree
__device__ inline double block_tree_sum(double* s, double v)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int half = kLayoutTile / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// ---- steps 1 (the slices in order), 2, 3 (the gather over the row), 4 (per node and per block) ----------------------
__global__ __launch_bounds__(kLayoutTile) void k_layout_forces(LayoutDev l, double gravity)
{
    __shared__ double s_red[kLayoutTile];
    const int i = blockIdx.x * kLayoutTile + threadIdx.x;
    double ms = 0.0, mt = 0.0;
    if (i < l.n) {
        double fx = 0.0, fy = 0.0;
        for (int s = 0; s < l.slices; s++) {
            fx += l.px[(size_t)s * l.n + i];
            fy += l.py[(size_t)s * l.n + i];
        }
        const double xi = l.x[i], yi = l.y[i], mi = l.mass[i];
        const double g = gravity * mi;
        fx -= g * xi;
        fy -= g * yi;
        const int a = l.ptr[i], b = l.ptr[i + 1];
        for (int t = a; t < b; t++) {
            const int j = l.idx[t];
            if (j == i) continue;
            const double fac = l.efac[t];
            fx += (xi - l.x[j]) * fac;
            fy += (yi - l.y[j]) * fac;
        }
        const double ox = l.ox[i], oy = l.oy[i];
        const double sx = ox - fx, sy = oy - fy, tx = ox + fx, ty = oy + fy;
        const double sw = sqrt(sx * sx + sy * sy), tr = sqrt(tx * tx + ty * ty);
        l.fx[i] = fx;
        l.fy[i] = fy;
        l.sw[i] = sw;
        ms = mi * sw;
        mt = mi * tr;
    }
    const double bs = block_tree_sum(s_red, ms);
    const double bt = block_tree_sum(s_red, mt);
    if (threadIdx.x == 0) {
        l.bs[blockIdx.x] = bs;
        l.bt[blockIdx.x] = bt;
    }
}

// ---- step 5: one block sums the blocks' sums (a lane its stride, then the tree), lane 0 sets the speed -----------------
__global__ __launch_bounds__(kLayoutTile) void k_layout_speed(LayoutDev l, LayoutParams p)
{
    __shared__ double s_red[kLayoutTile];
    double vs = 0.0, vt = 0.0;
    for (int b = threadIdx.x; b < l.blocks; b += kLayoutTile) {
        vs += l.bs[b];
        vt += l.bt[b];
    }
    const double S = block_tree_sum(s_red, vs);
    const double T = 0.5 * block_tree_sum(s_red, vt);
    if (threadIdx.x != 0) return;
    LayoutState st = *l.state;
    st.S = S;
    st.T = T;
    st.moved = T != 0.0;
    if (st.moved) {
        double jt = p.jitter * fmax(p.sqrt_est, fmin(10.0, p.est * T / p.nn));
        if (S / T > 2.0) {
            if (st.eff > 0.05) st.eff *= 0.5;
            jt = fmax(jt, p.jitter);
        }
        const double target = S > 0.0 ? jt * st.eff * T / S : INFINITY;
        if (S > jt * T) {
            if (st.eff > 0.05) st.eff *= 0.7;
        } else if (st.speed < 1000.0) {
            st.eff *= 1.3;
        }
        st.speed += fmin(target - st.speed, 0.5 * st.speed);
    }
    *l.state = st;
}

// ---- step 6 -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLayoutTile) void k_layout_move(LayoutDev l)
{
    const int i = blockIdx.x * kLayoutTile + threadIdx.x;
    if (i >= l.n || !l.state->moved) return;
    const double speed = l.state->speed;
    const double fx = l.fx[i], fy = l.fy[i];
    const double den = 1.0 + sqrt(speed * l.mass[i] * l.sw[i]);
    l.x[i] += fx * speed / den;
    l.y[i] += fy * speed / den;
    l.ox[i] = fx;
    l.oy[i] = fy;
}

}  // namespace

void launch_layout_setup(const MasterDev& m, const LayoutDev& l, bool distributed, int influence_kind, const double* pow_w, hipStream_t s)
{
    if (l.n <= 0) return;
    hipLaunchKernelGGL(k_layout_setup, dim3(l.blocks), dim3(kLayoutTile), 0, s, l.ptr, l.idx, m.edge_bits, l.n, m.d, m.wf, distributed ? 1 : 0,
                       influence_kind, pow_w, l.mass, l.efac);
}

void launch_layout_iteration(const LayoutDev& l, const LayoutParams& p, hipStream_t s)
{
    if (l.n <= 0) return;
    hipLaunchKernelGGL(k_layout_repulse, dim3(l.blocks, l.slices), dim3(kLayoutTile), 0, s, (const double*)l.x, (const double*)l.y,
                       (const double*)l.mass, l.n, l.slice_len, p.scaling, l.px, l.py);
    launch_layout_rest(l, p, s);
}

void launch_layout_rest(const LayoutDev& l, const LayoutParams& p, hipStream_t s)
{
    if (l.n <= 0) return;
    hipLaunchKernelGGL(k_layout_forces, dim3(l.blocks), dim3(kLayoutTile), 0, s, l, p.gravity);
    hipLaunchKernelGGL(k_layout_speed, dim3(1), dim3(kLayoutTile), 0, s, l, p);
    hipLaunchKernelGGL(k_layout_move, dim3(l.blocks), dim3(kLayoutTile), 0, s, l);
}

}  // namespace nemk

using namespace nemk;

namespace {

void layout_free(nemgpu_layout* l)
{
    if (l->bh) layout_bh_free(l->bh);
    if (l->block) (void)hipFree(l->block);
    if (l->stream) (void)hipStreamDestroy(l->stream);
    delete l;
}

template <class T>
T* carve(char* base, size_t* at, size_t count)
{
    T* p = reinterpret_cast<T*>(base + *at);
    *at += a256(count * sizeof(T));
    return p;
}

// x and y of the device as [n][2] of the host
hipError_t fetch_pairs(const nemgpu_layout* l, const double* x, const double* y, double* out)
{
    const size_t n = (size_t)l->dev.n;
    std::vector<double> hx(n), hy(n);
    hipError_t err = hipMemcpyAsync(hx.data(), x, n * 8, hipMemcpyDeviceToHost, l->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(hy.data(), y, n * 8, hipMemcpyDeviceToHost, l->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l->stream);
    if (err != hipSuccess) return err;
    for (size_t i = 0; i < n; i++) { out[2 * i] = hx[i]; out[2 * i + 1] = hy[i]; }
    return hipSuccess;
}

}  // namespace

int nemgpu_layout_slices(int n, int* tile, int* slice_grain)
{
    if (tile) *tile = kLayoutTile;
    if (slice_grain) *slice_grain = kLayoutSliceGrain;
    return layout_slices(n);
}

int nemk::layout_create(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos, const char* name,
                        const double* theta)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (!m || !cfg) return NEMGPU_E_FUNCARG;
    const std::string who = name;
    if (cfg->lin_log) { set_error(who + ": the LinLog mode is not supported"); return NEMGPU_E_ARG; }
    if (cfg->adjust_sizes) { set_error(who + ": adjust_sizes (the anti-collision forces) is not supported"); return NEMGPU_E_ARG; }
    if (!cfg->strong_gravity) { set_error(who + ": only the strong gravity mode is supported"); return NEMGPU_E_ARG; }
    if (!std::isfinite(cfg->scaling_ratio) || !std::isfinite(cfg->gravity) || !std::isfinite(cfg->edge_weight_influence) ||
        !std::isfinite(cfg->jitter_tolerance)) {
        set_error(who + ": a parameter is not finite"); return NEMGPU_E_ARG;
    }
    if (m->directed) {
        set_error(who + ": a master built with directed = 1 (a DiGraph's weight is per direction, the master holds the sum)"); return NEMGPU_E_ARG;
    }
    const int n = m->n, nnz = m->nnz;
    if (n > 0 && !pos) { set_error(who + ": the start positions [n][2] are needed"); return NEMGPU_E_FUNCARG; }
    for (size_t k = 0; k < (size_t)n * 2; k++)
        if (!std::isfinite(pos[k])) { set_error(who + ": a start position is not finite"); return NEMGPU_E_ARG; }
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    nemgpu_layout* l = new nemgpu_layout();
    l->device = m->device;
    LayoutDev& v = l->dev;
    v.n = n; v.nnz = nnz;
    v.slices = theta ? 1 : layout_slices(n);                  // (the walk writes one sum per body)
    v.slice_len = n > 0 ? (n + v.slices - 1) / v.slices : 1;
    v.blocks = (n + kLayoutTile - 1) / kLayoutTile;
    const double est = 0.05 * std::sqrt((double)n);
    l->par = LayoutParams{cfg->scaling_ratio, cfg->gravity, cfg->jitter_tolerance, est, std::sqrt(est), (double)n * (double)n};
    const int kind = cfg->edge_weight_influence == 1.0 ? kInfluenceOne : cfg->edge_weight_influence == 0.0 ? kInfluenceZero : kInfluencePow;
    std::vector<double> pow_w;
    if (kind == kInfluencePow)
        for (int w = 0; w <= m->d; w++) pow_w.push_back(std::pow((double)w, cfg->edge_weight_influence));
    // one block: the sections start on 256 bytes
    const size_t sn = a256((size_t)n * 8);
    const size_t bytes = a256(((size_t)n + 1) * 4) + a256((size_t)nnz * 4) + a256((size_t)nnz * 8) + 8 * sn + 2 * a256((size_t)v.slices * n * 8) +
                         2 * a256((size_t)v.blocks * 8) + a256(sizeof(LayoutState)) + a256(pow_w.size() * 8);
    hipError_t err = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking);
    if (err == hipSuccess) err = hipMalloc((void**)&l->block, bytes);
    if (err != hipSuccess) { layout_free(l); return device_status(who, err); }
    size_t at = 0;
    int* ptr = carve<int>(l->block, &at, (size_t)n + 1);
    int* idx = carve<int>(l->block, &at, nnz);
    v.ptr = ptr; v.idx = idx;
    v.efac = carve<double>(l->block, &at, nnz);
    v.mass = carve<double>(l->block, &at, n);
    v.x = carve<double>(l->block, &at, n);  v.y = carve<double>(l->block, &at, n);
    v.fx = carve<double>(l->block, &at, n); v.fy = carve<double>(l->block, &at, n);
    v.ox = carve<double>(l->block, &at, n); v.oy = carve<double>(l->block, &at, n);
    v.sw = carve<double>(l->block, &at, n);
    v.px = carve<double>(l->block, &at, (size_t)v.slices * n);
    v.py = carve<double>(l->block, &at, (size_t)v.slices * n);
    v.bs = carve<double>(l->block, &at, v.blocks);
    v.bt = carve<double>(l->block, &at, v.blocks);
    v.state = carve<LayoutState>(l->block, &at, 1);
    double* pow_dev = carve<double>(l->block, &at, pow_w.size());
    // the master's stream first (its arrays are complete behind it), then this layout's own
    err = hipStreamSynchronize(m->stream);
    hipStream_t s = l->stream;
    if (err == hipSuccess) err = hipMemsetAsync(l->block, 0, bytes, s);
    if (err == hipSuccess && n) err = hipMemcpyAsync(ptr, m->dev.nei_ptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && nnz) err = hipMemcpyAsync(idx, m->dev.nei_idx, (size_t)nnz * 4, hipMemcpyDeviceToDevice, s);
    if (err == hipSuccess && !pow_w.empty()) err = hipMemcpyAsync(pow_dev, pow_w.data(), pow_w.size() * 8, hipMemcpyHostToDevice, s);
    std::vector<double> hx(n), hy(n);
    for (int i = 0; i < n; i++) { hx[i] = pos[2 * (size_t)i]; hy[i] = pos[2 * (size_t)i + 1]; }
    if (err == hipSuccess && n) err = hipMemcpyAsync(v.x, hx.data(), (size_t)n * 8, hipMemcpyHostToDevice, s);
    if (err == hipSuccess && n) err = hipMemcpyAsync(v.y, hy.data(), (size_t)n * 8, hipMemcpyHostToDevice, s);
    const LayoutState start{1.0, 1.0, 0.0, 0.0, 0, 0};
    if (err == hipSuccess) err = hipMemcpyAsync(v.state, &start, sizeof(start), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) {
        launch_layout_setup(m->dev, v, cfg->outbound_attraction_distribution != 0, kind, pow_w.empty() ? nullptr : pow_dev, s);
        err = hipGetLastError();
    }
    if (err == hipSuccess && theta) err = layout_bh_create(&l->bh, n, *theta, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);     // (the host vectors above go out of scope; the master may be destroyed)
    if (err != hipSuccess) { layout_free(l); return device_status(who, err); }
    *out = l;
    return NEMGPU_OK;
}

int nemgpu_layout_create(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos)
{
    return layout_create(out, m, cfg, pos, "nemgpu_layout_create", nullptr);
}

int nemgpu_layout_run(nemgpu_layout* l, int iterations)
{
    if (!l) return NEMGPU_E_FUNCARG;
    if (iterations < 0) { set_error("nemgpu_layout_run: iterations < 0"); return NEMGPU_E_ARG; }
    HIPCHK(hipSetDevice(l->device));
    hipError_t err = hipSuccess;
    for (int it = 0; it < iterations && err == hipSuccess; it++) {
        if (l->bh) {
            err = launch_layout_bh_repulse(l->dev, l->par, l->bh, false, l->stream);
            if (err == hipSuccess) launch_layout_rest(l->dev, l->par, l->stream);
        } else {
            launch_layout_iteration(l->dev, l->par, l->stream);
        }
    }
    l->iterations += iterations;
    return device_status("nemgpu_layout_run", err != hipSuccess ? err : hipGetLastError());
}

int nemgpu_layout_fetch(nemgpu_layout* l, double* pos, double* forces, double* state)
{
    if (!l) return NEMGPU_E_FUNCARG;
    const std::string who = "nemgpu_layout_fetch";
    HIPCHK(hipSetDevice(l->device));
    hipError_t err = hipSuccess;
    if (pos && l->dev.n) err = fetch_pairs(l, l->dev.x, l->dev.y, pos);
    if (err == hipSuccess && forces && l->dev.n) err = fetch_pairs(l, l->dev.fx, l->dev.fy, forces);
    LayoutState st{};
    if (err == hipSuccess) err = hipMemcpyAsync(&st, l->dev.state, sizeof(st), hipMemcpyDeviceToHost, l->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(l->stream);
    if (err != hipSuccess) return device_status(who, err);
    if (state) { state[0] = st.speed; state[1] = st.eff; state[2] = st.S; state[3] = st.T; state[4] = (double)l->iterations; }
    return NEMGPU_OK;
}

void nemgpu_layout_destroy(nemgpu_layout* l)
{
    if (!l) return;
    (void)hipSetDevice(l->device);
    if (l->stream) (void)hipStreamSynchronize(l->stream);
    layout_free(l);
}
