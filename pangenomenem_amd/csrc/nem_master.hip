// nem_master.hip -- the resident master pangenome's host side: made from arrays (nemgpu_master_create,
// _create_counts) or on the device from the gene orders (_create_orders, nem_orders.hpp), appended to (_append_orders),
// merged with another (_merge, nem_merge.hpp), projected from (_project, nem_project.hpp), read back (_shape, _fetch) and destroyed.  Everything refused is refused
// on the host before the first HIP call, so the refusals can be tested without a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "nem_internal.hpp"
#include "nem_master.hpp"
#include "nem_merge.hpp"
#include "nem_orders.hpp"
#include "nem_project.hpp"

using namespace nemk;

namespace {

// A master's one block: the organism-major presence rows | the CSR's row pointers | its neighbours | the edges' organism
// sets | the extras' row pointers, organisms and counts - 1.  No multi-copy pair (nx = 0): no extras at all, the bits-only
// kernels.
struct MasterLayout {
    int n, d, wf, nw64, nnz, nx;
    size_t b_xt, b_ptr, b_idx, b_eb, b_xptr, b_xorg;
    uint64_t* xt = nullptr;
    uint32_t* eb = nullptr;
    int *ptr = nullptr, *idx = nullptr, *xptr = nullptr, *xorg = nullptr, *xadd = nullptr;
    MasterLayout(int n_, int d_, int nnz_, int nx_) : n(n_), d(d_), wf((d_ + 31) / 32), nw64((n_ + 63) / 64), nnz(nnz_), nx(nx_)
    {
        b_xt = a256((size_t)d * nw64 * 8); b_ptr = a256(((size_t)n + 1) * 4); b_idx = a256((size_t)std::max(nnz, 1) * 4);
        b_eb = a256((size_t)std::max(nnz, 1) * wf * 4);
        b_xptr = nx > 0 ? a256(((size_t)nnz + 1) * 4) : 0; b_xorg = nx > 0 ? a256((size_t)nx * 4) : 0;
    }
    // m's sizes, its block and its device view; false: no device memory
    bool alloc(nemgpu_master* m)
    {
        m->n = n; m->d = d; m->wf = wf; m->nw64 = nw64; m->nnz = nnz; m->nx = nx;
        if (hipMalloc(&m->block, b_xt + b_ptr + b_idx + b_eb + b_xptr + 2 * b_xorg) != hipSuccess) return false;
        char* b = m->block;
        xt = (uint64_t*)b; ptr = (int*)(b += b_xt); idx = (int*)(b += b_ptr); eb = (uint32_t*)(b += b_idx);
        if (nx > 0) { xptr = (int*)(b += b_eb); xorg = (int*)(b += b_xptr); xadd = (int*)(b += b_xorg); }
        m->dev = MasterDev{n, d, wf, nw64, nnz, xt, ptr, idx, eb, xptr, xorg, xadd};
        return true;
    }
};

// a half-made master given up: nothing of it stays; returns rc
int master_abandon(nemgpu_master* m, OrdersBuild* build, int rc, const std::string& what)
{
    orders_free(build);
    if (m->block) (void)hipFree(m->block);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    set_error(what);
    return rc;
}

// A new master's handle with its stream, the device made current.  who: the entry point that names the device, which
// is then checked; null: another master's device (hipSetDevice's failure is worded as HIPCHK words it at either call)
int master_open(nemgpu_master** out, int device, const char* who)
{
    if (who) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no usable HIP device: this library has no CPU fallback"); return NEMGPU_E_DEVICE; }
        if (device < 0 || device >= ndev) { set_error(std::string(who) + ": bad device index"); return NEMGPU_E_ARG; }
    }
    note_hip_used();
    const hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        set_error(std::string(who ? "hipSetDevice(device)" : "hipSetDevice(old->device)") + " failed: " + hipGetErrorString(err));
        return NEMGPU_E_DEVICE;
    }
    nemgpu_master* m = new nemgpu_master();
    m->device = device;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) return master_abandon(m, nullptr, NEMGPU_E_DEVICE, "hipStreamCreate failed");
    *out = m;
    return NEMGPU_OK;
}

// the multi-copy pairs of a counts master, checked on the host (no HIP call before them: testable without a device);
// *total = extra_ptr[nnz]
int check_extras(int d, int nnz, int wf, const uint32_t* edge_bits, const int32_t* extra_ptr, const int32_t* extra_org,
                 const int32_t* extra_count, int* total)
{
    if (extra_ptr[0] != 0) { set_error("edge counts: extra_ptr[0] must be 0"); return NEMGPU_E_ARG; }
    for (int e = 0; e < nnz; e++) if (extra_ptr[e + 1] < extra_ptr[e]) { set_error("edge counts: extra_ptr not monotone"); return NEMGPU_E_ARG; }
    *total = extra_ptr[nnz];
    if (*total > 0 && (!extra_org || !extra_count)) { set_error("edge counts: extras need their organisms and counts"); return NEMGPU_E_FUNCARG; }
    const uint32_t last = (d & 31) ? (1u << (d & 31)) - 1u : ~0u;
    for (int e = 0; e < nnz; e++) {
        const uint32_t* row = edge_bits + (size_t)e * wf;
        long long sum = 0;                                    // the edge's count over all organisms
        for (int w = 0; w < wf; w++) sum += __builtin_popcount(w == wf - 1 ? row[w] & last : row[w]);
        for (int t = extra_ptr[e]; t < extra_ptr[e + 1]; t++) {
            const int o = extra_org[t];
            if (o < 0 || o >= d) { set_error("edge counts: edge " + std::to_string(e) + ": organism out of range"); return NEMGPU_E_ARG; }
            if (t > extra_ptr[e] && o <= extra_org[t - 1]) { set_error("edge counts: edge " + std::to_string(e) + ": organisms not strictly increasing"); return NEMGPU_E_ARG; }
            if (!((row[o >> 5] >> (o & 31)) & 1u)) { set_error("edge counts: edge " + std::to_string(e) + ": organism " + std::to_string(o) + " not in its edge_bits"); return NEMGPU_E_ARG; }
            if (extra_count[t] < 2) { set_error("edge counts: edge " + std::to_string(e) + ": a count below 2"); return NEMGPU_E_ARG; }
            sum += extra_count[t] - 1;
        }
        if (sum > (1ll << 24)) { set_error("edge counts: edge " + std::to_string(e) + ": total count above 2^24 (a float weight would not be exact)"); return NEMGPU_E_ARG; }
    }
    return NEMGPU_OK;
}

// The master of checked gene orders on the device: nemgpu_master_create_orders (old null), or nemgpu_master_append_orders'
// old master grown by them (in.d: the grown master's organisms)
int master_from_orders(nemgpu_master** out, const nemgpu_master* old, int device, const std::string& who, OrdersIn in)
{
    nemgpu_master* m = nullptr;
    { const int r = master_open(&m, device, old ? nullptr : who.c_str()); if (r != NEMGPU_OK) return r; }
    OrdersBuild* build = nullptr;
    auto fail = [&](int rc, const std::string& what) { return master_abandon(m, build, rc, what); };
    if (old) { in.n_old = old->n; in.order_old = old->order.empty() ? nullptr : old->order.data(); }
    int n = 0, nnz = 0, nx = 0;                               // (an append: first the update's entries and pairs)
    hipError_t err = orders_stage(in, m->stream, &build, &n, &nnz, &nx);
    if (err == hipErrorInvalidValue && n == 0 && !old) return fail(NEMGPU_E_ARG, "orders: no gene is kept (every family is repeated)");
    if (err == hipErrorInvalidValue) return fail(NEMGPU_E_ARG, "orders: too many families for this many organisms (2 bits(n) + bits(d) > 63)");
    if (err == hipSuccess && old) err = orders_append_plan(build, old->dev, m->stream, &nnz);
    if (err == hipErrorInvalidValue) return fail(NEMGPU_E_ARG, "nemgpu_master_append_orders: more than 2^31 - 1 CSR entries");
    if (err != hipSuccess) return fail(NEMGPU_E_DEVICE, who + ": " + hipGetErrorString(err));
    if (old && (long long)old->nx + nx > 0x7fffffff) return fail(NEMGPU_E_ARG, "nemgpu_master_append_orders: more than 2^31 - 1 multi-copy pairs");
    MasterLayout L(n, in.d, nnz, old ? old->nx + nx : nx);
    if (!L.alloc(m)) return fail(NEMGPU_E_DEVICE, who + ": device memory");
    m->order.resize((size_t)n);
    int over = 0;
    if (!old) err = orders_fill(build, L.xt, L.nw64, L.ptr, L.idx, L.eb, L.wf, L.xptr, L.xorg, L.xadd, m->order.data(), &over, m->stream);
    else {
        if (old->order.empty()) for (int i = 0; i < old->n; i++) m->order[(size_t)i] = i;
        else std::copy(old->order.begin(), old->order.end(), m->order.begin());
        err = orders_append_fill(build, old->dev, old->nx, nnz, L.xt, L.nw64, L.ptr, L.idx, L.eb, L.wf, L.xptr, L.xorg, L.xadd,
                                 m->order.data() + old->n, &over, m->stream);
    }
    if (err != hipSuccess) return fail(NEMGPU_E_DEVICE, who + ": " + hipGetErrorString(err));
    if (over) return fail(NEMGPU_E_ARG, "edge counts: an edge's total count above 2^24 (a float weight would not be exact)");
    orders_free(build);
    m->f_old = in.f;
    m->directed = in.directed != 0;
    *out = m;
    return NEMGPU_OK;
}

}  // namespace

// Gene orders checked on the host (no HIP call before them): the build's and the append's, or the projection's (d: the
// master's organisms), which has no contig_circular, allows no gene at all and has refused in its own words what it needs
int nemk::check_orders(bool projection, int d, int f, int g, int c, const int32_t* genes, const int32_t* contig_ptr, const int32_t* contig_org,
                 const uint8_t* contig_circular)
{
    if (!projection) {
        if (d <= 0 || f <= 0 || g <= 0 || c <= 0 || !genes || !contig_ptr || !contig_org || !contig_circular) {
            set_error("nemgpu_master_create_orders: sizes, genes and contigs are needed"); return NEMGPU_E_FUNCARG;
        }
        if ((d + 31) / 32 > chunk_mask_words_max()) { set_error("nemgpu_master_create_orders: more than 131 072 organisms"); return NEMGPU_E_ARG; }
    }
    if ((long long)g + c >= (1ll << 30)) { set_error("orders: genes + contigs must stay below 2^30"); return NEMGPU_E_ARG; }
    if (contig_ptr[0] != 0 || contig_ptr[c] != g) { set_error("orders: contig_ptr must run from 0 to the number of genes"); return NEMGPU_E_ARG; }
    for (int j = 0; j < c; j++) {
        if (contig_ptr[j + 1] < contig_ptr[j]) { set_error("orders: contig_ptr not monotone"); return NEMGPU_E_ARG; }
        if (contig_org[j] < 0 || contig_org[j] >= d) { set_error("orders: contig " + std::to_string(j) + ": organism out of range"); return NEMGPU_E_ARG; }
    }
    for (int p = 0; p < g; p++)
        if (genes[p] < 0 || genes[p] >= f) { set_error("orders: gene " + std::to_string(p) + ": family id out of range"); return NEMGPU_E_ARG; }
    return NEMGPU_OK;
}

int nemgpu_master_create(nemgpu_master** out, int device, int n, int d, const uint32_t* xbits, const int32_t* nei_ptr,
                         const int32_t* nei_idx, const uint32_t* edge_bits)
{
    return nemgpu_master_create_counts(out, device, n, d, xbits, nei_ptr, nei_idx, edge_bits, nullptr, nullptr, nullptr);
}

int nemgpu_master_create_counts(nemgpu_master** out, int device, int n, int d, const uint32_t* xbits, const int32_t* nei_ptr,
                                const int32_t* nei_idx, const uint32_t* edge_bits, const int32_t* extra_ptr, const int32_t* extra_org,
                                const int32_t* extra_count)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    if (n <= 0 || d <= 0 || !xbits || !nei_ptr) { set_error("nemgpu_master_create: sizes, bit rows and row pointers are needed"); return NEMGPU_E_FUNCARG; }
    const int wf = (d + 31) / 32;
    if (wf > chunk_mask_words_max()) { set_error("nemgpu_master_create: more than 131 072 organisms"); return NEMGPU_E_ARG; }
    const long long nnz_ll = (long long)nei_ptr[n] - nei_ptr[0];
    if (nei_ptr[0] != 0 || nnz_ll < 0 || nnz_ll > 0x7fffffff) { set_error("graph: ptr[0] must be 0 and ptr non-decreasing"); return NEMGPU_E_ARG; }
    const int nnz = (int)nnz_ll;
    for (int i = 0; i < n; i++) if (nei_ptr[i + 1] < nei_ptr[i]) { set_error("graph: ptr not monotone"); return NEMGPU_E_ARG; }
    if (nnz > 0 && (!nei_idx || !edge_bits)) { set_error("nemgpu_master_create: a graph needs neighbour indices and edge organism sets"); return NEMGPU_E_FUNCARG; }
    for (int t = 0; t < nnz; t++) if (nei_idx[t] < 0 || nei_idx[t] >= n) { set_error("graph: neighbour index out of range"); return NEMGPU_E_ARG; }
    int nx = 0;                                               // multi-copy (edge, organism) pairs
    if (extra_ptr) { const int r = check_extras(d, nnz, wf, edge_bits, extra_ptr, extra_org, extra_count, &nx); if (r != NEMGPU_OK) return r; }
    nemgpu_master* m = nullptr;
    { const int r = master_open(&m, device, "nemgpu_master_create"); if (r != NEMGPU_OK) return r; }
    uint32_t* xf_tmp = nullptr;
    auto fail = [&](const char* what) { if (xf_tmp) (void)hipFree(xf_tmp); return master_abandon(m, nullptr, NEMGPU_E_DEVICE, what); };
    MasterLayout L(n, d, nnz, nx);
    if (!L.alloc(m)) return fail("nemgpu_master_create: device memory");
    if (hipMalloc(&xf_tmp, a256((size_t)n * wf * 4)) != hipSuccess) return fail("nemgpu_master_create: device memory");
    std::vector<int32_t> xadd(extra_count ? (size_t)nx : 0);
    for (int t = 0; t < nx; t++) xadd[(size_t)t] = extra_count[t] - 1;
    // the bits above organism d - 1 in a row's last word are not data
    std::vector<uint32_t> rows(xbits, xbits + (size_t)n * wf);
    if (d & 31) { const uint32_t keep = (1u << (d & 31)) - 1u; for (int i = 0; i < n; i++) rows[(size_t)i * wf + wf - 1] &= keep; }
    hipError_t err = hipMemcpyAsync(xf_tmp, rows.data(), (size_t)n * wf * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(L.ptr, nei_ptr, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess && nnz > 0) err = hipMemcpyAsync(L.idx, nei_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess && nnz > 0) err = hipMemcpyAsync(L.eb, edge_bits, (size_t)nnz * wf * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess && nx > 0) err = hipMemcpyAsync(L.xptr, extra_ptr, ((size_t)nnz + 1) * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess && nx > 0) err = hipMemcpyAsync(L.xorg, extra_org, (size_t)nx * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess && nx > 0) err = hipMemcpyAsync(L.xadd, xadd.data(), (size_t)nx * 4, hipMemcpyHostToDevice, m->stream);
    if (err == hipSuccess) { launch_master_transpose(xf_tmp, n, wf, d, L.nw64, L.xt, m->stream); err = hipGetLastError(); }
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    if (err != hipSuccess) return fail("nemgpu_master_create: upload failed");
    (void)hipFree(xf_tmp);
    m->f_old = n;
    m->bits_only = extra_ptr == nullptr;
    *out = m;
    return NEMGPU_OK;
}

int nemgpu_master_create_orders(nemgpu_master** out, int device, int d, int f, int directed, const int32_t* genes, int g,
                                const int32_t* contig_ptr, const int32_t* contig_org, const uint8_t* contig_circular, int c,
                                const uint8_t* repeated)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    { const int r = check_orders(false, d, f, g, c, genes, contig_ptr, contig_org, contig_circular); if (r != NEMGPU_OK) return r; }
    return master_from_orders(out, nullptr, device, "nemgpu_master_create_orders",
                              OrdersIn{d, f, directed ? 1 : 0, g, c, genes, contig_ptr, contig_org, contig_circular, repeated});
}

int nemgpu_master_append_orders(nemgpu_master** out, const nemgpu_master* old, int d_new, int f, const int32_t* genes, int g,
                                const int32_t* contig_ptr, const int32_t* contig_org, const uint8_t* contig_circular, int c,
                                const uint8_t* repeated)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    // the orders first: what does not depend on the master is refused without one (testable without a device)
    const int d_old = old ? old->d : 0;
    if (d_new <= 0) { set_error("nemgpu_master_append_orders: d_new must be positive"); return NEMGPU_E_ARG; }
    const long long d_ll = (long long)d_old + d_new;
    if ((d_ll + 31) / 32 > chunk_mask_words_max()) { set_error("nemgpu_master_append_orders: more than 131 072 organisms"); return NEMGPU_E_ARG; }
    const int d = (int)d_ll;
    { const int r = check_orders(false, d, f, g, c, genes, contig_ptr, contig_org, contig_circular); if (r != NEMGPU_OK) return r; }
    for (int j = 0; j < c; j++)
        if (contig_org[j] < d_old) { set_error("orders: contig " + std::to_string(j) + ": organism out of range (a column of the old master)"); return NEMGPU_E_ARG; }
    if (!old) { set_error("nemgpu_master_append_orders: a master is needed"); return NEMGPU_E_FUNCARG; }
    if (old->directed) {
        set_error("nemgpu_master_append_orders: the master was built directed (a row's predecessor / successor order cannot be "
                  "recovered from its summed counts); rebuild it from all the orders");
        return NEMGPU_E_ARG;
    }
    if (old->bits_only) {
        set_error("nemgpu_master_append_orders: a bits-only master (nemgpu_master_create): its counts are not known");
        return NEMGPU_E_ARG;
    }
    if (f < old->f_old) { set_error("nemgpu_master_append_orders: f is below the master's " + std::to_string(old->f_old) + " family ids"); return NEMGPU_E_ARG; }
    return master_from_orders(out, old, old->device, "nemgpu_master_append_orders",
                              OrdersIn{d, f, 0, g, c, genes, contig_ptr, contig_org, contig_circular, repeated});
}

// Two masters merged on the device (nem_merge.hpp): everything that does not need the numbering or the plan is refused on
// the host before any HIP call
int nemgpu_master_merge(nemgpu_master** out, const nemgpu_master* a, const nemgpu_master* b, const int32_t* ids_b, int f)
{
    if (!out) return NEMGPU_E_FUNCARG;
    *out = nullptr;
    const std::string who = "nemgpu_master_merge";
    if (f <= 0) { set_error(who + ": f must lie above every family id"); return NEMGPU_E_ARG; }
    if (!a || !b) { set_error(who + ": two masters are needed"); return NEMGPU_E_FUNCARG; }
    for (const nemgpu_master* m : {a, b}) {
        const char* side = m == a ? "the first" : "the second";
        if (m->directed) {
            set_error(who + ": " + side + " master was built directed (a row's predecessor / successor order cannot be recovered from "
                      "its summed counts); rebuild it from all the orders");
            return NEMGPU_E_ARG;
        }
        if (m->bits_only) { set_error(who + ": " + side + " master is a bits-only master (nemgpu_master_create): its counts are not known"); return NEMGPU_E_ARG; }
    }
    if (a->device != b->device) { set_error(who + ": the masters are on different devices"); return NEMGPU_E_ARG; }
    if (f < a->f_old) { set_error(who + ": f is below the first master's " + std::to_string(a->f_old) + " family ids"); return NEMGPU_E_ARG; }
    std::vector<int32_t> ids((size_t)b->n);                   // B's ids in A's id space (ids_b null: its own numbering's)
    for (int j = 0; j < b->n; j++) ids[(size_t)j] = ids_b ? ids_b[j] : b->order.empty() ? j : b->order[(size_t)j];
    std::vector<uint8_t> seen((size_t)f, 0);
    for (int j = 0; j < b->n; j++) {
        const int id = ids[(size_t)j];
        if (id < 0 || id >= f) {
            set_error(ids_b ? who + ": ids_b[" + std::to_string(j) + "]: family id out of range" : who + ": f is not above the second master's family ids");
            return NEMGPU_E_ARG;
        }
        if (seen[(size_t)id]) { set_error(who + ": ids_b[" + std::to_string(j) + "]: family id " + std::to_string(id) + " used twice"); return NEMGPU_E_ARG; }
        seen[(size_t)id] = 1;
    }
    const long long d_ll = (long long)a->d + b->d;
    if ((d_ll + 31) / 32 > chunk_mask_words_max()) { set_error(who + ": more than 131 072 organisms"); return NEMGPU_E_ARG; }
    const int d = (int)d_ll;
    nemgpu_master* m = nullptr;
    { const int r = master_open(&m, a->device, nullptr); if (r != NEMGPU_OK) return r; }
    MergeBuild* build = nullptr;
    auto fail = [&](int rc, const std::string& what) { merge_free(build); return master_abandon(m, nullptr, rc, what); };
    int n = 0;
    std::vector<int32_t> fresh((size_t)b->n);                 // the ids of the families the first master lacks
    hipError_t err = merge_number(a->dev, a->order.empty() ? nullptr : a->order.data(), b->dev, ids.data(), f, m->stream, &build, &n, fresh.data());
    if (err != hipSuccess) return fail(NEMGPU_E_DEVICE, who + ": " + hipGetErrorString(err));
    if (!orders_key_fits(n, d)) return fail(NEMGPU_E_ARG, who + ": too many families for this many organisms (2 bits(n) + bits(d) > 63)");
    long long nnz = 0;
    if ((err = merge_plan(build, m->stream, &nnz)) != hipSuccess) return fail(NEMGPU_E_DEVICE, who + ": " + hipGetErrorString(err));
    if (nnz > 0x7fffffff) return fail(NEMGPU_E_ARG, who + ": more than 2^31 - 1 CSR entries");
    if ((long long)a->nx + b->nx > 0x7fffffff) return fail(NEMGPU_E_ARG, who + ": more than 2^31 - 1 multi-copy pairs");
    MasterLayout L(n, d, (int)nnz, a->nx + b->nx);
    if (!L.alloc(m)) return fail(NEMGPU_E_DEVICE, who + ": device memory");
    int over = 0;
    err = merge_fill(build, a->nx, b->nx, (int)nnz, L.xt, L.nw64, L.ptr, L.idx, L.eb, L.wf, L.xptr, L.xorg, L.xadd, &over, m->stream);
    if (err != hipSuccess) return fail(NEMGPU_E_DEVICE, who + ": " + hipGetErrorString(err));
    if (over) return fail(NEMGPU_E_ARG, "edge counts: an edge's total count above 2^24 (a float weight would not be exact)");
    merge_free(build);
    m->order.resize((size_t)n);
    if (a->order.empty()) for (int i = 0; i < a->n; i++) m->order[(size_t)i] = i;
    else std::copy(a->order.begin(), a->order.end(), m->order.begin());
    std::copy(fresh.begin(), fresh.begin() + (n - a->n), m->order.begin() + a->n);
    m->f_old = f;
    *out = m;
    return NEMGPU_OK;
}

// A partition projected onto the organisms (nem_project.hpp): everything refused is refused on the host, before any launch
int nemgpu_master_project(const nemgpu_master* m, const uint8_t* part, int f, const int32_t* genes, int g,
                          const int32_t* contig_ptr, const int32_t* contig_org, int c, const uint8_t* repeated,
                          int32_t* org_counts, int32_t* nei_counts, int32_t* gene_family, int32_t* gene_copies)
{
    if (!m) return NEMGPU_E_FUNCARG;
    if (!part || f <= 0 || g < 0 || c < 0 || !contig_ptr || (g > 0 && !genes) || (c > 0 && !contig_org)) {
        set_error("nemgpu_master_project: the classes, f > 0, genes and contigs are needed"); return NEMGPU_E_FUNCARG;
    }
    if (m->directed) {
        set_error("nemgpu_master_project: the master was built directed (nx.all_neighbors of a DiGraph lists a family that is both "
                  "predecessor and successor twice, its row holds it once: the neighbour counts cannot be recovered)");
        return NEMGPU_E_ARG;
    }
    for (int i = 0; i < m->n; i++)
        if (part[i] > 3) { set_error("nemgpu_master_project: family " + std::to_string(i) + ": class " + std::to_string((int)part[i]) + " (P 0, S 1, C 2, U 3)"); return NEMGPU_E_ARG; }
    { const int r = check_orders(true, m->d, f, g, c, genes, contig_ptr, contig_org, nullptr); if (r != NEMGPU_OK) return r; }
    note_hip_used();
    HIPCHK(hipSetDevice(m->device));
    const ProjectIn in{{f, g, c, genes, contig_ptr, contig_org, repeated, m->order.empty() ? nullptr : m->order.data()}, part};
    const hipError_t err = project(m->dev, in, org_counts, nei_counts, gene_family, gene_copies, m->stream);
    if (err != hipSuccess) { (void)hipGetLastError(); set_error(std::string("nemgpu_master_project: ") + hipGetErrorString(err)); return NEMGPU_E_DEVICE; }
    return NEMGPU_OK;
}

int nemgpu_master_shape(const nemgpu_master* m, int* n, int* d, int* nnz, int* n_extra)
{
    if (!m) return NEMGPU_E_FUNCARG;
    if (n) *n = m->n;
    if (d) *d = m->d;
    if (nnz) *nnz = m->nnz;
    if (n_extra) *n_extra = m->nx;
    return NEMGPU_OK;
}

int nemgpu_master_fetch(const nemgpu_master* m, uint32_t* xbits, int32_t* nei_ptr, int32_t* nei_idx, uint32_t* edge_bits,
                        int32_t* extra_ptr, int32_t* extra_org, int32_t* extra_count, int32_t* order)
{
    if (!m) return NEMGPU_E_FUNCARG;
    HIPCHK(hipSetDevice(m->device));
    const MasterDev& M = m->dev;
    uint32_t* xf = nullptr;
    if (xbits) {
        HIPCHK(hipMalloc(&xf, (size_t)m->n * m->wf * 4));
        launch_master_rows(M.xt, m->n, m->wf, m->d, m->nw64, xf, m->stream);
    }
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && xbits) err = hipMemcpyAsync(xbits, xf, (size_t)m->n * m->wf * 4, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && nei_ptr) err = hipMemcpyAsync(nei_ptr, M.nei_ptr, ((size_t)m->n + 1) * 4, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && nei_idx && m->nnz > 0) err = hipMemcpyAsync(nei_idx, M.nei_idx, (size_t)m->nnz * 4, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && edge_bits && m->nnz > 0) err = hipMemcpyAsync(edge_bits, M.edge_bits, (size_t)m->nnz * m->wf * 4, hipMemcpyDeviceToHost, m->stream);
    if (err == hipSuccess && m->nx > 0) {
        if (extra_ptr) err = hipMemcpyAsync(extra_ptr, M.extra_ptr, ((size_t)m->nnz + 1) * 4, hipMemcpyDeviceToHost, m->stream);
        if (err == hipSuccess && extra_org) err = hipMemcpyAsync(extra_org, M.extra_org, (size_t)m->nx * 4, hipMemcpyDeviceToHost, m->stream);
        if (err == hipSuccess && extra_count) err = hipMemcpyAsync(extra_count, M.extra_add, (size_t)m->nx * 4, hipMemcpyDeviceToHost, m->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(m->stream);
    if (xf) (void)hipFree(xf);
    if (err != hipSuccess) { set_error(std::string("nemgpu_master_fetch: ") + hipGetErrorString(err)); return NEMGPU_E_DEVICE; }
    if (m->nx > 0 && extra_count) for (int t = 0; t < m->nx; t++) extra_count[t] += 1;       // (the device keeps count - 1)
    if (m->nx == 0 && extra_ptr) std::fill(extra_ptr, extra_ptr + (size_t)m->nnz + 1, 0);
    if (order) { if (m->order.empty()) for (int i = 0; i < m->n; i++) order[i] = i; else std::copy(m->order.begin(), m->order.end(), order); }
    return NEMGPU_OK;
}

void nemgpu_master_destroy(nemgpu_master* m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    if (m->block) (void)hipFree(m->block);
    delete m;
}
