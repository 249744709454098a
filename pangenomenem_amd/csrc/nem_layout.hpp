// nem_layout.hpp -- the pangenome graph laid out on the device: ForceAtlas2 (Jacomy et al. 2014) with an exact all-pairs
// repulsion, strong gravity, the attraction as a gather over the master's CSR rows and the speed control on the device
// (nem_layout.hip; pangenomenem_amd/layout.py's layout_arrays is the statement).  float64 throughout; no float atomics,
// no wait of one block for another: an iteration is four plain launches in stream order.  A layout made by
// nemgpu_layout_create_bh takes step 1 from nem_layout_bh.hpp instead (a Barnes-Hut sum, one slice); steps 2 - 6 are the same
// three launches.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/nem_mi355x.h"
#include "nem_chunks.hpp"

namespace nemk {

constexpr int kLayoutTile = 256;          // a block's threads = its nodes = the j's of one LDS tile
constexpr int kLayoutSliceGrain = 64;     // no slice of the j range is shorter than this (but the last)
constexpr int kLayoutBlocksTarget = 1024; // the repulsion's blocks a small graph is cut into
constexpr int kLayoutSlicesMax = 64;

// the slices every node's j range is cut into: a function of n alone
inline int layout_slices(int n)
{
    if (n <= 0) return 1;
    const int nb = (n - 1) / kLayoutTile + 1;
    int s = (n - 1) / kLayoutSliceGrain + 1;
    const int fill = (kLayoutBlocksTarget + nb - 1) / nb;
    if (s > fill) s = fill;
    if (s > kLayoutSlicesMax) s = kLayoutSlicesMax;
    return s < 1 ? 1 : s;
}

// what the speed control carries from one iteration to the next (device memory)
struct LayoutState {
    double speed, eff, S, T;
    int moved;                            // the last iteration's T was not 0: its step 6 ran
    int pad;
};

struct LayoutDev {
    int n, nnz, slices, slice_len, blocks;
    const int* ptr;                       // [n + 1] the layout's copy of the master's CSR
    const int* idx;                       // [nnz]
    double* efac;                         // [nnz]  step 3's factor of the entry's edge (unused for a self-loop)
    double* mass;                         // [n]
    double *x, *y;                        // [n]
    double *fx, *fy;                      // [n]    this iteration's forces
    double *ox, *oy;                      // [n]    the previous iteration's
    double* sw;                           // [n]    swinging
    double *px, *py;                      // [slices][n] the repulsion per slice
    double *bs, *bt;                      // [blocks] per block of nodes: sum of mass * swinging, of mass * traction
    LayoutState* state;
};

struct LayoutParams {
    double scaling, gravity, jitter;
    double est, sqrt_est, nn;             // 0.05 sqrt(n), its root, n * n
};

// masses and edge factors from the master (only read); pow_w [d + 1]: weight ** influence for influence not 0 or 1, else null
void launch_layout_setup(const MasterDev& m, const LayoutDev& l, bool distributed, int influence_kind, const double* pow_w, hipStream_t s);
// one iteration with the exact repulsion
void launch_layout_iteration(const LayoutDev& l, const LayoutParams& p, hipStream_t s);
// steps 2 - 6 of one iteration, behind whichever step 1 filled l.px, l.py
void launch_layout_rest(const LayoutDev& l, const LayoutParams& p, hipStream_t s);

struct LayoutBh;                          // nem_layout_bh.hpp

}  // namespace nemk

// A layout on the device: its own allocation and stream; the master is read at creation only
struct nemgpu_layout {
    int device = 0;
    hipStream_t stream = nullptr;
    char* block = nullptr;
    nemk::LayoutDev dev{};
    nemk::LayoutParams par{};
    long long iterations = 0;
    nemk::LayoutBh* bh = nullptr;         // made by nemgpu_layout_create_bh: the tree's arrays, else null
};

namespace nemk {

// nemgpu_layout_create (theta null) and nemgpu_layout_create_bh (theta checked by the caller) under the name `who`
int layout_create(nemgpu_layout** out, const nemgpu_master* m, const nemgpu_layout_config* cfg, const double* pos, const char* who,
                  const double* theta);

}  // namespace nemk
