// nem_layout_bh.hpp -- the layout's repulsion as a Barnes-Hut sum (nem_layout_bh.hip; pangenomenem_amd/layout_bh.py's
// tree_arrays and walk are the statement, rule by rule, and the device is held to them bit for bit).  Per iteration, in
// stream order and in place of k_layout_repulse: the bodies' square (a two-level min / max), a 32-bit Morton key per body,
// rocPRIM's radix sort of (key, index), the bodies gathered in sorted order, the cells found per sorted position and
// numbered by one scan over (level, position), their extents and links, the moments level by level from the deepest up,
// and the walk: a lane per sorted body, stackless over first-child and rope links, accumulating in registers in the
// statement's order.  No float atomics, no wait of one block for another; the launches depend on kBhDepth, never on n, and
// everything is allocated once, for the statement's bound on the cells, when the layout is made.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_layout.hpp"

namespace nemk {

constexpr int kBhDepth = 16;              // the levels below the root: a key holds 2 * kBhDepth bits
constexpr int kBhLeaf = 8;                // a run of at most this many bodies is not split

// the cells a tree of n bodies can have (layout_bh.py: cell_bound)
inline long long bh_cell_bound(int n)
{
    const long long under = 4ll * (n / (kBhLeaf + 1));
    return 1 + (long long)kBhDepth * (n < under ? n : under);
}
// the most cells of one level below the root
inline int bh_level_bound(int n)
{
    const long long under = 4ll * (n / (kBhLeaf + 1));
    return (int)(n < under ? n : under);
}

struct BhBox {
    double x0, y0, side;
    int live, pad;                        // side > 0: there is a tree
};

struct BhCell { int lo, hi, child, rope; };       // the sorted bodies [lo, hi); the first child (-1: a leaf); the next cell when skipped (-1: the end)
struct BhCentre { double cx, cy, M, s2; };        // what the acceptance test and an accepted cell's term read

struct LayoutBh {
    int n = 0, box_blocks = 0;
    long long cell_cap = 0;
    double theta = 0.0, theta2 = 0.0;
    char* block = nullptr;                // every array below, and the sort's temporary storage
    size_t sort_bytes = 0;
    void* sort_tmp = nullptr;
    double* part = nullptr;               // [box_blocks][4] per block of bodies: min x, max x, min y, max y
    BhBox* box = nullptr;
    uint32_t *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;      // [n] the sort's double buffers
    double *sx = nullptr, *sy = nullptr, *sm = nullptr;                       // [n] the bodies in sorted order
    int *flag = nullptr, *cid = nullptr;  // [kBhDepth + 1][n] a cell starts at (level, sorted position); the cells before it
    int *scan_partial = nullptr, *cells = nullptr;
    BhCell* cell = nullptr;               // [cell_cap]
    BhCentre* centre = nullptr;
    int* level = nullptr;
    double *M = nullptr, *Sx = nullptr, *Sy = nullptr;
    int *accepted = nullptr, *visited = nullptr;                              // [n] the walk's counters, written for _bh_tree only
    const uint32_t* skey = nullptr;       // the halves of the double buffers that hold the last sort's result
    const uint32_t* order = nullptr;
};

// everything above for n bodies (the stream is only used to clear the block); *out is null on failure
hipError_t layout_bh_create(LayoutBh** out, int n, double theta, hipStream_t s);
void layout_bh_free(LayoutBh* b);
// step 1 of an iteration: the tree of l's positions and the walk into l.px, l.py [0][body]; counters: the walk also
// writes b->accepted, b->visited
hipError_t launch_layout_bh_repulse(const LayoutDev& l, const LayoutParams& p, LayoutBh* b, bool counters, hipStream_t s);

}  // namespace nemk
