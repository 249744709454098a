// nem_master.hpp -- the resident master pangenome's handle (nem_master.hip makes, appends to, projects from, reads back
// and destroys it; nem_engine.hip forms the chunks, the votes and the resamples from it).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "nem_chunks.hpp"

// A master pangenome on the device (nemgpu_master_create): what the chunks of PPanGGOLiN's voting loop are formed from
// (nem_chunks.hpp).  One allocation; the stream carries the formation's phase 1.
struct nemgpu_master {
    int device = 0, n = 0, d = 0, wf = 0, nw64 = 0, nnz = 0;
    int nx = 0;                                       // (edge, organism) pairs with count >= 2
    hipStream_t stream = nullptr;
    char* block = nullptr;
    nemk::MasterDev dev{};
    std::vector<int32_t> order;                       // nemgpu_master_create_orders: family i = caller id order[i] (else empty: i)
    // what nemgpu_master_append_orders must know of how the master was made
    int f_old = 0;                                    // the caller-id space (made from arrays: n)
    bool directed = false;                            // built as a DiGraph: a row's order cannot be continued
    bool bits_only = false;                           // nemgpu_master_create: its counts are not known
};

namespace nemk {

// the sections of a device block start on 256 bytes
inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// Gene orders checked on the host (no HIP call before them; nem_master.hip): the build's and the append's, or the
// projection's (d: the master's organisms), which has no contig_circular and allows no gene at all -- the family table's
// too.  NEMGPU_OK, or the status with nemgpu_last_error's text set.
int check_orders(bool projection, int d, int f, int g, int c, const int32_t* genes, const int32_t* contig_ptr, const int32_t* contig_org,
                 const uint8_t* contig_circular);

}  // namespace nemk
