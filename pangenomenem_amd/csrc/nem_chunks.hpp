// nem_chunks.hpp -- device-side formation of the NEM problems of PPanGGOLiN's chunk voting loop.
//
// The reference solves a pangenome of more than 500 organisms as many NEM problems, each on a random sample of the
// organisms (`partition()`, ppanggolin.py:995-1097: `orgs = sample(organisms, chunck_size)`), and writes every sample's
// five input files from ONE graph (`__write_nem_input_files`, ppanggolin.py:821-930):
//   * the columns of the presence/absence matrix are the sampled organisms, in sample order (:850);
//   * a family with no sampled organism is dropped, the others are numbered in the master's order (:849-852);
//   * an edge's weight is its `coverage` (:866-878): the sum over the sampled organisms of the adjacency's occurrence
//     count in that organism (`graph[a][b][org]`, which __add_link increments, :451), sens + antisens when the graph is
//     directed; an edge with coverage 0 is dropped, the neighbours of a family keep the master's order.
// Here the master lives on the device (organism-major bit rows, the graph in CSR, per directed edge the bit set of the
// organisms that carry it, count >= 1, and sparse extras for the (edge, organism) pairs whose count is 2 or more) and a
// problem is FORMED there: no matrix, no graph crosses PCIe per chunk.  The coverage of edge e in a sample is
// popc(edge_bits[e] & mask) + sum over e's extras in the sample of (count - 1); a master without extras (every count 1)
// is the bits alone.
//
// A plan may also carry a SELECTION of the master's families and an edge rule: the sub-problem of
// `__write_nem_input_files(..., filter_by_partition="shell")` (ppanggolin.py:844 and :859, what partition_shell solves).
// A family is then kept iff it is selected and present in a sampled organism; the numbering stays the master's order.
//   * kEdgeInduced: an edge is kept iff its coverage is positive and both ends are kept (the induced subgraph, the
//     writer's evident intent);
//   * kEdgeReference: the writer as written.  Its test at :859 is inverted -- a neighbour that IS selected is skipped --
//     so no edge is ever kept, and a neighbour of positive coverage that is NOT selected has no index (its KeyError):
//     phase 1 reports the smallest CSR entry of a kept family that has one.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nemk {

// the master on the device (pointers only; nem_master.hip owns the memory)
struct MasterDev {
    int n, d, wf, nw64, nnz;
    const uint64_t* xt;           // [d][nw64]: bit i of row o = family i present in organism o
    const int* nei_ptr;           // [n + 1]
    const int* nei_idx;           // [nnz]
    const uint32_t* edge_bits;    // [nnz][wf]: organisms that carry the directed edge (count >= 1)
    const int* extra_ptr;         // [nnz + 1] CSR over the edges of the pairs with count >= 2; null: every count is 1
    const int* extra_org;         // [extra_ptr[nnz]] their organisms, increasing per edge
    const int* extra_add;         // [extra_ptr[nnz]] count - 1
};

// per chunk, phase 1 (what decides the problem's sizes) ...
struct ChunkPlan {
    const int* organisms;         // [dc] device copy of the sample, column order
    int dc;
    uint32_t* mask;               // [wf]     the sample as a bit set of the master's organisms
    uint64_t* keep;               // [nw64]   families with at least one sampled organism
    int* list;                    // [n]      kept family j -> master index
    int* map;                     // [n]      master index -> kept number, -1: dropped
    uint32_t* cov;                // [nnz]    coverage of every directed master edge in the sample
    int* ptr;                     // [n + 1]  CSR row pointers of the chunk's graph (kept rows)
    int* counts;                  // [2]      {kept families, kept directed edges}
    const uint64_t* select = nullptr;   // [nw64] the selected families as a bit set; null: every family
    int edge_rule = 0;            // kEdgeInduced | kEdgeReference
    int* outside = nullptr;       // [1] kEdgeReference: the smallest CSR entry (kept family -> unselected family, coverage
                                  //     > 0), INT_MAX: none; null: not asked for
};
constexpr int kEdgeInduced = 0, kEdgeReference = 1;
// ... and phase 2 (the engine's own buffers, filled in place)
struct ChunkFill {
    int nc, dc, wfc, npad;        // kept families, organisms of the sample, words per bit row, families padded to 256
    uint32_t* xf;                 // [nc][wfc] family-major bit rows (the engine's staging rows)
    int* perm;                    // [npad]   lane order of the density kernels: inside every 256-family tile by popcount
    int* out_ptr; int* out_idx; float* out_w;   // the engine's graph block
};

void launch_master_transpose(const uint32_t* xf, int n, int wf, int d, int nw64, uint64_t* xt, hipStream_t s);
// phase 1 for `count` chunks: plans[] is an array in DEVICE memory
void launch_chunk_plan(const MasterDev& m, const ChunkPlan* plans_dev, int count, int max_dc, hipStream_t s);
// phase 2 for one chunk
void launch_chunk_fill(const MasterDev& m, const ChunkPlan& plan, const ChunkFill& fill, hipStream_t s);
// a selection given as one byte per family (non-zero: selected) packed to the bit set a plan takes, [nw64] words
void launch_select_pack(const uint8_t* bytes, int n, int nw64, uint64_t* bits, hipStream_t s);
int chunk_mask_words_max();

}  // namespace nemk
