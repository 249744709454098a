// nem_merge.hpp -- two resident masters merged on the device: PPanGGOLiN's `+=` (`__iadd__`, ppanggolin.py:368-391).
//
// The reference throws its graph away and walks every annotation of both pangenomes again.  What a master (nem_chunks.hpp)
// holds is enough: the union of two undirected masters A and B with known counts, as nx.Graph would hold it had B's
// organisms been walked after A's, is a function of the two masters and of B's family ids in A's id space alone
// (chunks.master_arrays_merge states it in numpy):
//   organisms  A's columns 0 .. d_a - 1, then B's as d_a .. d_a + d_b - 1;
//   families   A's keep their numbers; B's whose id A lacks are numbered n_a, n_a + 1, ... in B's order;
//   rows       an entry of A keeps its place; an entry of B that A lacks goes behind its row's A entries in the order B's
//              row lists them (B's CSR is in nx.all_neighbors order already: no sort);
//   per entry  edge_bits = A's words (the bits above organism d_a - 1 dropped) OR B's bits shifted up by d_a bits; the
//              extras A's, then B's with organism + d_a; no count is added within a pair (the column ranges are
//              disjoint), an entry's total count may not pass 2^24;
//   presence   A's organism rows re-strided, B's with their family bits permuted by the map.
// All integer; every output item is written by one thread from what it gathers: the result does not depend on the order
// of execution.  The scans are nem_scan.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"

namespace nemk {

struct MergeBuild;                // the device buffers between the stages

// the numbering: A's numbers scattered into an id table of f entries (order_a: HOST, family i of A = id order_a[i]; null:
// i), B's ids (ids_b: HOST [b.n], distinct, in [0, f): the caller has checked) looked up in it, the scan of the "new"
// flags = B's map.  *n: the merged master's families; new_ids (HOST, room for b.n): the ids of families n_a .. *n - 1.
// Waits.
hipError_t merge_number(const MasterDev& a, const int32_t* order_a, const MasterDev& b, const int32_t* ids_b, int f, hipStream_t s,
                        MergeBuild** out, int* n, int32_t* new_ids);
// the plan: every entry of B mapped and looked up in A's row (a walk); *nnz = A's entries + B's that A lacks.  Waits.
hipError_t merge_plan(MergeBuild* m, hipStream_t s, long long* nnz);
// the merged master's arrays (device; extra_* null when neither master has extras; nnz: merge_plan's, nw64 and wf: the
// merged strides).  *over: some entry's count in A + its count in B exceeds 2^24.  Waits.
hipError_t merge_fill(MergeBuild* m, int nx_a, int nx_b, int nnz, uint64_t* xt, int nw64, int* ptr, int* idx, uint32_t* edge_bits, int wf,
                      int* extra_ptr, int* extra_org, int* extra_add, int* over, hipStream_t s);
void merge_free(MergeBuild* m);

}  // namespace nemk
