// nem_matrix.hpp -- the per-family table of the pangenome matrix and the .Rtab cell block, from the resident master.
//
// PPanGGOLiN.write_matrix (ppanggolin.py:1400-1452) walks neighbors_graph.nodes(data=True) and writes per family its
// number of organisms and genes, the min / max / mean over the SET of its genes' lengths (node["length"], :426-430) and,
// per organism, len(node[org]) (:1429).  With the master on the device and the flat orders of all its organisms that is:
//   1. per GENE its organism and master family (the projection's inverse numbering) and two keys: (family, organism)
//      and (family, length), a gene that is not kept (a repeated family) keyed behind every family;
//   2. both key arrays sorted (rocPRIM's radix sort, as the build's records are): a family's genes are one segment of
//      either, the same positions in both, found by one search per family -- its genes, its cells, its distinct lengths
//      and their sum are differences of inclusive scans (nem_scan.hpp) at the segment's ends, its min and max the
//      segment's first and last key: no per-gene atomic, a hub family of thousands of genes costs what its genes cost;
//   3. per run of equal (family, organism) -- a CELL -- its length is the copy count; the cell must have its bit in the
//      master's presence rows, and the number of cells must be the number of set bits: together every cell, both
//      directions; a gene whose family the master lacks fails the same check;
//   4. the cells of count >= 2 compacted into a CSR over the families (multi_ptr, multi_org increasing per family,
//      multi_cnt) with, per entry, the exclusive prefix of the digits it writes beyond one (multi_xpre): the sparse
//      form of the per-line scan of the cell widths.  A line of d cells is 2 d bytes + its extra digits, so a line's
//      start is an affine term + the prefix at the family's first entry.
// The .Rtab block (k_rtab): a block takes 256 families x 256 organisms.  It loads the organism-major presence words so
// that adjacent lanes read adjacent words (4 words = 32 B per organism row), transposes them through LDS into one 256-bit
// row per family, then each wave writes its 64 families' segments, one family at a time with all lanes on one line:
// a segment with no cell >= 2 is pure "digit, separator" text whose aligned 8-byte words are computed straight from the
// bits and stored whole; a segment with one is laid out in LDS at the global address's alignment (per cell its position
// from multi_xpre, its digits) and copied out in the same aligned 8-byte words.  Only a segment's first and last
// partial words are stored by bytes.  matrix.family_table_arrays / matrix.rtab_cells_host (Python) state the same.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"
#include "nem_project.hpp"

namespace nemk {

struct MatrixIn {
    GeneOrdersIn o;               // of ALL the master's organisms
    const int32_t* gene_len;      // [g] END - START, any int32 (HOST)
};

// the table on the device (owned by nem_matrix.hip's handle)
struct FamilyTableDev {
    int n = 0, d = 0, nm = 0;
    int *nb_genes = nullptr, *nb_org = nullptr, *len_min = nullptr, *len_max = nullptr, *len_distinct = nullptr;
    long long* len_sum = nullptr;
    int *multi_ptr = nullptr, *multi_org = nullptr, *multi_cnt = nullptr;
    long long* multi_xpre = nullptr;   // [nm + 1]
    long long* fam_xpre = nullptr;     // [n + 1] multi_xpre at every family's first entry
};

enum { kMatrixOk = 0, kMatrixNoFamily = 1, kMatrixNotPresent = 2, kMatrixCount = 4 };

// Fills *t (its arrays allocated with hipMalloc; the caller frees them, also after a failure).  *mismatch: kMatrixOk or
// why the orders are not this master's (then the arrays hold nothing).  The master is only read.  Waits.
hipError_t family_table(const MasterDev& m, const MatrixIn& in, FamilyTableDev* t, int* mismatch, hipStream_t s);

// the text of families row0 .. row0 + rows - 1 into text (DEVICE, `bytes` long: the batch's size exactly)
void launch_rtab(const MasterDev& m, const FamilyTableDev& t, int row0, int rows, char* text, hipStream_t s);

}  // namespace nemk
