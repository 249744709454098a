// nem_project.hpp -- a partition projected onto the organisms, from the resident master.
//
// PPanGGOLiN.projection (ppanggolin.py:1698-1755) walks every gene of the organisms to project; a gene whose family is
// not repeated (:1719) is counted under its family's `partition`, its `partition_exact` and "pangenome" (:1720-1722)
// and gets a line with len(node[family][organism]) (:1731) and the number of the family's neighbours
// (nx.all_neighbors, :1723) that are persistent / shell / cloud (:1733-1735).  With the master on the device that is:
//   1. per CSR ENTRY its neighbour's class, reduced over the lanes of one row inside a wave (wave_segment), one integer
//      atomic per (row, class, wave): a hub's row of thousands of entries is spread over as many lanes as a row of two
//      (a lane or a wave per row would serialise it or idle on the common short rows);
//   2. per family its class and whether it is present in all d organisms (a column count over the organism-major
//      presence rows, once per family);
//   3. the orders on the device and the inverse of the master's numbering (caller id -> family, -2 where there is none):
//      upload_orders, which the family table and the edge table call too;
//   4. per GENE its contig's organism (a search of contig_ptr), its family, its class: the seven counters of its organism
//      reduced inside the wave over every run of lanes of one organism (genes arrive organism by organism; an organism
//      whose contigs are not adjacent makes several runs), one integer atomic per run and non-zero counter -- integer
//      adds, so the result does not depend on the order;
//   5. the kept genes' keys (organism, family) sorted (rocPRIM's radix sort, as the build's records are), the runs'
//      starts from the scan of their heads (nem_scan.hpp), every run's length written back to its genes' positions.
// projection.projection_arrays (Python) states the same in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"
#include "nem_scan.hpp"

namespace nemk {

// the flat gene orders every reader of the master takes (the projection, the family table, the edge table)
struct GeneOrdersIn {             // HOST arrays, checked by the caller
    int f, g, c;
    const int32_t* genes;         // [g] caller ids < f
    const int32_t* contig_ptr;    // [c + 1]
    const int32_t* contig_org;    // [c] master columns
    const uint8_t* repeated;      // [f] or null
    const int32_t* order;         // [n] master family i = caller id order[i]; null: i
};

// the same on the device, with step 3's inverse numbering
struct GeneOrdersDev {
    int *genes, *cptr, *corg, *inv;   // inv[f]: the master family of every caller id, -2 where there is none
    uint8_t* rep;                     // [f] or null
};

// allocates them in mem, copies the orders up and fills inv (n: the master's families); g > 0
hipError_t upload_orders(seg::Scratch& mem, const GeneOrdersIn& in, int n, hipStream_t s, GeneOrdersDev* out);

struct ProjectIn {
    GeneOrdersIn o;
    const uint8_t* part;          // [n] classes 0 .. 3 (HOST)
};

constexpr int kProjectCounters = 7;   // persistent, shell, cloud, undefined, core_exact, accessory, pangenome

// HOST outputs, any may be null: org_counts[d][7], nei_counts[n][3], gene_family[g], gene_copies[g].  The master is only
// read.  Scratch is allocated for the call and freed.  Waits.
hipError_t project(const MasterDev& m, const ProjectIn& in, int32_t* org_counts, int32_t* nei_counts, int32_t* gene_family,
                   int32_t* gene_copies, hipStream_t s);

}  // namespace nemk
