// nem_orders.hpp -- a master pangenome built on the device from the organisms' gene orders.
//
// PPanGGOLiN makes its neighbours graph by walking every organism's contigs gene by gene (`__neighborhood_computation`,
// ppanggolin.py:463-530): a gene of a repeated family does not exist (:485-488, :505); every other gene is an occurrence
// of its family's node in its organism (`__add_gene`, :414) and, unless it is the first kept gene of its contig, one
// link (its family, the previous kept gene's family, organism) (:513); a circular contig adds the link (first kept
// family, last kept family, organism) (:518-519); `__add_link` (:432-459) counts the links per (edge, organism).  What
// a master (nem_chunks.hpp) holds of that graph is a function of the flat gene orders alone:
//   genes[g]            family id (< f) of every gene in walk order: organisms, their contigs, their genes
//   contig_ptr[c + 1]   the genes of contig j are genes[contig_ptr[j] .. contig_ptr[j + 1])
//   contig_org[c]       the contig's organism (the master's column, < d);  contig_circular[c]: 0 / 1
//   repeated[f]         0 / 1 per family id, or null
// The build, all integer and exact:
//   1. kept flags; an inclusive max-scan of (kept ? position : -1) gives every gene its previous kept gene, which is in
//      the same contig iff it lies at or after the contig's start;
//   2. first kept position per family id (atomicMin), sorted: the graph's node order, hence the master's numbering;
//   3. per kept gene at most one link with a TIME (a gene link: position + contig index; a circular link: the contig's
//      end + contig index -- after its last gene, before the next contig's first), written as two half-edge records
//      (row, neighbour, organism | time): an undirected link (a, b) as (a, b) and (b, a) (once when a = b), a directed
//      link a -> b as the successor record (a, b) and the predecessor record (b, a), the successor's time with bit 31
//      set;
//   4. the records sorted by (row, neighbour, organism); run lengths = the counts (a directed pair's sens + antisens, a
//      directed self-loop twice); the minimum of an edge's times = when `add_edge` first saw it, a predecessor's before
//      any successor's: `nx.all_neighbors` order;
//   5. the edges sorted by (row, that minimum) = the CSR; the organisms of every edge OR-ed into its bit row, the
//      (edge, organism) pairs with count >= 2 listed behind it; the presence bits OR-ed into the organism-major rows.
// The radix sorts are rocPRIM's; the rest is here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"

namespace nemk {

struct OrdersIn {                 // HOST arrays, checked by the caller
    int d, f, directed, g, c;
    const int32_t* genes;
    const int32_t* contig_ptr;
    const int32_t* contig_org;
    const uint8_t* contig_circular;
    const uint8_t* repeated;      // or null
    // an append (n_old > 0): the families the old master has keep their numbers, order_old[i] = the caller id of family
    // i (null: i); d is then the grown master's organisms, contig_org its columns
    int n_old = 0;
    const int32_t* order_old = nullptr;
};

struct OrdersBuild;               // the device buffers between the two stages

// bits of the sort key: 2 * bits(n - 1) + bits(d - 1) may not exceed 63
bool orders_key_fits(int n, int d);
// stage 1: numbering, records, sorts, run lengths.  *n families, *nnz CSR entries, *nx pairs with count >= 2.
// Returns hipSuccess, or hipErrorInvalidValue with *n = 0 (no kept gene) / *n > 0 (the key does not fit).  Waits.
hipError_t orders_stage(const OrdersIn& in, hipStream_t s, OrdersBuild** out, int* n, int* nnz, int* nx);
// stage 2: the master's arrays (device; extra_* null when nx = 0) and the numbering order_host[n] (family i = caller
// id order_host[i]).  *over: some edge's total count exceeds 2^24.  Waits.
hipError_t orders_fill(OrdersBuild* b, uint64_t* xt, int nw64, int* ptr, int* idx, uint32_t* edge_bits, int wf, int* extra_ptr,
                       int* extra_org, int* extra_add, int32_t* order_host, int* over, hipStream_t s);
void orders_free(OrdersBuild* b);

// An append: a new master = an old one (undirected, its counts known) + the gene orders of new organisms alone, whose
// columns lie behind the old ones.  orders_stage (n_old > 0) makes the update's records, runs and edges in the GROWN
// numbering: an id the old master has keeps its number, the others with a kept gene follow in order of first kept gene.
//   * every edge of the update is looked up in its old row (a walk); the edges not found are ranked per row by first
//     time (the scan of their flags in (row, first time) order): a row = its old entries, then these;
//   * ptr = the scan of old degree + new edges; old idx / edge_bits / extras scattered to their places, the old bit rows
//     and presence rows re-strided; the update's organisms OR-ed in, its pairs with count >= 2 behind the entry's old
//     extras (every new column is larger than every old one); old + new count bounded by 2^24.
// orders_append_plan: *nnz_new = the grown master's CSR entries (its extras: nx_old + orders_stage's *nx).  Waits.
hipError_t orders_append_plan(OrdersBuild* b, const MasterDev& old, hipStream_t s, int* nnz_new);
// the grown master's arrays (device; extra_* null when it has no extras); order_host: room for the new families' caller
// ids (n - old.n).  Waits.
hipError_t orders_append_fill(OrdersBuild* b, const MasterDev& old, int nx_old, int nnz, uint64_t* xt, int nw64, int* ptr, int* idx,
                              uint32_t* edge_bits, int wf, int* extra_ptr, int* extra_org, int* extra_add, int32_t* order_host, int* over,
                              hipStream_t s);

// organism-major bit rows [d][nw64] -> family-major bit rows [n][wf] (launch_master_transpose's inverse)
void launch_master_rows(const uint64_t* xt, int n, int wf, int d, int nw64, uint32_t* xf, hipStream_t s);

}  // namespace nemk
