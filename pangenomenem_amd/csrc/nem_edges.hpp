// nem_edges.hpp -- the per-edge table of the pangenome graph's GEXF export and the edges' organism <attvalue> text, from
// the resident master.
//
// PPanGGOLiN.export_to_GEXF (ppanggolin.py:1294-1362) walks neighbors_graph.edges(data=True) and turns every edge's SET
// of link lengths (`__add_link`'s `length`, :456-459) into avg / med / min / max, and every node's set of gene lengths
// into the same; nx.write_gexf then writes per edge one <attvalue> per organism on it.  The master holds the edges, their
// organisms and the counts, but no length.  With the master on the device and the flat orders of all its organisms:
//   1. the EDGES are the CSR entries with idx >= row, numbered by the exclusive scan of that flag: nx.Graph.edges()'s
//      order; their keys (src, dst) sorted once (rocPRIM's radix sort) are what a link finds its edge in;
//   2. per kept GENE at most one link, as the build makes them (nem_orders.hpp): the previous kept gene of its contig
//      from an inclusive max-scan, or the contig's last kept gene for the first kept gene of a circular contig; its
//      length in 64 bits; its edge by one binary search of the sorted edge keys; two keys: (edge, organism) and
//      (edge, length);
//   3. both key arrays sorted: an edge's links are one segment of either, the same positions in both, found by one search
//      per edge -- its weight, its distinct lengths and their sum are differences of inclusive scans (nem_scan.hpp) at
//      the segment's ends, its min and max the segment's first and last key, its two middle distinct lengths one search
//      each of the scan of the distinct flags: no per-link atomic, no walk of a row; a pair of families adjacent
//      thousands of times costs what its links cost;
//   4. per run of equal (edge, organism) its length is the count: the organism's bit must be set in the edge's bit row
//      and the count must be 1 + the pair's extra (a search of the edge's extras); the number of runs must be the set
//      bits of the edges' rows, the runs of 2 or more the edges' extras, the edges with a link all the edges: together
//      every (edge, organism, count), both directions;
//   5. the same segment arithmetic over (family, gene length) keys gives every family's two middle distinct lengths;
//   6. per word of 32 organisms one block walks the edges in order with an exclusive OR-scan per tile of 256: the first
//      edge that carries each organism (nx numbers an attribute where it first meets it).
// The <attvalue> text (k_att_text): one wave per edge; per 64 organisms a lane per organism, the lines' offsets from a
// wave scan of their widths, laid out in LDS at the global address's alignment and copied out in aligned 8-byte words
// (only a run's first and last partial words by bytes); a group of 64 organisms none of which is on the edge costs one
// load and one ballot.  gexf.edge_table_arrays / gexf.attvalues_host (Python) state the same.
//
// The METADATA lines (nem_edge_meta.hip; export_to_GEXF's metadata=, :1339-1354): per edge and attribute the sorted set
// of the values of the edge's organisms.  The host ranks every attribute's distinct values in sorted order, so the set
// is a bit mask over the ranks and "sorted" is "increasing bit":
//   k_meta_masks   one wave per edge; per attribute the mask is zeroed in the wave's LDS, the edge's bit row is read 64
//                  organisms at a time as k_att_text reads it and every set organism ORs one-hot(rank) into LDS (an LDS
//                  atomic; no global atomic), then the words go out to masks[rows][mask_words];
//   k_meta_sizes / k_meta_text   one wave per edge, both read those masks and take a line's width from
//                  meta_line_width; the text pass puts a line's tail at its start + width - 5, so an edge's bytes stay
//                  in [edge_end[e - 1], edge_end[e]).  A value's bytes are copied by the wave, a lane per byte, straight
//                  from the blob: nothing of a value is staged, so a value's length has no bound of its own.
// Bounds (refused on the host before any launch): an attribute has 1 .. kMetaValuesMax distinct values -- its mask is
// kMetaValuesMax / 32 words = 8 KiB of LDS per wave, 32 KiB per block of 4 waves; the blob's bytes plus the number of
// values is at most kMetaTextMax, so a line's width fits an int.  gexf.edge_metadata_arrays / gexf.metavalues_host
// (Python) state the same.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"
#include "nem_project.hpp"

namespace nemk {

struct EdgesIn {                  // HOST arrays, checked by the caller
    GeneOrdersIn o;               // of ALL the master's organisms, contig_org non-decreasing
    const int32_t* gene_start;    // [g]
    const int32_t* gene_end;      // [g]
    const int32_t* contig_size;   // [c] a circular contig's size, -1: linear
    bool bits_only;               // the master's counts are not known: only the bits are checked
};

// the table on the device (owned by nem_edges.hip's handle)
struct EdgeTableDev {
    int n = 0, d = 0, ne = 0;
    int *src = nullptr, *dst = nullptr, *entry = nullptr;     // [ne]; entry: the edge's CSR entry (its bit row, its extras)
    int *weight = nullptr, *len_min = nullptr, *len_max = nullptr, *len_distinct = nullptr, *len_mid_lo = nullptr, *len_mid_hi = nullptr;
    long long* len_sum = nullptr;
    int *fam_mid_lo = nullptr, *fam_mid_hi = nullptr;         // [n]
    int* org_first_edge = nullptr;                            // [d]
};

enum { kEdgesOk = 0, kEdgesNoFamily = 1, kEdgesNoEdge = 2, kEdgesNoBit = 4, kEdgesCount = 8, kEdgesMissing = 16, kEdgesLength = 32 };

// Fills *t (its arrays allocated with hipMalloc; the caller frees them, also after a failure).  *mismatch: kEdgesOk or
// why no table was made (then the arrays hold nothing).  The master is only read.  Waits.
hipError_t edge_table(const MasterDev& m, const EdgesIn& in, EdgeTableDev* t, int* mismatch, hipStream_t s);

// per edge row0 .. row0 + rows - 1 the bytes of its lines into sizes[rows] (DEVICE); attr_id [d] (DEVICE)
void launch_att_sizes(const MasterDev& m, const EdgeTableDev& t, const int* attr_id, int row0, int rows, long long* sizes, hipStream_t s);
// the lines themselves; ends[rows] (DEVICE): the inclusive scan of the sizes; text (DEVICE): ends[rows - 1] bytes
void launch_att_text(const MasterDev& m, const EdgeTableDev& t, const int* attr_id, int row0, int rows, const long long* ends, char* text,
                     hipStream_t s);

// ---- the metadata lines (nem_edge_meta.hip) -------------------------------------------------------------------
constexpr int kMetaValuesMax = 65536;             // distinct values of one attribute: the wave's mask in LDS
constexpr long long kMetaTextMax = 1ll << 30;     // the values' bytes + the number of values

// a table's metadata on the device (owned by nem_edges.hip's handle)
struct EdgeMetaDev {
    int n_attr = 0, mask_words = 0;               // mask_words: an edge's masks, the attributes' one after the other
    int *attr_id = nullptr, *n_values = nullptr;  // [n_attr]
    int* rank = nullptr;                          // [n_attr][d]: the organism's value as its rank among the attribute's
    int* mask_off = nullptr;                      // [n_attr + 1]: the attribute's first word in an edge's masks
    int* val_base = nullptr;                      // [n_attr]: the attribute's first value in val_ptr
    int* val_ptr = nullptr;                       // [values + 1]: a value's bytes in blob
    char* blob = nullptr;
};

// per edge row0 .. row0 + rows - 1 the present-value masks into masks[rows][mask_words] (DEVICE)
void launch_meta_masks(const MasterDev& m, const EdgeTableDev& t, const EdgeMetaDev& meta, int row0, int rows, uint32_t* masks, hipStream_t s);
// from those masks: per edge the bytes of its lines into sizes[rows] (DEVICE)
void launch_meta_sizes(const EdgeMetaDev& meta, int rows, const uint32_t* masks, long long* sizes, hipStream_t s);
// the lines themselves; ends[rows] (DEVICE): the inclusive scan of the sizes; text (DEVICE): ends[rows - 1] bytes
void launch_meta_text(const EdgeMetaDev& meta, int rows, const uint32_t* masks, const long long* ends, char* text, hipStream_t s);

}  // namespace nemk
