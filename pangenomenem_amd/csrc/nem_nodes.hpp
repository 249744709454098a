// nem_nodes.hpp -- the nodes' <attvalue> text of the pangenome graph's GEXF export, from the resident master, the flat
// orders of all its organisms and the (offset, length) spans of every gene's ID, NAME and PRODUCT in the load's text.
//
// PPanGGOLiN.export_to_GEXF (ppanggolin.py:1294-1362) gives every node, per organism, the "|"-joined ids of the
// family's genes in it, and the joined distinct names and products of all its genes; nx.write_gexf numbers an attribute
// where it first meets it.  gexf.node_text_host (Python) states the bytes; here, with the master on the device:
//   create   k_nodes_keys     a lane per gene: its family (n: not kept) and its organism;
//            one stable radix sort (rocPRIM) of the genes by family: a family's kept genes are one segment, grouped by
//            organism in walk order (contig_org is non-decreasing);
//            k_nodes_runs     a lane per sorted gene: the head of its (family, organism) run, whose presence bit must be
//                             set in the master; one atomicMin per run gives every organism's first family;
//            k_nodes_popcount the master's presence bits: their number must be the number of runs -- together: the cells
//                             of the orders are exactly the master's;
//   text     per batch of whole files, uploaded for the call: k_nodes_widths (a lane per (gene, span): its escaped width,
//            esc_width), an exclusive scan, k_nodes_gather (the same lane copies the span, escaped by esc_put, into the
//            batch's part of the blob).  The GFF text is freed; the blob and one (offset, length) per (gene, span) stay;
//   finish   the parts joined into one blob; per NAME and per PRODUCT an open-addressing table with linear probes keyed
//            by (family, bytes) -- a probe compares the bytes in full, so nothing relies on the hash -- in which a class
//            keeps its least sorted gene, the first of the walk: k_nodes_insert, k_nodes_emit;
//   ids      the numbering on the host from the organisms' first families (d numbers); then k_nodes_contrib: per sorted
//            gene the bytes it adds to its organism's line (the line's head where its run starts, a separator elsewhere,
//            the line's tail where the run ends), to the name line and to the product line (only a class's least gene
//            adds its value); three inclusive scans; k_nodes_sizes: per family its first run's end (one binary search) and
//            its node's bytes, full and light; their scans are the nodes' ends;
//   lines    k_nodes_pieces: a lane per sorted gene of the batch's families writes its pieces at the difference of the
//            scans; k_nodes_frames: a lane per family writes the head and the tail of its name and product lines.
// No kernel walks a node: a family of thousands of genes costs what its genes cost.  No LDS is staged.
//
// Bounds, refused on the host before any launch:
//   g <= kNodesGenesMax     3 g lanes of a batch and a table of at most 2^31 slots are counted in int;
//   a span <= kNodesSpanMax its escaped width (at most 6 times) fits an int;
//   the blob <= kNodesBlobMax bytes; offsets into it and into a batch's text are 64-bit;
//   an attribute id has at most 10 digits (an int): seg::digits_of;
//   spans lie inside the batch's text; batches arrive in gene order and cover every gene before finish;
//   a text call's rows lie inside the table and its buffer holds the batch (nem_table.hpp).
#pragma once
#include <cstdint>

namespace nemk {

constexpr int kNodesGenesMax = 0x7fffffff / 3;
constexpr int kNodesSpanMax = 1 << 24;
constexpr long long kNodesBlobMax = 1ll << 40;
constexpr int kNodesLineFixed = 39;               // a line without its id and its value: 25 + 9 + 5
constexpr int kNodesLineHead = 34;                // ... its bytes before the value, without the id

enum { kNodesOk = 0, kNodesNoFamily = 1, kNodesNoBit = 2, kNodesMissing = 4 };

}  // namespace nemk
