// nem_gff.hpp -- the organisms' GFF files and the families table on the device (PPanGGOLiN("file", ...):
// __initialize_from_files and __load_gff, ppanggolin.py:180-315).  loader.py states the same in plain Python
// (_batch_host, families_table_host) and does the small remainder on the host; include/nem_mi355x.h has the entry points.
//
// A batch is the bytes of whole files joined by one '\n', with every file's [start, end).  Its lines are marked by a
// byte kernel (kGffTile bytes a block, 16 a thread), every other step has a thread per line, per CDS or per token:
//   lines      a line starts at byte 0 and after "\n", after "\r\n" and after a lone "\r"; a line that starts at or
//              after its file's end (the joint) is none
//   ##FASTA    the first such line of a file ends it (a minimum per file)
//   parse      tab-split up to nine fields and strip them; field 3 "CDS" makes a gene: START and END as int32, the
//              attributes' ID, NAME, GENE and PRODUCT (keys upper-cased, the last of a key wins), the ID looked up in
//              the families table; the first thing wrong with a line is its error code
//   contigs    a file's contig names dense by first appearance: a table keyed by (file, name bytes) keeps the least gene
//   duplicates a table keyed by (file, ID bytes) the same way: a gene that is not its ID's least one is refused
//   sort       one stable radix sort of the genes by (contig, START), whatever the contigs' sizes
//   error      the least (file, line, code), packed into 64 bits
// The tables are open addressing with linear probes over a 64-bit hash of the bytes; a probe compares the bytes in full,
// so nothing relies on the hash (hash_bits > 0 keeps only that many of its bits: tests make every probe collide).
#pragma once
#include <cstdint>

namespace nemk {

constexpr int kGffThreads = 256;
constexpr int kGffBytes = 16;                              // bytes of text a thread marks
constexpr int kGffTile = kGffThreads * kGffBytes;          // bytes a block marks
constexpr int kGffSpans = 5;                               // ID, NAME, PRODUCT, strand, contig name
constexpr int kGffStages = 6;                              // upload, lines, parse, contigs and IDs, sort, gather and download
constexpr unsigned long long kGffNoError = ~0ull;

enum GffError { kGffFields3 = 1, kGffFields9, kGffAttr, kGffNoId, kGffUnknown, kGffStart, kGffEnd, kGffDup };

}  // namespace nemk
