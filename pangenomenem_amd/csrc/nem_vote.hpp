// nem_vote.hpp -- the vote of PPanGGOLiN's chunk loop on the device (partition(), ppanggolin.py:1015-1105).
//
// Every sample's NCEM run votes P/S/C/U for each family it keeps (run_partitioning, ppanggolin.py:1886-1980); the votes
// are counted per family, sample after sample, and a family is validated once it has enough of them
// (validate_family, ppanggolin.py:1015-1037).  The loop stops after the sample that validates the last family of the
// pangenome.  Here the count lives on the device for one master and one organism selection:
//   cnt[n][4]   votes per family and code (P = 0, S = 1, C = 2, U = 3)
//   st[n]       VOTE_IN_PAN | VOTE_CORE | VOTE_VALIDATED | VOTE_FORCED_U
//   first[n]    the sample (counted from the first) whose vote validated the family, -1: not (yet)
// and a batch of samples is voted through a [batch][n] matrix of codes (0xFF: the family is not in that sample).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace nemk {

enum : uint8_t { VOTE_IN_PAN = 1, VOTE_CORE = 2, VOTE_VALIDATED = 4, VOTE_FORCED_U = 8 };
constexpr uint8_t kVoteNone = 0xFF;          // V[slot][f]: family f is not in that sample
constexpr int kVoteMapStride = 4;            // a sample's code map: maps[s][label], label 0..2; entry 3 is always U

// one sample of a batch, as the class-map and scatter kernels see it
struct VoteDesc {
    const uint8_t* lab;           // [n] NCEM labels of the sample's kept families (bit 7: not a label bit)
    const int* list;              // [n] kept family j -> master index
    const float* center;          // [k][dc] the run's final centres
    const float* disp;            // [k][dc] the run's final dispersions
    int n, dc, status, slot;      // kept families, organisms, run status (0: OK), row of the vote matrix
};

struct VoteState {
    int n;                        // master families
    int32_t* cnt;                 // [n][4]
    uint8_t* st;                  // [n]
    int32_t* first;               // [n]
};

// st / cnt / first for the organism selection sel[d_sel] (indices into the master's organisms)
void launch_vote_init(const VoteState& v, const uint64_t* xt, int nw64, const int* sel, int d_sel, hipStream_t s);
// maps[s][0..3] for `count` samples of k = 3 classes
void launch_vote_classmap(const VoteDesc* desc, int count, int k, uint8_t* maps, hipStream_t s);
// V[desc.slot][list[j]] = maps[s][lab[j]] for every kept family j of every sample
void launch_vote_scatter(const VoteDesc* desc, int count, int max_n, const uint8_t* maps, uint8_t* V, int n, hipStream_t s);
// the batch's `count` rows of V counted in order from the committed state: a scan that finds where (if anywhere) the last
// family validates, then a commit of exactly the rows up to there.  words[0] = families still unvalidated after the
// batch, words[1] = 1 + the last row at which a family validated (0: none); both set before the commit pass.
void launch_vote_scan(const VoteState& v, const uint8_t* V, int count, double quotient, int d_sel, int64_t base,
                      int* words, hipStream_t s);

}  // namespace nemk
