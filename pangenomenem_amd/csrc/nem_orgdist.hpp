// nem_orgdist.hpp -- the organisms of a resident master clustered for the presence/absence plot: what the R script of
// PPanGGOLiN's CLI computes with `hclust(dist(t(binary_matrix), method="binary"))` (command_line.py:57, :79) and the
// raster it then draws (:84-101).
//
//   1. the DISTANCES.  For organisms i, j with family sets A, B: inter = |A & B|, uni = |A| + |B| - inter,
//      dist = (double)(uni - inter) / uni, 0 where uni == 0 (R_dist_binary with every cell above 1 counted as 1: the
//      master's presence bit).  The counts are exact integers and the distance one IEEE double division of them, so every
//      distance is a function of the bits alone.  A block takes kOrgTile x kOrgTile organisms and stages kOrgChunk 64-bit
//      words of both tiles' rows of MasterDev::xt in LDS (rows padded by one word: a wave's 16 different rows fall on 16
//      different bank pairs); a lane keeps a 4 x 4 micro-tile of int32 counts, rows lane / 16 + 16 r against rows lane %
//      16 + 16 c, and adds __popcll(a & b) per word.  Only the tiles on or above the diagonal are computed; a tile goes
//      through LDS once more and is stored twice, as it stands and transposed, both in whole rows: the result is the FULL
//      symmetric square double [d][d], which the clustering reads by rows.  d <= kOrgMax (8 d^2 bytes stay resident, the
//      same again while the merges run).
//   2. the CLUSTERING: R's hclust(method = "complete"), Murtagh's nearest-neighbour chain of hclust.f, as
//      tileplot.hclust_complete_host states it.  NN(i) = the nearest live j > i and DISNN(i), found with a strict <;
//      d - 1 times: the live i of least DISNN (lowest i on a tie), I2 = min(i, NN(i)), J2 = max, J2 retired,
//      d(I2, k) = max(d(I2, k), d(J2, k)) for the live k, NN(I2) found anew, and every live row whose NN was I2 or J2
//      searched again.  Every step compares or copies stored doubles -- no addition -- so any reduction order gives the
//      statement's bits as long as a minimum is the lexicographic (value, index) one.  One workgroup of kMergeThreads
//      lanes walks all d - 1 merges on a copy of the square (rows in HBM, NN and DISNN in HBM, the live set in LDS),
//      __syncthreads() only: no host round trip per merge and no wait between workgroups.  The rows to search again are
//      listed and the 16 waves shared among them (all on one row, one each from 16 rows up).
//   3. the RASTER: uint8 [rows][d], cell (r, c) = family fam[r] present in organism org[c], gathered from xt.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_chunks.hpp"

namespace nemk {

constexpr int kOrgTile = 64;          // organisms per side of a distance tile
constexpr int kOrgChunk = 32;         // 64-bit words of a row staged per step
constexpr int kOrgMax = 32768;        // organisms a clustering takes
constexpr int kMergeThreads = 1024;   // the merge loop's one workgroup

// pop[d] = every organism's families
void launch_org_popcount(const MasterDev& m, int* pop, hipStream_t s);
// dist[d][d], symmetric, zero diagonal
void launch_org_distances(const MasterDev& m, const int* pop, double* dist, hipStream_t s);
// the d - 1 merges on `work` (a copy of the square, changed), into i2, j2 [d - 1], height [d - 1] (DEVICE); nn [d] int,
// disnn [d] double, list [d] int: scratch.  d >= 2.
void launch_org_merges(double* work, int d, int* nn, double* disnn, int* list, int* i2, int* j2, double* height, hipStream_t s);
// out[rows][d] (DEVICE) for the families fam[0 .. rows) and the organisms org[0 .. d) (DEVICE)
void launch_org_cells(const MasterDev& m, const int* fam, const int* org, int rows, uint8_t* out, hipStream_t s);

}  // namespace nemk
