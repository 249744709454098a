// nem_resample.hpp -- the stats of PPanGGOLiN's evolution curve on the device (command_line.py:262-281, 591-625).
//
// `--evolution` partitions many resamples of the organisms with partition(just_stats=True) (ppanggolin.py:932-1173)
// and keeps six integers of each: the persistent / shell / cloud / undefined counts of the run's partition and the
// core_exact / accessory counts of the selection.  A resample of at most chunk_size organisms is one NCEM run on
// exactly its columns, so a batch of them is what nemgpu_solve_chunks solves; these kernels reduce every run to its
// row of stats[count][6] where it ends, and no label crosses PCIe:
//   k_resample_core    columns 4, 5 (core_exact, accessory) from the master's organism-major bits, all samples at once
//   k_resample_tally   columns 0 .. 3 (P, S, C, U) of one lock-step group, read from the engines' label buffers
//                      through the class maps of launch_vote_classmap (nem_vote.hpp)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "nem_vote.hpp"

namespace nemk {

constexpr int kResampleStats = 6;            // persistent, shell, cloud, undefined, core_exact, accessory
constexpr int kResampleCoreWave = 64;        // k_resample_core: threads per block, one 64-family word each

// stats[s][4] += core_exact, stats[s][5] += accessory of every sample s < count: sample s is the organisms
// org[off[s] .. off[s + 1]) (indices into the master's organisms).  stats must be zeroed before.
void launch_resample_core(const uint64_t* xt, int n, int nw64, const int* org, const int* off, int count, int32_t* stats,
                          hipStream_t s);
// stats[desc[b].slot][0 .. 3] = the P, S, C, U counts of the run of desc[b], its labels mapped through maps[b]
// (launch_vote_classmap), for b < count
void launch_resample_tally(const VoteDesc* desc, int count, const uint8_t* maps, int32_t* stats, hipStream_t s);

}  // namespace nemk
