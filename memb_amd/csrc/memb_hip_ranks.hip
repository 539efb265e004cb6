// The rank of a given candidate per row (gensim's rank and closer_than as a count), gfx950 / CDNA4
// (include/memb_hip_ranks.h): how many columns of every row of a dense fp32 matrix precede the row's mark in the
// selection's total order, the columns the row's list of non-candidates names left out.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_ranks_launch.h) through the selectors below (hip_ranks.h). The key is hip_query_topk_kernels.h's.
//   rank_count   a block of 256 threads inside one row counts a run of 2048 columns: eight coalesced loads per thread
//                issued back to back, the key from integer operations, a ballot and a population count per load, the four
//                wavefronts through LDS, one partial count stored to the workspace
//   rank_fold    one wavefront per row: lane e tests entry e of the row's list of non-candidates (inside the launch, first
//                of its value) and a ballot says how many rank_count counted of them; the lanes add the row's partials;
//                the count is stored, or added to what is there
// Bound by reading 4 bytes per (row, column). No atomics, no scratch, nothing allocated; every count depends on the inputs
// alone.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_ranks.h"
#include "hip_ranks.h"

namespace {

constexpr int WAVE = 64;

#include "hip_query_topk_kernels.h"
#include "hip_ranks_kernels.h"

__global__ __launch_bounds__(memb_ranks::COUNT_THREADS) void rank_count(RankParams p)
{
    __shared__ uint32_t waveCounts[memb_ranks::COUNT_THREADS / WAVE];
    rankCountOfBlock(p, waveCounts);
}

__global__ __launch_bounds__(memb_ranks::FOLD_WAVES * WAVE) void rank_fold(RankParams p)
{
    rankFoldOfWave(p);
}

}  // namespace

namespace memb_ranks {

memb::KernelHandle countKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&rank_count), "rank_count"};
}

memb::KernelHandle foldKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&rank_fold), "rank_fold"};
}

}  // namespace memb_ranks
