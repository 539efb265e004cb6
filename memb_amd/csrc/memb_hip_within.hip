// The candidates that precede a mark, listed (gensim's closer_than as words, a radius search), gfx950 / CDNA4
// (include/memb_hip_within.h): the columns of every row of a dense fp32 matrix that precede the row's mark in the
// selection's total order, the columns the row's list of non-candidates names left out, as positions (and values) in CSR
// form, ascending within a row -- an ordered stream compaction.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_within_launch.h) through the selectors below (hip_within.h). The key is hip_query_topk_kernels.h's and the
// predicate hip_ranks_kernels.h's.
//   within_count    a block of 256 threads inside one row over a run of 2048 columns: the row's non-candidates inside the
//                   run packed into LDS by the first wavefront (usually none), eight coalesced loads per thread issued
//                   back to back, a ballot and a population count per load, one total stored to the workspace
//   within_starts   one wavefront per row: an exclusive scan of the row's totals, 64 at a time with a carry, into each
//                   block's absolute int64 start; the row's cursor is stored, or grows
//   within_write    within_count's block again: the same loads and predicate, the 32 (step, wavefront) counts through LDS
//                   and scanned by every wavefront, destination = start + parts before + listed lanes below; stores the
//                   int64 position and the value's bits inside the row's segment only
// Bound by reading 4 bytes per (row, column), twice. No atomics, no scratch, nothing allocated; every entry's place depends
// on the inputs alone.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_within.h"
#include "hip_within.h"

namespace {

constexpr int WAVE = 64;

#include "hip_query_topk_kernels.h"
#include "hip_ranks_kernels.h"
#include "hip_within_kernels.h"

__global__ __launch_bounds__(memb_ranks::COUNT_THREADS) void within_count(WithinParams p)
{
    __shared__ WithinNamed named;
    __shared__ uint32_t waveCounts[WITHIN_WAVES];
    withinCountOfBlock(p, &named, waveCounts);
}

__global__ __launch_bounds__(memb_within::STARTS_WAVES * WAVE) void within_starts(WithinParams p)
{
    withinStartsOfWave(p);
}

__global__ __launch_bounds__(memb_ranks::COUNT_THREADS) void within_write(WithinParams p)
{
    __shared__ WithinNamed named;
    __shared__ uint32_t partCounts[WITHIN_PARTS];
    withinWriteOfBlock(p, &named, partCounts);
}

}  // namespace

namespace memb_within {

memb::KernelHandle countKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&within_count), "within_count"};
}

memb::KernelHandle startsKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&within_starts), "within_starts"};
}

memb::KernelHandle writeKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&within_write), "within_write"};
}

}  // namespace memb_within
