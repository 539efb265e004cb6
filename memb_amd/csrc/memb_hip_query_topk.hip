// The k best columns of every row of a dense fp32 matrix, in the total order of include/memb_hip_query_topk.h, gfx950 /
// CDNA4: the selection behind memb_hip_dense_topk_device and, slice after slice of query_matrix_trained's matrix,
// memb_hip_query_topk_device.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_query_topk_launch.h) through the selectors below (hip_query_topk.h). The device code is hip_query_topk_kernels.h's;
// no other device header is needed, since the kernels see a matrix and never a model.
//   topk_select   one wavefront per (row, segment of the columns): 64 columns per load instruction, coalesced, four loads
//                 in flight; the best k so far as a sorted list with one rank per lane; a batch is tested with ONE ballot
//                 against rank k - 1 (value, then column), each survivor is broadcast and inserted by a shift of one lane.
//                 The list goes to the workspace
//   topk_merge    one wavefront per row: the row's segment lists and, when merging, the k entries the output holds, through
//                 the same insertion; stores values and base + column, -inf and -1 in the ranks nothing filled
// The result is the first k of a stable descending sort, so it depends on the matrix alone: never on the segments, the
// grid or the order candidates are offered in. No atomics, no LDS, no scratch, nothing allocated; a value travels as its
// bits, so a NaN keeps its payload and a zero its sign.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_query_topk.h"
#include "hip_query_topk.h"

namespace {

constexpr int WAVE = 64;

#include "hip_query_topk_kernels.h"

__global__ __launch_bounds__(memb_query_topk::WAVES_PER_BLOCK * WAVE) void topk_select(TopkParams p)
{
    topkSelectOfWave(p);
}

__global__ __launch_bounds__(memb_query_topk::WAVES_PER_BLOCK * WAVE) void topk_merge(TopkParams p)
{
    topkMergeOfWave(p);
}

}  // namespace

namespace memb_query_topk {

memb::KernelHandle selectKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&topk_select), "topk_select"};
}

memb::KernelHandle mergeKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&topk_merge), "topk_merge"};
}

}  // namespace memb_query_topk
