// What an analogy query (king - man + woman) needs beyond the selection of memb_hip_query_topk.hip, gfx950 / CDNA4
// (include/memb_hip_analogies.h): a selection that knows which positions of a row are no candidates, and the sum of
// weighted rows in a fixed order that builds the query.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_analogies_launch.h) through the selectors below (hip_analogies.h). The insertion is hip_query_topk_kernels.h's.
//   topk_select_excluding   topk_select with the row's exclusion list in one register, entry e in lane e as a column of
//                           the launch. A survivor of the batch's ballot is compared with the list by one more ballot when
//                           it is broadcast; a hit is not inserted. The lists it writes hold no excluded column, so
//                           topk_merge of memb_hip_query_topk.hip runs behind it unchanged
//   weighted_rows_sum       one thread per output element walks its bag of rows of a dense fp32 matrix in entry order:
//                           out = out + (weight * value), each rounded to float32, from +0.0
// No atomics, no LDS, no scratch, nothing allocated; every result depends on the inputs alone.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_analogies.h"
#include "hip_analogies.h"

namespace {

constexpr int WAVE = 64;

#include "hip_query_topk_kernels.h"
#include "hip_analogies_kernels.h"

__global__ __launch_bounds__(memb_query_topk::WAVES_PER_BLOCK * WAVE) void topk_select_excluding(TopkParams p, ExcludedList e)
{
    topkSelectExcludingOfWave(p, e);
}

__global__ __launch_bounds__(memb_analogies::SUM_THREADS) void weighted_rows_sum(WeightedSumParams p)
{
    weightedSumOfThread(p);
}

}  // namespace

namespace memb_analogies {

memb::KernelHandle selectExcludingKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&topk_select_excluding), "topk_select_excluding"};
}

memb::KernelHandle weightedRowsSumKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&weighted_rows_sum), "weighted_rows_sum"};
}

}  // namespace memb_analogies
