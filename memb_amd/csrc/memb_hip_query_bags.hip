// The cosine similarity of every query vector against every pooled bag of rows (include/memb_hip_query_bags.h), fused with
// the pooling, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches this kernel
// (hip_query_bags_launch.h) through the selector below (hip_query_bags.h). The device code below the kernel is
// hip_query_bags_kernels.h's, on top of hip_pooled_kernels.h's, hip_norms_kernels.h's, hip_pairs_kernels.h's,
// hip_queries_kernels.h's and hip_query_matrix_kernels.h's, which are included as they are.
//   query_bags_trained<HAS_SUB, FAST>   bag_pairs_trained's pooling -- per bag the sequential sum (and the mean's one
//                                       division) of the lane's two 16-byte pieces -- with query_matrix_trained's scoring
//                                       where a pair would be finished: BAG_GROUP finished rows wait in registers, their
//                                       bb and roots once per bag, then a block of QUERY_BLOCK queries at a time, per
//                                       (query, bag) the products of the lane's two pieces and ONE butterfly; the product
//                                       of the norms and the division once per result, in the lane that stores it. NO
//                                       pooled row and no decoded row is stored
// The contract is the composition of two ORDERS the headers spell out: the pooled row of memb_hip_pooled.h, then the
// reduction of memb_hip_pairs.h over (query, pooled row). Every product and sum is one v_mul_f32 / v_add_f32 (mulRn,
// addRn) in the contract's tree, a lane owns its columns for the whole bag, so nothing depends on launch geometry or on how
// queries and bags are blocked. No matrix instructions: their summation order is not the contract's. Nothing is
// allocated, nothing but the named outputs is written, no atomics, no packed fp32 arithmetic, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_query_bags.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_query_bags.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

#include "hip_pooled_kernels.h"
#include "hip_norms_kernels.h"
#include "hip_pairs_kernels.h"
#include "hip_queries_kernels.h"
#include "hip_query_matrix_kernels.h"
#include "hip_query_bags_kernels.h"

// The wavefronts per SIMD the launch plans for (memb_query_bags::TRAINED_WAVES_PER_SIMD).
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(5))) void query_bags_trained(
    TrainedParams p, PoolParams pool, QueryMatrixParams queries)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    queryBagsOfWave<HAS_SUB, FAST>(p, pool, queries, lds);
}

// Every instance, indexed [HAS_SUB][FAST]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and
// <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct QueryBagsTable {
    const void* trained[2][2] = {};

    QueryBagsTable()
    {
        trained[false][true] = reinterpret_cast<const void*>(&query_bags_trained<false, true>);
        trained[false][false] = reinterpret_cast<const void*>(&query_bags_trained<false, false>);
        trained[true][false] = reinterpret_cast<const void*>(&query_bags_trained<true, false>);
    }
};

}  // namespace

namespace memb_query_bags {

memb::KernelHandle trainedKernel(bool hasSub, bool fast)
{
    static const QueryBagsTable table;
    return memb::KernelHandle{table.trained[hasSub][fast], "query_bags_trained"};
}

}  // namespace memb_query_bags
