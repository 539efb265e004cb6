// The cosine similarity of every query vector against every row of ONE shared candidate list (include/memb_hip_query_matrix.h),
// fused with the decode, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches this kernel
// (hip_query_matrix_launch.h) through the selector below (hip_query_matrix.h). The device code below the kernel is
// hip_query_matrix_kernels.h's, on top of hip_pooled_kernels.h's, hip_norms_kernels.h's, hip_pairs_kernels.h's and
// hip_queries_kernels.h's, which are included as they are.
//   query_matrix_trained<HAS_SUB, FAST>   query_trained's walk over a list every query shares: a tile is decoded ONCE and
//                                         scored against all queries, a block of QUERY_BLOCK queries in registers at a
//                                         time. bb and its root once per candidate, aa and its root once per query and
//                                         wavefront, per (query, candidate) the products of the lane's two 16-byte pieces
//                                         and ONE butterfly, the block's side by side; the product of the norms and the division
//                                         once per result, in the lane that stores it. One query alone: the
//                                         word's dot and its bb as the two sums of one block. NO row is stored
// The contract is memb_hip_queries.h's for one group of all n rows per query, word for word. Every product and sum is one
// v_mul_f32 / v_add_f32 (mulRn, addRn) in the contract's tree, so nothing depends on launch geometry or on how the queries
// are blocked. No matrix instructions: their summation order is not the contract's. Nothing is allocated, nothing but the
// named outputs is written, no atomics, no packed fp32 arithmetic, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_query_matrix.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_pooled.h"
#include "hip_query_matrix.h"

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

// The wavefronts per SIMD the launch plans for (memb_query_matrix::TRAINED_WAVES_PER_SIMD): query_trained's means.
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void query_matrix_trained(TrainedParams p, QueryMatrixParams queries)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    queryMatrixOfWave<HAS_SUB, FAST>(p, queries, lds);
}

// Every instance, indexed [HAS_SUB][FAST]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and
// <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct QueryMatrixTable {
    const void* trained[2][2] = {};

    QueryMatrixTable()
    {
        trained[false][true] = reinterpret_cast<const void*>(&query_matrix_trained<false, true>);
        trained[false][false] = reinterpret_cast<const void*>(&query_matrix_trained<false, false>);
        trained[true][false] = reinterpret_cast<const void*>(&query_matrix_trained<true, false>);
    }
};

}  // namespace

namespace memb_query_matrix {

memb::KernelHandle trainedKernel(bool hasSub, bool fast)
{
    static const QueryMatrixTable table;
    return memb::KernelHandle{table.trained[hasSub][fast], "query_matrix_trained"};
}

}  // namespace memb_query_matrix
