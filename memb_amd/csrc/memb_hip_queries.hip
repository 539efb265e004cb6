// The cosine similarity of query vectors against groups of candidate rows (include/memb_hip_queries.h), fused with the
// decode, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches this kernel
// (hip_queries_launch.h) through the selector below (hip_queries.h). The device code below the kernel is
// hip_queries_kernels.h's, on top of hip_pooled_kernels.h's, hip_norms_kernels.h's and hip_pairs_kernels.h's, which are
// included as they are.
//   query_trained<HAS_SUB, FAST>   pairs_trained's walk split by entries, x an fp32 query that stays in eight registers
//                                  per lane while the wavefront walks that query's candidates: per candidate the products
//                                  and squares of the lane's two 16-byte pieces, three butterflies side by side, two
//                                  roots, one product, one division: at most three floats per candidate, NO row
// The contract is memb_hip_pairs.h's applied to the pair (query of the entry's group, the entry's decoded row), word for
// word. Every product and sum is one v_mul_f32 / v_add_f32 (mulRn, addRn) and a wavefront reduces one pair at a time, so
// nothing depends on launch geometry. Nothing is allocated, nothing but the named outputs is written, no atomics, no
// packed fp32 arithmetic, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_queries.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_pooled.h"
#include "hip_queries.h"

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

// Seven wavefronts per SIMD, which the launch plans for (memb_queries::TRAINED_WAVES_PER_SIMD): pairs_trained's means.
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void query_trained(TrainedParams p, QueryParams queries)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    queriesOfWave<HAS_SUB, FAST>(p, queries, lds);
}

// Every instance, indexed [HAS_SUB][FAST]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and
// <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct QueryTable {
    const void* trained[2][2] = {};

    QueryTable()
    {
        trained[false][true] = reinterpret_cast<const void*>(&query_trained<false, true>);
        trained[false][false] = reinterpret_cast<const void*>(&query_trained<false, false>);
        trained[true][false] = reinterpret_cast<const void*>(&query_trained<true, false>);
    }
};

}  // namespace

namespace memb_queries {

memb::KernelHandle trainedKernel(bool hasSub, bool fast)
{
    static const QueryTable table;
    return memb::KernelHandle{table.trained[hasSub][fast], "query_trained"};
}

}  // namespace memb_queries
