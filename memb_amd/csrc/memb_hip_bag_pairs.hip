// The cosine similarity of pairs of bags of rows (include/memb_hip_bag_pairs.h), fused with the pooling, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches this kernel
// (hip_bag_pairs_launch.h) through the selector below (hip_bag_pairs.h). The device code below the kernel is
// hip_bag_pairs_kernels.h's, on top of hip_pooled_kernels.h's, hip_norms_kernels.h's and hip_pairs_kernels.h's, which are
// included as they are.
//   bag_pairs_trained<HAS_SUB, FAST>   pool_trained's register form over the 2n bags of n pairs, a wavefront owning whole
//                                      pairs: per bag the sequential sum (and the mean's one division) of the lane's two
//                                      16-byte pieces, per pair pairs_trained's products and squares, three butterflies
//                                      side by side, two roots, one product, one division: at most four floats per pair,
//                                      NO row
// The contract is the composition of two ORDERS the headers spell out: the pooled row of memb_hip_pooled.h, then the
// reduction of memb_hip_pairs.h over two such rows. Every product and sum is one v_mul_f32 / v_add_f32 (mulRn, addRn), a
// lane owns its columns for the whole bag and a wavefront reduces one pair at a time, so nothing depends on launch
// geometry. Nothing is allocated, nothing but the named outputs is written, no atomics, no packed fp32 arithmetic, no
// scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_bag_pairs.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_bag_pairs.h"

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
#include "hip_bag_pairs_kernels.h"

// Seven wavefronts per SIMD, which the launch plans for (memb_bag_pairs::TRAINED_WAVES_PER_SIMD): pairs_trained's means.
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void bag_pairs_trained(
    TrainedParams p, PoolParams pool, BagPairParams pairs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    bagPairsOfWave<HAS_SUB, FAST>(p, pool, pairs, lds);
}

// Every instance, indexed [HAS_SUB][FAST]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false> and
// <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct BagPairTable {
    const void* trained[2][2] = {};

    BagPairTable()
    {
        trained[false][true] = reinterpret_cast<const void*>(&bag_pairs_trained<false, true>);
        trained[false][false] = reinterpret_cast<const void*>(&bag_pairs_trained<false, false>);
        trained[true][false] = reinterpret_cast<const void*>(&bag_pairs_trained<true, false>);
    }
};

}  // namespace

namespace memb_bag_pairs {

memb::KernelHandle trainedKernel(bool hasSub, bool fast)
{
    static const BagPairTable table;
    return memb::KernelHandle{table.trained[hasSub][fast], "bag_pairs_trained"};
}

}  // namespace memb_bag_pairs
