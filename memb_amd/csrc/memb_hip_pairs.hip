// The cosine similarity of pairs of rows (include/memb_hip_pairs.h), fused with the decode, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_pairs_launch.h) through the selectors below (hip_pairs.h). The device code below the kernels is
// hip_pairs_kernels.h's, on top of hip_norms_kernels.h's, which is included as it is.
//   pairs_trained<HAS_SUB, FAST>   norms_trained's walk over the 2n entries of n pairs, in tiles of an even number of
//                                  words: per pair the products and squares of the lane's two 16-byte pieces of both
//                                  words, three butterflies side by side, two roots, one product, one division: at most
//                                  four floats per pair, NO row
//   pairs_dense                    one wavefront per pair of fp32 rows already in memory, any dim and alignment
// The contract is an ORDER (the header spells it out), that of memb_hip_norms.h with a product of two rows where the norm
// has a square; the norms are that header's, bit for bit. Every product and sum is one v_mul_f32 / v_add_f32 (mulRn, addRn),
// and every kernel reduces one pair per wavefront at a time, so nothing depends on launch geometry. Nothing is allocated,
// nothing but the named outputs is written, no atomics, no packed fp32 arithmetic, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_pairs.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_pairs.h"

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

// Seven wavefronts per SIMD, which the launch plans for (ONE_TILE_WAVES_PER_CU): norms_trained's means.
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void pairs_trained(TrainedParams p, PairParams pairs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    pairsOfWave<HAS_SUB, FAST>(p, pairs, lds);
}

__global__ void pairs_dense(DensePairParams p)
{
    densePairOfWave(p);
}

// Every trained instance, indexed [HAS_SUB][FAST]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys, <false, false>
// and <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct PairTable {
    const void* trained[2][2] = {};

    PairTable()
    {
        trained[false][true] = reinterpret_cast<const void*>(&pairs_trained<false, true>);
        trained[false][false] = reinterpret_cast<const void*>(&pairs_trained<false, false>);
        trained[true][false] = reinterpret_cast<const void*>(&pairs_trained<true, false>);
    }
};

}  // namespace

namespace memb_pairs {

memb::KernelHandle trainedKernel(bool hasSub, bool fast)
{
    static const PairTable table;
    return memb::KernelHandle{table.trained[hasSub][fast], "pairs_trained"};
}

memb::KernelHandle denseKernel()
{
    return memb::KernelHandle{reinterpret_cast<const void*>(&pairs_dense), "pairs_dense"};
}

}  // namespace memb_pairs
