// Row norms and rows of unit length (include/memb_hip_norms.h), fused with the decode, gfx950 / CDNA4.
//
// A translation unit of its own, linked into libmemb_hip.so beside memb_hip.hip, which plans and launches these kernels
// (hip_norms_launch.h) through the selectors below (hip_norms.h). The device code below the kernels is hip_norms_kernels.h's.
//   norms_trained<HAS_SUB, FAST>   decode_trained's stages up to the symbol tile (decodePoolTile), then per word the squares
//                                  of the lane's two 16-byte pieces, the butterfly and the root: one float per row, NO row
//   unit_trained<HAS_SUB, FAST>    the same body; the pieces held in registers are divided and stored, the norm optionally
//   norms_dense, unit_dense        one wavefront per fp32 row already in memory, any dim and alignment; unit_dense may run
//                                  in place
// The contract is an ORDER (the header spells it out): piece sums ((v0 v0 + v1 v1) + v2 v2) + v3 v3, lane partials over
// the pieces l, l + 64, .., a butterfly of strides 1 .. 32, a correctly rounded root, one correctly rounded division per
// element. Every product and sum is one v_mul_f32 / v_add_f32 (mulRn, addRn: the packed forms flush subnormals on this
// part). Lane l of the trained kernels holds the pieces l and l + 64 of a row -- the contract's layout -- and every kernel
// reduces one row per wavefront at a time, so nothing depends on launch geometry. Nothing is allocated, nothing but the
// norms and the unit rows' columns is written, no atomics, no packed fp32 arithmetic, no scratch.
#include <hip/hip_runtime.h>

#include "../../include/memb_hip_norms.h"
#include "../../include/memb_hip_narrow.h"   // (MEMB_HIP_OUT_*, which hip_pooled_kernels.h stores by)
#include "codec.h"
#include "hip_norms.h"

#define MEMB_HIP_LOOKUP_KERNELS_ONLY

namespace {

constexpr int WAVE = 64;
constexpr uint32_t MISSING = MEMB_HIP_MISSING_ROW;

#include "hip_device_common.h"
#include "hip_trained_kernels.h"
#include "hip_rowwise_kernels.h"

#include "hip_pooled_kernels.h"
#include "hip_norms_kernels.h"

// Seven wavefronts per SIMD, which the launch plans for (ONE_TILE_WAVES_PER_CU): the scalar-register budget of the
// one-tile kernels, and the wavefront count asked of the compiler as pool_trained_narrow does.
template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void norms_trained(TrainedParams p, NormParams norms)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    normsOfWave<HAS_SUB, FAST, false>(p, norms, lds);
}

template <bool HAS_SUB, bool FAST>
__global__ MEMB_SGPR_BUDGET __attribute__((amdgpu_waves_per_eu(7))) void unit_trained(TrainedParams p, NormParams norms)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    normsOfWave<HAS_SUB, FAST, true>(p, norms, lds);
}

__global__ void norms_dense(DenseNormParams p)
{
    denseRowOfWave<false>(p);
}

__global__ void unit_dense(DenseNormParams p)
{
    denseRowOfWave<true>(p);
}

// Every trained instance, indexed [HAS_SUB][FAST][unit]. Key forms <HAS_SUB, FAST>: <false, true> nibble keys,
// <false, false> and <true, false> byte keys (hip_kernel_table.h: KernelTable).
struct NormTable {
    const void* trained[2][2][2] = {};

    NormTable()
    {
        addKeyForm<false, true>();
        addKeyForm<false, false>();
        addKeyForm<true, false>();
    }

private:
    template <bool HAS_SUB, bool FAST>
    void addKeyForm()
    {
        trained[HAS_SUB][FAST][0] = reinterpret_cast<const void*>(&norms_trained<HAS_SUB, FAST>);
        trained[HAS_SUB][FAST][1] = reinterpret_cast<const void*>(&unit_trained<HAS_SUB, FAST>);
    }
};

}  // namespace

namespace memb_norms {

memb::KernelHandle trainedKernel(bool hasSub, bool fast, bool unit)
{
    static const NormTable table;
    return memb::KernelHandle{table.trained[hasSub][fast][unit], unit ? "unit_trained" : "norms_trained"};
}

memb::KernelHandle denseKernel(bool unit)
{
    return unit ? memb::KernelHandle{reinterpret_cast<const void*>(&unit_dense), "unit_dense"}
                : memb::KernelHandle{reinterpret_cast<const void*>(&norms_dense), "norms_dense"};
}

}  // namespace memb_norms
